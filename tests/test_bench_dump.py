"""bench.py --dump-outputs: the file format (CPU; the GPU runs are in
test_bench_modes_gpu.py)."""
import numpy as np

import bench


def test_dump_outputs_formats(tmp_path):
    """u8 / u16 as float32, u32 as float64, 64-bit as two exact halves; signed
    storage (torch has no unsigned 16 / 32 / 64) reads as unsigned."""
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, 1000, dtype=np.uint8)
    i16 = rng.integers(0, 1 << 16, 1000, dtype=np.uint16).view(np.int16)
    i32 = rng.integers(0, 1 << 32, 1000, dtype=np.uint32).view(np.int32)
    i64 = rng.integers(0, 1 << 64, 1000, dtype=np.uint64).view(np.int64)
    bench.dump_outputs(tmp_path, {"a": u8, "b": i16, "c": i32, "d": i64})
    got = {p.name: np.load(p) for p in tmp_path.iterdir()}
    assert set(got) == {"a.npy", "b.npy", "c.npy", "d_lo.npy", "d_hi.npy"}
    assert got["a.npy"].dtype == np.float32 and (got["a.npy"] == u8).all()
    assert got["b.npy"].dtype == np.float32 and (got["b.npy"] == i16.view(np.uint16)).all()
    assert got["c.npy"].dtype == np.float64 and (got["c.npy"] == i32.view(np.uint32)).all()
    u = i64.view(np.uint64)
    assert (got["d_lo.npy"] == (u & 0xFFFFFFFF)).all() and (got["d_hi.npy"] == (u >> 32)).all()


def test_dump_outputs_budget(tmp_path):
    """An array over its share of the 64 MB goes out as a fixed, seeded
    sample in index order; the files together stay within the budget."""
    big = (np.arange(40 << 20, dtype=np.uint32) * 2654435761 >> 24).astype(np.uint8)
    small = np.arange(5000, dtype=np.uint16)
    for k in range(2):
        bench.dump_outputs(tmp_path / str(k), {"big": big, "small": small})
    a, b = (np.load(tmp_path / str(k) / "big.npy") for k in range(2))
    assert sum(p.stat().st_size for p in (tmp_path / "0").iterdir()) <= 64 << 20
    assert (8 << 20) - 64 <= a.size < big.size and (a == b).all()
    assert (np.load(tmp_path / "0" / "small.npy") == small).all()
    # the sample is big's own elements at sorted seeded indices
    idx = np.sort(np.random.default_rng(0xD0).integers(0, big.size, a.size))
    assert (a == big[idx]).all()
