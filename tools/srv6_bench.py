"""Kernel time of cgsr_apply (capsule_amd/csrc/srv6.hip), by device events
over many launches.

  (a) ENCAP, n = 3 segments, on n x 256-B Eth/IPv6/TCP frames (256-B slots in,
      320-B slots out)
  (b) DECAP of (a)'s output (312-B frames)

Every launch works on another copy of its inputs and outputs; the input
copies of one case add up to more than 512 MB, twice the 256 MiB Infinity
Cache, as in bench.py.  Bytes are the algorithm's: frames, descriptors, ops
(and policy indices) read, frames, lengths and statuses written.  Prints one
JSON line per case.  Run bench.py --config nat64_4to6 beside it for the
closest existing rewrite.

    python tools/srv6_bench.py [--n 1048576] [--launches 1000]
"""
import argparse
import ctypes
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from capsule_amd import _native as N  # noqa: E402
from capsule_amd import packets  # noqa: E402

CACHE = 256 << 20
PEAK = 8e12


class Srv6Launcher:
    """A cgsr_apply call with prebuilt ctypes arguments."""

    def __init__(self, ctx, batch, op, pidx, pol, out_arena, out_off):
        n = batch.n
        self.len = torch.empty(n, dtype=torch.int16, device=op.device)
        self.status = torch.empty(n, dtype=torch.uint8, device=op.device)
        self._cb = batch.cbatch()
        self._cp = pol.cstruct() if pol is not None else None
        self._keep = (batch, op, pidx, pol, out_arena, out_off)
        self.out = packets.PacketBatch(out_arena, out_off, self.len)
        vp = ctypes.c_void_p
        self._fn = ctx.L.cgsr_apply
        self._args = [ctx.handle, ctypes.byref(self._cb), vp(op.data_ptr()),
                      vp(pidx.data_ptr()) if pidx is not None else None,
                      ctypes.byref(self._cp) if self._cp is not None else None,
                      N.F_ACCEPT_TCP, 2048, vp(out_arena.data_ptr()), out_arena.numel(),
                      vp(out_off.data_ptr()), vp(self.len.data_ptr()), vp(self.status.data_ptr()),
                      vp(torch.cuda.current_stream().cuda_stream)]

    def __call__(self):
        rc = self._fn(*self._args)
        if rc:
            N.check(rc, "cgsr_apply")


def timed(launchers, launches, warmup=20):
    for k in range(warmup):
        launchers[k % len(launchers)]()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(launches):
        launchers[k % len(launchers)]()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches  # us per launch


def report(name, us, rd, wr, copies, n, launches):
    rate = (rd + wr) / (us * 1e-6)
    print(json.dumps(dict(case=name, n=n, launches=launches, copies=copies,
                          us_per_launch=round(us, 2), bytes_read=rd, bytes_written=wr,
                          bytes_per_s=round(rate, -9), share_of_8TBps=round(rate / PEAK, 4),
                          device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("srv6_bench: no GPU (a CPU run measures nothing)")
    n, dev = a.n, "cuda:0"
    ctx = packets.Context(0)

    def slots(slot):
        o = torch.arange(n, device=dev, dtype=torch.int64) * slot
        return torch.where(o >= 1 << 31, o - (1 << 32), o).to(torch.int32)

    hdr = bytes.fromhex("020000ffffff02000000000186dd") + bytes([0x60, 0, 0, 0, 0, 202, 6, 64]) + \
        bytes.fromhex("20010db8000000000000000000000001") + bytes.fromhex("20010db8000000000000000000000002")
    rng = np.random.default_rng(0)
    segs = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(3)]
    pol = packets.srv6_policies([(segs, 2, 0, N.SR_P_SET_DST)], dev)
    copies = max(2, -(-(2 * CACHE + 1) // (n * 256)))
    in_off, out_off = slots(256), slots(320)
    ln = torch.full((n,), 256, dtype=torch.int16, device=dev)
    op = torch.full((n,), N.SR_OP["ENCAP"], dtype=torch.uint8, device=dev)
    pidx = torch.zeros(n, dtype=torch.int32, device=dev)
    enc = []
    for _ in range(copies):
        arena = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device=dev)
        arena[:, :54] = torch.tensor(list(hdr), dtype=torch.uint8, device=dev)
        b = packets.PacketBatch(arena.view(-1), in_off, ln)
        enc.append(Srv6Launcher(ctx, b, op, pidx, pol, torch.empty(n * 320, dtype=torch.uint8, device=dev),
                                out_off))
    us = timed(enc, a.launches)
    assert int(enc[0].status.max()) == 0 and int(enc[0].len.min()) == 312
    report("srv6_encap3_256B", us, n * (256 + 4 + 2 + 1 + 4 + 4), n * (312 + 3), copies, n, a.launches)

    op = torch.full((n,), N.SR_OP["DECAP"], dtype=torch.uint8, device=dev)
    dec = [Srv6Launcher(ctx, e.out, op, None, None, torch.empty(n * 256, dtype=torch.uint8, device=dev), in_off)
           for e in enc]
    us = timed(dec, a.launches)
    assert int(dec[0].status.max()) == 0 and int(dec[0].len.min()) == 256
    report("srv6_decap3_312B", us, n * (312 + 4 + 2 + 1 + 4), n * (256 + 3), copies, n, a.launches)
    ctx.check()
    ctx.close()


if __name__ == "__main__":
    main()
