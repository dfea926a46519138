"""tests/build_cases.py hits what it aims at: every generator of the build
kernel's edge tests (test_build_edges_gpu.py) through tests/pyref_build.py
alone.  The statuses are the designed ones, and the kernel's chunk counts,
alignments, regimes and arena edges that a case is there for really occur in
it.  No GPU."""
import numpy as np
import pytest

import build_cases as C
import pyref_build as B


def built(c):
    """pyref_build's (len, status) of a case, the statuses being the designed
    ones and nothing built outside [off, off + len) of the arena."""
    arena, ln, st, frames = B.build_batch(c.records, c.out_off, c.out_size, c.pay_arena, c.pay_off,
                                          c.pay_len, room=c.room)
    assert (st == c.status).all(), np.nonzero(st != c.status)[0][:8]
    assert ((ln == 0) == (st != B.OK)).all()
    return ln.astype(np.int64), st


def regimes(c):
    chains = list(zip(c.records["version"].tolist(), c.records["protocol"].tolist()))
    return np.array([C.regime(ch, int(p)) if ch in C.HDR else -1 for ch, p in zip(chains, c.pay_len)])


@pytest.mark.parametrize("bnd", C.BOUNDARIES)
def test_boundary_cases_straddle_the_boundary(bnd):
    """Over the deltas of one boundary: chunk counts bnd and bnd + 1 both
    occur at every destination and every source alignment (a frame of bnd + 1
    = 129 chunks that still fits the 2048-B room starts at alignment 2 or
    more); every chain is on both sides; with an unaligned out base too."""
    lens, cases = [], []
    for delta in C.DELTAS:
        c = C.boundary_case(bnd, delta)
        ln, st = built(c)
        flen = C.hdr_len(list(zip(c.records["version"].tolist(), c.records["protocol"].tolist()))) + c.pay_len
        assert ((flen >= c.room) == (st == B.NO_ROOM)).all()
        if delta != "random":
            assert (C.dst_align(c) + flen == 16 * bnd + delta).all()
        assert bnd == 128 or (st == B.OK).all()
        ff = C.boundary_case(bnd, delta, 0xFF)
        assert (ff.pay_arena == 0xFF).all() and (ff.status == c.status).all()
        assert ff.records.tobytes() == c.records.tobytes() and (ff.out_off == c.out_off).all()
        assert (ff.pay_off == c.pay_off).all() and (ff.pay_len == c.pay_len).all()
        lens.append(ln)
        cases.append(c)
    if bnd == 128:  # 2047 is built, 2048 is not, and both in one burst
        assert any((ln == 2047).any() and (c.status == B.NO_ROOM).any() for c, ln in zip(cases, lens))
        assert any(((C.hdr_len(list(zip(c.records["version"].tolist(), c.records["protocol"].tolist())))
                     + c.pay_len) == 2048).any() for c in cases)
    for base in (0, 5):
        for side in (bnd, bnd + 1):
            da, sa, protos = set(), set(), set()
            for c, ln in zip(cases, lens):
                m = C.nch(c, ln, base) == side
                da |= set(C.dst_align(c, base)[m].tolist())
                sa |= set(C.src_align(c)[m].tolist())
                protos |= set(zip(c.records["version"][m].tolist(), c.records["protocol"][m].tolist()))
            assert protos == set(C.CHAINS), (side, base)
            if base == 0:
                assert da >= set(range(2 if side == 129 else 0, 16)), (side, da)
                assert sa == set(range(16)), (side, sa)


def full_waves(c):
    return [slice(w, w + C.WAVE) for w in range(0, len(c.records) - C.WAVE + 1, C.WAVE)]


@pytest.mark.parametrize("n", C.MIXED_N)
def test_mixed_cases_mix_within_a_wave(n):
    c = C.mixed_case(n)
    ln, st = built(c)
    reg = regimes(c)
    assert set(st.tolist()) == {B.OK, B.BAD_RECORD, B.NO_ROOM, B.BAD_PAYLOAD}
    assert 0.05 < (st != B.OK).mean() < 0.25
    whole = [w for w in full_waves(c)
             if set(st[w].tolist()) == {0, 1, 2, 3} and set(reg[w][st[w] == B.OK].tolist()) == set(range(5))]
    assert whole, "no wave with every status and every regime"
    # long and short teams side by side in more than the one wave made for it
    k = C.nch(c, ln)
    assert sum(1 for w in full_waves(c) if (k[w] > 32).any() and ((k[w] > 0) & (k[w] <= 8)).any()) >= 2
    assert len(set(C.dst_align(c).tolist())) >= 12 and len(set(C.src_align(c).tolist())) >= 12
    gaps = c.out_off[1:].astype(np.int64) - (c.out_off[:-1].astype(np.int64) + ln[:-1])
    both = (st[1:] == B.OK) & (st[:-1] == B.OK)
    assert (gaps[both] >= 0).all() and (gaps[both] <= 3).all() and (gaps[both] == 0).any()


def test_structured_cases_are_what_they_say():
    """Chunk counts over 32 (the wave copy) exactly where the case puts them."""
    c = C.structured_case("one_long")
    k = C.nch(c, built(c)[0])
    for w, s in enumerate(full_waves(c)):
        assert (np.nonzero(k[s] > 32)[0] == [w]).all() and (k[s][np.arange(16) != w] <= 9).all()
    assert len(full_waves(c)) == 16 and (k > 96).any() and ((k > 32) & (k <= 96)).any() and (k == 0).any()

    c = C.structured_case("two_long")
    k = C.nch(c, built(c)[0])
    for w, s in enumerate(full_waves(c)):
        assert tuple(np.nonzero(k[s] > 32)[0]) == tuple(sorted(C.PAIRS[w]))

    c = C.structured_case("one_dead")
    ln, st = built(c)
    k = C.nch(c, ln)
    dead = set()
    for w, s in enumerate(full_waves(c)):
        assert (k[s] > 32).sum() == 15 and (k[s] == 0).sum() == 1
        dead.add(int(st[s][k[s] == 0][0]))
    assert dead == {B.BAD_RECORD, B.BAD_PAYLOAD, B.NO_ROOM}

    c = C.structured_case("dead_long")
    ln, st = built(c)
    k = C.nch(c, ln)
    flen = C.hdr_len(list(zip(c.records["version"].tolist(), c.records["protocol"].tolist()))) + c.pay_len
    for s in full_waves(c):
        assert (k[s] <= 9).all() and (st[s] == B.NO_ROOM).sum() == 1
        assert flen[s][st[s] == B.NO_ROOM][0] > 512 and (flen[s][st[s] == B.OK] <= 127).all()


@pytest.mark.parametrize("room", C.ROOMS)
def test_jumbo_cases(room):
    c = C.jumbo_case(room)
    ln, st = built(c)
    protos = list(zip(c.records["version"].tolist(), c.records["protocol"].tolist()))
    for ch in C.CHAINS:
        m = np.array([p == ch for p in protos])
        assert sorted(ln[m & (st == B.OK)].tolist()) == list(C.jumbo_lengths(room))
        assert (m & (st == B.NO_ROOM)).sum() == 1
    dead = st == B.NO_ROOM
    if room == 65536:
        assert (c.pay_len[dead] == 65535).all()
    else:
        assert (C.hdr_len(protos)[dead] + c.pay_len[dead] == room).all()
    assert len(c.records) <= 32
    assert {1, 3, 5, 15} <= set(C.dst_align(c).tolist()) and {1, 3, 15} <= set(C.src_align(c).tolist())
    assert (C.jumbo_case(room, 0xFF).pay_arena == 0xFF).all()


def test_payload_edge_cases():
    assert {a % 16 for a in C.PAY_END_LENS if a >= 1700} == set(range(16))
    for a in C.PAY_END_LENS:
        c = C.payload_end_case(a)
        ln, st = built(c)
        ok = st == B.OK
        assert len(c.pay_arena) == a
        assert (c.pay_off[ok].astype(np.int64) + c.pay_len[ok] == a).all()
        assert (c.pay_off[~ok].astype(np.int64) + c.pay_len[~ok] == a + 1).all() and (st[~ok] == B.BAD_PAYLOAD).all()
        want = {p for p in C.EDGE_PLENS + (600, 1700) if p <= a}
        assert set(c.pay_len[ok].tolist()) == want and (~ok).sum() == 3
        assert len(set(C.dst_align(c).tolist())) == min(16, len(c.records))
    seen = set()
    for g in range(C.PAY_START_GROUPS):
        c = C.payload_start_case(g)
        ln, st = built(c)
        for po in range(4 * g, 4 * g + 4):
            m = c.pay_off == po
            assert set(c.pay_len[m].tolist()) == set(C.EDGE_PLENS + (600,))
            seen.add(po)
        assert set(C.dst_align(c).tolist()) == set(range(16))
    assert seen == set(range(16))


def test_out_edge_cases():
    for r in range(16):
        for last, (lo, hi) in enumerate(C.OUT_EDGE_LAST):
            c, o = C.out_edge_case(r, last, False), C.out_edge_case(r, last, True)
            ln, st = built(c)
            lno, sto = built(o)
            assert c.out_size % 16 == r and c.out_off[0] == 0 and ln[0] > 512
            assert int(c.out_off[-1]) + ln[-1] == c.out_size and lo <= ln[-1] <= hi
            assert (st == B.OK).all() and sto.tolist() == [0, 0, 0, B.NO_ROOM]
            assert o.out_size == c.out_size and (o.out_off == c.out_off).all()
            assert o.pay_len[-1] == c.pay_len[-1] + 1 and (o.pay_len[:-1] == c.pay_len[:-1]).all()
            assert int(o.out_off[-1]) + C.HDR[(int(o.records["version"][-1]), int(o.records["protocol"][-1]))] \
                + int(o.pay_len[-1]) == o.out_size + 1
            assert int(o.pay_len[-1]) + C.HDR[(int(o.records["version"][-1]), int(o.records["protocol"][-1]))] < o.room


def test_nopay_case():
    c = C.nopay_case()
    ln, st = built(c)
    assert c.pay_arena is None and len(c.records) < 300
    protos = list(zip(c.records["version"].tolist(), c.records["protocol"].tolist()))
    for ch in C.CHAINS:
        m = np.array([p == ch for p in protos])
        assert set(C.dst_align(c)[m].tolist()) == set(range(16))
        assert (st[m] == (B.BAD_RECORD if ch in C.ICMP else B.OK)).all()
        assert (ln[m] == (0 if ch in C.ICMP else C.HDR[ch])).all()
    live = st == B.OK
    gaps = c.out_off[live][1:].astype(np.int64) - (c.out_off[live][:-1].astype(np.int64) + ln[live][:-1])
    assert (gaps >= 0).all() and (gaps <= 1).all() and (gaps == 1).sum() <= 4
    assert B.build_frame(c.records[-1])[1][40:42] == b"\xff\xff"


def test_base_cases_cover_the_bases():
    """Unaligned bases: the pairs asked for, and over all of them chunk
    counts on both sides of 8, 32, 96 and 128 in memory (the out base moves
    the chunk grid)."""
    pairs = [p for k in range(1, 16) for p in C.base_pairs(k)]
    for k in range(1, 16):
        assert (k, 16 - k) in pairs and (k, k) in pairs
    assert sum(1 for o, p in pairs if p == 0) >= 3 and sum(1 for o, p in pairs if o == 0) >= 3
    counts = set()
    for k in range(1, 16):
        for c in C.base_cases(k)[:2]:
            ln, _ = built(c)
            for ob, _ in C.base_pairs(k):
                counts |= set(C.nch(c, ln, ob).tolist())
    for bnd in C.BOUNDARIES:
        assert {bnd, bnd + 1} <= counts
