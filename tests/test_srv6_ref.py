"""tests/pyref_srv6.py, the independent restatement of the SRv6 edits, pinned
by srh.rs's own tests on the golden fixtures and cross-checked against the
oracle's parse + reconcile on every generated case; and the generators of
tests/srv6_cases.py reach what they claim.  No GPU."""
import json
import pathlib
import struct

import numpy as np
import pytest

import oracle_lib
import pyref_srv6 as R
import srv6_cases as C
from capsule_amd import _native as N
from capsule_amd import synth

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
PACKETS = json.loads((GOLD / "reference_packets.json").read_text())
NAMES = ("IPV6_TCP_PACKET", "SR_TCP_PACKET", "IPV6_FRAGMENT_PACKET", "ICMPV6_PACKET",
         "VLAN_DOT1Q_PACKET", "VLAN_QINQ_PACKET", "IPV4_UDP_PACKET", "ROUTER_ADVERT_PACKET")


def fixture(name):
    return bytes.fromhex(PACKETS[name]["hex"])


def v6(i):
    return bytes(15) + bytes([i])


def test_insert_segment_routing_packet():
    """srh.rs insert_segment_routing_packet: push on IPV6_TCP_PACKET."""
    f = fixture("IPV6_TCP_PACKET")
    st, g = R.apply(f, R.OP_ENCAP, ([bytes(16)], 0, 0, 0), R.ACCEPT_TCP)
    assert st == R.OK and len(g) == len(f) + 24
    assert g[54 + 1] == 2 and g[54 + 2] == 4 and g[54] == 6 and g[20] == 43
    assert struct.unpack_from(">H", g, 78)[0] == 36869
    assert struct.unpack_from(">H", g, 18)[0] == struct.unpack_from(">H", f, 18)[0] + 24


def test_remove_segment_routing_packet():
    f = fixture("SR_TCP_PACKET")
    st, g = R.apply(f, R.OP_DECAP, None, R.ACCEPT_TCP)
    assert st == R.OK and g[20] == 6 and struct.unpack_from(">H", g, 54)[0] == 3464
    assert len(g) == len(f) - 8 - 16 * (f[58] + 1)


def test_set_segments():
    f = fixture("SR_TCP_PACKET")
    st, g = R.apply(f, R.OP_SET, ([v6(1)], 0, 0, 0), R.ACCEPT_TCP)
    assert st == R.OK and g[55] == 2 and g[58] == 0 and g[62:78] == v6(1)
    assert struct.unpack_from(">H", g, 78)[0] == 3464
    st, h = R.apply(g, R.OP_SET, ([v6(1), v6(2), v6(3), v6(4)], 0, 0, 0), R.ACCEPT_TCP)
    assert st == R.OK and h[55] == 8 and h[58] == 3 and h[62:126] == v6(1) + v6(2) + v6(3) + v6(4)
    assert struct.unpack_from(">H", h, 126)[0] == 3464
    assert R.apply(f, R.OP_SET, ([], 0, 0, 0))[0] == R.BAD_POLICY


def test_compute_checksum():
    """srh.rs compute_checksum: the pseudo-header's dst is segments[0]."""
    f = fixture("SR_TCP_PACKET")
    sums = []
    for sg, sl in (([v6(1), v6(2), v6(3), v6(4)], 3), ([v6(1)], 0), ([v6(1)], 0)):
        st, f = R.apply(f, R.OP_SET, (sg, sl, 0, 0), R.ACCEPT_TCP)
        assert st == R.OK
        sums.append(struct.unpack_from(">H", f, 54 + 8 + 16 * len(sg) + 16)[0])
    assert sums[0] != 0 and sums[0] == sums[1] == sums[2]


def oracle_reconciled(frames, accept):
    """or_parse_batch_ext, or_reconcile at L4, then at L3 for what that skipped."""
    flags = accept | N.F_ACCEPT_V6 | N.F_V6_EXT
    arena, off, ln = synth.pack_frames(frames, 64)
    meta = oracle_lib.parse_batch_ext(arena, off, ln, flags)[0]
    out, st = oracle_lib.reconcile(arena, off, ln, meta, flags, N.LAYER_L4)
    skipped = st == N.RECON_SKIPPED
    out3, st3 = oracle_lib.reconcile(out, off, ln, meta, flags, N.LAYER_L3)
    res = []
    for i, f in enumerate(frames):
        src = out3 if skipped[i] else out
        res.append(bytes(src[off[i]:off[i] + len(f)]))
    return res


def test_round_trip_is_the_oracles_fixture():
    f = fixture("SR_TCP_PACKET")
    n = f[58] + 1
    sg = [f[62 + 16 * j:78 + 16 * j] for j in range(n)]
    st, g = R.apply(f, R.OP_DECAP, None, R.ACCEPT_TCP)
    assert st == R.OK
    tag = struct.unpack_from(">H", f, 60)[0]
    st, h = R.apply(g, R.OP_ENCAP, (sg, f[57], tag, 0), R.ACCEPT_TCP)
    assert st == R.OK
    want = bytearray(oracle_reconciled([f], R.ACCEPT_TCP)[0])
    want[59] = 0  # push writes flags 0 (SegmentRoutingHeader::default)
    assert h[:59] + h[60:] == bytes(want[:59] + want[60:]) and (h[59] == 0)


def all_cases():
    fx = [fixture(k) for k in NAMES]
    cs = [C.fixtures_cross(fx, 2048), C.fixtures_cross(fx, 65536), C.alignments(), C.zero_udp_sum(),
          C.mixed_wave(32), C.mixed_wave(65), C.room_edges(), C.final_from_packet(), C.big_policy(5)]
    cs += [C.suffix_lengths(o, l4) for o in (1, 2, 3, 4) for l4 in (17, 6, 58)]
    cs += [C.truncated(o) for o in (1, 2, 3, 4)] + C.arena_end(0) + C.arena_end(-1)
    return cs


CASES = all_cases()


@pytest.mark.parametrize("k", range(len(CASES)))
def test_restatement_agrees_with_the_oracle(k):
    c = CASES[k]
    st, ln, want_st, outs = None, None, None, None
    _, _, want_st, outs = C.expect(c)
    pre, idx = [], []
    for i, f in enumerate(c.frames):
        if outs[i] is None or c.op[i] == R.OP_NONE:
            continue
        p = int(c.policy_idx.view(np.uint32)[i])
        s, sp = R.spliced(f, int(c.op[i]), c.policies[p] if p < len(c.policies) else None, c.room)
        assert s == R.OK
        pre.append(sp), idx.append(i)
    if not pre:
        return
    with oracle_lib.data_room(65536):
        got = oracle_reconciled(pre, c.accept)
    for i, g in zip(idx, got):
        assert g == outs[i], (k, i)


def test_generators_reach_what_they_claim():
    w = C.expect(C.mixed_wave(32))
    assert set(C.ST_ALL) <= set(w[2].tolist())
    assert set(C.mixed_wave(32).op.tolist()) >= {0, 1, 2, 3, 4}
    lens = [C.nch(int(o), int(n)) for o, n in zip(C.mixed_wave(32).out_off, w[1])]
    assert max(lens) > C.TEAM_CHUNKS + C.WAVE_STEP and min(x for x in lens if x) < 8
    a = C.alignments()
    assert {(int(i) % 16, int(o) % 16) for i, o in zip(a.in_off, a.out_off)} == \
        {(i, o) for i in range(16) for o in range(16)}
    for op in (1, 2, 3, 4):
        c = C.suffix_lengths(op, 17)
        w = C.expect(c)
        assert (w[2] == 0).all()
        n = {C.nch(11 + int(o), int(x)) for o, x in zip(c.out_off, w[1])}
        assert {8, 9, 32, 33, 96, 97} <= n, (op, sorted(n))
        assert {int(o) % 2 for o in c.out_off} == {0, 1}
    assert C.expect(C.room_edges())[2].tolist() == [0, 0, 13, 13, 0, 0, 0, 0]
    for f in C.expect(C.zero_udp_sum())[3]:
        assert f[len(f) - 23:len(f) - 21] == b"\xff\xff"
    for spare, last in ((0, 0), (-1, R.NOT_RESIZED)):
        for c in C.arena_end(spare):
            assert C.expect(c)[2].tolist() == [0, 0, last]
    for op in (2, 3, 4):
        w = C.expect(C.truncated(op))
        assert {R.EXT_BAD_OFFSET, R.EXT_OUT_OF_BUFFER, R.L3_OUT_OF_BUFFER} <= set(w[2].tolist())
        assert w[2][-1] == 0 and (w[2][:-9] != 0).all()
