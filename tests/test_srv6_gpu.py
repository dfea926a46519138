"""cgsr_apply on the device against tests/pyref_srv6.py, bit for bit: frames,
len and status; every byte the call must not write is compared against a
0xA5 canary fill of the out arena."""
import json
import pathlib

import numpy as np
import pytest
import torch

import pyref_srv6 as R
import srv6_cases as C
from capsule_amd import _native as N
from capsule_amd import batch, packets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64  # bytes kept around an arena that is a slice of a larger tensor
PACKETS = json.loads((pathlib.Path(__file__).resolve().parent / "golden" /
                      "reference_packets.json").read_text())
FIXTURES = [bytes.fromhex(PACKETS[k]["hex"]) for k in
            ("IPV6_TCP_PACKET", "SR_TCP_PACKET", "IPV6_FRAGMENT_PACKET", "ICMPV6_PACKET",
             "VLAN_DOT1Q_PACKET", "VLAN_QINQ_PACKET", "IPV4_UDP_PACKET", "ROUTER_ADVERT_PACKET")]


def sliced(size, base, fill, data=None):
    """A device tensor of `size` bytes that starts `base` bytes above a 16-B
    boundary, as a slice of a larger one filled with `fill` -> (whole, slice)."""
    whole = torch.full((GUARD + 16 + size + GUARD,), fill, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 16 == 0 and 0 <= base < 16
    part = whole[GUARD + base: GUARD + base + size]
    if data is not None:
        part.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.uint8)))
    assert part.data_ptr() % 16 == base and part.is_contiguous()
    return whole, part


def device_policies(pols, seg_base=0):
    """The case's policies as the device sees them; a None entry becomes a
    record whose list runs past the segment arena."""
    rec = np.zeros(len(pols), np.dtype(N.SR_POLICY_FIELDS))
    sg = []
    for i, p in enumerate(pols):
        if p is None:
            rec[i] = (0xFFFFFFF0, 3, 0, 0, 0, 0)
            continue
        rec[i] = (len(sg), len(p[0]), p[1], p[2], p[3], 0)
        sg.extend(p[0])
    arena = np.frombuffer(b"".join(sg), np.uint8)
    pol = torch.from_numpy(rec.view(np.uint8).reshape(-1, 16).copy()).to(DEV)
    st = sliced(len(arena), seg_base, 0x3C, arena)[1].view(-1, 16)
    return packets.Srv6Policies(pol, st, max(len(p[0]) for p in pols if p is not None))


def run(ctx, c, in_base=0, out_base=0, seg_base=0):
    """One call over a canary-filled out arena -> (arena, len, status) as
    numpy.  Both arenas are slices of larger tensors that start in_base /
    out_base bytes above a 16-B boundary; the out tensor is 0xA5 all over and
    has to be outside the slice afterwards too, the in tensor is 0x3C around
    the frames, which pyref_srv6, given the frames alone, never sees."""
    n = len(c.frames)
    in_size = int(max((int(o) + len(f) for o, f in zip(c.in_off, c.frames)), default=0)) + 1
    host = np.full(in_size, 0x3C, np.uint8)
    for o, f in zip(c.in_off, c.frames):
        host[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
    _, ia = sliced(in_size, in_base, 0x3C, host)
    whole, oa = sliced(c.out_size, out_base, 0xA5)
    pb = packets.PacketBatch.from_numpy(np.zeros(0, np.uint8), c.in_off,
                                        np.asarray([len(f) for f in c.frames], np.uint16), DEV)
    pb = packets.PacketBatch(ia, pb.off, pb.len)
    op = torch.from_numpy(c.op).to(DEV)
    pi = torch.from_numpy(c.policy_idx).to(DEV)
    oo = torch.from_numpy(c.out_off.view(np.int32)).to(DEV)
    ob, st = packets.srv6(ctx, pb, op, pi, device_policies(c.policies, seg_base), flags=c.accept,
                          room=c.room, out=(oa, oo))
    torch.cuda.synchronize()
    lo = GUARD + out_base
    outside = torch.cat((whole[:lo], whole[lo + c.out_size:])).cpu().numpy()
    bad = np.nonzero(outside != 0xA5)[0]
    assert bad.size == 0, ("bytes written outside the out arena", out_base, bad[:16] - lo)
    assert n == ob.n
    return oa.cpu().numpy(), ob.len.cpu().numpy().view(np.uint16), st.cpu().numpy()


def check(got, want):
    assert (got[2] == want[2]).all(), ("status", np.nonzero(got[2] != want[2])[0][:8],
                                       got[2][got[2] != want[2]][:8], want[2][got[2] != want[2]][:8])
    assert (got[1] == want[1]).all(), ("len", np.nonzero(got[1] != want[1])[0][:8])
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, ("arena bytes", bad[:16], got[0][bad[:16]], want[0][bad[:16]])


def both(ctx, c, **kw):
    want = C.expect(c)
    check(run(ctx, c, **kw), want)
    return want


@pytest.mark.parametrize("room", [2048, 65536])
def test_fixtures_all_ops_all_policies(ctx, room):
    c = C.fixtures_cross(FIXTURES, room)
    want = both(ctx, c)
    big = np.asarray([c.policies[p][0].__len__() == 127 and o in (R.OP_ENCAP, R.OP_SET)
                      for p, o in zip(c.policy_idx, c.op)])
    v6 = want[2][big] != R.NOT_IPV6
    if room == 2048:  # 127 segments do not fit DPDK's default data room
        assert (want[2][big][v6] != R.OK).all() and (want[2][big] == R.NOT_RESIZED).any()
    else:
        assert (want[2][big] == R.OK).any()


def test_all_alignments(ctx):
    both(ctx, C.alignments())


@pytest.mark.parametrize("l4", [17, 6, 58])
@pytest.mark.parametrize("op", [R.OP_ENCAP, R.OP_DECAP, R.OP_END, R.OP_SET])
def test_suffix_lengths(ctx, op, l4):
    want = both(ctx, C.suffix_lengths(op, l4), in_base=5, out_base=11)
    assert (want[2] == R.OK).all()


def test_udp_sum_zero_is_stored_as_ffff(ctx):
    c = C.zero_udp_sum()
    want = both(ctx, c)
    for f in want[3]:
        assert f[len(f) - 29 + 6:len(f) - 29 + 8] == b"\xff\xff"


@pytest.mark.parametrize("n", [1, 16, 32, 63, 64, 65, 200])
def test_every_op_and_status_side_by_side(ctx, n):
    c = C.mixed_wave(n)
    want = both(ctx, c, in_base=9, out_base=2, seg_base=7)
    if n >= 32:
        assert set(C.ST_ALL) <= set(want[2].tolist())


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_n_127_at_room_65536(ctx, n):
    want = both(ctx, C.big_policy(n))
    assert (want[2] == R.OK).all()


def test_room_edges(ctx):
    want = both(ctx, C.room_edges())
    assert want[2].tolist() == [0, 0, R.NOT_RESIZED, R.NOT_RESIZED, 0, 0, 0, 0]


@pytest.mark.parametrize("spare", [0, -1])
def test_last_frame_at_the_arena_end(ctx, spare):
    for c in C.arena_end(spare):
        want = both(ctx, c, out_base=13)
        assert want[2][:2].tolist() == [0, 0] and want[2][2] == (0 if spare == 0 else R.NOT_RESIZED)


@pytest.mark.parametrize("base", range(1, 16))
def test_unaligned_arena_bases(ctx, base):
    both(ctx, C.mixed_wave(32, seed=base), in_base=base, out_base=(base * 7) % 16 or 1,
         seg_base=(base * 3) % 16)


@pytest.mark.parametrize("op", [R.OP_ENCAP, R.OP_SET, R.OP_END, R.OP_DECAP])
def test_truncated_inputs(ctx, op):
    both(ctx, C.truncated(op))


def test_final_from_packet_keeps_the_checksum(ctx):
    c = C.final_from_packet()
    want = both(ctx, c)
    for f, g in zip(c.frames, want[3]):
        l4 = 54 + (40 if f[20] == 43 else 0)  # the input's L4 offset (2 segments)
        assert g[len(g) - (len(f) - l4):] == f[l4:]  # Udp length, checksums and all


def test_batch_srv6_combinator(ctx):
    """ENCAP for even packets, NONE for odd ones, aborts for bad ones; the
    output parsed again on the device."""
    rng = np.random.default_rng(11)
    sg = C.rand_segs(3, rng)
    pols = packets.srv6_policies([(sg, 2, 0x1234, N.SR_P_SET_DST)], DEV)
    frames = [C.frame(rng, (17, 6)[i % 2], 20 + i) for i in range(10)]
    frames[4] = frames[4][:30]  # L3_OUT_OF_BUFFER
    rx = batch.Channel()
    rx.transmit(frames)

    def pick(sub):
        i = torch.arange(sub.n, device=DEV)
        return (i % 2 == 0).to(torch.uint8) * N.SR_OP["ENCAP"], torch.zeros(sub.n, dtype=torch.int32, device=DEV)

    pipe = batch.Poll(ctx, rx, DEV).srv6(pols, pick)
    pipe.replenish()
    b = pipe.next_burst()
    disp = b.dispositions()
    assert disp == [batch.ACT] * 4 + [batch.ABORT] + [batch.ACT] * 5
    assert int(b.status[4].item()) == N.PKT["L3_OUT_OF_BUFFER"]
    r = packets.parse(ctx, b.batch, flags=packets.parse_flags() | N.F_V6_EXT, ext=True)
    torch.cuda.synchronize()
    ext = r.ext.cpu().numpy().view(np.dtype(N.EXT_RECORD_FIELDS)).reshape(-1)
    meta = r.meta.cpu().numpy().view(np.uint32)
    for i in (0, 2, 6, 8):
        assert ext[i]["kind"] == N.EXT_SRH and ext[i]["segments_left"] == 2 and ext[i]["last_entry"] == 2
        assert bytes(ext[i]["segment0"]) == sg[0] and meta[i] & N.META_L4_CSUM_OK
        assert b.batch.frame(i)[38:54] == sg[2]
    for i in (1, 3, 5, 7, 9):
        assert b.batch.frame(i) == frames[i]
