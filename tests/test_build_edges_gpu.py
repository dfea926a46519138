"""cgtx_build_batch at its seams, against tests/pyref_build.py bit for bit
(frames, len, status, and the 0xA5 canary wherever the call must not write):
the chunk counts at which the copy changes hands (8: held chunks -> team
loop, 32: team -> wave loop, 96: second wave step), the data room, waves
whose teams disagree, jumbo frames up to the u16 len, both arenas' first and
last bytes, arenas that start off a 16-B boundary, and no payload arena.

The inputs come from tests/build_cases.py; tests/test_build_cases.py checks
without a GPU that they hit what they aim at."""
import numpy as np
import pytest

import build_cases as C
import pyref_build as B
from test_build_gpu import check, run

pytestmark = pytest.mark.gpu


def build_and_check(ctx, c, out_base=None, pay_base=None, want=None):
    got, want = run(ctx, c.records, c.out_off, c.out_size, c.payload(), room=c.room,
                    out_base=out_base, pay_base=pay_base, want=want)
    assert (want[2] == c.status).all(), np.nonzero(want[2] != c.status)[0][:8]
    assert (want[1][c.status != B.OK] == 0).all() and (want[1][c.status == B.OK] != 0).all()
    check(got, want)
    return got, want


@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("bnd", C.BOUNDARIES)
def test_regime_boundaries(ctx, bnd, fill):
    """256 packets a burst, every destination alignment against every source
    alignment, (destination alignment + frame_len) == 16 * bnd + delta for
    each delta of C.DELTAS and drawn per packet; random and all-0xFF payload
    bytes (the same records and layout).  At bnd 128 the frames of 2048 bytes
    and more are NO_ROOM."""
    for delta in C.DELTAS:
        build_and_check(ctx, C.boundary_case(bnd, delta, fill))


@pytest.mark.parametrize("n", C.MIXED_N)
def test_mixed_waves(ctx, n):
    """Every regime (header only .. 2047 B) and every status in one burst,
    packed back to back at random alignments."""
    build_and_check(ctx, C.mixed_case(n))


@pytest.mark.parametrize("what", C.STRUCTURED)
def test_structured_waves(ctx, what):
    """One long packet at each team position, two long ones, a wave long
    everywhere but for one dead team, a wave whose only long packet is
    NO_ROOM (C.structured_case)."""
    build_and_check(ctx, C.structured_case(what))


@pytest.mark.parametrize("room", C.ROOMS)
def test_jumbo_frames(ctx, room):
    """Frames of 9000 and 9215 bytes, and of 65534 and 65535 under room
    65536; plen 65535 (frame length past the u16 len) and frame_len == room
    are NO_ROOM with nothing written."""
    for fill in C.FILLS:
        got, _ = build_and_check(ctx, C.jumbo_case(room, fill))
        assert got[1].max() == (65535 if room == 65536 else 9215)


@pytest.mark.parametrize("arena_len", C.PAY_END_LENS)
def test_payload_ends_on_the_arena_end(ctx, arena_len):
    """Every payload ends on its arena's last byte, arena lengths of every
    residue modulo 16 and arenas shorter than a chunk; one byte further is
    BAD_PAYLOAD."""
    build_and_check(ctx, C.payload_end_case(arena_len))


@pytest.mark.parametrize("group", range(C.PAY_START_GROUPS))
def test_payload_starts_in_the_first_chunk(ctx, group):
    """pay_off 0..15 at every destination alignment."""
    build_and_check(ctx, C.payload_start_case(group))


@pytest.mark.parametrize("residue", range(16))
def test_out_arena_edges(ctx, residue):
    """The first frame at offset 0 and the last one ending on the final byte
    of an out arena of size % 16 == residue, short and long (wave-copied) last
    frames; the same call with that frame one byte longer leaves the arena's
    tail untouched."""
    for last in range(len(C.OUT_EDGE_LAST)):
        for over in (False, True):
            build_and_check(ctx, C.out_edge_case(residue, last, over))


@pytest.mark.parametrize("k", range(1, 16))
def test_unaligned_arena_bases(ctx, k):
    """Both arenas as slices that start off a 16-B boundary, out / payload
    bases (k, 16 - k), (k, k) and for some k (k, 0), (0, k): a mixed burst, a
    boundary burst and the payload-edge bursts.  run() asserts that the out
    tensor is untouched around the slice; the payload tensor's 0x3C around
    its slice is unknown to pyref_build, so no frame may hold it."""
    for c in C.base_cases(k):
        want = None  # the reference does not depend on the bases
        for ob, pb in C.base_pairs(k):
            _, want = build_and_check(ctx, c, out_base=ob, pay_base=pb, want=want)


def test_no_payload_arena(ctx):
    """payload=None: all six chains at every destination alignment, the ICMP
    ones BAD_RECORD, and a zero UDP checksum stored as 0xFFFF."""
    c = C.nopay_case()
    got, _ = build_and_check(ctx, c)
    o = int(c.out_off[-1])
    assert got[0][o + 40] == 0xFF and got[0][o + 41] == 0xFF
