"""Inputs for the SRv6 kernel's tests (test_srv6_gpu.py) and the CPU checks
that they hit what they aim at and that tests/pyref_srv6.py agrees with the
oracle on them (test_srv6_ref.py).  numpy only: importable without a GPU.

Every generator returns a Case: frames (list of bytes), in_off, op,
policy_idx, policies (pyref form: (segments, segments_left, tag, flags) or
None for an entry the device sees as broken), out_off, out_size, room,
accept.

The kernel (capsule_amd/csrc/srv6.hip) cuts an output frame into 16-B chunks
of the out arena's memory; nch(), below, is its chunk count.  Chunks 0..31
are made by the packet's team of 4 lanes in steps of 4, chunks from 32 on by
the whole wave in steps of 64 (32..95, 96..159, ...)."""
import collections
import struct

import numpy as np

import pyref_srv6 as R

WAVE = 16  # packets a wave edits (teams of 4 lanes)
UDP, TCP, ICMP = R.ACCEPT_UDP, R.ACCEPT_TCP, R.ACCEPT_ICMP
ALL = UDP | TCP | ICMP
TEAM_CHUNKS, WAVE_STEP = 32, 64

Case = collections.namedtuple("Case", "frames in_off op policy_idx policies out_off out_size room accept")


def nch(out_off, length):
    """Chunks of a frame of `length` bytes at byte `out_off` of a 16-B aligned arena."""
    return 0 if length == 0 else ((out_off + length + 15) // 16) - out_off // 16


def seg(i, fill=0x20):
    return bytes([fill, 0x01, 0x0D, 0xB8]) + bytes(10) + struct.pack(">H", i)


def segs(n, base=1):
    return [seg(base + j) for j in range(n)]


def rand_segs(n, rng):
    return [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(n)]


def eth_hdr(vlan, rng):
    h = bytes(rng.integers(0, 256, 12, dtype=np.uint8))
    if vlan == 1:
        h += b"\x81\x00" + bytes(rng.integers(0, 256, 2, dtype=np.uint8))
    elif vlan == 2:
        h += b"\x88\xa8" + bytes(rng.integers(0, 256, 2, dtype=np.uint8))
        h += b"\x81\x00" + bytes(rng.integers(0, 256, 2, dtype=np.uint8))
    return h + b"\x86\xdd"


def frame(rng, l4=17, body=32, vlan=0, srh=None, sl=None, frag=False):
    """Ethernet / Ipv6 [/ SRH with `srh` random segments | / Fragment] / `body`
    random bytes behind the IPv6 (extension) headers, next header `l4`; the
    length and checksum fields are random (stale)."""
    ext = b""
    nh = l4
    if frag:
        ext = bytes([nh, 0]) + bytes(rng.integers(0, 256, 6, dtype=np.uint8))
        nh = 44
    if srh is not None:
        sl = srh - 1 if sl is None else sl
        ext = bytes([nh, 2 * srh, 4, sl, srh - 1, int(rng.integers(0, 256))]) + \
            bytes(rng.integers(0, 256, 2, dtype=np.uint8)) + b"".join(rand_segs(srh, rng)) + ext
        nh = 43
    ip6 = bytes([0x60 | int(rng.integers(0, 16))]) + bytes(rng.integers(0, 256, 5, dtype=np.uint8)) + \
        bytes([nh, int(rng.integers(1, 256))]) + bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    return eth_hdr(vlan, rng) + ip6 + ext + bytes(rng.integers(0, 256, body, dtype=np.uint8))


def pack(lengths, base=0, gap=0):
    """Back-to-back offsets from `base` with `gap` spare bytes between."""
    off, o = [], base
    for ln in lengths:
        off.append(o)
        o += ln + gap
    return np.asarray(off, np.uint32), o


def out_len(f, op, pol):
    st, s = R.spliced(f, op, pol, room=1 << 20)
    return len(s) if st == R.OK else 0


def case(frames, op, pidx, policies, room=2048, accept=ALL, in_base=0, out_base=0, in_gap=0,
         out_gap=0, out_size=None, out_off=None):
    in_off, _ = pack([len(f) for f in frames], in_base, in_gap)
    if out_off is None:
        lens = []
        for f, o, p in zip(frames, op, pidx):
            pol = policies[p] if 0 <= p < len(policies) else None
            lens.append(out_len(f, o, pol))
        out_off, end = pack(lens, out_base, out_gap)
        out_size = end + 16 if out_size is None else out_size
    return Case(list(frames), in_off, np.asarray(op, np.uint8), np.asarray(pidx, np.uint32).view(np.int32),
                list(policies), np.asarray(out_off, np.uint32), int(out_size), int(room), int(accept))


def expect(c):
    """pyref_srv6.apply_batch of the case."""
    return R.apply_batch(c.frames, c.op, c.policy_idx.view(np.uint32), c.policies, c.out_off,
                         c.out_size, c.accept, c.room)


POLICY_N = (1, 2, 3, 4, 16, 127)


def std_policies(rng):
    """One policy per n of POLICY_N, with varied flags."""
    out = []
    for j, n in enumerate(POLICY_N):
        fl = (0, R.P_SET_DST, R.P_FINAL_FROM_PACKET, R.P_SET_DST | R.P_FINAL_FROM_PACKET)[j % 4]
        out.append((rand_segs(n, rng), n - 1 if j % 2 else 0, int(rng.integers(0, 65536)), fl))
    return out


def fixtures_cross(fixtures, room):
    """Every fixture under every op and every policy of POLICY_N."""
    rng = np.random.default_rng(1)
    pols = std_policies(rng)
    fr, op, pi = [], [], []
    for f in fixtures:
        for o in (R.OP_NONE, R.OP_END, R.OP_DECAP):
            fr.append(f), op.append(o), pi.append(0)
        for o in (R.OP_ENCAP, R.OP_SET):
            for p in range(len(pols)):
                fr.append(f), op.append(o), pi.append(p)
    return case(fr, op, pi, pols, room=room, out_gap=1)


def alignments():
    """All 16 x 16 in / out alignments (mod 16) of an ENCAP (n = 2) over a
    UDP frame with a 100-B suffix (more than one 64-B team step)."""
    rng = np.random.default_rng(2)
    pols = [(rand_segs(2, rng), 1, 7, R.P_SET_DST)]
    fr = [frame(rng, 17, 100) for _ in range(256)]
    in_off = np.asarray([i * 256 + (i % 16) for i in range(256)], np.uint32)
    out_off = np.asarray([i * 256 + (i // 16) for i in range(256)], np.uint32)
    c = case(fr, [R.OP_ENCAP] * 256, [0] * 256, pols, out_off=out_off, out_size=256 * 256)
    return c._replace(in_off=in_off)


def boundary_lengths(head):
    """Output lengths (at offset 0 mod 16) one below, at and one above every
    regime boundary of the kernel: a team step, the team / wave hand-over at
    32 chunks, the wave's first and second 64-chunk step."""
    out = set()
    for ch in (4, 8, TEAM_CHUNKS, TEAM_CHUNKS + 1, TEAM_CHUNKS + WAVE_STEP, TEAM_CHUNKS + WAVE_STEP + 1):
        for d in (-17, -16, -15, -1, 0, 1):
            if 16 * ch + d > head:
                out.add(16 * ch + d)
    return sorted(out)


def suffix_lengths(op, l4):
    """Suffix (L4 header + payload) lengths 0..130 and around the regime
    boundaries, at odd and even out offsets, under ENCAP (n = 1) / DECAP
    (n = 2) / END / SET (3 -> 1)."""
    rng = np.random.default_rng(3 + op + l4)
    pols = [(rand_segs(1, rng), 0, 1, 0)]
    srh = {R.OP_ENCAP: None, R.OP_DECAP: 2, R.OP_END: 2, R.OP_SET: 3}[op]
    head = 54 + (24 if op == R.OP_ENCAP else 0 if op == R.OP_DECAP else 40 if op == R.OP_END else 24)
    bodies = list(range(0, 131)) + [b - head for b in boundary_lengths(head)]
    fr = [frame(rng, l4, b, srh=srh) for b in bodies]
    c = case(fr, [op] * len(fr), [0] * len(fr), pols, out_gap=0, in_gap=0, in_base=1)
    return c


def zero_udp_sum():
    """A UDP datagram whose computed checksum is 0, so 0xFFFF is stored
    (udp.rs:132-141): plain, behind a new SRH, and after DECAP."""
    rng = np.random.default_rng(4)
    pols = [(rand_segs(2, rng), 0, 0, R.P_FINAL_FROM_PACKET)]
    fr, op = [], []
    for o, srh in ((R.OP_ENCAP, None), (R.OP_DECAP, 1), (R.OP_END, 2), (R.OP_SET, 2)):
        f = bytearray(frame(rng, 17, 8 + 21, srh=srh))
        f[-5:-3] = b"\0\0"
        st, out = R.apply(bytes(f), o, pols[0], UDP)
        assert st == R.OK
        l4o = len(out) - 29
        ck = struct.unpack_from(">H", out, l4o + 6)[0]
        w = (0xFFFF - (~ck & 0xFFFF)) & 0xFFFF  # ck was ~c: the word that makes c 0xFFFF
        f[-5:-3] = struct.pack(">H", w)
        fr.append(bytes(f)), op.append(o)
    return case(fr, op, [0] * len(fr), pols, accept=UDP)


ST_ALL = (R.OK, R.ETH_BAD_OFFSET, R.ETH_OUT_OF_BUFFER, R.NOT_IPV6, R.L3_BAD_OFFSET,
          R.L3_OUT_OF_BUFFER, R.NOT_RESIZED, R.EXT_BAD_OFFSET, R.EXT_OUT_OF_BUFFER,
          R.SRH_INCONSISTENT, R.BAD_OP, R.BAD_POLICY, R.NOT_ROUTING, R.NO_SEGMENTS_LEFT,
          R.BAD_SEGMENTS_LEFT)


def mixed_wave(n=2 * WAVE, seed=5):
    """Every op and every status side by side in two waves (a wave edits 16
    packets; 14 failures and 5 ops do not fit one), long (wave-copied) and
    short frames mixed across team positions; VLAN depths 0-2; UDP, TCP,
    ICMPv6, an unaccepted next header, a Fragment header and ENCAP over an
    SRH."""
    rng = np.random.default_rng(seed)
    pols = [(rand_segs(3, rng), 2, 0xBEEF, R.P_SET_DST), (rand_segs(1, rng), 0, 1, 0), None,
            (rand_segs(40, rng), 5, 2, R.P_FINAL_FROM_PACKET)]
    T = lambda f, k: f[:k]
    inc = bytearray(frame(rng, 6, 30, srh=2))
    inc[54 + 1] = 6
    nosl = frame(rng, 17, 20, srh=2, sl=0)
    badsl = frame(rng, 17, 20, srh=2, sl=4)
    v4 = bytearray(frame(rng, 17, 20))
    v4[12:14] = b"\x08\x00"
    pat = [
        (frame(rng, 17, 900, vlan=1), R.OP_ENCAP, 0),           # long, wave-copied
        (frame(rng, 6, 20, srh=3), R.OP_DECAP, 0),
        (frame(rng, 58, 12, vlan=2, srh=2), R.OP_END, 0),
        (frame(rng, 6, 1400, srh=2), R.OP_SET, 3),              # long, list grows past 512 B
        (b"", R.OP_ENCAP, 0),                                   # ETH_BAD_OFFSET
        (T(frame(rng), 13), R.OP_DECAP, 0),                     # ETH_OUT_OF_BUFFER
        (bytes(v4), R.OP_ENCAP, 0),                             # NOT_IPV6
        (T(frame(rng), 14), R.OP_ENCAP, 0),                     # L3_BAD_OFFSET
        (T(frame(rng, vlan=1), 57), R.OP_ENCAP, 0),             # L3_OUT_OF_BUFFER
        (frame(rng, 17, 2048 - 54 - 56 - 1), R.OP_ENCAP, 0),    # NOT_RESIZED (grow == T)
        (T(frame(rng, srh=1), 54), R.OP_END, 0),                # EXT_BAD_OFFSET
        (T(frame(rng, srh=2), 54 + 8 + 31), R.OP_SET, 1),       # EXT_OUT_OF_BUFFER
        (bytes(inc), R.OP_DECAP, 0),                            # SRH_INCONSISTENT
        (frame(rng), 9, 0),                                     # BAD_OP
        (frame(rng, 6, 40), R.OP_ENCAP, 2),                     # BAD_POLICY (broken entry)
        (frame(rng, 17, 700), R.OP_DECAP, 0),                   # NOT_ROUTING, long input
        (nosl, R.OP_END, 0),                                    # NO_SEGMENTS_LEFT
        (badsl, R.OP_END, 0),                                   # BAD_SEGMENTS_LEFT
        (frame(rng, 17, 64), R.OP_ENCAP, 7),                    # BAD_POLICY (index)
        (frame(rng, 59, 33), R.OP_ENCAP, 1),                    # unaccepted next header
        (frame(rng, 17, 40, frag=True), R.OP_ENCAP, 1),         # Fragment behind IPv6
        (frame(rng, 6, 40, srh=2), R.OP_ENCAP, 0),              # ENCAP over an SRH
        (frame(rng, 17, 40, srh=1, frag=True), R.OP_DECAP, 0),  # DECAP uncovers a Fragment
        (frame(rng, 6, 2000, vlan=2), R.OP_NONE, 0),            # NONE, long
        (frame(rng, 58, 77, srh=4, sl=2), R.OP_END, 0),
        (frame(rng, 6, 21, srh=5), R.OP_SET, 1),                # SET shrink
        (frame(rng, 17, 9, srh=1), R.OP_SET, 0),                # SET grow
        (frame(rng, 17, 0), R.OP_ENCAP, 1),                     # no L4 header at all
        (frame(rng, 6, 19), R.OP_ENCAP, 1),                     # short TCP header
        (frame(rng, 17, 31, srh=3), R.OP_SET, 0),               # SET, equal counts
        (frame(rng, 17, 1100, srh=2), R.OP_DECAP, 0),           # long DECAP
        (frame(rng, 6, 5, vlan=1), R.OP_NONE, 0),
    ]
    rows = [pat[i % len(pat)] for i in range(n)]
    fr, op, pi = zip(*rows)
    return case(fr, op, pi, pols, out_gap=0, in_base=3, out_base=5)


def room_edges():
    """grow == T - 1 edits and grow == T does not (ENCAP and SET); a SET
    shrink at T = 0; SET with equal counts at T = 0; n = 127 at room 65536."""
    rng = np.random.default_rng(6)
    room = 512
    pols = [(rand_segs(2, rng), 0, 0, 0), (rand_segs(4, rng), 1, 0, 0), (rand_segs(1, rng), 0, 0, 0)]
    rows = []
    for slack in (1, 0):  # T - grow
        rows.append((frame(rng, 17, room - 54 - 40 - slack), R.OP_ENCAP, 0))            # grow 40
        rows.append((frame(rng, 6, room - 54 - 40 - 32 - slack, srh=2), R.OP_SET, 1))   # grow 32
    rows.append((frame(rng, 17, room - 54 - 56, srh=3), R.OP_SET, 2))  # shrink at T = 0
    rows.append((frame(rng, 17, room - 54 - 40, srh=2), R.OP_SET, 0))  # equal counts at T = 0
    rows.append((frame(rng, 17, room - 54 - 24, srh=1), R.OP_DECAP, 0))
    rows.append((frame(rng, 17, room - 54 - 24, srh=1, sl=1), R.OP_END, 0))
    fr, op, pi = zip(*rows)
    return case(fr, op, pi, pols, room=room)


def arena_end(spare):
    """The last frame ends `spare` bytes before the out arena's end
    (spare = -1: one byte past it, NOT_RESIZED), for each op."""
    rng = np.random.default_rng(7)
    pols = [(rand_segs(2, rng), 1, 0, R.P_SET_DST)]
    out = []
    for o, srh in ((R.OP_ENCAP, None), (R.OP_SET, 1), (R.OP_END, 2), (R.OP_DECAP, 2), (R.OP_NONE, None)):
        fr = [frame(rng, 17, 50, srh=srh) for _ in range(3)]
        c = case(fr, [o] * 3, [0] * 3, pols, out_base=7)
        out.append(c._replace(out_size=int(c.out_off[2]) + out_len(fr[2], o, pols[0]) + spare))
    return out


def truncated(op):
    """An SRH frame (2 segments, VLAN'd) cut at every length below its L4."""
    rng = np.random.default_rng(8)
    pols = [(rand_segs(1, rng), 0, 0, 0)]
    f = frame(rng, 17, 8, vlan=1, srh=2)
    fr = [f[:k] for k in range(0, 58 + 8 + 32 + 1)]
    return case(fr, [op] * len(fr), [0] * len(fr), pols, in_gap=0, out_gap=0)


def final_from_packet():
    """Valid checksums in, CGSR_P_FINAL_FROM_PACKET: ENCAP and SET keep the
    stored L4 checksum (the pseudo-header does not change)."""
    rng = np.random.default_rng(9)
    pols = [(rand_segs(3, rng), 2, 5, R.P_FINAL_FROM_PACKET | R.P_SET_DST),
            (rand_segs(1, rng), 0, 5, R.P_FINAL_FROM_PACKET)]
    fr, op, pi = [], [], []
    for l4, body in ((17, 60), (6, 333), (58, 12)):
        for srh in (None, 2):
            f = R.reconcile(frame(rng, l4, body, srh=srh), ALL)
            for p in (0, 1):
                fr.append(f), op.append(R.OP_ENCAP if srh is None else R.OP_SET), pi.append(p)
    return case(fr, op, pi, pols)


def big_policy(n_pkts):
    """n_pkts packets (1, 63, 64, 65: partial and whole workgroups) under
    n = 127 at room 65536."""
    rng = np.random.default_rng(10 + n_pkts)
    pols = [(rand_segs(127, rng), 126, 0, R.P_SET_DST), (rand_segs(2, rng), 0, 0, 0)]
    fr = [frame(rng, (17, 6, 58)[i % 3], 8 + (i * 37) % 300, vlan=i % 3) for i in range(n_pkts)]
    return case(fr, [R.OP_ENCAP] * n_pkts, [0 if i % 8 == 0 else 1 for i in range(n_pkts)], pols,
                room=65536)
