"""Independent restatement of the SRv6 edits on `bytes`, written from the
reference's sources (no library call, no oracle call; test-side only).

  Mbuf::extend / shrink     core/src/dpdk/mbuf.rs:225-247, 256-275
  read_data / _slice        mbuf.rs:313-327, 365-380 (BadOffset / OutOfBuffer)
  Ethernet::try_parse       packets/ethernet.rs:164-192, 279-300 (VLAN aware)
  Ipv6::try_parse, set_dst  packets/ip/v6/mod.rs:274-289, 331-334 (reconcile)
  SegmentRouting            packets/ip/v6/srh.rs: try_parse :299-327, try_push
                            :342-370, set_segments :210-233, remove :384-391,
                            header defaults :509-522, dst() = segments[0] :456-470
  Udp / Tcp / Icmpv6        udp.rs:350-354 (0 -> 0xFFFF :132-141), tcp.rs:619-621,
                            icmp/v6/mod.rs:260-262
  checksum                  packets/checksum.rs:53-77, 145-168

A policy is (segments: list of 16-byte strings, segments_left, tag, flags).
"""
import numpy as np

# enum cgpu_pkt_status values used here, and enum cgsr_status
OK, ETH_BAD_OFFSET, ETH_OUT_OF_BUFFER, NOT_IPV6 = 0, 1, 2, 4
L3_BAD_OFFSET, L3_OUT_OF_BUFFER, NOT_RESIZED = 6, 7, 13
EXT_BAD_OFFSET, EXT_OUT_OF_BUFFER, SRH_INCONSISTENT = 17, 18, 19
BAD_OP, BAD_POLICY, NOT_ROUTING, NO_SEGMENTS_LEFT, BAD_SEGMENTS_LEFT = 64, 65, 66, 67, 68

OP_NONE, OP_ENCAP, OP_SET, OP_END, OP_DECAP = 0, 1, 2, 3, 4
P_SET_DST, P_FINAL_FROM_PACKET = 1, 2
ACCEPT_UDP, ACCEPT_TCP, ACCEPT_ICMP = 1 << 2, 1 << 3, 1 << 7


class Failed(Exception):
    def __init__(self, status):
        self.status = status


def read_data(data_len, offset, size, bad_offset, out_of_buffer):
    """mbuf.rs:313-327: offset < data_len, then offset + size <= data_len."""
    if not offset < data_len:
        raise Failed(bad_offset)
    if not offset + size <= data_len:
        raise Failed(out_of_buffer)


class Mbuf:
    """A single-segment mbuf with `room` bytes of data room."""

    def __init__(self, data, room):
        self.data = bytearray(data)
        self.room = room

    def tailroom(self):
        return self.room - len(self.data)

    def extend(self, offset, n):
        if not n > 0 or not offset <= len(self.data) or not n < self.tailroom():
            raise Failed(NOT_RESIZED)
        self.data[offset:offset] = bytes(n)

    def shrink(self, offset, n):
        if not n > 0 or not offset + n <= len(self.data):
            raise Failed(NOT_RESIZED)
        del self.data[offset:offset + n]

    def resize(self, offset, n):
        if n < 0:
            self.shrink(offset, -n)
        else:
            self.extend(offset, n)


def parse_eth_ipv6(f):
    """parse::<Ethernet>().parse::<Ipv6>() -> eth_len."""
    n = len(f)
    read_data(n, 0, 14, ETH_BAD_OFFSET, ETH_OUT_OF_BUFFER)
    marker = (f[12] << 8) | f[13]
    eth = 18 if marker == 0x8100 else 22 if marker == 0x88A8 else 14
    if not n >= eth:
        raise Failed(ETH_OUT_OF_BUFFER)
    if (f[eth - 2] << 8) | f[eth - 1] != 0x86DD:
        raise Failed(NOT_IPV6)
    read_data(n, eth, 40, L3_BAD_OFFSET, L3_OUT_OF_BUFFER)
    return eth


def parse_srh(f, eth):
    """parse::<SegmentRouting<Ipv6>>() -> the number of segments."""
    x = eth + 40
    if f[eth + 6] != 43:
        raise Failed(NOT_ROUTING)
    read_data(len(f), x, 8, EXT_BAD_OFFSET, EXT_OUT_OF_BUFFER)
    hdr_ext_len, nseg = f[x + 1], f[x + 4] + 1
    if not (hdr_ext_len != 0 and 2 * nseg == hdr_ext_len):
        raise Failed(SRH_INCONSISTENT)
    read_data(len(f), x + 8, 16 * nseg, EXT_BAD_OFFSET, EXT_OUT_OF_BUFFER)
    return nseg


def bad_policy(pol):
    if pol is None:
        return True
    segs, sl, _tag, fl = pol
    return not 1 <= len(segs) <= 127 or bool(fl & P_SET_DST and sl >= len(segs))


def splice(frame, op, pol=None, room=2048):
    """The edit without reconcile_all -> frame bytes; raises Failed(status)."""
    if op == OP_NONE:
        return bytes(frame)
    if not 0 <= op <= 4:
        raise Failed(BAD_OP)
    eth = parse_eth_ipv6(frame)
    x = eth + 40
    old_n = parse_srh(frame, eth) if op in (OP_SET, OP_END, OP_DECAP) else 0
    if op in (OP_ENCAP, OP_SET) and bad_policy(pol):
        raise Failed(BAD_POLICY)
    m = Mbuf(frame, room)
    d = m.data
    if op in (OP_ENCAP, OP_SET):
        segs, sl, tag, fl = pol
        segs = list(segs)
        if op == OP_ENCAP:
            if fl & P_FINAL_FROM_PACKET:
                segs[0] = bytes(d[eth + 24:eth + 40])
            m.extend(x, 24)  # a default list of one (srh.rs:347-355)
            d[x:x + 8] = bytes([d[eth + 6], 2, 4, 0, 0, 0, 0, 0])
            d[eth + 6] = 43
            old_n = 1
        elif fl & P_FINAL_FROM_PACKET:
            segs[0] = bytes(d[x + 8:x + 24])
        if len(segs) != old_n:  # set_segments (srh.rs:210-233)
            m.resize(x + 8, 16 * (len(segs) - old_n))
        d[x + 8:x + 8 + 16 * len(segs)] = b"".join(segs)
        d[x + 1] = 2 * len(segs)
        d[x + 4] = len(segs) - 1
        d[x + 3] = sl
        d[x + 6:x + 8] = bytes([tag >> 8, tag & 0xFF])
        if fl & P_SET_DST:
            d[eth + 24:eth + 40] = segs[sl]
    elif op == OP_DECAP:  # remove (srh.rs:384-391)
        nh = d[x]
        m.shrink(x, 8 + 16 * old_n)
        d[eth + 6] = nh
    return m


def end_checks(m_or_bytes, eth):
    d = m_or_bytes
    x = eth + 40
    sl = d[x + 3]
    if sl == 0:
        raise Failed(NO_SEGMENTS_LEFT)
    if sl - 1 > d[x + 4]:
        raise Failed(BAD_SEGMENTS_LEFT)
    d[x + 3] = sl - 1
    d[eth + 24:eth + 40] = d[x + 8 + 16 * (sl - 1):x + 24 + 16 * (sl - 1)]


def fold(s):
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def l4_checksum(src, dst, proto, data):
    """compute(pseudo.sum(), data) with the checksum field already zero."""
    s = proto + (len(data) & 0xFFFF)
    for a in (src, dst):
        for i in range(0, 16, 2):
            s += (a[i] << 8) | a[i + 1]
    s = fold(s)
    n = len(data)
    if n % 2:
        s += data[n - 1] << 8
    for i in range(0, n - n % 2, 2):
        s += (data[i] << 8) | data[i + 1]
    return ~fold(s) & 0xFFFF


def reconcile(frame, accept):
    """reconcile_all() from the deepest layer the one-extension-level parse
    of `frame` (Ethernet, Ipv6 known good) reaches under `accept`."""
    if accept & (ACCEPT_UDP | ACCEPT_TCP | ACCEPT_ICMP) == 0:
        accept |= ACCEPT_UDP | ACCEPT_TCP
    f = bytearray(frame)
    eth = parse_eth_ipv6(f)
    x, n = eth + 40, len(f)
    proto, l4o, dst = f[eth + 6], x, bytes(f[eth + 24:eth + 40])
    try:
        if proto == 43:
            nseg = parse_srh(f, eth)
            dst = bytes(f[x + 8:x + 24])
            proto, l4o = f[x], x + 8 + 16 * nseg
        elif proto == 44:
            read_data(n, x, 8, EXT_BAD_OFFSET, EXT_OUT_OF_BUFFER)
            proto, l4o = f[x], x + 8
        kind = None
        if proto == 17 and accept & ACCEPT_UDP:
            kind, hl, cs = "udp", 8, 6
        elif proto == 6 and accept & ACCEPT_TCP:
            kind, hl, cs = "tcp", 20, 16
        elif proto == 58 and accept & ACCEPT_ICMP:
            kind, hl, cs = "icmp", 4, 2
        if kind is not None:
            read_data(n, l4o, hl, 11, 12)
    except Failed:
        kind = None
    if kind is not None:
        span = n - l4o
        if kind == "udp":
            f[l4o + 4:l4o + 6] = bytes([(span >> 8) & 0xFF, span & 0xFF])
        f[l4o + cs:l4o + cs + 2] = b"\0\0"
        ck = l4_checksum(bytes(f[eth + 8:eth + 24]), dst, proto, f[l4o:])
        if kind == "udp" and ck == 0:
            ck = 0xFFFF
        f[l4o + cs:l4o + cs + 2] = bytes([ck >> 8, ck & 0xFF])
    pl = (n - x) & 0xFFFF
    f[eth + 4:eth + 6] = bytes([pl >> 8, pl & 0xFF])
    return bytes(f)


def spliced(frame, op, pol=None, room=2048):
    """(status, the frame after the edit and before reconcile_all, or None)."""
    try:
        m = splice(frame, op, pol, room)
        if op == OP_NONE:
            return OK, m
        if op == OP_END:
            end_checks(m.data, parse_eth_ipv6(frame))
        return OK, bytes(m.data)
    except Failed as e:
        return e.status, None


def apply(frame, op, pol=None, accept=0, room=2048, out_room=None):
    """(status, output frame or None).  out_room: bytes left in the out arena
    from the frame's slot on (a frame past it is NOT_RESIZED, which comes
    before END's own errors)."""
    try:
        m = splice(frame, op, pol, room)
        new_len = len(m) if op == OP_NONE else len(m.data)
        if out_room is not None and new_len > out_room:
            raise Failed(NOT_RESIZED)
        if op == OP_NONE:
            return OK, m
        if op == OP_END:
            end_checks(m.data, parse_eth_ipv6(frame))
        return OK, reconcile(m.data, accept)
    except Failed as e:
        return e.status, None


def apply_batch(frames, op, policy_idx, policies, out_off, out_arena_len, accept=0, room=2048,
                fill=0xA5):
    """The whole call -> (out arena with `fill` where nothing is written,
    len u16 [n], status u8 [n], frames list)."""
    n = len(frames)
    arena = np.full(out_arena_len, fill, np.uint8)
    ln = np.zeros(n, np.uint16)
    st = np.zeros(n, np.uint8)
    outs = [None] * n
    for i in range(n):
        pol = None
        if policy_idx is not None and 0 <= int(policy_idx[i]) < len(policies):
            pol = policies[int(policy_idx[i])]
        o = int(out_off[i])
        s, f = apply(frames[i], int(op[i]), pol, accept, room, out_arena_len - o)
        st[i] = s
        if f is not None:
            arena[o:o + len(f)] = np.frombuffer(f, np.uint8)
            ln[i] = len(f)
            outs[i] = f
    return arena, ln, st, outs
