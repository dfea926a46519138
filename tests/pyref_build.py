"""Independent restatement of packet construction: Mbuf::new, push, the
setters and reconcile_all, written from the reference's sources (no library
call, no oracle call; test-side only).

  Mbuf::extend           core/src/dpdk/mbuf.rs:225-247 (len > 0, offset <= data_len, len < tailroom)
  Ethernet::try_push     packets/ethernet.rs:308-325 (14 bytes)
  Ipv4 / Ipv6 push       packets/ip/v4.rs:455-470, ip/v6/mod.rs:302-317; Default impls
                         v4.rs:594-608, v6/mod.rs:453-462, DEFAULT_IP_TTL ip/mod.rs:33
  Udp / Tcp push         packets/udp.rs:318-333, tcp.rs:589-604; TcpHeader::default tcp.rs:648-661
  echo messages          packets/icmp/v4/echo_reply.rs:197-205, icmp/v4/mod.rs:228 (a generic
                         ICMP header cannot be pushed), icmp/v6/echo_*.rs
  reconcile              v4.rs:486-489, v6/mod.rs:331-334, udp.rs:350-354 (0 -> 0xFFFF :132-141),
                         tcp.rs:619-621, icmp/v4/mod.rs:246 (no pseudo-header), icmp/v6/mod.rs:260
  checksum               packets/checksum.rs:72-77, 93-128, 145-168

A record is a numpy record of the cgpu_hdr_record dtype; which of its fields
are taken and which derived is the contract of include/capsule_gpu_tx.h.
"""
import numpy as np

OK, BAD_RECORD, NO_ROOM, BAD_PAYLOAD = 0, 1, 2, 3


class NotResized(Exception):
    pass


class Mbuf:
    """A single-segment mbuf with `room` bytes of data room and data_off 0
    taken off it already (tailroom = room - data_len)."""

    def __init__(self, room):
        self.room = room
        self.data = bytearray()

    def extend(self, offset, n):
        if not n > 0 or not offset <= len(self.data) or not n < self.room - len(self.data):
            raise NotResized()
        self.data[offset:offset] = bytes(n)

    def write(self, offset, b):
        self.data[offset:offset + len(b)] = b


def be16(v):
    return bytes([(v >> 8) & 0xFF, v & 0xFF])


def be32(v):
    return bytes([(v >> 24) & 0xFF, (v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF])


def fold(s):
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def compute(pseudo_sum, data):
    """checksum::compute (checksum.rs:145-168)."""
    s = pseudo_sum
    n = len(data)
    if n % 2:
        s += data[n - 1] << 8
    for i in range(0, n - n % 2, 2):
        s += (data[i] << 8) | data[i + 1]
    return ~fold(s) & 0xFFFF


def pseudo_sum(src, dst, length, proto):
    """PseudoHeader::sum (checksum.rs:53-77): 16-bit words of both addresses,
    the protocol and the packet length, folded."""
    s = proto + length
    for a in (src, dst):
        for i in range(0, len(a), 2):
            s += (a[i] << 8) | a[i + 1]
    return fold(s)


def chain_of(rec):
    """(version, l4 name) or None when the record names no push chain."""
    v, p = int(rec["version"]), int(rec["protocol"])
    if v not in (4, 6):
        return None
    if p == 17:
        return v, "udp"
    if p == 6:
        return v, "tcp"
    if p == (1 if v == 4 else 58):
        t = int(rec["src_port"])
        if t in ((8, 0) if v == 4 else (128, 129)):
            return v, "icmp"
    return None


def build_frame(rec, payload=b"", room=2048):
    """(status, frame bytes or None) for one record."""
    ch = chain_of(rec)
    if ch is None:
        return BAD_RECORD, None
    v, l4 = ch
    if l4 == "icmp" and len(payload) < 4:
        return BAD_RECORD, None
    m = Mbuf(room)
    try:
        # push::<Ethernet>, set_dst, set_src; the Ipv4/Ipv6 push sets ether_type
        m.extend(0, 14)
        m.write(0, bytes(rec["dst_mac"]) + bytes(rec["src_mac"]) + be16(0x0800 if v == 4 else 0x86DD))
        proto = {"udp": 17, "tcp": 6, "icmp": 1 if v == 4 else 58}[l4]
        if v == 4:
            m.extend(14, 20)
            fl = int(rec["ip_flags"])
            ff = (0x4000 if fl & 1 else 0) | (0x2000 if fl & 2 else 0) | (int(rec["fragment_offset"]) & 0x1FFF)
            tos = ((int(rec["dscp"]) << 2) & 0xFF) | (int(rec["ecn"]) & 0x03)
            src, dst = bytes(rec["src_ip"][:4]), bytes(rec["dst_ip"][:4])
            m.write(14, bytes([0x45, tos]) + be16(0) + be16(int(rec["identification"])) + be16(ff) +
                    bytes([int(rec["ttl"]), proto]) + be16(0) + src + dst)
            l4o = 34
        else:
            m.extend(14, 40)
            w = (6 << 28) | ((int(rec["dscp"]) << 22) & 0x0FC00000) | \
                ((int(rec["ecn"]) << 20) & 0x00300000) | (int(rec["flow_label"]) & 0x000FFFFF)
            src, dst = bytes(rec["src_ip"]), bytes(rec["dst_ip"])
            m.write(14, be32(w) + be16(0) + bytes([proto, int(rec["ttl"])]) + src + dst)
            l4o = 54
        if l4 == "udp":
            m.extend(l4o, 8)
            m.write(l4o, be16(int(rec["src_port"])) + be16(int(rec["dst_port"])) + be16(0) + be16(0))
            hl, cs_at = 8, 6
        elif l4 == "tcp":
            m.extend(l4o, 20)
            b12 = ((int(rec["data_offset"]) << 4) & 0xF0) | (int(rec["ns"]) & 0x01)
            m.write(l4o, be16(int(rec["src_port"])) + be16(int(rec["dst_port"])) +
                    be32(int(rec["seq_no"])) + be32(int(rec["ack_no"])) +
                    bytes([b12, int(rec["tcp_flags"])]) + be16(int(rec["udp_length_or_window"])) +
                    be16(0) + be16(int(rec["urgent_pointer"])))
            hl, cs_at = 20, 16
        else:
            # the 4-byte ICMP header, then the message body's fixed part
            # (identifier, seq_no: 4 bytes) in the message's own push
            m.extend(l4o, 4)
            m.write(l4o, bytes([int(rec["src_port"]) & 0xFF, int(rec["dst_port"]) & 0xFF]) + be16(0))
            m.extend(l4o + 4, 4)
            m.write(l4o + 4, payload[:4])
            payload = payload[4:]
            hl, cs_at = 8, 2
        if payload:  # the data behind the headers (set_data's resize + write)
            m.extend(l4o + hl, len(payload))
            m.write(l4o + hl, payload)
    except NotResized:
        return NO_ROOM, None
    # reconcile_all: L4 first, then its envelopes
    f = m.data
    span = len(f) - l4o
    if l4 == "udp":
        f[l4o + 4:l4o + 6] = be16(span)
    f[l4o + cs_at:l4o + cs_at + 2] = b"\0\0"
    ps = 0 if (l4 == "icmp" and v == 4) else pseudo_sum(src, dst, span & 0xFFFF, proto)
    ck = compute(ps, f[l4o:])
    if l4 == "udp" and ck == 0:
        ck = 0xFFFF
    f[l4o + cs_at:l4o + cs_at + 2] = be16(ck)
    if v == 4:
        f[16:18] = be16(len(f) - 14)
        f[24:26] = b"\0\0"
        f[24:26] = be16(compute(0, f[14:34]))
    else:
        f[18:20] = be16(len(f) - 54)
    return OK, bytes(f)


def build_batch(records, out_off, out_arena_len, pay_arena=None, pay_off=None, pay_len=None,
                room=2048, fill=0xA5):
    """The whole call: -> (out arena filled with `fill` where nothing is
    written, len u16 [n], status u8 [n], frames list).  Precedence of the
    per-packet statuses: BAD_RECORD, BAD_PAYLOAD, NO_ROOM."""
    n = len(records)
    arena = np.full(out_arena_len, fill, np.uint8)
    ln = np.zeros(n, np.uint16)
    st = np.zeros(n, np.uint8)
    frames = [None] * n
    for i in range(n):
        po, pl = (int(pay_off[i]), int(pay_len[i])) if pay_arena is not None else (0, 0)
        in_arena = pay_arena is None or po + pl <= len(pay_arena)
        payload = bytes(pay_arena[po:po + pl]) if (pay_arena is not None and in_arena) else b""
        if not in_arena:
            # a record that is bad anyway says so first
            s, f = build_frame(records[i], bytes(pl), room)
            s, f = (BAD_RECORD, None) if s == BAD_RECORD else (BAD_PAYLOAD, None)
        else:
            s, f = build_frame(records[i], payload, room)
        if s == OK and int(out_off[i]) + len(f) > out_arena_len:
            s, f = NO_ROOM, None
        st[i] = s
        if f is not None:
            o = int(out_off[i])
            arena[o:o + len(f)] = np.frombuffer(f, np.uint8)
            ln[i] = len(f)
            frames[i] = f
    return arena, ln, st, frames
