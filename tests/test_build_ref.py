"""tests/pyref_build.py (the independent restatement of push + setters +
reconcile_all) against what is already pinned: the reference's own packet
fixtures, the CPU oracle's parse, and the values the reference's unit tests
assert.  No GPU.

No reference test holds the bytes of a pushed packet, so parity of
construction rests on the Default impls, the reconcile rules the oracle
already pins, this round trip and the second restatement."""
import json
import pathlib

import numpy as np
import pytest

import oracle_lib
import pyref_build as B
from capsule_amd import _native as N

ROOT = pathlib.Path(__file__).resolve().parents[1]
REC = np.dtype(N.HDR_RECORD_FIELDS)
GOLD = json.loads((ROOT / "tests" / "golden" / "reference_packets.json").read_text())
FLAGS = N.F_ACCEPT_ALL | N.F_ACCEPT_ICMP | N.F_CSUM_IP | N.F_CSUM_L4
FIXTURES = ("IPV4_UDP_PACKET", "IPV4_TCP_PACKET", "IPV6_TCP_PACKET", "ICMPV4_PACKET")


def parse(frames):
    from capsule_amd import synth

    arena, off, ln = synth.pack_frames(frames, 64)
    meta, csum, _, fl = oracle_lib.parse_batch(arena, off, ln, FLAGS, fields=True)
    return meta, csum, fl.view(REC).reshape(-1)


def qualifies(frame, meta, csum, rec):
    """No VLAN tag, no extension header, IHL 5, stored lengths and checksums
    equal to the reconciled ones."""
    if N.meta_status(meta) != 0 or rec["vlan"] != 0 or (meta >> 24) & 3:
        return False
    if rec["version"] == 4 and rec["ihl"] != 5:
        return False
    l3 = 14
    want_len = len(frame) - l3 - (40 if rec["version"] == 6 else 0)
    if rec["ip_length"] != want_len:
        return False
    if N.meta_l4(meta) == N.L4_UDP and rec["udp_length_or_window"] != len(frame) - l3 - 20 - (20 if rec["version"] == 6 else 0):
        return False
    ok = N.META_L4_CSUM_OK | (N.META_IP_CSUM_OK if rec["version"] == 4 else 0)
    return (meta & ok) == ok


def test_fixture_round_trip():
    """parse (oracle, with fields) -> pyref_build -> the original bytes.  The
    payload is everything behind the fixed L4 header (TCP options included:
    the data_offset nibble is stored as given).  IPV4_UDP_PACKET,
    IPV4_TCP_PACKET and ICMPV4_PACKET qualify.  IPV6_TCP_PACKET does not: its
    stored TCP checksum 0xa92c is the IPv4 fixture's (byte_arrays.rs:155
    reuses that segment), while the checksum over the IPv6 pseudo-header is
    0x1b1c, so its L4 checksum bit is clear; it is rebuilt too and compared
    everywhere but in those two bytes, which must hold 0x1b1c."""
    frames = [bytes.fromhex(GOLD[k]["hex"]) for k in FIXTURES]
    meta, csum, recs = parse(frames)
    done = []
    for k, f, m, c, r in zip(FIXTURES, frames, meta, csum, recs):
        l4o = 14 + (40 if r["version"] == 6 else 20)
        hl = {N.L4_UDP: 8, N.L4_TCP: 20, N.L4_ICMP: 4}[N.meta_l4(int(m))]
        st, g = B.build_frame(r, f[l4o + hl:])
        assert st == B.OK, k
        if not qualifies(f, int(m), int(c), r):
            assert k == "IPV6_TCP_PACKET"
            assert g[:70] == f[:70] and g[72:] == f[72:] and g[70:72] == b"\x1b\x1c"
            continue
        assert g == f, k
        done.append(k)
    assert done == ["IPV4_UDP_PACKET", "IPV4_TCP_PACKET", "ICMPV4_PACKET"]


def records():
    """Every chain with every settable field away from its default."""
    rng = np.random.default_rng(11)
    out = []
    for v, p in ((4, 17), (4, 6), (4, 1), (6, 17), (6, 6), (6, 58)):
        for rep in range(4):
            r = np.zeros(1, REC)
            r["version"], r["protocol"] = v, p
            r["ihl"] = 5 if v == 4 else 0
            r["dst_mac"] = rng.integers(0, 256, 6)
            r["src_mac"] = rng.integers(0, 256, 6)
            r["dscp"], r["ecn"], r["ttl"] = rng.integers(0, 64), rng.integers(0, 4), rng.integers(0, 256)
            r["src_ip"][0, : 4 if v == 4 else 16] = rng.integers(0, 256, 4 if v == 4 else 16)
            r["dst_ip"][0, : 4 if v == 4 else 16] = rng.integers(0, 256, 4 if v == 4 else 16)
            if v == 4:
                r["identification"] = rng.integers(0, 65536)
                r["ip_flags"], r["fragment_offset"] = rng.integers(0, 4), rng.integers(0, 0x2000)
            else:
                r["flow_label"] = rng.integers(0, 1 << 20)
            if p in (17, 6):
                r["src_port"], r["dst_port"] = rng.integers(0, 65536, 2)
            else:
                r["src_port"] = [(8, 0), (128, 129)][v == 6][rep & 1]
                r["dst_port"] = rng.integers(0, 256)
            if p == 6:
                r["seq_no"], r["ack_no"] = rng.integers(0, 1 << 32, 2)
                r["data_offset"], r["ns"], r["tcp_flags"] = 5, rep & 1, rng.integers(0, 256)
                r["udp_length_or_window"], r["urgent_pointer"] = rng.integers(0, 65536, 2)
            n = [0, 1, 33, 1400][rep] + (4 if p in (1, 58) else 0)
            out.append((r[0], bytes(rng.integers(0, 256, n, dtype=np.uint8))))
    return out


SET = {
    "eth": ("dst_mac", "src_mac"),
    4: ("version", "ihl", "dscp", "ecn", "identification", "ip_flags", "fragment_offset", "ttl",
        "protocol", "src_ip", "dst_ip"),
    6: ("version", "dscp", "ecn", "flow_label", "ttl", "protocol", "src_ip", "dst_ip"),
    17: ("src_port", "dst_port"),
    6.5: ("src_port", "dst_port", "seq_no", "ack_no", "data_offset", "ns", "tcp_flags",
          "udp_length_or_window", "urgent_pointer"),
    1: ("src_port", "dst_port"),
}


def test_oracle_parses_what_pyref_builds():
    """The oracle's parse of every pyref_build frame: status OK, both
    checksum bits (the IPv4 one where there is an IPv4 header), the set
    fields unchanged, the derived ones reconciled."""
    cases = records()
    frames = []
    for r, pay in cases:
        st, f = B.build_frame(r, pay)
        assert st == B.OK
        frames.append(f)
    meta, csum, got = parse(frames)
    for (r, pay), f, m, g in zip(cases, frames, meta, got):
        m = int(m)
        v, p = int(r["version"]), int(r["protocol"])
        assert N.meta_status(m) == 0 and N.meta_eth_len(m) == 14
        assert m & N.META_L4_CSUM_OK
        if v == 4:
            assert m & N.META_IP_CSUM_OK
        names = SET["eth"] + SET[v] + SET[{17: 17, 6: 6.5}.get(p, 1)]
        for name in names:
            assert np.array_equal(g[name], r[name]), (v, p, name)
        hl = {17: 8, 6: 20}.get(p, 4)
        l3 = 20 if v == 4 else 40
        assert len(f) == 14 + l3 + hl + len(pay)
        assert g["ether_type"] == (0x0800 if v == 4 else 0x86DD)
        assert g["ip_length"] == (len(f) - 14 if v == 4 else len(f) - 54)
        if p == 17:
            assert g["udp_length_or_window"] == 8 + len(pay)
        assert f[14 + l3 + hl:] == pay


def test_oracle_parses_long_pyref_frames():
    """The same at the lengths the device tests reach: frames of 2047, 9000
    and 65535 bytes (the longest buildable one) of every chain, room 65536."""
    rng = np.random.default_rng(12)
    cases = []
    for r, _ in records()[::4]:
        v, p = int(r["version"]), int(r["protocol"])
        hdr = 14 + (20 if v == 4 else 40) + {17: 8, 6: 20}.get(p, 4)
        for flen in (2047, 9000, 65535):
            cases.append((r, bytes(rng.integers(0, 256, flen - hdr, dtype=np.uint8)), flen))
    assert len(cases) == 18
    frames = []
    for r, pay, flen in cases:
        st, f = B.build_frame(r, pay, room=65536)
        assert st == B.OK and len(f) == flen
        frames.append(f)
    assert B.build_frame(cases[-1][0], cases[-1][1] + b"\0", room=65536)[0] == B.NO_ROOM
    meta, csum, got = parse(frames)
    for (r, pay, flen), f, m, g in zip(cases, frames, meta, got):
        m = int(m)
        v, p = int(r["version"]), int(r["protocol"])
        assert N.meta_status(m) == 0 and N.meta_eth_len(m) == 14
        assert m & N.META_L4_CSUM_OK
        if v == 4:
            assert m & N.META_IP_CSUM_OK
        for name in SET["eth"] + SET[v] + SET[{17: 17, 6: 6.5}.get(p, 1)]:
            assert np.array_equal(g[name], r[name]), (v, p, flen, name)
        assert g["ether_type"] == (0x0800 if v == 4 else 0x86DD)
        assert g["ip_length"] == (flen - 14 if v == 4 else flen - 54)
        if p == 17:
            assert g["udp_length_or_window"] == flen - 14 - (20 if v == 4 else 40)
        assert f[flen - len(pay):] == pay


def test_reference_unit_test_values():
    """echo_reply.rs:231-255 push_and_set_echo_reply: header_len 4, payload
    4 (the body) then 4 + 10 after set_data(&[0; 10]), type EchoReply, code
    0, checksum != 0 after reconcile_all; and the size_of tests
    (ethernet.rs:485, v4.rs:620, v6/mod.rs:475, udp.rs:383, tcp.rs:675,
    icmp/v4/mod.rs:456, echo_reply.rs:227)."""
    r = np.zeros(1, REC)[0]
    r["version"], r["protocol"], r["ttl"] = 4, 1, 64
    st, f = B.build_frame(r, bytes([0, 42, 0, 7]))  # set_identifier(42), set_seq_no(7)
    assert st == B.OK and len(f) - 34 == 4 + 4 and f[34] == 0 and f[35] == 0
    st, f = B.build_frame(r, bytes([0, 42, 0, 7]) + bytes(10))
    assert st == B.OK and len(f) - 34 - 4 == 4 + 10
    assert f[38:42] == bytes([0, 42, 0, 7]) and f[42:] == bytes(10)
    assert f[36:38] != b"\0\0"
    sizes = {(4, 17): 14 + 20 + 8, (4, 6): 14 + 20 + 20, (6, 17): 14 + 40 + 8, (6, 6): 14 + 40 + 20}
    for (v, p), want in sizes.items():
        r = np.zeros(1, REC)[0]
        r["version"], r["protocol"] = v, p
        st, f = B.build_frame(r)
        assert st == B.OK and len(f) == want
    # defaults as pushed: version_ihl 0x45, 6 << 28, offset_to_ns 5 << 4 from the record
    r["data_offset"] = 5
    assert B.build_frame(r)[1][14] == 0x60 and B.build_frame(r)[1][54 + 12] == 0x50


def test_room_and_statuses():
    """Mbuf::extend's len < tailroom: frame_len == room - 1 is built, == room
    is not; an ICMP body under 4 bytes and unknown chains are BAD_RECORD."""
    r = np.zeros(1, REC)[0]
    r["version"], r["protocol"] = 4, 17
    assert B.build_frame(r, bytes(100), room=143)[0] == B.OK
    assert B.build_frame(r, bytes(100), room=142)[0] == B.NO_ROOM
    assert B.build_frame(r, b"", room=43)[0] == B.OK and B.build_frame(r, b"", room=42)[0] == B.NO_ROOM
    for v, p, t in ((4, 1, 3), (6, 58, 8), (4, 58, 8), (6, 1, 128), (7, 17, 0), (4, 2, 0)):
        r["version"], r["protocol"], r["src_port"] = v, p, t
        assert B.build_frame(r, bytes(8))[0] == B.BAD_RECORD
    r["version"], r["protocol"], r["src_port"] = 4, 1, 8
    assert B.build_frame(r, bytes(3))[0] == B.BAD_RECORD and B.build_frame(r, bytes(4))[0] == B.OK


def test_udp_zero_checksum_is_stored_as_ffff():
    """A packet whose computed UDP checksum is 0: found by solving for the
    source port, and the rule fires."""
    r = np.zeros(1, REC)[0]
    r["version"], r["protocol"] = 4, 17
    r["src_port"] = 0
    st, f = B.build_frame(r, b"")
    ck = (f[40] << 8) | f[41]
    r["src_port"] = ck  # the sum rises by ck: the complement becomes 0
    st, f = B.build_frame(r, b"")
    assert f[40:42] == b"\xff\xff"
    meta, _, _ = parse([f])
    assert int(meta[0]) & N.META_L4_CSUM_OK
