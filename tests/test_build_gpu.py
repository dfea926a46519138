"""cgtx_build_batch on the device against tests/pyref_build.py, bit for bit:
frames, len and status; every byte the call must not write is compared
against a 0xA5 canary fill of the out arena."""
import numpy as np
import pytest
import torch

import pyref_build as B
from build_cases import CHAINS, HDR, REC, make_records, zero_checksum_record
from capsule_amd import _native as N
from capsule_amd import batch, packets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


GUARD = 64  # bytes kept around an arena that is a slice of a larger tensor


def sliced(size, base, fill, data=None):
    """A device tensor of `size` bytes that starts `base` bytes above a 16-B
    boundary, as a slice of a larger one filled with `fill` -> (whole, slice)."""
    whole = torch.full((GUARD + 16 + size + GUARD,), fill, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 16 == 0 and 0 <= base < 16
    part = whole[GUARD + base : GUARD + base + size]
    if data is not None:
        part.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.uint8)))
    assert part.data_ptr() % 16 == base and part.is_contiguous()
    return whole, part


def run(ctx, recs, out_off, out_size, pay=None, room=2048, out_base=None, pay_base=None, want=None):
    """One build call over a canary-filled arena -> (arena, len, status) as
    numpy, and the same from pyref_build.  With out_base / pay_base (0..15)
    that arena is a slice of a larger tensor and starts so many bytes above
    a 16-B boundary: the out tensor is 0xA5 all over, and has to be outside
    the slice afterwards too; the payload tensor is 0x3C around the slice,
    which pyref_build, given the slice alone, never sees."""
    n = len(recs)
    rt = torch.from_numpy(recs.view(np.uint8).reshape(n, 96).copy()).to(DEV)
    if out_base is None:
        whole = arena = torch.full((out_size,), 0xA5, dtype=torch.uint8, device=DEV)
    else:
        whole, arena = sliced(out_size, out_base, 0xA5)
    off = torch.from_numpy(np.asarray(out_off, np.uint32).view(np.int32)).to(DEV)
    pb = None
    if pay is not None and pay_base is None:
        pb = packets.PacketBatch.from_numpy(*pay, DEV)
    elif pay is not None:
        pb = packets.PacketBatch.from_numpy(np.zeros(0, np.uint8), pay[1], pay[2], DEV)
        pb = packets.PacketBatch(sliced(len(pay[0]), pay_base, 0x3C, pay[0])[1], pb.off, pb.len)
    ob, st = packets.build(ctx, rt, payload=pb, out_arena=arena, out_off=off, room=room)
    torch.cuda.synchronize()
    got = (arena.cpu().numpy(), ob.len.cpu().numpy().view(np.uint16), st.cpu().numpy())
    if out_base is not None:
        lo = GUARD + out_base
        outside = torch.cat((whole[:lo], whole[lo + out_size :])).cpu().numpy()
        bad = np.nonzero(outside != 0xA5)[0]
        assert bad.size == 0, ("bytes written outside the out arena", out_base, bad[:16] - lo)
    if want is None:  # else: what an earlier run of the same inputs returned
        want = B.build_batch(recs, out_off, out_size, *(pay if pay is not None else (None, None, None)),
                             room=room)
    return got, want


def check(got, want):
    assert (got[2] == want[2]).all(), ("status", np.nonzero(got[2] != want[2])[0][:8], got[2][:8], want[2][:8])
    assert (got[1] == want[1]).all(), ("len", np.nonzero(got[1] != want[1])[0][:8])
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, ("arena bytes", bad[:16], got[0][bad[:16]], want[0][bad[:16]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_all_chains_one_burst(ctx, n):
    """All six chains in one burst, frames packed back to back at whatever
    byte each one ends on (gaps of 0-3 bytes), payloads of 0-300 bytes at
    any source alignment."""
    rng = np.random.default_rng(n)
    chains = [CHAINS[(i + i // 6) % 6] for i in range(n)]
    recs = make_records(chains, rng)
    plen = rng.integers(0, 301, n)
    plen = np.where([c[1] in (1, 58) for c in chains], np.maximum(plen, 4), plen).astype(np.uint16)
    poff = (np.cumsum(plen + rng.integers(0, 5, n)) - plen).astype(np.uint32) + 3
    parena = rng.integers(0, 256, int(poff[-1]) + int(plen[-1]) + 7, dtype=np.uint8)
    flen = np.array([HDR[c] for c in chains]) + plen
    off = (np.cumsum(flen + rng.integers(0, 4, n)) - flen).astype(np.uint32) + 5
    got, want = run(ctx, recs, off, int(off[-1] + flen[-1]) + 9, (parena, poff, plen))
    assert (want[2] == B.OK).all() and (want[1] == flen).all()
    check(got, want)


@pytest.mark.parametrize("plen", [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129,
                                  1446, 1447])
def test_payload_lengths_at_every_alignment(ctx, plen):
    """One 256-packet burst per length: packet i reads its payload at source
    alignment i % 16 and writes its frame at destination alignment i // 16;
    random, all-0xFF and all-0x00 payload bytes (checksum folds carry, the
    UDP 0 -> 0xFFFF rule).  The last packet is built to have a zero UDP
    checksum, and the rule is asserted to have fired.  (ICMP chains with
    plen < 4 are BAD_RECORD, which pyref_build agrees on.)"""
    n = 257
    rng = np.random.default_rng(1000 + plen)
    chains = [CHAINS[(i * 7 + i // 16) % 6] for i in range(n - 1)] + [(4, 17)]
    recs = make_records(chains, rng)
    recs[-1:] = zero_checksum_record()
    pl = np.full(n, plen, np.uint16)
    pl[-1] = 0
    pslot = (plen + 16 + 63) // 64 * 64
    poff = (np.arange(n) * pslot + (np.arange(n) % 16)).astype(np.uint32)
    slot = (74 + plen + 16 + 63) // 64 * 64
    off = (np.arange(n) * slot + (np.arange(n) // 16) % 16).astype(np.uint32)
    for fill in ("random", 0xFF, 0x00):
        parena = (rng.integers(0, 256, n * pslot, dtype=np.uint8) if fill == "random"
                  else np.full(n * pslot, fill, np.uint8))
        got, want = run(ctx, recs, off, n * slot, (parena, poff, pl))
        built = want[2] == B.OK
        assert built[-1] and built.sum() >= n - 100
        check(got, want)
        o = int(off[-1])
        assert got[0][o + 40] == 0xFF and got[0][o + 41] == 0xFF  # stored as 0xFFFF


def test_statuses_in_a_mixed_burst(ctx):
    """Every per-packet status, each between packets that are built."""
    room = 200
    rng = np.random.default_rng(5)
    cases = [  # (chain, plen, what)
        ((4, 17), 10, "ok"),
        ((4, 17), room - 1 - 42, "ok"),        # frame_len == room - 1: built
        ((4, 17), room - 42, "room"),           # == room
        ((6, 6), 300, "room"),                  # > room
        ((4, 6), 20, "ok"),
        ((4, 17), 16, "pay"),                   # payload one byte past its arena
        ((6, 17), 33, "ok"),
        ((5, 17), 8, "rec"),                    # version
        ((4, 2), 8, "rec"),                     # protocol
        ((4, 58), 8, "rec"),                    # ICMPv6 under IPv4
        ((6, 1), 8, "rec"),
        ((4, 6), 5, "ok"),
        ((4, 1), 8, "type4"),                   # ICMPv4 type 3
        ((6, 58), 8, "type6"),                  # ICMPv6 type 8
        ((4, 1), 0, "rec"),                     # ICMP body 0 bytes
        ((6, 58), 3, "rec"),                    # ICMP body 3 bytes
        ((6, 58), 4, "ok"),
        ((4, 17), 30, "short"),                 # out arena one byte short
        ((4, 17), 30, "fits"),                  # ... and exactly long enough
    ]
    n = len(cases)
    recs = make_records([c[0] if c[0] in CHAINS else (4, 17) for c in cases], rng)
    for i, (c, _, what) in enumerate(cases):
        recs["version"][i], recs["protocol"][i] = c
        if what == "type4":
            recs["src_port"][i] = 3
        if what == "type6":
            recs["src_port"][i] = 8
    plen = np.array([c[1] for c in cases], np.uint16)
    poff = (np.arange(n) * 320 + 1).astype(np.uint32)
    pay_size = n * 320
    parena = rng.integers(0, 256, pay_size, dtype=np.uint8)
    poff[5] = pay_size - 16 + 1
    off = (np.arange(n) * 512 + np.arange(n) % 4).astype(np.uint32)
    out_size = n * 512
    off[-2] = out_size - 71  # a 72-byte frame would end one byte past the arena
    off[-1] = out_size - 72  # ... and this one ends on its last byte (the short one writes nothing)
    got, want = run(ctx, recs, off, out_size, (parena, poff, plen), room=room)
    expect = {"ok": B.OK, "fits": B.OK, "room": B.NO_ROOM, "short": B.NO_ROOM, "pay": B.BAD_PAYLOAD,
              "rec": B.BAD_RECORD, "type4": B.BAD_RECORD, "type6": B.BAD_RECORD}
    assert [int(s) for s in want[2]] == [expect[c[2]] for c in cases]
    assert want[1][1] == room - 1
    check(got, want)
    assert (got[1][want[2] != B.OK] == 0).all()


def test_device_parse_of_built_frames(ctx):
    """Round trip on the device: parse of the built frames gives OK, both
    checksum bits and the records' set fields."""
    rng = np.random.default_rng(9)
    n = 192
    chains = [CHAINS[i % 6] for i in range(n)]
    recs = make_records(chains, rng)
    recs["data_offset"] = 5
    plen = (rng.integers(4, 400, n)).astype(np.uint16)
    poff = (np.arange(n) * 400).astype(np.uint32)
    parena = rng.integers(0, 256, n * 400, dtype=np.uint8)
    rt = torch.from_numpy(recs.view(np.uint8).reshape(n, 96).copy()).to(DEV)
    ob, st = packets.build(ctx, rt, payload=packets.PacketBatch.from_numpy(parena, poff, plen, DEV), slot=512)
    flags = N.F_ACCEPT_ALL | N.F_ACCEPT_ICMP | N.F_CSUM_IP | N.F_CSUM_L4
    r = packets.parse(ctx, ob, flags, fields=True)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    meta = r.meta.cpu().numpy().view(np.uint32)
    got = r.fields_numpy()
    v4 = recs["version"] == 4
    assert ((meta & 0xFF) == 0).all()
    assert (meta & N.META_L4_CSUM_OK).all() and (meta[v4] & N.META_IP_CSUM_OK).all()
    common = ("dst_mac", "src_mac", "version", "dscp", "ecn", "ttl", "protocol", "src_port")
    tcp = recs["protocol"] == 6
    icmp = (recs["protocol"] == 1) | (recs["protocol"] == 58)
    for name in common:
        assert (got[name] == recs[name]).all(), name
    for name in ("identification", "ip_flags", "fragment_offset"):
        assert (got[name][v4] == recs[name][v4]).all(), name
    assert (got["src_ip"][v4, :4] == recs["src_ip"][v4, :4]).all()
    assert (got["dst_ip"][~v4] == recs["dst_ip"][~v4]).all()
    assert (got["flow_label"][~v4] == recs["flow_label"][~v4]).all()
    assert (got["dst_port"][~icmp] == recs["dst_port"][~icmp]).all()
    assert (got["dst_port"][icmp] == recs["dst_port"][icmp] & 0xFF).all()
    for name in ("seq_no", "ack_no", "data_offset", "ns", "tcp_flags", "udp_length_or_window",
                 "urgent_pointer"):
        assert (got[name][tcp] == recs[name][tcp]).all(), name
    flen = np.array([HDR[c] for c in chains]) + plen
    assert (ob.len.cpu().numpy().view(np.uint16) == flen).all()
    assert (got["ip_length"] == np.where(v4, flen - 14, flen - 54)).all()


def syn_flood_reference(src_mac, first_ip, n):
    recs = np.zeros(n, REC)
    recs["version"], recs["ihl"], recs["ttl"], recs["protocol"], recs["data_offset"] = 4, 5, 64, 6, 5
    recs["src_mac"] = list(src_mac)
    recs["dst_mac"] = [0x02, 0x00, 0x00, 0xFF, 0xFF, 0xFF]
    recs["dst_ip"][:, :4] = [10, 100, 1, 255]
    ip = first_ip + 1 + np.arange(n, dtype=np.uint64)
    for b in range(4):
        recs["src_ip"][:, b] = (ip >> (8 * (3 - b))) & 0xFF
    recs["tcp_flags"], recs["seq_no"], recs["udp_length_or_window"], recs["dst_port"] = 2, 1, 10, 80
    return [B.build_frame(r)[1] for r in recs]


def test_syn_flood_bursts(ctx):
    """Two consecutive bursts of 128 through PollFn equal the map closure of
    examples/syn-flood/main.rs:49-69, next_ip carried over (10.0.0.1 ..
    10.0.0.128, then 10.0.0.129 .. 10.0.1.0)."""
    mac = bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55])
    src = batch.PollFn(ctx, batch.syn_flood(ctx, 128, src_mac=mac, device=DEV), device=DEV)
    for k in range(2):
        src.replenish()
        b = src.next_burst()
        torch.cuda.synchronize()
        want = syn_flood_reference(mac, (10 << 24) + 128 * k, 128)
        assert b.n == 128
        assert (b.batch.len.cpu().numpy() == 54).all()
        for i in (0, 1, 63, 126, 127):
            assert b.batch.frame(i) == want[i], (k, i)
        arena = b.batch.arena.cpu().numpy().reshape(128, -1)[:, :54]
        assert arena.tobytes() == b"".join(want)
    assert want[127][26:30] == bytes([10, 0, 1, 0])


def test_echo_reply_pipeline(ctx):
    """ping4d: Poll -> parse -> replace(echo_reply_v4) -> send on a Channel."""
    rng = np.random.default_rng(3)

    def request(data_len, mtype=8):
        r = make_records([(4, 1)], rng)
        r["src_port"], r["dst_port"] = mtype, 0
        st, f = B.build_frame(r[0], bytes(rng.integers(0, 256, 4 + data_len, dtype=np.uint8)))
        assert st == B.OK
        return f

    udp = B.build_frame(make_records([(4, 17)], rng)[0], b"payload")[1]
    frames = [request(0), request(1), udp, request(56), request(0, mtype=0), request(1400),
              request(0)[:38], request(0)[:41]]
    kinds = ["ok", "ok", "udp", "ok", "reply", "ok", "body0", "body3"]

    def reply(f):
        r = np.zeros(1, REC)
        r["version"], r["ihl"], r["protocol"], r["ttl"] = 4, 5, 1, 255
        r["dst_mac"], r["src_mac"] = list(f[6:12]), list(f[0:6])
        r["src_ip"][0, :4], r["dst_ip"][0, :4] = list(f[30:34]), list(f[26:30])
        st, g = B.build_frame(r[0], f[38:])
        assert st == B.OK
        return g

    rx, tx = batch.Channel(), batch.Channel()
    rx.transmit(frames)
    pipe = (batch.Poll(ctx, rx, device=DEV)
            .parse(N.F_ACCEPT_V4 | N.F_ACCEPT_ICMP, fields=True)
            .replace(batch.echo_reply_v4(ctx))
            .send(tx))
    pipe.replenish()
    b = pipe.next_burst()
    torch.cuda.synchronize()
    want_disp, want_st, want_frames = [], [], []
    for f, kind in zip(frames, kinds):
        if kind == "ok":
            want_disp += [batch.ACT, batch.DROP]
            want_st += [0, 0]
            want_frames.append(reply(f))
        else:
            want_disp.append(batch.ABORT)
            want_st.append(N.PKT[{"udp": "NOT_ICMPV4", "reply": "NOT_ICMPV4", "body0": "L4_BAD_OFFSET",
                                  "body3": "L4_OUT_OF_BUFFER"}[kind]])
    assert b.dispositions() == want_disp
    assert b.status.cpu().tolist() == want_st
    assert (pipe.transmitted, pipe.dropped, pipe.aborted) == (4, 4, 4)
    sent = tx.receive()
    assert sent.n == 4
    for i, g in enumerate(want_frames):
        assert sent.frame(i) == g, i
    # the originals are still there, as Drop
    j = 0
    for f, kind in zip(frames, kinds):
        j += 1 if kind == "ok" else 0
        assert b.batch.frame(j) == f
        j += 1


def test_context_error_word_is_clear(ctx):
    ctx.check()
