"""Inputs for the build kernel's tests (test_build_gpu.py,
test_build_edges_gpu.py) and the CPU check that they hit what they aim at
(test_build_cases.py).  numpy only: importable without a GPU.

Every generator returns a Case: the tuple (records, pay_arena, pay_off,
pay_len, out_off, out_size, room), with the statuses the case is designed to
have in its .status attribute.

The kernel (capsule_amd/csrc/build.hip) cuts a frame into 16-B chunks of the
out arena's memory; nch(), below, is its chunk count.  Chunks 0..7 are held in
registers, 8..31 are copied by the packet's team of 4 lanes, chunks from 32 on
by the whole wave in steps of 64 chunks (32..95, 96..159, ...)."""
import collections

import numpy as np

import pyref_build as B
from capsule_amd import _native as N

REC = np.dtype(N.HDR_RECORD_FIELDS)
CHAINS = ((4, 17), (4, 6), (4, 1), (6, 17), (6, 6), (6, 58))
HDR = {(4, 17): 42, (4, 6): 54, (4, 1): 38, (6, 17): 62, (6, 6): 74, (6, 58): 58}
ICMP = ((4, 1), (6, 58))
NOT_ICMP = tuple(c for c in CHAINS if c not in ICMP)
WAVE = 16  # packets a wave builds (teams of 4 lanes)


class Case(collections.namedtuple("Case", "records pay_arena pay_off pay_len out_off out_size room")):
    """One build call's inputs; .status holds the designed statuses."""

    def payload(self):
        return None if self.pay_arena is None else (self.pay_arena, self.pay_off, self.pay_len)


def case(recs, parena, poff, plen, off, out_size, room, status):
    c = Case(recs, parena, None if parena is None else np.asarray(poff, np.uint32),
             None if parena is None else np.asarray(plen, np.uint16), np.asarray(off, np.uint32),
             int(out_size), int(room))
    c.status = np.asarray(status, np.uint8)
    return c


def make_records(chains, rng):
    """Records of the given chains with every settable field random."""
    n = len(chains)
    r = np.zeros(n, REC)
    v = np.array([c[0] for c in chains])
    p = np.array([c[1] for c in chains])
    r["version"], r["protocol"] = v, p
    r["ihl"] = np.where(v == 4, 5, 0)
    r["dst_mac"] = rng.integers(0, 256, (n, 6))
    r["src_mac"] = rng.integers(0, 256, (n, 6))
    r["dscp"], r["ecn"], r["ttl"] = rng.integers(0, 64, n), rng.integers(0, 4, n), rng.integers(0, 256, n)
    r["src_ip"] = rng.integers(0, 256, (n, 16))
    r["dst_ip"] = rng.integers(0, 256, (n, 16))
    r["identification"] = rng.integers(0, 65536, n)
    r["ip_flags"], r["fragment_offset"] = rng.integers(0, 4, n), rng.integers(0, 0x2000, n)
    r["flow_label"] = rng.integers(0, 1 << 20, n)
    r["src_port"], r["dst_port"] = rng.integers(0, 65536, n), rng.integers(0, 65536, n)
    icmp = (p == 1) | (p == 58)
    pick = rng.integers(0, 2, n)
    r["src_port"] = np.where(icmp, np.where(v == 4, np.where(pick, 8, 0), np.where(pick, 128, 129)), r["src_port"])
    r["dst_port"] = np.where(icmp, rng.integers(0, 256, n), r["dst_port"])
    r["seq_no"], r["ack_no"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    r["data_offset"], r["ns"], r["tcp_flags"] = rng.integers(0, 16, n), rng.integers(0, 2, n), rng.integers(0, 256, n)
    r["udp_length_or_window"], r["urgent_pointer"] = rng.integers(0, 65536, n), rng.integers(0, 65536, n)
    # what the build must ignore
    r["ether_type"], r["eth_len"], r["vlan"] = rng.integers(0, 65536, n), 18, rng.integers(0, 3, n)
    r["ip_length"], r["ip_checksum"], r["l4_checksum"] = (rng.integers(0, 65536, n) for _ in range(3))
    return r


def zero_checksum_record():
    """An IPv4/UDP record (no payload) whose computed checksum is 0: with
    src_port 0 the checksum is c, so src_port = c raises the sum to 0xFFFF."""
    r = np.zeros(1, REC)
    r["version"], r["protocol"], r["ihl"], r["ttl"] = 4, 17, 5, 64
    c = B.build_frame(r[0])[1][40:42]
    r["src_port"] = (c[0] << 8) | c[1]
    return r


def hdr_len(chains):
    return np.array([HDR[c] for c in chains], np.int64)


def nch(c, ln, out_base=0):
    """The kernel's chunk count of every frame (0: not built), ln being the
    call's len output; out_base: the out arena's address modulo 16."""
    ln = np.asarray(ln, np.int64)
    d = (c.out_off.astype(np.int64) + out_base) & 15
    return np.where(ln > 0, (d + ln + 15) // 16, 0)


def dst_align(c, out_base=0):
    return (c.out_off.astype(np.int64) + out_base) & 15


def src_align(c, pay_base=0):
    return (c.pay_off.astype(np.int64) + pay_base) & 15


def fill_bytes(fill, size, rng):
    if isinstance(fill, str):
        return rng.integers(0, 256, size, dtype=np.uint8)
    return np.full(size, fill, np.uint8)


def up(x, m):
    return (int(x) + m - 1) // m * m


# ---- 1. regime boundaries ---------------------------------------------------
BOUNDARIES = (8, 32, 96, 128)
DELTAS = (-17, -16, -15, -1, 0, 1, 15, 16, 17, "random")
FILLS = ("random", 0xFF)


def boundary_case(bnd, delta, fill="random", room=2048):
    """256 packets around chunk count `bnd`: packet i writes at destination
    alignment i % 16, reads its payload at source alignment (i // 16) % 16,
    and (destination alignment + frame_len) == 16 * bnd + delta (`delta`
    "random": drawn per packet from -20..20).  A frame of room bytes or more
    is NO_ROOM.  The layout and the records do not depend on `fill`."""
    n = 256
    rng = np.random.default_rng([bnd, DELTAS.index(delta)])
    i = np.arange(n)
    da, sa = i % 16, (i // 16) % 16
    chains = [CHAINS[(k * 7 + k // 16) % 6] for k in range(n)]
    recs = make_records(chains, rng)
    dl = rng.integers(-20, 21, n) if delta == "random" else np.full(n, delta)
    flen = 16 * bnd + dl - da
    plen = flen - hdr_len(chains)
    assert (plen >= 4).all()
    pslot = up(plen.max() + 16, 64)
    poff = i * pslot + sa
    parena = fill_bytes(fill, n * pslot, rng)
    slot = up(16 * bnd + 20 + 16, 64)
    off = i * slot + da
    return case(recs, parena, poff, plen, off, n * slot, room, np.where(flen >= room, B.NO_ROOM, B.OK))


# ---- 2. mixed waves ---------------------------------------------------------
# frame-length regimes: header only, <= 127, 128-511, 512-1535, 1536-2047
REGIME_LO = (0, 0, 128, 512, 1536)
REGIME_HI = (0, 127, 511, 1535, 2047)
DEAD = ("rec", "pay", "room", "edge", "wrap")
STATUS_OF = {"ok": B.OK, "rec": B.BAD_RECORD, "pay": B.BAD_PAYLOAD, "room": B.NO_ROOM, "edge": B.NO_ROOM,
             "wrap": B.NO_ROOM}


def min_plen(chain):
    """The shortest payload a chain is built with: ICMP echo messages carry
    their 4-byte identifier / sequence number."""
    return 4 if chain in ICMP else 0


def regime(chain, plen):
    """The regime of a frame, from its chain and payload length."""
    if plen == min_plen(chain):
        return 0
    f = HDR[chain] + plen
    return 1 if f <= 127 else 2 if f <= 511 else 3 if f <= 1535 else 4


def draw_plen(chain, reg, rng):
    if reg == 0:
        return min_plen(chain)
    lo = max(REGIME_LO[reg], HDR[chain] + min_plen(chain) + 1)
    return int(rng.integers(lo, REGIME_HI[reg] + 1)) - HDR[chain]


def assemble(chains, plen, kind, rng, room=2048):
    """A burst packed back to back with gaps of 0-3 bytes, in both arenas.
    kind[i]: "ok", or why packet i is not built:
      rec   the record names no chain (version, protocol or ICMP type)
      pay   the payload ends one byte past its arena
      room  the caller chose plen so that frame_len >= room
      edge  the frame would end one byte past the out arena
      wrap  out_off 0xFFFFFFF0
    A packet that is not built owns up to 96 bytes of the out arena all the
    same, which have to stay untouched."""
    n = len(chains)
    plen = np.asarray(plen, np.int64)
    recs = make_records(chains, rng)
    flen = hdr_len(chains) + plen
    for i, k in enumerate(kind):
        if k == "rec":
            if chains[i] in ICMP and i % 3 == 0:
                recs["src_port"][i] = 3 if chains[i][0] == 4 else 8
            elif i % 3 == 1:
                recs["protocol"][i] = 2
            else:
                recs["version"][i] = 5
        assert (flen[i] >= room) == (k == "room"), (i, k, flen[i])
    # payload arena: the payloads that lie inside it, back to back
    inside = np.array([k != "pay" for k in kind])
    sz = np.where(inside, plen, 0)
    poff = 3 + np.cumsum(sz + rng.integers(0, 4, n)) - sz
    pay_size = int(poff[-1] + sz[-1]) + int(rng.integers(0, 4))
    poff = np.where(inside, poff, pay_size - plen + 1)
    assert (poff >= 0).all()
    parena = rng.integers(0, 256, pay_size, dtype=np.uint8)
    # out arena
    live = np.array([k == "ok" for k in kind])
    own = np.where(live, flen, np.minimum(flen, 96))
    off = 5 + np.cumsum(own + rng.integers(0, 4, n)) - own
    out_size = int(off[-1] + own[-1]) + 9
    for i, k in enumerate(kind):
        if k == "edge":
            off[i] = out_size - flen[i] + 1
            assert off[i] >= 0
        elif k == "wrap":
            off[i] = 0xFFFFFFF0
    return case(recs, parena, poff, plen, off, out_size, room, [STATUS_OF[k] for k in kind])


def dead_plen(chain, k, reg, rng, room=2048):
    """The payload length of a packet that is not built for reason k."""
    if k == "room":
        return int(rng.integers(room, room + 150)) - HDR[chain]
    return draw_plen(chain, reg, rng)


MIXED_N = (64, 65, 257)


def mixed_case(n, seed=0):
    """n packets of every regime and status, about one in eight not built.
    The first wave holds every regime and every status; the rest is drawn."""
    rng = np.random.default_rng([n, seed])
    chains = [CHAINS[int(c)] for c in rng.integers(0, 6, n)]
    reg = rng.integers(0, 5, n)
    kind = ["ok" if rng.integers(0, 8) else DEAD[int(rng.integers(0, len(DEAD)))] for _ in range(n)]
    perm = rng.permutation(WAVE)
    for j in range(5):
        reg[perm[j]], kind[perm[j]] = j, "ok"
    for j, k in enumerate(("rec", "pay", "room")):
        kind[perm[5 + j]] = k
    plen = [draw_plen(c, r, rng) if k == "ok" else dead_plen(c, k, r, rng)
            for c, r, k in zip(chains, reg, kind)]
    return assemble(chains, plen, kind, rng)


STRUCTURED = ("one_long", "two_long", "one_dead", "dead_long")
PAIRS = ((0, 1), (0, 15), (3, 4), (7, 8), (14, 15), (5, 11), (2, 13), (4, 12))


def structured_case(what):
    """Waves of 16 packets in which the teams disagree on purpose:
      one_long   16 waves; wave w has one long (> 512 B) packet, at team w,
                 the other 15 are short (<= 127 B) or not built
      two_long   8 waves with long packets at the two teams of PAIRS
      one_dead   4 waves, long everywhere but for one team that is not built
      dead_long  8 waves whose only long packet is NO_ROOM; the rest is short"""
    rng = np.random.default_rng(STRUCTURED.index(what) + 100)
    waves = {"one_long": 16, "two_long": 8, "one_dead": 4, "dead_long": 8}[what]
    chains, plen, kind = [], [], []
    for w in range(waves):
        for t in range(WAVE):
            c = CHAINS[(w + t * 5) % 6]
            if what == "one_long":
                long_, k = t == w, "ok"
                if not long_ and rng.integers(0, 4) == 0:
                    k = ("rec", "pay", "edge", "wrap")[int(rng.integers(0, 4))]
            elif what == "two_long":
                long_, k = t in PAIRS[w], "ok"
            elif what == "one_dead":
                long_ = True
                k = DEAD[w] if t == (0, 5, 10, 15)[w] else "ok"
            else:
                long_ = t == (w * 7 + 3) % WAVE
                k = ("room", "edge", "wrap", "room")[w % 4] if long_ else "ok"
            r = (3 + (w + t // 2) % 2) if long_ else int(rng.integers(0, 2))
            chains.append(c)
            kind.append(k)
            plen.append(draw_plen(c, r, rng) if k == "ok" else dead_plen(c, k, r, rng))
    return assemble(chains, plen, kind, rng)


# ---- 3. jumbo frames and the u16 limit ---------------------------------------
ROOMS = (9216, 65536)
JUMBO_DA = (0, 1, 3, 5, 8, 11, 13, 15)
JUMBO_SA = (0, 3, 15, 1, 7, 8, 9, 2)


def jumbo_lengths(room):
    return (9000, 9215) + ((65534, 65535) if room == 65536 else ())


def jumbo_case(room, fill="random"):
    """Per chain the frame lengths of jumbo_lengths(room), all built, and one
    frame that is not: frame_len == room (9216), or plen 65535, where the
    frame length no longer fits the u16 len (65536).  Destination and source
    alignments from JUMBO_DA / JUMBO_SA; the payloads overlap."""
    rng = np.random.default_rng([room, 7])
    chains, plen, status = [], [], []
    for c in CHAINS:
        for f in jumbo_lengths(room):
            chains.append(c)
            plen.append(f - HDR[c])
            status.append(B.OK)
        chains.append(c)
        plen.append(65535 if room == 65536 else room - HDR[c])
        status.append(B.NO_ROOM)
    n = len(chains)
    recs = make_records(chains, rng)
    j = np.arange(n)
    plen = np.array(plen)
    poff = np.array(JUMBO_SA)[(j * 3) % 8]
    parena = fill_bytes(fill, 65535 + 16, rng)
    own = np.where(np.array(status) == B.OK, hdr_len(chains) + plen, 128)
    slot = np.array([up(x + 16, 64) for x in own])
    off = np.cumsum(slot) - slot + np.array(JUMBO_DA)[j % 8]
    return case(recs, parena, poff, plen, off, int(slot.sum()), room, status)


# ---- 4. arena edges ---------------------------------------------------------
EDGE_PLENS = tuple(range(1, 49))
PAY_END_LENS = tuple(range(1712, 1728)) + (1, 2, 3, 5, 15, 16, 17, 33)  # payload arena lengths


def chain_for(plen, k):
    """Chains rotate; a payload under 4 bytes goes to UDP / TCP, which are
    built with it."""
    return NOT_ICMP[k % 4] if plen < 4 else CHAINS[k % 6]


def payload_end_case(arena_len):
    """Every payload ends on the last byte of a payload arena of arena_len
    bytes (they overlap): plen 1..48, 600 and 1700 as far as the arena goes,
    twice each with another chain.  Then payloads one byte past the end,
    which are BAD_PAYLOAD."""
    rng = np.random.default_rng(arena_len)
    plens = [p for p in EDGE_PLENS + (600, 1700) if p <= arena_len]
    chains, plen, poff, status = [], [], [], []
    for rep in range(2):
        for p in plens:
            chains.append(chain_for(p, len(chains) + rep))
            plen.append(p)
            poff.append(arena_len - p)
            status.append(B.OK)
    for p in (plens[0], plens[len(plens) // 2], plens[-1]):
        chains.append(chain_for(p, len(chains)))
        plen.append(p)
        poff.append(arena_len - p + 1)
        status.append(B.BAD_PAYLOAD)
    n = len(chains)
    recs = make_records(chains, rng)
    parena = rng.integers(0, 256, arena_len, dtype=np.uint8)
    slot = up(74 + max(plens) + 16, 64)
    off = np.arange(n) * slot + (np.arange(n) * 5 + arena_len) % 16
    return case(recs, parena, poff, plen, off, n * slot, 2048, status)


PAY_START_GROUPS = 4


def payload_start_case(group):
    """Payloads that start at pay_off 4 * group .. 4 * group + 3, where the
    header chunks' source offset wraps below 0: plen 1..48 and 600, every
    destination alignment."""
    rng = np.random.default_rng(50 + group)
    chains, plen, poff = [], [], []
    for po in range(4 * group, 4 * group + 4):
        for p in EDGE_PLENS + (600,):
            chains.append(chain_for(p, len(chains) + po))
            plen.append(p)
            poff.append(po)
    n = len(chains)
    recs = make_records(chains, rng)
    parena = rng.integers(0, 256, 640, dtype=np.uint8)
    k = np.arange(n)
    off = k * 704 + (k * 3 + k // 16) % 16
    return case(recs, parena, poff, plen, off, n * 704, 2048, np.full(n, B.OK))


OUT_EDGE_LAST = ((38, 300), (513, 1535), (1537, 2046))  # frame length of the last frame


def out_edge_case(residue, last, over):
    """An out arena of out_size % 16 == residue: the first frame at offset 0,
    two in between, and the last frame (its length from OUT_EDGE_LAST[last])
    ending on the arena's final byte; with `over` it is one byte longer and
    NO_ROOM.  Nothing else differs between the two."""
    rng = np.random.default_rng([residue, last])
    chains = [CHAINS[int(c)] for c in rng.integers(0, 6, 4)]
    lo, hi = OUT_EDGE_LAST[last]
    flen = np.array([rng.integers(600, 2048), rng.integers(80, 600), rng.integers(1537, 2048),
                     rng.integers(max(lo, HDR[chains[3]] + 5), hi + 1)])
    plen = flen - hdr_len(chains)
    recs = make_records(chains, rng)
    sz = plen + 1
    poff = 1 + np.cumsum(sz + rng.integers(0, 4, 4)) - sz
    parena = rng.integers(0, 256, int(poff[-1] + sz[-1]), dtype=np.uint8)
    off = np.cumsum(flen + rng.integers(0, 4, 4)) - flen
    off[0] = 0
    out_size = up(off[3] + flen[3], 16) + 16 + residue
    off[3] = out_size - flen[3]
    if over:
        plen[3] += 1
    return case(recs, parena, poff, plen, off, out_size, 2048, [B.OK] * 3 + [B.NO_ROOM if over else B.OK])


# ---- 6. no payload arena ----------------------------------------------------
def nopay_case():
    """All six chains at every destination alignment without a payload arena,
    packed back to back (a one-byte gap where the alignment has to move on:
    the header lengths are all even).  UDP and TCP frames are header-only;
    the ICMP chains, whose body is under 4 bytes, are BAD_RECORD and own no
    bytes.  The last record is built to have a zero UDP checksum."""
    rng = np.random.default_rng(6)
    need = {(c, a) for c in CHAINS for a in range(16)}
    chains, off, cur = [], [], 3
    while need:
        ready = [c for c in CHAINS if (c, cur % 16) in need]
        if ready:
            c = ready[len(chains) % len(ready)]
        elif any(a % 2 == cur % 2 for _, a in need):
            c = NOT_ICMP[len(chains) % 4]  # once more, to move on by an even step
        else:
            cur += 1
            continue
        need.discard((c, cur % 16))
        chains.append(c)
        off.append(cur)
        cur += 0 if c in ICMP else HDR[c]
    chains.append((4, 17))
    off.append(cur)
    recs = make_records(chains, rng)
    recs[-1:] = zero_checksum_record()
    status = [B.BAD_RECORD if c in ICMP else B.OK for c in chains]
    return case(recs, None, None, None, off, cur + 42 + 7, 2048, status)


# ---- 5. unaligned arena bases -----------------------------------------------
def base_pairs(k):
    """(out base, payload base) pairs run for k in 1..15."""
    return [(k, 16 - k), (k, k)] + ([(k, 0), (0, k)] if k in (1, 7, 8, 15) else [])


def base_cases(k):
    """What runs over arenas at the bases of base_pairs(k)."""
    return [mixed_case(65, seed=k), boundary_case(BOUNDARIES[k % 4], "random"),
            payload_end_case(PAY_END_LENS[k]), payload_start_case(k % PAY_START_GROUPS)]
