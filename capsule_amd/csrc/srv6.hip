// srv6.hip — cgsr_apply: push, replace, advance or remove a SegmentRouting
// header on frames in device memory, lengths and checksums reconciled, in one
// launch (include/capsule_gpu_srv6.h; ip/v6/srh.rs:210-233, 299-391).
//
// An output frame is three pieces:
//   head     [0, hlen)      the first x = eth_len + 40 input bytes with the
//                           IPv6 payload_length / next_header / dst patched,
//                           the new SRH's fixed 8 bytes and, with
//                           CGSR_P_FINAL_FROM_PACKET, its segments[0];
//   list     [hlen, send)   the policy's segments, from the segment arena;
//   suffix   [send, len')   input bytes at a shifted offset.
//
// Work split.  A team of 4 lanes edits one packet (16 packets a wave, 64 a
// workgroup), as build.hip does.
//   * The team loads the frame's first 80 bytes once (one 16-B load a lane,
//     a fifth by lane 0) into LDS; every lane runs the parses on that
//     window.  The team's first lane alone fetches what only some ops need
//     (the address that becomes the IPv6 dst, segments[0] for the
//     pseudo-header, an extension header DECAP uncovers), patches the head
//     and leaves it in LDS as dwords of frame bytes -2.., so that the IPv6
//     header is dword aligned under all three Ethernet lengths.
//   * The output is cut into 16-B chunks aligned in the out arena; lane g of
//     the team owns chunks g, g + 4, ... below kTeamChunks (512 B).  A chunk
//     is the OR of its head bytes (LDS, v_alignbyte), its list bytes and its
//     suffix bytes; the latter two are one aligned 16-B load of their arena,
//     the dword behind it from the next lane (a shuffle; a lane whose
//     neighbour has none loads it), v_alignbyte by the source / destination
//     misalignment and a byte mask.  Suffix dwords at or behind the L4
//     header are added to the lane's checksum accumulator as they pass.
//   * Chunks from kTeamChunks on are copied by the whole wave, one packet at
//     a time, 1 KiB a step, and their sum is reduced over the wave.
//   * The one or two chunks that hold the Udp length / L4 checksum are kept
//     in a register (their old field bytes taken back out of the sum) until
//     the packet's sum is reduced, patched and stored then.  All other
//     chunks are stored at once.
// So every suffix and list byte is loaded once (the alignment dword at the
// end of a team's 64 B / the wave's 1 KiB step twice, and up to 26 suffix
// bytes that also lie in the 80-B parse window), and every output byte is
// stored once: whole chunks as one 16-B store, the partial first and last
// chunk as dword and byte stores of the frame's own bytes, so frames may
// abut at any byte.  Loads are whole aligned dwords / 16-B blocks holding at
// least one byte of the frame, clipped to the arena by the buffer descriptor.
//
// Checksums are summed as little-endian dwords of the out arena's address
// space (device_common.hpp); the sum of an L4 span that starts at an odd
// address is byte-swapped after folding.
#include "capsule_gpu_srv6.h"
#include "device_common.hpp"
#include "kernels.hpp"

namespace cgpu {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTeam = 4;                       // lanes per packet
constexpr uint32_t kTeamsPerBlock = kBlock / kTeam;  // packets per workgroup
constexpr uint32_t kWinDw = 20;       // parse window: 80 B from the frame's dword
constexpr uint32_t kWinBytes = 76;    // of which the frame's first 76 are usable
constexpr uint32_t kHeadDw = 24;      // head image: frame bytes -2 .. 93
constexpr uint32_t kTeamChunks = 32;  // chunks (512 B) a team copies itself

// Mask of the bytes b of a dword with lo <= b < hi.
__device__ __forceinline__ uint32_t byte_mask(int lo, int hi) {
  uint32_t m = 0xffffffffu;
  if (lo > 0) m = lo >= 4 ? 0u : (m << (8 * lo));
  if (hi < 4) m &= hi <= 0 ? 0u : (0xffffffffu >> (8 * (4 - hi)));
  return m;
}

// One packet's output as the copy loops see it.  Offsets are relative to the
// 16-B aligned base of the out arena's descriptor.
struct Plan {
  uint32_t d, end;  // the frame
  uint32_t hend;    // [d, hend): head image
  uint32_t send;    // [hend, send): policy segments; [send, end): suffix
  uint32_t sseg;    // segment arena offset of out byte a is sseg + a (mod 2^32)
  uint32_t sin;     // in arena offset of out byte a is sin + a (mod 2^32)
  uint32_t slo;     // [slo, end): the L4 span (== end: no L4 layer)
  uint32_t pp, pn;  // [pp, pp + pn): Udp length + checksum / L4 checksum (pn 0: none)
  uint32_t nch;     // chunks of the frame (0: nothing is written)
};

// The bytes [lo, hi) of the chunk at out offset `a` from the source whose
// offset for out byte a is sbase + a; zero elsewhere.  SUM: dwords' bytes at
// or behind slo are added to acc.  Called by every lane of the wave
// together; `on`: this lane has a chunk; `last`: the next lane does not hold
// the next chunk.
template <bool SUM>
__device__ __forceinline__ u32x4 src_chunk(rsrc_t rs, uint32_t rlen, uint32_t sbase, uint32_t a,
                                           uint32_t lo, uint32_t hi, uint32_t slo, bool on,
                                           bool last, uint64_t &acc) {
  const bool need = on && lo < hi && a < hi && a + 16u > lo;
  const uint32_t so = sbase + a, s2 = so & 3u;
  const uint32_t xs = need ? (so & ~3u) : 0xfffffff0u;  // off: past every arena, no access
  const u32x4 x = load16(rs, xs, rlen);
  uint32_t x4 = __shfl_down(x[0], 1);
  const bool nb = __shfl_down(need ? 1 : 0, 1) != 0;
  if (need && s2 != 0u && (last || !nb)) x4 = load4_tail(rs, xs + 16u, rlen);
  const uint32_t X[5] = {x[0], x[1], x[2], x[3], x4};
  u32x4 v;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t p = a + 4u * t;
    v[t] = __builtin_amdgcn_alignbyte(X[t + 1], X[t], s2) & byte_mask((int)(lo - p), (int)(hi - p));
    if (SUM) acc += (uint64_t)(v[t] & byte_mask((int)(slo - p), 4));
  }
  return v;
}

// The chunk at out offset `a` of packet k, whose head image is H.
__device__ __forceinline__ u32x4 make_chunk(rsrc_t irs, uint32_t ilen, rsrc_t srs, uint32_t slen,
                                            const uint32_t *H, const Plan &k, uint32_t a, bool on,
                                            bool last, uint64_t &acc) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (on && a < k.hend) {
    const int hb = (int)(a - k.d) + 2;  // H byte of the chunk's first byte (>= -13)
    const uint32_t s = (uint32_t)hb & 3u;
    const int q0 = (hb - (int)s) >> 2;
    uint32_t Hw[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int q = q0 + j;
      const int idx = q < 0 ? 0 : (q > (int)kHeadDw - 1 ? (int)kHeadDw - 1 : q);
      const uint32_t x = H[idx];
      Hw[j] = (q >= 0 && q < (int)kHeadDw) ? x : 0u;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t p = a + 4u * t;
      v[t] = __builtin_amdgcn_alignbyte(Hw[t + 1], Hw[t], s) &
             byte_mask((int)(k.d - p), (int)(k.hend - p));
    }
  }
  uint64_t none = 0;
  if (__ballot(on && k.hend < k.send && a < k.send && a + 16u > k.hend)) {
    const u32x4 w = src_chunk<false>(srs, slen, k.sseg, a, k.hend, k.send, 0u, on, last, none);
    v |= w;
  }
  if (__ballot(on && k.send < k.end && a + 16u > k.send)) {
    const u32x4 w = src_chunk<true>(irs, ilen, k.sin, a, k.send, k.end, k.slo, on, last, acc);
    v |= w;
  }
  return v;
}

// Store the bytes of the chunk at out offset `a` that belong to [d, end).
__device__ __forceinline__ void store_chunk(rsrc_t ors, uint32_t a, u32x4 v, uint32_t d,
                                            uint32_t end) {
  if (a >= d && a + 16u <= end) {
    __builtin_amdgcn_raw_buffer_store_b128(v, ors, (int)a, 0, 0);
    return;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t aa = a + 4u * t;
    const uint32_t m = byte_mask((int)(d - aa), (int)(end - aa));
    if (m == 0xffffffffu) {
      __builtin_amdgcn_raw_buffer_store_b32(v[t], ors, (int)aa, 0, 0);
    } else if (m != 0u) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if ((m >> (8 * b)) & 0xffu)
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v[t] >> (8 * b)), ors, (int)(aa + b), 0, 0);
    }
  }
}

// Whether the chunk at `a` holds a byte of the patch range.
__device__ __forceinline__ bool holds_patch(uint32_t a, uint32_t pp, uint32_t pn) {
  return pn != 0u && a < pp + pn && a + 16u > pp;
}

// The old bytes of the patch range leave the sum (they are replaced).
__device__ __forceinline__ void unsum_patch(u32x4 v, uint32_t a, uint32_t pp, uint32_t pn,
                                            uint64_t &acc) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int sh = (int)(pp - (a + 4u * t));
    acc -= (uint64_t)(v[t] & byte_mask(sh, sh + (int)pn));
  }
}

// The patch range's bytes become pv's (little-endian, in address order).
__device__ __forceinline__ u32x4 apply_patch(u32x4 v, uint32_t a, uint32_t pp, uint32_t pn,
                                             uint32_t pv) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int sh = (int)(pp - (a + 4u * t));
    const uint32_t m = byte_mask(sh, sh + (int)pn);
    const uint32_t val = sh >= 0 ? (sh < 4 ? pv << (8 * sh) : 0u) : (sh > -4 ? pv >> (8 * -sh) : 0u);
    v[t] = (v[t] & ~m) | (val & m);
  }
  return v;
}

// 16 bytes at any arena offset.
__device__ __forceinline__ void load_addr(rsrc_t rs, uint32_t off, uint32_t rlen, uint32_t (&A)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) A[j] = load4_any(rs, off + 4u * j, rlen);
}

__global__ __launch_bounds__(kBlock) void srv6_kernel(Srv6Args a) {
  __shared__ uint32_t win[kTeamsPerBlock][kWinDw];
  __shared__ uint32_t head[kTeamsPerBlock][kHeadDw];
  const uint32_t tid = threadIdx.x, g = tid & (kTeam - 1u), team = tid / kTeam, lane = tid & 63u;
  const uint32_t i = blockIdx.x * kTeamsPerBlock + team;
  // Descriptors over the arenas' 16-B aligned bases (kernel arguments only,
  // so wave-uniform): chunk alignment is then alignment in memory.
  const uint32_t pa_o = (uint32_t)(uintptr_t)a.out_arena & 15u;
  const uint32_t pa_i = (uint32_t)(uintptr_t)a.in_arena & 15u;
  const uint32_t pa_s = (uint32_t)(uintptr_t)a.segments & 15u;
  const rsrc_t ors = make_rsrc(a.out_arena - pa_o, a.out_arena_len + pa_o);
  const uint32_t ilen = a.in_arena_len + pa_i;
  const rsrc_t irs = make_rsrc(a.in_arena - pa_i, ilen);
  const uint32_t slen = a.segments ? 16u * a.n_segments_total + pa_s : 0u;
  const rsrc_t srs = make_rsrc(a.segments - pa_s, slen);

  const bool in = i < a.n;
  uint32_t ioff = 0u, len = 0u, ooff = 0u, op = CGSR_OP_NONE;
  if (in) {
    ioff = a.in_off[i];
    len = a.in_len[i];
    ooff = a.out_off[i];
    op = a.op[i];
  }
  const uint32_t s0 = ioff + pa_i;  // the frame's first byte under irs
  const bool edit = op >= CGSR_OP_ENCAP && op <= CGSR_OP_DECAP;

  // ---- the parse window, once per team -------------------------------------
  const uint32_t sh = s0 & 3u, wb = s0 - sh;
  const uint32_t wneed = edit ? (len < kWinBytes ? len : kWinBytes) : 0u;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const uint32_t c = g + kTeam * half;
    if (c >= kWinDw / 4u) continue;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (16u * c < sh + wneed) v = load16(irs, wb + 16u * c, ilen);
    uint32_t *w = &win[team][4u * c];
    w[0] = v[0];
    w[1] = v[1];
    w[2] = v[2];
    w[3] = v[3];
  }
  __syncthreads();

  // ---- parse::<Ethernet>, parse::<Ipv6>, parse::<SegmentRouting<Ipv6>> ------
  const uint32_t *W = win[team];
  uint32_t P[6];  // frame bytes 0..23
#pragma unroll
  for (int j = 0; j < 6; ++j) P[j] = __builtin_amdgcn_alignbyte(W[j + 1], W[j], sh);
  const uint32_t marker = be16_lo(P[3]);  // vlan_marker (ethernet.rs:164-167)
  const uint32_t eth = marker == 0x8100u ? 18u : (marker == 0x88a8u ? 22u : 14u);
  const uint32_t et = be16_lo(eth == 14u ? P[3] : (eth == 18u ? P[4] : P[5]));
  const uint32_t x = eth + 40u;
  uint32_t Q[12];  // the IPv6 header and the 8 bytes behind it
  {
    const uint32_t qb = sh + eth, qi = qb >> 2, qs = qb & 3u;
#pragma unroll
    for (int j = 0; j < 12; ++j) Q[j] = __builtin_amdgcn_alignbyte(W[qi + j + 1], W[qi + j], qs);
  }
  uint32_t st = CGPU_PKT_OK;
  if (op > CGSR_OP_DECAP) st = CGSR_BAD_OP;
  else if (edit) {
    if (len == 0u) st = CGPU_PKT_ETH_BAD_OFFSET;
    else if (len < 14u || len < eth) st = CGPU_PKT_ETH_OUT_OF_BUFFER;
    else if (et != 0x86ddu) st = CGPU_PKT_NOT_IPV6;
    else if (!(eth < len)) st = CGPU_PKT_L3_BAD_OFFSET;
    else if (x > len) st = CGPU_PKT_L3_OUT_OF_BUFFER;
  }
  const uint32_t nh = (Q[1] >> 16) & 0xffu;
  const uint32_t srh_nh = Q[10] & 0xffu, hel = (Q[10] >> 8) & 0xffu, sl_old = Q[10] >> 24;
  const uint32_t last_entry = Q[11] & 0xffu, old_n = last_entry + 1u;
  const bool has_srh = op == CGSR_OP_SET || op == CGSR_OP_END || op == CGSR_OP_DECAP;
  if (st == CGPU_PKT_OK && has_srh) {
    if (nh != 43u) st = CGSR_NOT_ROUTING;
    else if (!(x < len)) st = CGPU_PKT_EXT_BAD_OFFSET;
    else if (x + 8u > len) st = CGPU_PKT_EXT_OUT_OF_BUFFER;
    else if (hel == 0u || hel != 2u * old_n) st = CGPU_PKT_SRH_INCONSISTENT;
    else if (!(x + 8u < len)) st = CGPU_PKT_EXT_BAD_OFFSET;
    else if (x + 8u + 16u * old_n > len) st = CGPU_PKT_EXT_OUT_OF_BUFFER;
  }
  // ---- the policy -----------------------------------------------------------
  const bool takes_policy = op == CGSR_OP_ENCAP || op == CGSR_OP_SET;
  uint32_t seg_first = 0u, pn_seg = 0u, p_sl = 0u, p_tag = 0u, p_flags = 0u;
  if (st == CGPU_PKT_OK && takes_policy) {
    const uint32_t pi = a.policy_idx ? a.policy_idx[i] : 0xffffffffu;
    if (pi >= a.n_policies) {
      st = CGSR_BAD_POLICY;
    } else {
      const uint32_t *pw = reinterpret_cast<const uint32_t *>(a.policy) + 4u * (size_t)pi;
      const uint32_t w1 = pw[1];
      seg_first = pw[0];
      pn_seg = w1 & 0xffu;
      p_sl = (w1 >> 8) & 0xffu;
      p_tag = w1 >> 16;
      p_flags = pw[2] & 0xffu;
      if (pn_seg == 0u || pn_seg > 127u ||
          (uint64_t)seg_first + pn_seg > (uint64_t)a.n_segments_total ||
          ((p_flags & CGSR_P_SET_DST) && p_sl >= pn_seg))
        st = CGSR_BAD_POLICY;
    }
  }
  // ---- the splice: `rem` bytes leave at x, `ins` arrive ----------------------
  uint32_t ins = 0u, rem = 0u;
  if (op == CGSR_OP_ENCAP) ins = 8u + 16u * pn_seg;
  else if (op == CGSR_OP_SET) ins = 8u + 16u * pn_seg, rem = 8u + 16u * old_n;
  else if (op == CGSR_OP_END) ins = 8u, rem = 8u;  // the fixed header is rebuilt
  else if (op == CGSR_OP_DECAP) rem = 8u + 16u * old_n;
  const uint32_t L = len + ins - rem;
  if (st == CGPU_PKT_OK) {
    const int T = (int)a.room - (int)len;  // Mbuf::tailroom
    const int grow = (int)ins - (int)rem;
    if ((grow > 0 && !(grow < T)) || (uint64_t)ooff + L > (uint64_t)a.out_arena_len)
      st = CGPU_PKT_NOT_RESIZED;
    else if (op == CGSR_OP_END && sl_old == 0u) st = CGSR_NO_SEGMENTS_LEFT;
    else if (op == CGSR_OP_END && sl_old - 1u > last_entry) st = CGSR_BAD_SEGMENTS_LEFT;
  }
  const bool live = in && st == CGPU_PKT_OK;
  const bool final_pkt = takes_policy && (p_flags & CGSR_P_FINAL_FROM_PACKET);
  const uint32_t out_n = op == CGSR_OP_END ? old_n : pn_seg;  // segments of the output's SRH
  uint32_t hlen = 0u, send_rel = 0u;
  if (edit) {
    hlen = op == CGSR_OP_DECAP ? x : x + 8u + (final_pkt ? 16u : 0u);
    send_rel = takes_policy ? x + 8u + 16u * pn_seg : hlen;
  }

  // ---- the team's first lane: the head, and what reconcile needs -------------
  uint32_t l4o = 0u, l4kind = 0u;  // 0 none, 1 Udp, 2 Tcp, 3 Icmpv6
  uint64_t pbase = 0;              // pseudo-header sum but for the span's own bytes
  if (g == 0u && live && edit) {
    uint32_t dst[4] = {Q[6], Q[7], Q[8], Q[9]};  // the output's Ipv6::dst()
    uint32_t F[4] = {Q[6], Q[7], Q[8], Q[9]};    // FINAL_FROM_PACKET: the output's segments[0]
    uint32_t S0[4] = {0u, 0u, 0u, 0u};           // the output's SRH segments[0]
    bool behind_srh = op != CGSR_OP_DECAP;
    uint32_t proto = op == CGSR_OP_ENCAP ? nh : srh_nh;
    bool reach = true;
    l4o = x + (op == CGSR_OP_DECAP ? 0u : 8u + 16u * out_n);
    if (op == CGSR_OP_SET && final_pkt) load_addr(irs, s0 + x + 8u, ilen, F);
    if (takes_policy) {
      if (final_pkt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) S0[j] = F[j];
      } else {
        load_addr(srs, pa_s + 16u * seg_first, slen, S0);
      }
      if (p_flags & CGSR_P_SET_DST) {
        if (p_sl == 0u) {
#pragma unroll
          for (int j = 0; j < 4; ++j) dst[j] = S0[j];
        } else {
          load_addr(srs, pa_s + 16u * (seg_first + p_sl), slen, dst);
        }
      }
    } else if (op == CGSR_OP_END) {
      load_addr(irs, s0 + x + 8u, ilen, S0);
      load_addr(irs, s0 + x + 8u + 16u * (sl_old - 1u), ilen, dst);
    } else if (proto == 43u || proto == 44u) {
      // DECAP uncovered another extension header: one level is parsed
      // (srh.rs:299-327, fragment.rs:187-202)
      reach = x < L && x + 8u <= L;
      if (reach) {
        const uint32_t e0 = load4_any(irs, s0 + x + rem, ilen);
        const uint32_t e1 = load4_any(irs, s0 + x + rem + 4u, ilen);
        if (proto == 43u) {
          const uint32_t m = (e1 & 0xffu) + 1u, h2 = (e0 >> 8) & 0xffu;
          reach = h2 != 0u && h2 == 2u * m && x + 8u < L && x + 8u + 16u * m <= L;
          if (reach) load_addr(irs, s0 + x + rem + 8u, ilen, S0);
          behind_srh = true;
          l4o = x + 8u + 16u * m;
        } else {
          l4o = x + 8u;
        }
        proto = e0 & 0xffu;
      }
    }
    uint32_t acc_f = a.flags & (CGPU_F_ACCEPT_UDP | CGPU_F_ACCEPT_TCP | CGPU_F_ACCEPT_ICMP);
    if (acc_f == 0u) acc_f = CGPU_F_ACCEPT_UDP | CGPU_F_ACCEPT_TCP;
    uint32_t l4len = 0u;
    if (!reach) l4kind = 0u;
    else if ((acc_f & CGPU_F_ACCEPT_UDP) && proto == 17u) l4kind = 1u, l4len = 8u;
    else if ((acc_f & CGPU_F_ACCEPT_TCP) && proto == 6u) l4kind = 2u, l4len = 20u;
    else if ((acc_f & CGPU_F_ACCEPT_ICMP) && proto == 58u) l4kind = 3u, l4len = 4u;
    if (l4kind != 0u && !(l4o < L && l4o + l4len <= L)) l4kind = 0u;
    if (l4kind != 0u) {
      const uint32_t span = (L - l4o) & 0xffffu;
      pbase = (uint64_t)Q[2] + Q[3] + Q[4] + Q[5] + (proto << 8) + swap16(span);
      if (behind_srh) pbase += (uint64_t)S0[0] + S0[1] + S0[2] + S0[3];
      else pbase += (uint64_t)dst[0] + dst[1] + dst[2] + dst[3];
      if (l4kind == 1u) pbase += swap16(span);  // Udp::set_length (udp.rs:350-354)
    }
    // the head image: frame byte b at H byte b + 2
    uint32_t *H = head[team];
    H[0] = P[0] << 16;
#pragma unroll
    for (int j = 1; j < 6; ++j) H[j] = (P[j - 1] >> 16) | (P[j] << 16);
    const uint32_t e4 = (eth + 2u) >> 2;
    const uint32_t nh_out = op == CGSR_OP_DECAP ? srh_nh : 43u;
    H[e4] = Q[0];
    H[e4 + 1u] = swap16((L - x) & 0xffffu) | (nh_out << 16) | (Q[1] & 0xff000000u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      H[e4 + 2u + j] = Q[2 + j];
      H[e4 + 6u + j] = dst[j];
      H[e4 + 12u + j] = F[j];
    }
    uint32_t f0, f1;
    if (op == CGSR_OP_END) {
      f0 = (Q[10] & 0x00ffffffu) | ((sl_old - 1u) << 24);
      f1 = Q[11];
    } else if (op == CGSR_OP_SET) {
      f0 = srh_nh | ((2u * pn_seg) << 8) | (Q[10] & 0x00ff0000u) | (p_sl << 24);
      f1 = (pn_seg - 1u) | (Q[11] & 0x0000ff00u) | (swap16(p_tag) << 16);
    } else {  // SegmentRoutingHeader::default: routing_type 4 (srh.rs:509-522)
      f0 = nh | ((2u * pn_seg) << 8) | (4u << 16) | (p_sl << 24);
      f1 = (pn_seg - 1u) | (swap16(p_tag) << 16);
    }
    H[e4 + 10u] = f0;
    H[e4 + 11u] = f1;
  }
  __syncthreads();
  const uint32_t lead = lane & ~(kTeam - 1u);
  l4o = __shfl(l4o, lead);
  l4kind = __shfl(l4kind, lead);

  Plan k;
  k.d = ooff + pa_o;
  k.end = k.d + L;
  k.hend = k.d + hlen;
  k.send = k.d + send_rel;
  k.sseg = pa_s + 16u * seg_first - (k.d + x + 8u);
  k.sin = s0 + rem - ins - k.d;
  k.slo = l4kind ? k.d + l4o : k.end;
  k.pp = k.slo + (l4kind == 1u ? 4u : (l4kind == 2u ? 16u : 2u));
  k.pn = l4kind == 0u ? 0u : (l4kind == 1u ? 4u : 2u);
  const uint32_t A0 = k.d & ~15u;
  k.nch = live ? (k.end - A0 + 15u) >> 4 : 0u;

  // The patch value once the span's sum is known (the first lane's is real).
  const uint32_t span = (L - l4o) & 0xffffu;
  auto finish = [&](uint32_t sum) -> uint32_t {
    uint32_t ps = fold32(sum);
    if (k.slo & 1u) ps = swap16(ps);  // address parity -> span parity
    uint32_t ck = ~fold64(pbase + ps) & 0xffffu;
    if (l4kind == 1u && ck == 0u) ck = 0xffffu;  // Udp::set_checksum (udp.rs:132-141)
    return l4kind == 1u ? (swap16(span) | (ck << 16)) : ck;
  };

  // ---- the team's chunks ------------------------------------------------------
  uint64_t acc = 0;
  u32x4 keep = {0u, 0u, 0u, 0u};
  uint32_t keep_a = 0xffffffffu;
  {
    uint32_t top = k.nch < kTeamChunks ? k.nch : kTeamChunks;
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) {
      const uint32_t o = __shfl_xor(top, dlt);
      top = o > top ? o : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);
    for (uint32_t c0 = 0u; c0 < top; c0 += kTeam) {
      const uint32_t c = c0 + g, ao = A0 + 16u * c;
      const bool on = c < k.nch && c < kTeamChunks;
      const u32x4 v = make_chunk(irs, ilen, srs, slen, head[team], k, ao, on, g == kTeam - 1u, acc);
      if (on && holds_patch(ao, k.pp, k.pn)) {
        unsum_patch(v, ao, k.pp, k.pn, acc);
        keep = v;
        keep_a = ao;
      } else if (on) {
        store_chunk(ors, ao, v, k.d, k.end);
      }
    }
  }
  uint32_t psum = fold64(acc);
  psum += __shfl_xor(psum, 1);
  psum += __shfl_xor(psum, 2);
  // ---- long frames: the rest of each, over the wave ----------------------------
  unsigned long long longs = __ballot(g == 0u && k.nch > kTeamChunks);
  while (longs) {
    const int src = __builtin_ctzll(longs);
    longs &= longs - 1ull;
    Plan w;
    w.d = __builtin_amdgcn_readlane(k.d, src);
    w.end = __builtin_amdgcn_readlane(k.end, src);
    w.hend = __builtin_amdgcn_readlane(k.hend, src);
    w.send = __builtin_amdgcn_readlane(k.send, src);
    w.sseg = __builtin_amdgcn_readlane(k.sseg, src);
    w.sin = __builtin_amdgcn_readlane(k.sin, src);
    w.slo = __builtin_amdgcn_readlane(k.slo, src);
    w.pp = __builtin_amdgcn_readlane(k.pp, src);
    w.pn = __builtin_amdgcn_readlane(k.pn, src);
    w.nch = __builtin_amdgcn_readlane(k.nch, src);
    const uint32_t *wH = head[(tid >> 6) * (64u / kTeam) + ((uint32_t)src >> 2)];
    const uint32_t wA0 = w.d & ~15u;
    uint64_t wacc = 0;
    u32x4 wkeep = {0u, 0u, 0u, 0u};
    uint32_t wkeep_a = 0xffffffffu;
    for (uint32_t c0 = kTeamChunks; c0 < w.nch; c0 += 64u) {
      const uint32_t c = c0 + lane, ao = wA0 + 16u * c;
      const bool on = c < w.nch;
      const u32x4 v = make_chunk(irs, ilen, srs, slen, wH, w, ao, on, lane == 63u, wacc);
      if (on && holds_patch(ao, w.pp, w.pn)) {
        unsum_patch(v, ao, w.pp, w.pn, wacc);
        wkeep = v;
        wkeep_a = ao;
      } else if (on) {
        store_chunk(ors, ao, v, w.d, w.end);
      }
    }
    uint32_t ws = fold64(wacc);
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) ws += __shfl_xor(ws, dlt);
    if ((lane >> 2) == ((uint32_t)src >> 2)) psum += ws;
    const uint32_t pv = __builtin_amdgcn_readlane(finish(psum), src);
    if (wkeep_a != 0xffffffffu)
      store_chunk(ors, wkeep_a, apply_patch(wkeep, wkeep_a, w.pp, w.pn, pv), w.d, w.end);
  }
  // ---- the chunks kept back: Udp length / checksum patched, then stored ----------
  const uint32_t pv = __shfl(finish(psum), lead);
  if (keep_a != 0xffffffffu)
    store_chunk(ors, keep_a, apply_patch(keep, keep_a, k.pp, k.pn, pv), k.d, k.end);

  if (g == 0u && in) {
    a.out_len[i] = (uint16_t)(live ? L : 0u);
    if (a.status) a.status[i] = (uint8_t)st;
  }
}

}  // namespace

hipError_t launch_srv6(const Srv6Args &a, hipStream_t s) {
  const dim3 grid((a.n + kTeamsPerBlock - 1) / kTeamsPerBlock);
  hipLaunchKernelGGL(srv6_kernel, grid, dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace cgpu
