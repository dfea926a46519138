// build.hip — cgtx_build_batch: frames from header records (the inverse of
// the parse's field extraction), lengths and checksums reconciled, in one
// launch.
//
// Packet i is Mbuf::new(), push::<Ethernet>() (ethernet.rs:308-325),
// push::<Ipv4 | Ipv6>(), push::<Udp | Tcp | echo message>(), the setters,
// the payload and reconcile_all() (packets/mod.rs:297-300).
//
// Work split.  A team of 4 lanes builds one packet (16 packets a wave, 64 a
// workgroup).  The output is cut into 16-B chunks aligned in the out arena;
// lane g of the team owns chunks g, g + 4, ...  A chunk's bytes are the OR of
// a header part and a payload part:
//   * payload part: one aligned 16-B load of the payload arena, the dword
//     behind it from the next lane (a shuffle; the team's last lane loads it),
//     v_alignbyte by the source/destination misalignment, masked to the
//     payload's bytes, and added to the lane's checksum accumulator as it
//     passes.  Chunks behind the first eight are stored at once.
//   * header part: all lanes assemble the Ethernet/IP/L4 header in registers
//     from the record; once the team's (and the wave's, below) payload sums
//     are reduced and the L4 checksum is known, lane 0 puts the header's
//     dwords into LDS and every lane picks the five its chunk needs.  The
//     first eight chunks (two a lane, kept in registers) are stored then.
//   * long payloads: chunks from kTeamChunks on are copied by the whole wave,
//     one packet at a time, 1 KiB per step, and their sum is reduced over the
//     wave.
// So every payload byte is loaded from memory once (the alignment dword at
// the end of a team's / the wave's 64 B / 1 KiB step is asked for twice) and
// every frame byte is written once: whole chunks as one 16-B store, the
// partial first and last chunk as dword and byte stores of the frame's own
// bytes only -- neighbouring frames may abut at any byte, so nothing is read
// back or written outside [off, off + len).
//
// Checksums are summed as little-endian dwords of the destination address
// space (device_common.hpp); the payload sum of a frame whose payload starts
// at an odd address is byte-swapped after folding (a rotation by 8 is a
// multiplication by 256 = 2^-8 modulo 0xFFFF).
#include "capsule_gpu_tx.h"
#include "device_common.hpp"
#include "kernels.hpp"

namespace cgpu {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTeam = 4;                       // lanes per packet
constexpr uint32_t kTeamsPerBlock = kBlock / kTeam;  // packets per workgroup
constexpr uint32_t kHdrDw = 24;       // LDS dwords per team: 4 Ethernet + up to 15 IP/L4
constexpr uint32_t kTeamChunks = 32;  // chunks (512 B) a team copies itself

// Mask of the bytes b of a dword with lo <= b < hi.
__device__ __forceinline__ uint32_t byte_mask(int lo, int hi) {
  uint32_t m = 0xffffffffu;
  if (lo > 0) m = lo >= 4 ? 0u : (m << (8 * lo));
  if (hi < 4) m &= hi <= 0 ? 0u : (0xffffffffu >> (8 * (4 - hi)));
  return m;
}

// One packet as the copy loops see it; offsets are relative to the 16-B
// aligned bases of the two descriptors.
struct Span {
  uint32_t d;      // first byte of the frame
  uint32_t end;    // one past its last byte
  uint32_t dpay;   // first byte of the payload in the frame
  uint32_t plen;   // payload bytes (0: not built)
  uint32_t sbase;  // payload arena offset of out byte a is sbase + a (mod 2^32)
  uint32_t nch;    // chunks of the frame (0: not built)
};

// The payload part of the chunk at out offset `a` (zero outside the payload),
// added to acc.  Called by every lane of the wave together; `on`: this lane's
// chunk may need payload bytes; `last`: no next lane holds the next chunk.
__device__ __forceinline__ u32x4 pay_chunk(rsrc_t prs, uint32_t pay_len, const Span &k, uint32_t a,
                                           bool on, bool last, uint64_t &acc) {
  const uint32_t so = k.sbase + a, s2 = so & 3u;
  const uint32_t xs = on ? (so & ~3u) : 0xfffffff0u;  // off: past every arena, no access
  const u32x4 x = load16(prs, xs, pay_len);
  uint32_t x4 = __shfl_down(x[0], 1);
  if (last && s2 != 0u && on) x4 = load4_tail(prs, xs + 16u, pay_len);
  const uint32_t X[5] = {x[0], x[1], x[2], x[3], x4};
  u32x4 v;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int p0 = (int)(a + 4u * t - k.dpay);
    v[t] = __builtin_amdgcn_alignbyte(X[t + 1], X[t], s2) & byte_mask(-p0, (int)k.plen - p0);
    acc += (uint64_t)v[t];
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

__global__ __launch_bounds__(kBlock) void build_kernel(BuildArgs a) {
  __shared__ uint32_t hdr[kTeamsPerBlock][kHdrDw];
  const uint32_t tid = threadIdx.x, g = tid & (kTeam - 1u), team = tid / kTeam, lane = tid & 63u;
  const uint32_t i = blockIdx.x * kTeamsPerBlock + team;
  // Descriptors over the arenas' 16-B aligned bases (kernel arguments only,
  // so wave-uniform): chunk alignment is then alignment in memory.  Bytes
  // below the arena in its first 16-B block are never used or written.
  const uint32_t pa_o = (uint32_t)(uintptr_t)a.out_arena & 15u;
  const uint32_t pa_p = (uint32_t)(uintptr_t)a.pay_arena & 15u;
  const rsrc_t ors = make_rsrc(a.out_arena - pa_o, a.out_arena_len + pa_o);
  const uint32_t pay_len = a.pay_arena ? a.pay_len + pa_p : 0u;
  const rsrc_t prs = make_rsrc(a.pay_arena - pa_p, pay_len);

  const bool in = i < a.n;
  uint32_t R[24];
#pragma unroll
  for (int j = 0; j < 24; ++j) R[j] = 0u;
  uint32_t plen = 0u, poff = 0u, ooff = 0u;
  if (in) {
    const uint32_t *r = reinterpret_cast<const uint32_t *>(a.rec + i);
#pragma unroll
    for (int j = 0; j < 24; ++j)
      if (j != 3 && j != 9) R[j] = r[j];
    ooff = a.out_off[i];
    if (a.pay_arena) {
      plen = a.pay_plen[i];
      poff = a.pay_off[i];
    }
  }
  // ---- the chain (capsule_gpu_tx.h) ----------------------------------------
  const uint32_t version = R[4] & 0xffu, proto = R[7] & 0xffu;
  const bool v6 = version == 6u, v4 = version == 4u;
  const bool udp = proto == 17u, tcp = proto == 6u;
  const bool icmp = (v4 && proto == 1u) || (v6 && proto == 58u);
  const uint32_t mtype = R[18] & 0xffffu;
  const bool echo = v4 ? (mtype == 8u || mtype == 0u) : (mtype == 128u || mtype == 129u);
  const bool chain = (v4 || v6) && (udp || tcp || (icmp && echo));
  const uint32_t l3len = v6 ? 40u : 20u, l4hdr = udp ? 8u : (tcp ? 20u : 4u);
  const uint32_t H = 14u + l3len + l4hdr, L = H + plen, hn = (l3len + l4hdr) >> 2;
  uint32_t st = CGTX_BUILD_OK;
  if (!chain || (icmp && plen < 4u)) st = CGTX_BUILD_BAD_RECORD;
  else if ((uint64_t)poff + plen > (uint64_t)a.pay_len) st = CGTX_BUILD_BAD_PAYLOAD;
  else if (L >= a.room || (uint64_t)ooff + L > (uint64_t)a.out_arena_len) st = CGTX_BUILD_NO_ROOM;
  const bool live = in && st == CGTX_BUILD_OK;

  Span k;
  k.d = ooff + pa_o;
  k.end = k.d + L;
  k.dpay = k.d + H;
  k.plen = live ? plen : 0u;
  k.sbase = poff + pa_p - k.dpay;
  const uint32_t A0 = k.d & ~15u;
  k.nch = live ? (k.end - A0 + 15u) >> 4 : 0u;

  // ---- payload: the team's chunks ------------------------------------------
  uint64_t acc = 0;
  u32x4 held0 = {0u, 0u, 0u, 0u}, held1 = {0u, 0u, 0u, 0u};
  const bool any_pay = __ballot(k.plen != 0u) != 0ull;  // wave-uniform
  if (any_pay) {
    const bool last = g == kTeam - 1u;
    held0 = pay_chunk(prs, pay_len, k, A0 + 16u * g, live && g <= k.nch, last, acc);
    held1 = pay_chunk(prs, pay_len, k, A0 + 16u * (g + kTeam), live && g + kTeam <= k.nch, last, acc);
    // the wave's longest team decides the trip count (uniform: pay_chunk shuffles)
    uint32_t top = k.nch < kTeamChunks ? k.nch : kTeamChunks;
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) {
      const uint32_t o = __shfl_xor(top, dlt);
      top = o > top ? o : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);
    for (uint32_t c0 = 2u * kTeam; c0 < top; c0 += kTeam) {
      const uint32_t c = c0 + g, ao = A0 + 16u * c;
      const u32x4 v = pay_chunk(prs, pay_len, k, ao, live && c <= k.nch && c < kTeamChunks, last, acc);
      if (c < k.nch && c < kTeamChunks) store_chunk(ors, ao, v, k.d, k.end);
    }
  }
  uint32_t psum = fold64(acc);
  psum += __shfl_xor(psum, 1);
  psum += __shfl_xor(psum, 2);
  // ---- long payloads: the rest of each, over the wave -----------------------
  unsigned long long longs = __ballot(g == 0u && k.nch > kTeamChunks);
  while (longs) {
    const int src = __builtin_ctzll(longs);
    longs &= longs - 1ull;
    Span w;
    w.d = __shfl(k.d, src);
    w.end = __shfl(k.end, src);
    w.dpay = __shfl(k.dpay, src);
    w.plen = __shfl(k.plen, src);
    w.sbase = __shfl(k.sbase, src);
    w.nch = __builtin_amdgcn_readfirstlane(__shfl(k.nch, src));
    const uint32_t wA0 = w.d & ~15u;
    uint64_t wacc = 0;
    for (uint32_t c0 = kTeamChunks; c0 < w.nch; c0 += 64u) {
      const uint32_t c = c0 + lane, ao = wA0 + 16u * c;
      const u32x4 v = pay_chunk(prs, pay_len, w, ao, c <= w.nch, lane == 63u, wacc);
      if (c < w.nch) store_chunk(ors, ao, v, w.d, w.end);
    }
    uint32_t ws = fold64(wacc);
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) ws += __shfl_xor(ws, dlt);
    if ((lane >> 2) == ((uint32_t)src >> 2)) psum += ws;
  }
  psum = fold32(psum);
  if (k.dpay & 1u) psum = swap16(psum);  // address parity -> payload parity

  // ---- the header, in registers ---------------------------------------------
  const uint32_t dscp = (R[4] >> 16) & 0xffu, ecn = R[4] >> 24;
  const uint32_t ttl = (R[6] >> 8) & 0xffu;
  // Ethernet (dst, src, ether_type), as the dwords of frame bytes -2..13
  const uint32_t et = v6 ? 0xdd86u : 0x0008u;  // 0x86DD / 0x0800 on the wire
  const u32x4 E = {R[0] << 16, (R[0] >> 16) | (R[1] << 16), (R[1] >> 16) | (R[2] << 16),
                   (R[2] >> 16) | (et << 16)};
  // Ipv4 (v4.rs:594-608 defaults, setters, reconcile :486-489)
  uint32_t T4[5];
  {
    const uint32_t fl = R[6] & 0xffu;
    const uint32_t ff = ((fl & 1u) ? 0x4000u : 0u) | ((fl & 2u) ? 0x2000u : 0u) | ((R[6] >> 16) & 0x1fffu);
    T4[0] = 0x45u | ((((dscp << 2) & 0xfcu) | (ecn & 3u)) << 8) | (swap16(L - 14u) << 16);
    T4[1] = swap16(R[5] >> 16) | (swap16(ff) << 16);
    T4[2] = ttl | (proto << 8);
    T4[3] = R[10];
    T4[4] = R[14];
    const uint64_t s = (uint64_t)T4[0] + T4[1] + T4[2] + T4[3] + T4[4];
    T4[2] |= (~fold64(s) & 0xffffu) << 16;
  }
  // Ipv6 (v6/mod.rs:453-462, :331-334)
  const uint32_t w6 = (6u << 28) | ((dscp << 22) & 0x0fc00000u) | ((ecn << 20) & 0x00300000u) |
                      (R[8] & 0x000fffffu);
  const uint32_t T6_0 = be32(w6), T6_1 = swap16(L - 54u) | (proto << 16) | (ttl << 24);
  // L4
  const uint32_t l4len = L - 14u - l3len;
  uint32_t U[5] = {0u, 0u, 0u, 0u, 0u};
  U[0] = icmp ? ((mtype & 0xffu) | (((R[18] >> 16) & 0xffu) << 8))
              : (swap16(R[18] & 0xffffu) | (swap16(R[18] >> 16) << 16));
  if (udp) U[1] = swap16(l4len);
  if (tcp) {
    U[1] = be32(R[20]);
    U[2] = be32(R[21]);
    U[3] = (((R[22] & 0xfu) << 4) | ((R[22] >> 16) & 1u)) | (((R[22] >> 8) & 0xffu) << 8) |
           (swap16(R[19] & 0xffffu) << 16);
    U[4] = swap16(R[23] & 0xffffu) << 16;
  }
  uint64_t s4 = (uint64_t)U[0] + U[1] + U[2] + U[3] + U[4] + psum;
  if (!(icmp && v4)) {  // pseudo-header (checksum.rs:93-128); Icmpv4 has none
    s4 += (uint64_t)R[10] + R[14] + (proto << 8) + swap16(l4len);
    if (v6) s4 += (uint64_t)R[11] + R[12] + R[13] + R[15] + R[16] + R[17];
  }
  uint32_t ck = ~fold64(s4) & 0xffffu;
  if (udp && ck == 0u) ck = 0xffffu;  // Udp::set_checksum (udp.rs:132-141)
  if (udp) U[1] |= ck << 16;
  else if (tcp) U[4] |= ck;
  else U[0] |= ck << 16;

  if (g == 0u) {
    uint32_t *h = hdr[team];
    h[0] = E[0];
    h[1] = E[1];
    h[2] = E[2];
    h[3] = E[3];
    h[4] = v6 ? T6_0 : T4[0];
    h[5] = v6 ? T6_1 : T4[1];
    h[6] = v6 ? R[10] : T4[2];
    h[7] = v6 ? R[11] : T4[3];
    h[8] = v6 ? R[12] : T4[4];
    if (v6) {
      h[9] = R[13];
      h[10] = R[14];
      h[11] = R[15];
      h[12] = R[16];
      h[13] = R[17];
    }
    const uint32_t u0 = 4u + (l3len >> 2);
#pragma unroll
    for (int j = 0; j < 5; ++j) h[u0 + j] = U[j];
  }
  __syncthreads();

  // ---- the first eight chunks: header part | payload part --------------------
  const uint32_t s = (0u - (k.d + 14u)) & 3u;  // (chunk - L3 start) & 3
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const uint32_t c = g + kTeam * half, ao = A0 + 16u * c;
    if (c >= k.nch) continue;
    const int q0 = (int)(ao - (k.d + 14u)) >> 2;  // dword of the L3-relative stream
    uint32_t Hw[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int q = q0 + j;
      const int idx = q + 4 < 0 ? 0 : (q + 4 > (int)kHdrDw - 1 ? (int)kHdrDw - 1 : q + 4);
      const uint32_t x = hdr[team][idx];
      Hw[j] = (q >= -4 && q < (int)hn) ? x : 0u;
    }
    const u32x4 p = half ? held1 : held0;
    u32x4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = __builtin_amdgcn_alignbyte(Hw[t + 1], Hw[t], s) | p[t];
    store_chunk(ors, ao, v, k.d, k.end);
  }
  if (g == 0u && in) {
    a.out_len[i] = (uint16_t)(live ? L : 0u);
    if (a.status) a.status[i] = (uint8_t)st;
  }
}

}  // namespace

hipError_t launch_build(const BuildArgs &a, hipStream_t s) {
  const dim3 grid((a.n + kTeamsPerBlock - 1) / kTeamsPerBlock);
  hipLaunchKernelGGL(build_kernel, grid, dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace cgpu
