/*
 * capsule_gpu_srv6.h -- segment-routing extension of the C ABI: push,
 * replace, advance and remove a SegmentRouting<Ipv6> header (SRH) on frames
 * already in device memory, lengths and checksums reconciled, one launch.
 *
 * Why a third header.  include/capsule_gpu.h (CGPU_ABI_VERSION, the
 * binding's EXPORTS list) and include/capsule_gpu_tx.h (CGTX_ABI_VERSION,
 * TX_EXPORTS) are pinned byte for byte by tests/test_abi.py,
 * tests/test_abi_tx.py, tests/c/abi_check.c and tests/c/abi_tx_check.c.
 * Frame editing is therefore a separate, separately versioned surface: this
 * header, the prefix cgsr_ / CGSR_, the version CGSR_ABI_VERSION, exported
 * from the same libcapsule_gpu.so and bound through the binding's SR_EXPORTS
 * list.  It is pinned the same way by tests/test_abi_srv6.py and
 * tests/c/abi_srv6_check.c.  Bind it with a third allow-list entry `cgsr_.*`.
 *
 * Conventions are those of capsule_gpu.h: 0 or a negative errno-style code
 * (CGPU_E*, also kept for cgpu_last_error()), per-packet outcomes in a status
 * byte, plain device pointers and sizes, `void *stream` = a hipStream_t,
 * caller memory only borrowed.
 */
#ifndef CAPSULE_GPU_SRV6_H
#define CAPSULE_GPU_SRV6_H

#include "capsule_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CGSR_ABI_VERSION 1

/* One segment list and the header fields that go with it (device memory). */
typedef struct cgsr_policy {
  uint32_t seg_first;    /* index of segments[0] in the segment arena          */
  uint8_t n_segments;    /* 1..127 (srh.rs:210-233: `as u8`, hdr_ext_len = 2n) */
  uint8_t segments_left; /* SegmentRouting::set_segments_left (srh.rs:162-164) */
  uint16_t tag;          /* SegmentRouting::set_tag (srh.rs:187-189), host order */
  uint8_t flags;         /* CGSR_P_*                                           */
  uint8_t pad[7];
} cgsr_policy;

/* Ipv6::set_dst(segments[segments_left]) after the edit, as the remark at
 * srh.rs:159-160 advises.                                                   */
#define CGSR_P_SET_DST 1u
/* segments[0] is not taken from the arena but is the packet's dst() before
 * the edit (Ipv6::dst() for ENCAP, the old SRH's segments[0] for SET), so
 * the L4 pseudo-header (srh.rs:456-470) does not change.                    */
#define CGSR_P_FINAL_FROM_PACKET 2u

typedef struct cgsr_policies {
  const cgsr_policy *policy;
  uint32_t n_policies;
  const uint8_t *segments;   /* 16 B each, wire order, any alignment */
  uint32_t n_segments_total; /* <= 0x0FFF0000 */
} cgsr_policies;

enum cgsr_op {
  CGSR_OP_NONE = 0,  /* the frame, unchanged                                   */
  CGSR_OP_ENCAP = 1, /* Ipv6::push::<SegmentRouting> + set_segments + setters  */
  CGSR_OP_SET = 2,   /* set_segments, set_segments_left, set_tag on an SRH     */
  CGSR_OP_END = 3,   /* segments_left -= 1, Ipv6::set_dst(segments[that])      */
  CGSR_OP_DECAP = 4  /* SegmentRouting::remove                                 */
};

/* Per-packet status: enum cgpu_pkt_status for what the parses and the resize
 * say, and from 64 up (never a cgpu_pkt_status value):                      */
enum cgsr_status {
  CGSR_BAD_OP = 64,           /* op[i] is no enum cgsr_op                     */
  CGSR_BAD_POLICY = 65,       /* see below                                    */
  CGSR_NOT_ROUTING = 66,      /* "not an IPv6 routing packet." (srh.rs:300-303) */
  CGSR_NO_SEGMENTS_LEFT = 67, /* END with segments_left == 0                  */
  CGSR_BAD_SEGMENTS_LEFT = 68 /* END: segments_left - 1 > last_entry          */
};

/* Edit the n frames of `in` into `out_arena`, one kernel launch, asynchronous
 * on `stream`.  Frame i is read at in->off[i] (in->len[i] bytes), edited as
 * op[i] says with policy pol->policy[policy_idx[i]], and written at
 * out_off[i]; out_len[i] is its new data_len and status[i] (optional) its
 * outcome.  All offsets have any byte alignment and frames may abut.
 *
 * Offsets: eth_len is 14, 18 or 22 from the VLAN-aware Ethernet parse
 * (ethernet.rs:164-192, 279-300); x = eth_len + 40; T = room - in->len[i] is
 * Mbuf::tailroom with `room` bytes of data room (as in cgtx_build_batch).
 *
 * Every op but NONE does parse::<Ethernet>() and parse::<Ipv6>(); a failure
 * is that parse's cgpu_pkt_status (ETH_*, NOT_IPV6, L3_*).  SET, END and
 * DECAP then do parse::<SegmentRouting<Ipv6>>() (srh.rs:299-327):
 * next_header != 43 is CGSR_NOT_ROUTING, a short header or list
 * CGPU_PKT_EXT_BAD_OFFSET / _OUT_OF_BUFFER, hdr_ext_len == 0 or
 * != 2 * (last_entry + 1) CGPU_PKT_SRH_INCONSISTENT.
 *
 * ENCAP  Ipv6::push::<SegmentRouting> (srh.rs:342-370), then set_segments
 *        (:210-233), set_segments_left, set_tag and, with CGSR_P_SET_DST,
 *        Ipv6::set_dst.  8 + 16 n bytes are inserted at x: {next_header = the
 *        old ipv6.next_header, hdr_ext_len 2n, routing_type 4, segments_left,
 *        last_entry n - 1, flags 0, tag} and the list; ipv6.next_header := 43.
 *        What follows the IPv6 header is not looked at.  Mbuf::extend
 *        (mbuf.rs:225-247) needs len < tailroom for the push (24) and for the
 *        resize (16 (n - 1), none when n == 1): 8 + 16 n < T, else
 *        CGPU_PKT_NOT_RESIZED.
 * SET    set_segments on the parsed SRH, then set_segments_left and set_tag
 *        (and set_dst with the flag).  The list is resized by
 *        16 (n - old_n) at x + 8; a grow needs delta < T, a shrink always
 *        fits, equal counts resize nothing.  hdr_ext_len and last_entry are
 *        rewritten; routing_type, flags and next_header are kept.
 * END    takes no policy.  segments_left == 0: CGSR_NO_SEGMENTS_LEFT;
 *        segments_left - 1 > last_entry: CGSR_BAD_SEGMENTS_LEFT (the
 *        reference would index out of range).  Else set_segments_left(sl - 1)
 *        and Ipv6::set_dst(segments[sl - 1]); the length is unchanged.
 * DECAP  SegmentRouting::remove (srh.rs:384-391): 8 + 16 (last_entry + 1)
 *        bytes leave at x, ipv6.next_header := srh.next_header; the IPv6
 *        destination is not touched.
 * NONE   the frame goes to its out slot unchanged: no parse, no reconcile.
 *
 * Reconcile.  After every op but NONE, reconcile_all() (packets/mod.rs:
 * 297-300) runs from the deepest layer the one-extension-level parse of the
 * output frame reaches under `flags` (CGPU_F_ACCEPT_UDP | _TCP | _ICMP; none
 * of them means UDP | TCP; IPv6 and CGPU_F_V6_EXT are implied): if that L4
 * header fits, Udp length and checksum (0 stored as 0xFFFF), Tcp or Icmpv6
 * checksum, with the output's segments[0] as the pseudo-header's destination
 * behind a routing header; then Ipv6::reconcile (payload_length := len - x).
 * If no L4 layer is reached (a next header outside the accept set, a second
 * extension level, a short L4 header) only the IPv6 layer is reconciled.
 * These are the rules of cgpu_reconcile.
 *
 * CGSR_BAD_OP: op[i] > 4.  CGSR_BAD_POLICY (ENCAP and SET only; END and
 * DECAP ignore policy_idx): policy_idx is NULL or policy_idx[i] >=
 * n_policies, n_segments is 0 or > 127, seg_first + n_segments >
 * n_segments_total, or CGSR_P_SET_DST with segments_left >= n_segments.  A
 * frame that does not fit the out arena (out_off[i] + new_len >
 * out_arena_len) is CGPU_PKT_NOT_RESIZED, under every op.  Precedence:
 * BAD_OP, parse errors, BAD_POLICY, NOT_RESIZED, the END errors.  A packet
 * whose status is not CGPU_PKT_OK has out_len[i] = 0 and no byte of the out
 * arena is written for it.  Frames of one call must lie inside the in arena
 * and their out slots must not overlap each other (not checked).
 *
 * Call-level errors (checked before the context or the device is touched):
 * CGPU_EINVAL for a NULL ctx, in, in->arena, in->off, in->len, op,
 * out_arena, out_off or out_len; a non-NULL policy_idx with a NULL pol,
 * pol->policy or pol->segments; in->n > CGPU_MAX_BATCH; room == 0 or
 * room > 65536; an arena longer than 0xFFFF0000; n_segments_total >
 * 0x0FFF0000; an out range that overlaps the in range.  in->n == 0 then
 * returns 0 without a launch.                                              */
int cgsr_apply(cgpu_ctx *ctx, const cgpu_batch *in, const uint8_t *op, const uint32_t *policy_idx,
               const cgsr_policies *pol, uint32_t flags, uint32_t room, uint8_t *out_arena,
               uint64_t out_arena_len, const uint32_t *out_off, uint16_t *out_len,
               uint8_t *status, void *stream);

/* Text of a per-packet status: cgpu_pkt_status_str below 64, the CGSR_ ones
 * above, "unknown status" outside both tables.                             */
const char *cgsr_status_str(int status);
int cgsr_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CAPSULE_GPU_SRV6_H */
