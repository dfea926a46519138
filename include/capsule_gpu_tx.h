/*
 * capsule_gpu_tx.h -- transmit-side extension of the C ABI: packet
 * construction on the device (Mbuf::new + push + setters + reconcile_all).
 *
 * Why a second header.  include/capsule_gpu.h, CGPU_ABI_VERSION, the
 * binding's EXPORTS list, the status enum and every struct of the receive
 * side are pinned byte for byte by tests/test_abi.py and tests/c/abi_check.c
 * (28 entry points, CGPU_PKT_STATUS_COUNT == 20, sizeof(cgpu_parse_out) ==
 * 40).  Construction is therefore a separate, separately versioned surface:
 * this header, the prefix cgtx_ / CGTX_, the version CGTX_ABI_VERSION,
 * exported from the same libcapsule_gpu.so and bound through the binding's
 * TX_EXPORTS list.  It is pinned the same way by tests/test_abi_tx.py and
 * tests/c/abi_tx_check.c.  Bind it with a second allow-list entry `cgtx_.*`.
 *
 * Conventions are those of capsule_gpu.h: 0 or a negative errno-style code
 * (CGPU_E*, also kept for cgpu_last_error()), per-packet outcomes in a status
 * byte, plain pointers and sizes, `void *stream` = a hipStream_t, caller
 * memory only borrowed.
 */
#ifndef CAPSULE_GPU_TX_H
#define CAPSULE_GPU_TX_H

#include "capsule_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CGTX_ABI_VERSION 1

/* Optional payload bytes, one range per packet.  All device pointers; a NULL
 * struct or a NULL arena means no packet has a payload.                    */
typedef struct cgtx_payload {
  const uint8_t *arena;
  uint64_t arena_len;  /* <= 0xFFFF0000 */
  const uint32_t *off; /* [n] byte offset of packet i's payload, any alignment */
  const uint16_t *len; /* [n] its length                                   */
} cgtx_payload;

/* Where the frames go.  All device pointers.                               */
typedef struct cgtx_frames_out {
  uint8_t *arena;
  uint64_t arena_len;  /* <= 0xFFFF0000 */
  const uint32_t *off; /* [n] where frame i goes, any byte alignment        */
  uint16_t *len;       /* [n] data_len written, 0 if not built              */
  uint8_t *status;     /* [n] optional, enum cgtx_build_status              */
} cgtx_frames_out;

enum cgtx_build_status {
  CGTX_BUILD_OK = 0,
  CGTX_BUILD_BAD_RECORD = 1,  /* no such push chain, or an ICMP body under 4 B */
  CGTX_BUILD_NO_ROOM = 2,     /* Mbuf::extend NotResized, or past the out arena */
  CGTX_BUILD_BAD_PAYLOAD = 3  /* payload range past its arena                */
};

/* Build n frames from header records (the inverse of the parse's field
 * extraction), one kernel launch, asynchronous on `stream`.
 *
 * Packet i is Mbuf::new(); push::<Ethernet>(); push::<Ipv4 | Ipv6>();
 * push::<Udp | Tcp | EchoRequest | EchoReply>(); the setters named below;
 * the payload; reconcile_all().
 *
 * Chain: rec.version 4 / 6 selects Ipv4 / Ipv6.  rec.protocol 17 is Udp, 6 is
 * Tcp, 1 under IPv4 and 58 under IPv6 is an ICMP echo message whose msg_type
 * is rec.src_port and whose code is the low byte of rec.dst_port (the
 * parse's convention); msg_type must be 8 or 0 (IPv4), 128 or 129 (IPv6): the
 * reference cannot push a generic ICMP header (icmp/v4/mod.rs:228).
 * Ethernet::try_push writes 14 bytes (ethernet.rs:308-325): no VLAN tag is
 * built, rec.vlan and rec.eth_len are ignored.  Anything else: BAD_RECORD.
 *
 * Taken from the record (the fields the reference has setters for):
 *   Ethernet  dst_mac, src_mac
 *   Ipv4      dscp, ecn, identification, ip_flags, fragment_offset, ttl,
 *             src_ip[0..4], dst_ip[0..4]
 *   Ipv6      dscp, ecn, flow_label, ttl (hop limit), src_ip, dst_ip
 *   Udp       src_port, dst_port
 *   Tcp       src_port, dst_port, seq_no, ack_no, data_offset (the nibble as
 *             given; the header is the fixed 20 B of tcp.rs), ns, tcp_flags,
 *             udp_length_or_window, urgent_pointer
 *   ICMP echo msg_type, code; the message body (identifier, sequence number,
 *             data) is the payload, so a payload under 4 B is BAD_RECORD
 * Derived (the record's values are ignored): ether_type, version_ihl = 0x45,
 * protocol / next_header, total_length / payload_length and the IPv4 header
 * checksum (ip/v4.rs:486-489, ip/v6/mod.rs:331-334), Udp length (udp.rs:
 * 350-354) and the L4 checksum (udp.rs:204-219 with 0 stored as 0xFFFF,
 * tcp.rs:619-621, icmp/v4/mod.rs:246 without a pseudo-header, icmp/v6/
 * mod.rs:260 with the IPv6 pseudo-header and protocol 58): the rules
 * cgpu_reconcile implements.
 *
 * Room: every push is an Mbuf::extend, which needs len < tailroom
 * (mbuf.rs:225-233); with `room` bytes of data room the pushes' lengths add
 * up, so the last one binds: a frame is built only if frame_len < room.  It
 * must also fit the arena: out.off[i] + frame_len <= out.arena_len.
 * Otherwise NO_ROOM.  pay.off[i] + pay.len[i] > pay.arena_len is
 * BAD_PAYLOAD, and nothing is read through it.  Precedence when several
 * apply: BAD_RECORD, BAD_PAYLOAD, NO_ROOM.  A packet that is not built has
 * out.len[i] = 0 and no byte of the out arena is written for it.  Frames of
 * one call must not overlap each other (not checked).
 *
 * Call-level errors (checked before the context or the device is touched):
 * CGPU_EINVAL for a NULL ctx, rec, out, out->arena, out->off or out->len;
 * n > CGPU_MAX_BATCH; room == 0 or room > 65536; an arena longer than
 * 0xFFFF0000; a payload arena without off / len; an out arena range that
 * overlaps the payload arena range.  n == 0 then returns 0 without a launch. */
int cgtx_build_batch(cgpu_ctx *ctx, const cgpu_hdr_record *rec, uint32_t n,
                     const cgtx_payload *pay, const cgtx_frames_out *out, uint32_t room,
                     void *stream);

/* Host only: fill *rec with the reference's Default impls of the chain
 * (version, protocol): version; ihl = 5 under IPv4 (Ipv4Header::default,
 * v4.rs:594-608; IPv6 has none, v6/mod.rs:453-462); ttl = 64
 * (DEFAULT_IP_TTL, ip/mod.rs:33); protocol; data_offset = 5 for TCP
 * (tcp.rs:648-661); everything else zero.  An ICMP record's msg_type is
 * therefore 0: an echo reply under IPv4, and to be set (128 / 129) under
 * IPv6.  CGPU_EINVAL for a NULL rec or a pair cgtx_build_batch cannot build. */
int cgtx_hdr_defaults(uint32_t version, uint32_t protocol, cgpu_hdr_record *rec);

const char *cgtx_build_status_str(int status);
int cgtx_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CAPSULE_GPU_TX_H */
