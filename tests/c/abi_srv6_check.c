/* Plain-C (C11, no HIP) consumer of include/capsule_gpu_srv6.h, the
 * segment-routing extension: the stand-in for the bindgen step with the
 * allow-list entry `cgsr_.*`.  It compiles the header as C, pins the layout
 * of its structs and its op / status values, links every cgsr_ entry point
 * through a pointer of its exact C type and runs the host-only ones.  Built
 * and run by tests/test_abi_srv6.py with gcc -std=c11 -Wall -Wextra -Werror
 * -pedantic. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "capsule_gpu_srv6.h"

_Static_assert(CGSR_ABI_VERSION == 1, "extension version");
_Static_assert(sizeof(cgsr_policy) == 16, "cgsr_policy size");
_Static_assert(offsetof(cgsr_policy, n_segments) == 4, "cgsr_policy.n_segments");
_Static_assert(offsetof(cgsr_policy, segments_left) == 5, "cgsr_policy.segments_left");
_Static_assert(offsetof(cgsr_policy, tag) == 6, "cgsr_policy.tag");
_Static_assert(offsetof(cgsr_policy, flags) == 8, "cgsr_policy.flags");
_Static_assert(sizeof(cgsr_policies) == 32, "cgsr_policies size");
_Static_assert(offsetof(cgsr_policies, n_policies) == 8, "cgsr_policies.n_policies");
_Static_assert(offsetof(cgsr_policies, segments) == 16, "cgsr_policies.segments");
_Static_assert(offsetof(cgsr_policies, n_segments_total) == 24, "cgsr_policies.n_segments_total");
_Static_assert(CGSR_OP_NONE == 0 && CGSR_OP_ENCAP == 1 && CGSR_OP_SET == 2 && CGSR_OP_END == 3 &&
                   CGSR_OP_DECAP == 4, "op values");
_Static_assert(CGSR_BAD_OP == 64 && CGSR_BAD_POLICY == 65 && CGSR_NOT_ROUTING == 66 &&
                   CGSR_NO_SEGMENTS_LEFT == 67 && CGSR_BAD_SEGMENTS_LEFT == 68, "status values");
_Static_assert((int)CGSR_BAD_OP >= (int)CGPU_PKT_STATUS_COUNT, "no collision with cgpu_pkt_status");
_Static_assert(CGSR_P_SET_DST == 1u && CGSR_P_FINAL_FROM_PACKET == 2u, "policy flags");
/* the other two headers' versions did not move */
_Static_assert(CGPU_ABI_VERSION == 6, "receive-side version");

static int (*const p_apply)(cgpu_ctx *, const cgpu_batch *, const uint8_t *, const uint32_t *,
                            const cgsr_policies *, uint32_t, uint32_t, uint8_t *, uint64_t,
                            const uint32_t *, uint16_t *, uint8_t *, void *) = cgsr_apply;
static const char *(*const p_str)(int) = cgsr_status_str;
static int (*const p_version)(void) = cgsr_abi_version;

int main(void) {
  int entry_points = 0;
  if (p_version() != CGSR_ABI_VERSION) return 1;
  ++entry_points;
  if (strcmp(p_str(CGSR_NOT_ROUTING), "not an IPv6 routing packet.") != 0) return 2;
  if (strcmp(p_str(CGPU_PKT_NOT_RESIZED), cgpu_pkt_status_str(CGPU_PKT_NOT_RESIZED)) != 0) return 3;
  if (strcmp(p_str(63), "unknown status") != 0) return 4;
  ++entry_points;
  /* argument checks only: nothing is launched */
  if (p_apply(NULL, NULL, NULL, NULL, NULL, 0, 2048, NULL, 0, NULL, NULL, NULL, NULL) != CGPU_EINVAL ||
      cgpu_last_error() != CGPU_EINVAL)
    return 5;
  ++entry_points;
  printf("abi srv6 ok: %d entry points, version %d\n", entry_points, p_version());
  return 0;
}
