/* Plain-C (C11, no HIP) consumer of include/capsule_gpu_tx.h, the
 * transmit-side extension: the stand-in for the bindgen step with the
 * allow-list entry `cgtx_.*`.  It compiles the header as C, pins the layout
 * of its two descriptor structs and its status values, links every cgtx_
 * entry point through a pointer of its exact C type and runs the host-only
 * ones.  Built and run by tests/test_abi_tx.py with gcc -std=c11 -Wall
 * -Wextra -Werror -pedantic. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "capsule_gpu_tx.h"

_Static_assert(CGTX_ABI_VERSION == 1, "extension version");
_Static_assert(sizeof(cgtx_payload) == 32, "cgtx_payload size");
_Static_assert(offsetof(cgtx_payload, arena_len) == 8, "cgtx_payload.arena_len");
_Static_assert(offsetof(cgtx_payload, off) == 16, "cgtx_payload.off");
_Static_assert(offsetof(cgtx_payload, len) == 24, "cgtx_payload.len");
_Static_assert(sizeof(cgtx_frames_out) == 40, "cgtx_frames_out size");
_Static_assert(offsetof(cgtx_frames_out, off) == 16, "cgtx_frames_out.off");
_Static_assert(offsetof(cgtx_frames_out, len) == 24, "cgtx_frames_out.len");
_Static_assert(offsetof(cgtx_frames_out, status) == 32, "cgtx_frames_out.status");
_Static_assert(CGTX_BUILD_OK == 0 && CGTX_BUILD_BAD_RECORD == 1 && CGTX_BUILD_NO_ROOM == 2 &&
                   CGTX_BUILD_BAD_PAYLOAD == 3, "build status values");
/* the receive side's header comes along unchanged */
_Static_assert(sizeof(cgpu_hdr_record) == 96, "cgpu_hdr_record size");
_Static_assert(CGPU_ABI_VERSION == 6, "receive-side version");

static int (*const p_build)(cgpu_ctx *, const cgpu_hdr_record *, uint32_t, const cgtx_payload *,
                            const cgtx_frames_out *, uint32_t, void *) = cgtx_build_batch;
static int (*const p_defaults)(uint32_t, uint32_t, cgpu_hdr_record *) = cgtx_hdr_defaults;
static const char *(*const p_str)(int) = cgtx_build_status_str;
static int (*const p_version)(void) = cgtx_abi_version;

int main(void) {
  cgpu_hdr_record r;
  int entry_points = 0;
  if (p_version() != CGTX_ABI_VERSION) return 1;
  ++entry_points;
  if (p_defaults(4, 6, &r) != 0 || r.version != 4 || r.ihl != 5 || r.ttl != 64 ||
      r.protocol != 6 || r.data_offset != 5)
    return 2;
  if (p_defaults(5, 6, &r) != CGPU_EINVAL || cgpu_last_error() != CGPU_EINVAL) return 3;
  ++entry_points;
  if (strcmp(p_str(CGTX_BUILD_NO_ROOM), "buffer not resized") != 0) return 4;
  ++entry_points;
  /* argument checks only: nothing is launched */
  if (p_build(NULL, NULL, 0, NULL, NULL, 2048, NULL) != CGPU_EINVAL) return 5;
  ++entry_points;
  printf("abi tx ok: %d entry points, version %d\n", entry_points, p_version());
  return 0;
}
