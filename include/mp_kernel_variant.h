/* mp_kernel_variant.h — which frame kernels an engine runs, or a pack would get, as a plain C
 * function.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and this wrapper
 * builds the MpKernelVariant request that mp_snapshot carries (mp_engine.h documents the
 * semantics).  Returns MP_KERNEL_GENERIC or MP_KERNEL_STOCK, or a negative MP_ERR_*. */
#ifndef MP_KERNEL_VARIANT_H_
#define MP_KERNEL_VARIANT_H_

#include <string.h>

#include "mp_engine.h"

/* eng != NULL: what `eng` runs.  eng == NULL: what mp_create(pack, pack_len, cfg) would select,
 * decided on the host alone; `fields` (NULL, or fields_cap bytes) takes the folded fields' text. */
static inline int mp_kernel_variant(MpEngine* eng, const void* pack, uint64_t pack_len,
                                    const MpConfig* cfg, char* fields, uint64_t fields_cap) {
  MpKernelVariant r;
  int rc;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  r.fields = fields;
  r.fields_cap = fields_cap;
  rc = mp_snapshot(eng, &r, sizeof r);
  return rc != MP_OK ? rc : r.variant;
}

#endif /* MP_KERNEL_VARIANT_H_ */
