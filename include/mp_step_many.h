/* mp_step_many.h — K steps of every world in one submission, as a plain C function.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and this wrapper
 * builds the MpStepMany request that mp_restore carries (mp_engine.h documents the semantics,
 * the maximum K and the refusals).  Same return codes as every entry point. */
#ifndef MP_STEP_MANY_H_
#define MP_STEP_MANY_H_

#include <string.h>

#include "mp_engine.h"

/* actions_device: int32 [steps][N][P] (fields = 0) or [steps][N][P][A] (fields = 1), two steps'
 * blocks actions_step_bytes apart (0: the same block every step).  per_step / per_step_bytes:
 * the five optional per-step buffers (REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT, EVENTS) and
 * the distances between their rows; both may be NULL when none is wanted.  Stream-ordered, no
 * synchronisation. */
static inline int mp_step_many(MpEngine* eng, const int32_t* actions_device, int32_t steps,
                               int32_t fields, uint64_t actions_step_bytes,
                               void* const per_step[5], const uint64_t per_step_bytes[5]) {
  MpStepMany r;
  int i;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.steps = steps;
  r.fields = fields;
  r.actions = actions_device;
  r.actions_step_bytes = actions_step_bytes;
  for (i = 0; i < 5; ++i) {
    r.per_step[i] = per_step ? per_step[i] : NULL;
    r.per_step_bytes[i] = per_step_bytes ? per_step_bytes[i] : 0;
  }
  return mp_restore(eng, &r, sizeof r);
}

#endif /* MP_STEP_MANY_H_ */
