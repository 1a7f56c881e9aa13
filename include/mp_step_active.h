/* mp_step_active.h — stepping some of the worlds: K steps in one submission under a device mask
 * that says, per step and per world, whether the world runs, as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpStepActive request that mp_restore carries (mp_engine.h documents the semantics, the
 * carry rule for the rows of a skipped step and the refusals).  Same return codes as every entry
 * point. */
#ifndef MP_STEP_ACTIVE_H_
#define MP_STEP_ACTIVE_H_

#include <string.h>

#include "mp_engine.h"

/* actions_device, rows: as mp_step_trajectory takes them (mp_step_trajectory.h).  active_device:
 * uint8 [steps][N], two steps' rows active_step_bytes apart (0: the same [N] row every step);
 * world w runs step k where active_device[k][w] != 0 and is not touched otherwise.
 * Stream-ordered, no synchronisation. */
static inline int mp_step_many_active(MpEngine* eng, const int32_t* actions_device, int32_t steps,
                                      int32_t fields, uint64_t actions_step_bytes,
                                      const MpStepRow* rows, int32_t num_rows,
                                      const uint8_t* active_device, uint64_t active_step_bytes) {
  MpStepActive r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.steps = steps;
  r.fields = fields;
  r.num_rows = num_rows;
  r.actions = actions_device;
  r.actions_step_bytes = actions_step_bytes;
  r.rows = rows;
  r.active = active_device;
  r.active_step_bytes = active_step_bytes;
  return mp_restore(eng, &r, sizeof r);
}

/* One step of the worlds active_device (uint8 [N]) selects: actions_device is int32 [N][P]
 * (fields = 0) or [N][P][A] (fields = 1). */
static inline int mp_step_active(MpEngine* eng, const int32_t* actions_device, int32_t fields,
                                 const uint8_t* active_device) {
  return mp_step_many_active(eng, actions_device, 1, fields, 0, NULL, 0, active_device, 0);
}

#endif /* MP_STEP_ACTIVE_H_ */
