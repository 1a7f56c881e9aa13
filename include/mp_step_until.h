/* mp_step_until.h — stopping worlds inside a K-step submission: a world that ends its episode, or
 * is paid, stops there for the rest of the request, and the request hands back how many steps each
 * world ran and the discounted sum of its rewards over them, as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpStepUntil request that mp_restore carries (mp_engine.h documents the semantics, the
 * defining identity with the loop of masked single steps, and the refusals).  Same return codes as
 * every entry point. */
#ifndef MP_STEP_UNTIL_H_
#define MP_STEP_UNTIL_H_

#include <string.h>

#include "mp_engine.h"

/* actions_device, rows, active_device, active_step_bytes: as mp_step_many_active takes them
 * (mp_step_active.h); active_device may be NULL for "every world-step is active".  stop: MP_STOP_*
 * bits.  stopped_device: uint8 [N], read (non-zero: the world does not run) and written (the reason
 * bits of a world that stops), or NULL.  ran_device: int32 [N] or NULL.  returns_device: float64
 * [N][P] or NULL, the sum of gamma^j * REWARD over the steps j = 0, 1, .. that ran.
 * Stream-ordered, no synchronisation. */
static inline int mp_step_many_until(MpEngine* eng, const int32_t* actions_device, int32_t steps,
                                     int32_t fields, uint64_t actions_step_bytes,
                                     const MpStepRow* rows, int32_t num_rows,
                                     const uint8_t* active_device, uint64_t active_step_bytes,
                                     uint32_t stop, uint8_t* stopped_device, int32_t* ran_device,
                                     double* returns_device, double gamma) {
  MpStepUntil r;
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
  r.stop = stop;
  r.stopped = stopped_device;
  r.ran = ran_device;
  r.returns = returns_device;
  r.gamma = gamma;
  return mp_restore(eng, &r, sizeof r);
}

/* One step of the worlds whose stopped_device byte is 0 (uint8 [N]); a world the step leaves on
 * LAST, or pays, gets its reason bits (`stop` says which of the two count).  The closed loop that
 * needs no host synchronisation: call it every step with the same tensor. */
static inline int mp_step_until(MpEngine* eng, const int32_t* actions_device, int32_t fields,
                                uint32_t stop, uint8_t* stopped_device) {
  return mp_step_many_until(eng, actions_device, 1, fields, 0, NULL, 0, NULL, 0, stop, stopped_device,
                            NULL, NULL, 1.0);
}

#endif /* MP_STEP_UNTIL_H_ */
