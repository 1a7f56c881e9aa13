/* mp_step_trajectory.h — K steps of every world in one submission with per-step rows of any
 * non-pixel observation kind, as a plain C function.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and this wrapper
 * builds the MpStepTrajectory request that mp_restore carries (mp_engine.h documents the
 * semantics, the carry rule and the refusals).  Same return codes as every entry point. */
#ifndef MP_STEP_TRAJECTORY_H_
#define MP_STEP_TRAJECTORY_H_

#include <string.h>

#include "mp_engine.h"

/* actions_device: int32 [steps][N][P] (fields = 0) or [steps][N][P][A] (fields = 1), two steps'
 * blocks actions_step_bytes apart (0: the same block every step).  rows: a host array of
 * num_rows entries, each naming a kind once with its device buffer and the distance between two
 * of its rows (NULL with num_rows = 0: no rows).  Stream-ordered, no synchronisation. */
static inline int mp_step_trajectory(MpEngine* eng, const int32_t* actions_device, int32_t steps,
                                     int32_t fields, uint64_t actions_step_bytes,
                                     const MpStepRow* rows, int32_t num_rows) {
  MpStepTrajectory r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.steps = steps;
  r.fields = fields;
  r.num_rows = num_rows;
  r.actions = actions_device;
  r.actions_step_bytes = actions_step_bytes;
  r.rows = rows;
  return mp_restore(eng, &r, sizeof r);
}

#endif /* MP_STEP_TRAJECTORY_H_ */
