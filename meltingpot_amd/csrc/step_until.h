// step_until.h — what the host hands the K-step kernels with stop conditions (step_until.hip)
// besides a checked StepManyLaunch: the stop state and the sums of an MpStepUntil request
// (include/mp_engine.h).  A header of its own: step_many.h, and every unit that includes only it,
// are what they were.
#ifndef MP_STEP_UNTIL_H_INTERNAL_
#define MP_STEP_UNTIL_H_INTERNAL_

#include "step_many.h"

// stop: MP_STOP_* bits (0: nothing stops a world).  stopped: uint8 [N], read on entry (non-zero:
// the world does not run in this call) and written with the reason bits where a world stops, or
// NULL: every world starts unstopped and the reason is not kept.  ran: int32 [N] or NULL.
// returns: f64 [N][P] or NULL, the sum of gamma^j * REWARD over the steps j = 0, 1, .. that ran.
struct UntilArgs {
  uint32_t stop;
  uint8_t* stopped;
  int32_t* ran;
  double* returns;
  double gamma;
};

// launch_step_active (step_active.hip) with the stop state `u`; l.active.active may be NULL (every
// world-step is active).
void launch_step_until(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                       const StepManyLaunch& l, const UntilArgs& u, hipStream_t stream);
int prepare_step_until();

#endif  // MP_STEP_UNTIL_H_INTERNAL_
