// step_listed.h — what the host hands the K-step kernels of a world list (step_listed.hip)
// besides a checked StepManyLaunch and the stop state: the list of an MpStepListed request
// (include/mp_engine.h) and the engine's claim table.  step_masked.h includes it for the body the
// three masked families share; step_many.h and step_until.h do not know it.
#ifndef MP_STEP_LISTED_H_INTERNAL_
#define MP_STEP_LISTED_H_INTERNAL_

#include "step_until.h"

// worlds: device int32 [count], entry i is stepped by wave i.  claim: device u64 [N], the
// engine's; listed_tag(generation, i) (mp_common.h) of the entry that owns world w in this request
// (the claim launch in front of the step kernels takes the maximum, so the lowest i of a
// generation wins; the generation grows with every request, so the table is never cleared).
struct ListArgs {
  const int32_t* worlds;
  int count;
  unsigned long long* claim;
  uint32_t generation;
};

// The claim launch and then the step kernels: ceil(count / worlds per group) workgroups.
void launch_step_listed(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const StepManyLaunch& l, const UntilArgs& u, const ListArgs& list,
                        hipStream_t stream);
int prepare_step_listed();

#endif  // MP_STEP_LISTED_H_INTERNAL_
