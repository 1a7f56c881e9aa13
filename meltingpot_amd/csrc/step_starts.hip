// step_starts.hip — the stand-alone step kernels with registered episode starts (MpEpisodeStarts,
// include/mp_engine.h; step_load.h: start_world): what an engine launches for a step while a
// registration is set.  A unit of its own: the kernels of step_kernels.hip are compiled from
// exactly what they were compiled from before, one caller of each level's step in their unit.
#include "step_levels.h"

namespace {

using namespace stepk;

#include "step_one.h"   // run_one_world

#define MP_STEP_STARTS_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_starts_##level(DevTables t, TablesT c, \
                                                                                StepArgs args, StartArgs st) { \
    run_one_world<TablesT, SitesT, true>(t, c, args, extra_bytes(c), &st);                           \
  }
MP_STEP_LEVELS(MP_STEP_STARTS_KERNEL)
#undef MP_STEP_STARTS_KERNEL

}  // namespace

int prepare_step_starts() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member) reinterpret_cast<const void*>(&k_step_starts_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

// launch_step (step_kernels.hip) with the engine's registered episode starts.
void launch_step_starts(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const stepk::StartArgs& st, hipStream_t stream) {
  const StepGeometry g = step_geometry(t, s, args.num_worlds);
#define MP_LEVEL(level, TablesT, SitesT, sub, member) \
  case sub: hipLaunchKernelGGL(k_step_starts_##level, g.grid, g.block, g.lds, stream, t, s.member, args, st); break;
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
}
