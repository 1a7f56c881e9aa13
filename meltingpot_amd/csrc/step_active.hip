// step_active.hip — the K-step kernels under a device mask (MpStepActive, include/mp_engine.h):
// in step k world w runs only where active[k][w] != 0, and is not touched otherwise.  The body is
// run_many_masked<.., Until = false> (step_masked.h: one body for this family, step_until.hip's and
// step_listed.hip's).  A unit of its own: the families of
// step_many.hip, step_kernels.hip and step_starts.hip keep one caller of each level's step in
// their unit (step_starts.hip says why).
#include "step_levels.h"
#include "step_masked.h"

namespace {

using namespace stepk;

#define MP_MANY_ACTIVE_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_many_active_##level(                     \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s, HashRows h,        \
      StartArgs st, ActiveArgs am) {                                                                 \
    run_many_masked<TablesT, SitesT, false>(t, c, args, m, r, extra_bytes(c), s, h, st, am);         \
  }
MP_STEP_LEVELS(MP_MANY_ACTIVE_KERNEL)
#undef MP_MANY_ACTIVE_KERNEL

}  // namespace

int prepare_step_active() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member) reinterpret_cast<const void*>(&k_many_active_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

// launch_step_many (step_many.hip) under the mask l.active: the same geometry, one family.
void launch_step_active(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const StepManyLaunch& l, hipStream_t stream) {
  const StepGeometry g = step_geometry(t, s, args.num_worlds);
  const StepRows r = step_rows_of(l, args.out);
  const stepk::StartArgs st = l.starts ? *l.starts : stepk::StartArgs{};
#define MP_LEVEL(level, TablesT, SitesT, sub, member)                                              \
  case sub:                                                                                        \
    hipLaunchKernelGGL(k_many_active_##level, g.grid, g.block, g.lds, stream, t, s.member, args,   \
                       l.many, r, l.state, l.hash, st, l.active);                                  \
    break;
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
}
