// step_until.hip — the K-step kernels with stop conditions (MpStepUntil, include/mp_engine.h): the
// masked request of step_active.hip in which a world that ends its episode, or is paid, stops
// there for the rest of the launch, and which hands back how many steps each world ran and the
// discounted sum of its rewards over them.  The body is run_many_masked<.., Until = true>
// (step_masked.h), which step_listed.hip's kernels share.  A unit of its own: every other family
// keeps one caller of each level's step in its unit (step_starts.hip says why).
#include "step_levels.h"
#include "step_masked.h"

namespace {

using namespace stepk;

// (coop's loop needs 132 VGPRs with the sum's six, one band above k_many_active_coop's 124: at 4096
// worlds a CU then held 12 waves instead of 16 and a 64-step request took 1.24 of the masked one's
// time (profiles/r22_step_until.md).  Asked to keep four waves a SIMD the compiler fits it into
// 128.  The definition below inherits the attribute from this declaration.)
__global__ __attribute__((amdgpu_waves_per_eu(4, 4))) void k_many_until_coop(
    DevTables, CoopTables, StepArgs, ManyArgs, StepRows, StateRows, HashRows, StartArgs, ActiveArgs, UntilArgs);

#define MP_MANY_UNTIL_KERNEL(level, TablesT, SitesT, sub, member)                                    \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_many_until_##level(                      \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s, HashRows h,        \
      StartArgs st, ActiveArgs am, UntilArgs um) {                                                   \
    run_many_masked<TablesT, SitesT, true>(t, c, args, m, r, extra_bytes(c), s, h, st, am, &um);     \
  }
MP_STEP_LEVELS(MP_MANY_UNTIL_KERNEL)
#undef MP_MANY_UNTIL_KERNEL
// (a parameter list above that differs from the macro's would declare an overload, and the kernel
// that is launched would be without the attribute: then this address is ambiguous and does not compile)
static_assert(&k_many_until_coop != nullptr, "k_many_until_coop: one declaration, one definition");

}  // namespace

int prepare_step_until() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member) reinterpret_cast<const void*>(&k_many_until_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

// launch_step_active (step_active.hip) with the stop state `u`: the same geometry, one family.
void launch_step_until(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                       const StepManyLaunch& l, const UntilArgs& u, hipStream_t stream) {
  const StepGeometry g = step_geometry(t, s, args.num_worlds);
  const StepRows r = step_rows_of(l, args.out);
  const stepk::StartArgs st = l.starts ? *l.starts : stepk::StartArgs{};
#define MP_LEVEL(level, TablesT, SitesT, sub, member)                                              \
  case sub:                                                                                        \
    hipLaunchKernelGGL(k_many_until_##level, g.grid, g.block, g.lds, stream, t, s.member, args,    \
                       l.many, r, l.state, l.hash, st, l.active, u);                               \
    break;
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
}
