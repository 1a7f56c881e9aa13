// step_listed.hip — the K-step kernels of a world list (MpStepListed, include/mp_engine.h): the
// request of step_until.hip launched with one wave per ENTRY of a device index list instead of one
// per world of the engine, so count entries are ceil(count / 4) workgroups whatever N is, the
// running worlds sit four to a workgroup, and the actions, the mask and every per-call tensor have
// count columns.  In front of it the claim kernel, which decides which entry owns a world.  The
// body is run_many_masked<.., Until = true, Listed = true> (step_masked.h), which resolves the
// entry and keeps the world and the column apart.  A unit of its own: every family keeps one caller
// of each level's step in its unit (step_starts.hip says why).
#include "step_levels.h"
#include "step_masked.h"

namespace {

using namespace stepk;

// One thread an entry: the entry's tag into its world's word, the maximum wins.  A value that is
// no world is never an index (the step kernel reports it).
__global__ __launch_bounds__(256) void k_claim_listed(const int32_t* __restrict__ worlds, int count,
                                                      int num_worlds, unsigned long long* claim,
                                                      uint32_t generation) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= count) return;
  const int w = worlds[i];
  if (w < 0 || w >= num_worlds) return;
  atomicMax(&claim[w], listed_tag(generation, i));
}

// (coop's loop needs 130 VGPRs here, one band above k_many_active_coop's 124, as
// k_many_until_coop's did: asked to keep four waves a SIMD the compiler fits it into 128 — see
// step_until.hip.  The definition below inherits the attribute from this declaration.)
__global__ __attribute__((amdgpu_waves_per_eu(4, 4))) void k_many_listed_coop(
    DevTables, CoopTables, StepArgs, ManyArgs, StepRows, StateRows, HashRows, StartArgs, ActiveArgs, UntilArgs,
    ListArgs);

#define MP_MANY_LISTED_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_many_listed_##level(                     \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s, HashRows h,        \
      StartArgs st, ActiveArgs am, UntilArgs um, ListArgs la) {                                      \
    run_many_masked<TablesT, SitesT, true, true>(t, c, args, m, r, extra_bytes(c), s, h, st, am,     \
                                                 &um, &la);                                          \
  }
MP_STEP_LEVELS(MP_MANY_LISTED_KERNEL)
#undef MP_MANY_LISTED_KERNEL
// (a parameter list above that differs from the macro's would declare an overload without the attribute)
static_assert(&k_many_listed_coop != nullptr, "k_many_listed_coop: one declaration, one definition");

}  // namespace

int prepare_step_listed() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member) reinterpret_cast<const void*>(&k_many_listed_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

// The claim launch, then launch_step_until's launch (step_until.hip) with the geometry of
// list.count worlds: one family.
void launch_step_listed(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const StepManyLaunch& l, const UntilArgs& u, const ListArgs& list,
                        hipStream_t stream) {
  hipLaunchKernelGGL(k_claim_listed, dim3((list.count + 255) / 256), dim3(256), 0, stream, list.worlds,
                     list.count, args.num_worlds, list.claim, list.generation);
  const StepGeometry g = step_geometry(t, s, list.count);
  const StepRows r = step_rows_of(l, args.out);
  const stepk::StartArgs st = l.starts ? *l.starts : stepk::StartArgs{};
#define MP_LEVEL(level, TablesT, SitesT, sub, member)                                              \
  case sub:                                                                                        \
    hipLaunchKernelGGL(k_many_listed_##level, g.grid, g.block, g.lds, stream, t, s.member, args,   \
                       l.many, r, l.state, l.hash, st, l.active, u, list);                         \
    break;
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
}
