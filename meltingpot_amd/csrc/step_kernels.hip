// step_kernels.hip — the stand-alone step kernels: one wavefront per world, four
// worlds per workgroup (they share the read-only LDS tables).  They run the same wave-level step functions
// (step_<substrate>.h) as the fused step + render kernels of frame.hip, and are
// what an engine launches when no RGB observation is bound to a step (and for
// mp_reset).  A bound "N.LAYER" is written by the wave that stepped the world.  Reference path replaced: api:advance / api:start
// (lua/modules/api_factory.lua:85-111) — see step_clean_up.h.
#include "step_levels.h"

namespace {

using namespace stepk;

#include "step_one.h"   // run_one_world

#define MP_STEP_KERNEL(level, TablesT, SitesT, sub, member)                                          \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_##level(DevTables t, TablesT c, StepArgs args) { \
    run_one_world<TablesT, SitesT>(t, c, args, extra_bytes(c));                                      \
  }
MP_STEP_LEVELS(MP_STEP_KERNEL)
#undef MP_STEP_KERNEL

// "N.LAYER" (avatar_library.lua:246-257): the player's layer view with
// orientation 'N', as sprite ids (A17; oracle/render.c: orc_layer_view), read straight
// from the records in HBM: one thread per (world, player, window cell).  What
// mp_observe(MP_OBS_LAYER) launches; a bound LAYER is written by the launch that steps
// the worlds instead (stepk::write_layer).
__global__ void k_layer_view(DevTables t, const uint8_t* __restrict__ state,
                             int32_t* __restrict__ out, int num_worlds) {
  const int VW = t.vl + t.vr + 1, VH = t.vf + t.vb + 1, HW = t.H * t.W;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)num_worlds * t.P * VH * VW) return;
  const int vx = (int)(i % VW), vy = (int)((i / VW) % VH);
  const int p = (int)((i / (VW * VH)) % t.P), w = (int)(i / ((long long)VW * VH * t.P));
  const uint8_t* rec = state + (size_t)w * t.world_stride;
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
  const int32_t* remap = t.view_sprite_map + (size_t)p * t.nsprites;
  int32_t* dst = out + (size_t)i * t.L;
  int x = tail->ax[p] + (vx - t.vl), y = tail->ay[p] + (vy - t.vf);
  bool in = true;
  if (t.topology == 1) { x = ((x % t.W) + t.W) % t.W; y = ((y % t.H) + t.H) % t.H; }
  else in = x >= 0 && x < t.W && y >= 0 && y < t.H;
  if (!in || !tail->aalive[p]) {   // A6: an off-grid viewer sees only OutOfBounds
    for (int l = 0; l < t.L; ++l) dst[l] = 1 + remap[0];
    return;
  }
  for (int l = 0; l < t.L; ++l) {
    const int s = rec[l * HW + y * t.W + x];
    const int sprite = s ? t.state_sprite[s] : -1;
    dst[l] = sprite >= 0 ? 1 + remap[sprite] : 0;
  }
}

}  // namespace

void launch_layer_view(const DevTables& t, const uint8_t* state, int32_t* out, int num_worlds,
                       hipStream_t stream) {
  const long long n = (long long)num_worlds * t.P * (t.vl + t.vr + 1) * (t.vf + t.vb + 1);
  hipLaunchKernelGGL(k_layer_view, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, t,
                     state, out, num_worlds);
}

// LDS of a stand-alone step launch of `wpg` worlds per workgroup: the tables and wpg records
// with their scratch (four 64 x 64 clean_up records are 170 KB)
int step_lds_bytes(const DevTables& t, const SubstrateTables& s, int wpg) {
  int extra = 0;
#define MP_LEVEL(level, TablesT, SitesT, sub, member) \
  if (s.substrate == sub) extra = stepk::extra_bytes(s.member);
  MP_STEP_LEVELS(MP_LEVEL)
#undef MP_LEVEL
  return stepk::tables_bytes(t) + wpg * (t.world_stride + stepk::scratch_bytes(t) + extra);
}

// Worlds per workgroup of the stand-alone step launch: kWorldsPerGroup (every stock pack), or
// fewer for a large map; 0 when even one record does not fit (mp_create refuses the pack).
int step_worlds_per_group(const DevTables& t, const SubstrateTables& s) {
  for (int wpg = kWorldsPerGroup; wpg >= 1; wpg >>= 1)
    if (step_lds_bytes(t, s, wpg) <= 160 * 1024) return wpg;
  return 0;
}

int prepare_step() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member) reinterpret_cast<const void*>(&k_step_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

void launch_step(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                 hipStream_t stream) {
  const StepGeometry g = step_geometry(t, s, args.num_worlds);
#define MP_LEVEL(level, TablesT, SitesT, sub, member) \
  case sub: hipLaunchKernelGGL(k_step_##level, g.grid, g.block, g.lds, stream, t, s.member, args); break;
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
}
