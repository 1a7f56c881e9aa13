// step_kernels.hip — the stand-alone step kernels: one wavefront per world, four
// worlds per workgroup (they share the read-only LDS tables).  They run the same wave-level step functions
// (step_<substrate>.h) as the fused step + render kernels of frame.hip, and are
// what an engine launches when no RGB observation is bound to a step (and for
// mp_reset).  A bound "N.LAYER" is written by the wave that stepped the world.  Reference path replaced: api:advance / api:start
// (lua/modules/api_factory.lua:85-111) — see step_clean_up.h.
#include "../../include/mp_pack.h"
#include "step_clean_up.h"
#include "step_coins.h"
#include "step_commons.h"
#include "step_coop.h"
#include "step_gift.h"
#include "step_mushroom.h"
#include "step_cook.h"
#include "step_matrix.h"
#include "step_territory.h"
#include "step_load.h"

namespace {

using namespace stepk;

#include "step_one.h"   // kWorldsPerGroup, run_one_world

__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_clean_up(DevTables t, CleanUpTables c, StepArgs args) {
  run_one_world<CleanUpTables, CleanUpSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_commons(DevTables t, CommonsTables c, StepArgs args) {
  run_one_world<CommonsTables, CommonsSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_coins(DevTables t, CoinsTables c, StepArgs args) {
  run_one_world<CoinsTables, CoinsSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_coop(DevTables t, CoopTables c, StepArgs args) {
  run_one_world<CoopTables, CoopSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_gift(DevTables t, GiftTables c, StepArgs args) {
  run_one_world<GiftTables, GiftSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_cook(DevTables t, CookTables c, StepArgs args) {
  run_one_world<CookTables, CookSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_mushroom(DevTables t, MushroomTables c, StepArgs args) {
  run_one_world<MushroomTables, MushroomSites>(t, c, args, extra_bytes(c));
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_matrix(DevTables t, MatrixTables c, StepArgs args) {
  run_one_world<MatrixTables, MatrixSites>(t, c, args, 0);
}
__global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_territory(DevTables t, TerritoryTables c, StepArgs args) {
  run_one_world<TerritoryTables, TerritorySites>(t, c, args, extra_bytes(c));
}

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
  const int extra = s.substrate == MPK_SUBSTRATE_TERRITORY ? stepk::extra_bytes(s.tr)
                    : s.substrate == MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS ? stepk::extra_bytes(s.em) : 0;
  return stepk::tables_bytes(t) + wpg * (t.world_stride + stepk::scratch_bytes(t) + extra);
}

// Worlds per workgroup of the stand-alone step launch: kWorldsPerGroup (every stock pack), or
// fewer for a large map; 0 when even one record does not fit (mp_create refuses the pack).
int step_worlds_per_group(const DevTables& t, const SubstrateTables& s) {
  for (int wpg = kWorldsPerGroup; wpg >= 1; wpg >>= 1)
    if (step_lds_bytes(t, s, wpg) <= 160 * 1024) return wpg;
  return 0;
}

// The step kernels may take all 160 KB of a CU's LDS (mp_create refuses a pack that needs more).
int prepare_step() {
  const void* k[9] = {
      reinterpret_cast<const void*>(&k_step_clean_up), reinterpret_cast<const void*>(&k_step_commons),
      reinterpret_cast<const void*>(&k_step_coins), reinterpret_cast<const void*>(&k_step_territory),
      reinterpret_cast<const void*>(&k_step_matrix), reinterpret_cast<const void*>(&k_step_coop),
      reinterpret_cast<const void*>(&k_step_gift), reinterpret_cast<const void*>(&k_step_cook),
      reinterpret_cast<const void*>(&k_step_mushroom)};
  for (const void* f : k)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return 1;
  return 0;
}

void launch_step(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                 hipStream_t stream) {
  const int wpg = step_worlds_per_group(t, s);   // (>= 1: mp_create)
  const size_t lds = (size_t)step_lds_bytes(t, s, wpg);
  const dim3 grid((args.num_worlds + wpg - 1) / wpg), block(wpg * 64);
  switch (s.substrate) {
    case MPK_SUBSTRATE_CLEAN_UP:
      hipLaunchKernelGGL(k_step_clean_up, grid, block, lds, stream, t, s.cu, args);
      break;
    case MPK_SUBSTRATE_COMMONS_HARVEST:
      hipLaunchKernelGGL(k_step_commons, grid, block, lds, stream, t, s.ch, args);
      break;
    case MPK_SUBSTRATE_COINS:
      hipLaunchKernelGGL(k_step_coins, grid, block, lds, stream, t, s.co, args);
      break;
    case MPK_SUBSTRATE_TERRITORY:
      hipLaunchKernelGGL(k_step_territory, grid, block, lds, stream, t, s.tr, args);
      break;
    case MPK_SUBSTRATE_THE_MATRIX:
      hipLaunchKernelGGL(k_step_matrix, grid, block, lds, stream, t, s.mx, args);
      break;
    case MPK_SUBSTRATE_COOP_MINING:
      hipLaunchKernelGGL(k_step_coop, grid, block, lds, stream, t, s.cm, args);
      break;
    case MPK_SUBSTRATE_GIFT_REFINEMENTS:
      hipLaunchKernelGGL(k_step_gift, grid, block, lds, stream, t, s.gr, args);
      break;
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING:
      hipLaunchKernelGGL(k_step_cook, grid, block, lds, stream, t, s.cc, args);
      break;
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS:
      hipLaunchKernelGGL(k_step_mushroom, grid, block, lds, stream, t, s.em, args);
      break;
  }
}
