// step_starts.hip — the stand-alone step kernels with registered episode starts (MpEpisodeStarts,
// include/mp_engine.h; step_load.h: start_world): what an engine launches for a step while a
// registration is set.  A unit of its own: the kernels of step_kernels.hip are compiled from
// exactly what they were compiled from before, one caller of each level's step in their unit.
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
#include "step_many.h"   // (the launch geometry of step_kernels.hip)

namespace {

using namespace stepk;

#include "step_one.h"   // kWorldsPerGroup, run_one_world

#define MP_STEP_STARTS_KERNEL(name, TablesT, SitesT, extra)                                          \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void name(DevTables t, TablesT c, StepArgs args, \
                                                               StartArgs st) {                       \
    run_one_world<TablesT, SitesT, true>(t, c, args, extra, &st);                                    \
  }
MP_STEP_STARTS_KERNEL(k_step_starts_clean_up, CleanUpTables, CleanUpSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_commons, CommonsTables, CommonsSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_coins, CoinsTables, CoinsSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_coop, CoopTables, CoopSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_gift, GiftTables, GiftSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_cook, CookTables, CookSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_mushroom, MushroomTables, MushroomSites, extra_bytes(c))
MP_STEP_STARTS_KERNEL(k_step_starts_matrix, MatrixTables, MatrixSites, 0)
MP_STEP_STARTS_KERNEL(k_step_starts_territory, TerritoryTables, TerritorySites, extra_bytes(c))
#undef MP_STEP_STARTS_KERNEL

}  // namespace

// These kernels may take all 160 KB of a CU's LDS, like the ones they stand in for.
int prepare_step_starts() {
  const void* k[9] = {
      reinterpret_cast<const void*>(&k_step_starts_clean_up), reinterpret_cast<const void*>(&k_step_starts_commons),
      reinterpret_cast<const void*>(&k_step_starts_coins), reinterpret_cast<const void*>(&k_step_starts_territory),
      reinterpret_cast<const void*>(&k_step_starts_matrix), reinterpret_cast<const void*>(&k_step_starts_coop),
      reinterpret_cast<const void*>(&k_step_starts_gift), reinterpret_cast<const void*>(&k_step_starts_cook),
      reinterpret_cast<const void*>(&k_step_starts_mushroom)};
  for (const void* f : k)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return 1;
  return 0;
}

// launch_step (step_kernels.hip) with the engine's registered episode starts.
void launch_step_starts(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const stepk::StartArgs& st, hipStream_t stream) {
  const int wpg = step_worlds_per_group(t, s);   // (>= 1: mp_create)
  const size_t lds = (size_t)step_lds_bytes(t, s, wpg);
  const dim3 grid((args.num_worlds + wpg - 1) / wpg), block(wpg * 64);
  switch (s.substrate) {
    case MPK_SUBSTRATE_CLEAN_UP:
      hipLaunchKernelGGL(k_step_starts_clean_up, grid, block, lds, stream, t, s.cu, args, st);
      break;
    case MPK_SUBSTRATE_COMMONS_HARVEST:
      hipLaunchKernelGGL(k_step_starts_commons, grid, block, lds, stream, t, s.ch, args, st);
      break;
    case MPK_SUBSTRATE_COINS:
      hipLaunchKernelGGL(k_step_starts_coins, grid, block, lds, stream, t, s.co, args, st);
      break;
    case MPK_SUBSTRATE_TERRITORY:
      hipLaunchKernelGGL(k_step_starts_territory, grid, block, lds, stream, t, s.tr, args, st);
      break;
    case MPK_SUBSTRATE_THE_MATRIX:
      hipLaunchKernelGGL(k_step_starts_matrix, grid, block, lds, stream, t, s.mx, args, st);
      break;
    case MPK_SUBSTRATE_COOP_MINING:
      hipLaunchKernelGGL(k_step_starts_coop, grid, block, lds, stream, t, s.cm, args, st);
      break;
    case MPK_SUBSTRATE_GIFT_REFINEMENTS:
      hipLaunchKernelGGL(k_step_starts_gift, grid, block, lds, stream, t, s.gr, args, st);
      break;
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING:
      hipLaunchKernelGGL(k_step_starts_cook, grid, block, lds, stream, t, s.cc, args, st);
      break;
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS:
      hipLaunchKernelGGL(k_step_starts_mushroom, grid, block, lds, stream, t, s.em, args, st);
      break;
  }
}
