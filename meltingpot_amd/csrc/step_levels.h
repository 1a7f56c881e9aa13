// step_levels.h — the nine levels of the stand-alone step kernels, listed ONCE, and what every
// unit that defines one kernel a level shares on the host side: the launch geometry and the LDS
// attribute.  Included by the six step units (step_kernels.hip, step_starts.hip, step_many.hip,
// step_active.hip, step_until.hip, step_listed.hip) and by nothing else.
#ifndef MP_STEP_LEVELS_H_
#define MP_STEP_LEVELS_H_

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
#include "step_many.h"

// X(level, Tables, Sites, substrate, member): the suffix of the level's kernel names, its tables
// and site lists (stepk), its MPK_SUBSTRATE_* value and its member of SubstrateTables.  (The LDS
// extras need no column: extra_bytes(c) is 0 for a level without them, step_common.h.)
#define MP_STEP_LEVELS(X)                                                              \
  X(clean_up, CleanUpTables, CleanUpSites, MPK_SUBSTRATE_CLEAN_UP, cu)                 \
  X(commons, CommonsTables, CommonsSites, MPK_SUBSTRATE_COMMONS_HARVEST, ch)           \
  X(coins, CoinsTables, CoinsSites, MPK_SUBSTRATE_COINS, co)                           \
  X(coop, CoopTables, CoopSites, MPK_SUBSTRATE_COOP_MINING, cm)                        \
  X(gift, GiftTables, GiftSites, MPK_SUBSTRATE_GIFT_REFINEMENTS, gr)                   \
  X(cook, CookTables, CookSites, MPK_SUBSTRATE_COLLABORATIVE_COOKING, cc)              \
  X(mushroom, MushroomTables, MushroomSites, MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS, em)  \
  X(matrix, MatrixTables, MatrixSites, MPK_SUBSTRATE_THE_MATRIX, mx)                   \
  X(territory, TerritoryTables, TerritorySites, MPK_SUBSTRATE_TERRITORY, tr)

constexpr int kWorldsPerGroup = 4;   // waves of a workgroup at most; they share the LDS tables

// The geometry of a stand-alone step launch: one wave a world, step_worlds_per_group (>= 1:
// mp_create) worlds a workgroup, the tables and their records in LDS.
struct StepGeometry {
  dim3 grid, block;
  size_t lds;
};
inline StepGeometry step_geometry(const DevTables& t, const SubstrateTables& s, int num_worlds) {
  const int wpg = step_worlds_per_group(t, s);
  return {dim3((num_worlds + wpg - 1) / wpg), dim3(wpg * 64), (size_t)step_lds_bytes(t, s, wpg)};
}

// The step kernels may take all 160 KB of a CU's LDS (mp_create refuses a pack that needs more).
template <int N>
inline int step_take_all_lds(const void* const (&kernels)[N]) {
  for (const void* f : kernels)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return 1;
  return 0;
}

// A K-step launch's rows with the level kinds' sources resolved: this submission's buffers.
inline StepRows step_rows_of(const StepManyLaunch& l, const StepOutputs& out) {
  StepRows r = l.rows;
  for (int i = 0; i < r.n_level; ++i) r.level[i].src = level_source(out, r.level[i].which);
  return r;
}

#endif  // MP_STEP_LEVELS_H_
