// state_obs_rules.h — the scalar observations that are functions of a record, as device functions:
// what load_world's block of record functions and load_level_obs (step_load.h) write for a loaded
// world.  Shared by state_obs.hip (k_state_obs: every player of a row) and state_view.hip
// (k_view_scalar: one player of a row); device code only, included behind step_load.h.
#pragma once
#include "step_load.h"

namespace {

using namespace stepk;

// "N.INVENTORY": how many classes a level has (an avatar's values in the observation), how many
// of them the record holds, and where it keeps avatar p's count of class k (step_load.h:
// load_level_obs)
template <class Tables>
__device__ inline int inventory_classes(const Tables&) { return 0; }
__device__ inline int inventory_classes(const GiftTables& c) { return c.ntypes; }
__device__ inline int inventory_classes(const MatrixTables& c) { return c.R; }
template <class Tables>
__device__ inline int inventory_held(const Tables& c) { return inventory_classes(c); }
__device__ inline int inventory_held(const GiftTables& c) { return c.ntypes < 3 ? c.ntypes : 3; }

template <class Tables>
__device__ inline double inventory_of(const DevTables&, const Tables&, const uint8_t*, int, int) { return 0.0; }
__device__ inline double inventory_of(const DevTables& t, const GiftTables&, const uint8_t* rec, int p, int k) {
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
  return (double)(k == 0 ? tail->flag0[p] : k == 1 ? tail->flag1[p] : tail->level[p]);
}
__device__ inline double inventory_of(const DevTables&, const MatrixTables& c, const uint8_t* rec, int p, int k) {
  return (double)reinterpret_cast<const MxPlayer*>(rec + c.player_block)[p].inv[k];
}

// READY_TO_SHOOT as load_world writes it ... (lr: the level's load_rules)
template <class Tables>
__device__ inline double ready_of(const Tables& c, const WorldTail* tail, int p) {
  const double v = 1.0 - (double)tail->ztimer[p] / (double)load_rules(c).ready_cooldown;
  return tail->aalive[p] ? (v > 0.0 ? v : 0.0) : 0.0;
}
// ... and as the matrix games' load_level_obs does: it does not look at the avatar's state
__device__ inline double ready_of(const MatrixTables& c, const WorldTail* tail, int p) {
  return 1.0 - (double)tail->ztimer[p] / (double)c.cooldown;
}

}  // namespace
