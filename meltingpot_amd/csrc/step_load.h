// step_load.h — STEP_MODE_LOAD (mp_load_worlds): world w starts from a saved record.
//
// A record is the whole of a world (mp_common.h): every draw is Philox keyed by its own seed and
// counted by (index, stream, step, episode), so a world's future is a function of its record and
// the actions it gets.  A load is therefore a masked reset whose feeder takes the record from row
// src[w] of a bank instead of building a fresh episode: the same launch (k_frame, or the
// stand-alone step kernels), the same views drawn from the record in LDS, the same ring slot.
//
// What the launch writes for a loaded world (include/mp_engine.h lists the kinds):
//   (A) kinds that are functions of the record — POSITION, ORIENTATION, READY_TO_SHOOT,
//       INVENTORY, the pixels and LAYER — as the source's last launch wrote them;
//   (B) transition kinds as a reset writes them: STEP_TYPE FIRST, zero REWARD, COLLECTIVE_REWARD,
//       DISCOUNT, AUX0, ZAP_MATRIX (clean_up, commons_harvest), AUX1-4 (clean_up), the matrix's
//       INTERACTION_INVENTORIES and cumulants, and the reset's EVENTS (AVATAR_STARTED per avatar;
//       SET_SANCTIONING_LEVEL(p, 1) after them where the level's avatars carry a sanctioning mark).
//       A row saved from a finished world reports what a frozen world reports instead: LAST,
//       discount 0, reward 0, no events.
// The destination keeps its WorldTail::ctr[] and reward_fx: they only feed mp_counters.
#ifndef MP_STEP_LOAD_H_
#define MP_STEP_LOAD_H_

#include "step_clean_up.h"
#include "step_coins.h"
#include "step_commons.h"
#include "step_coop.h"
#include "step_gift.h"
#include "step_mushroom.h"
#include "step_cook.h"
#include "step_matrix.h"
#include "step_territory.h"

namespace stepk {

// What each level's reset and finish() write that the record does not say.
struct LoadRules {
  int ready_cooldown;      // the zap cooldown the level hands finish() for READY_TO_SHOOT
  bool zeroes_zap_matrix;  // a reset zeroes the world's ZAP_MATRIX block (when bound)
  bool zeroes_dbg;         // a reset writes 0 to AUX1..AUX4 (when bound)
  bool sanction_events;    // a reset reports SET_SANCTIONING_LEVEL(p + 1, 1) after AVATAR_STARTED
};
__device__ inline LoadRules load_rules(const CleanUpTables& c) { return {c.zap.cooldown, true, true, false}; }
__device__ inline LoadRules load_rules(const CommonsTables& c) { return {c.zap.cooldown, true, false, false}; }
__device__ inline LoadRules load_rules(const CoinsTables&) { return {1, false, false, false}; }
__device__ inline LoadRules load_rules(const CoopTables& c) { return {c.cooldown, false, false, false}; }
__device__ inline LoadRules load_rules(const GiftTables& c) { return {c.cooldown, false, false, false}; }
__device__ inline LoadRules load_rules(const CookTables& c) {
  return {c.cooldown > 0 ? c.cooldown : 1, false, false, false};
}
__device__ inline LoadRules load_rules(const MatrixTables& c) {
  return {c.cooldown > 0 ? c.cooldown : 1, false, false, false};
}
__device__ inline LoadRules load_rules(const MushroomTables& c) { return {c.zap.cooldown, false, false, true}; }
__device__ inline LoadRules load_rules(const TerritoryTables& c) { return {c.zap.cooldown, false, false, true}; }

// Level-specific observations of a loaded world (lane p < P: avatar p), after the common ones.
template <class Tables>
__device__ inline void load_level_obs(const DevTables&, const Tables&, const uint8_t*,
                                      const StepOutputs&, int, int) {}
// gift_refinements: "N.INVENTORY" lives in the tail bytes flag0 / flag1 / level (step_gift.h)
__device__ inline void load_level_obs(const DevTables& t, const GiftTables& c, const uint8_t* rec,
                                      const StepOutputs& out, int w, int lane) {
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
  if (lane < t.P && out.inventory) {
    const size_t o = ((size_t)w * t.P + lane) * c.ntypes;
    if (c.ntypes > 0) out.inventory[o] = (double)tail->flag0[lane];
    if (c.ntypes > 1) out.inventory[o + 1] = (double)tail->flag1[lane];
    if (c.ntypes > 2) out.inventory[o + 2] = (double)tail->level[lane];
  }
}
// *_in_the_matrix: "N.INVENTORY" from the record's MxPlayer block; READY_TO_SHOOT does not look
// at the avatar's state (step_matrix.h); a reset writes zero interaction inventories and cumulants
__device__ inline void load_level_obs(const DevTables& t, const MatrixTables& c, const uint8_t* rec,
                                      const StepOutputs& out, int w, int lane) {
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
  const MxPlayer* players = reinterpret_cast<const MxPlayer*>(rec + c.player_block);
  if (lane >= t.P) return;
  const int R = c.R;
  const size_t o = (size_t)w * t.P + lane;
  for (int k = 0; k < R; ++k) {
    out.inventory[o * R + k] = (double)players[lane].inv[k];
    out.interaction[(o * 2 + 0) * R + k] = 0.0;
    out.interaction[(o * 2 + 1) * R + k] = 0.0;
  }
  if (out.cumulants)
    for (int k = 0; k < 1 + 3 * R; ++k) out.cumulants[o * (1 + 3 * R) + k] = 0.0;
  out.ready[o] = 1.0 - (double)tail->ztimer[lane] / (double)c.cooldown;
}

// The record in LDS -> HBM (finish()'s write-back).
__device__ inline void store_record(const DevTables& t, const uint8_t* rec, uint8_t* gw, int lane) {
  const int nvec = t.world_stride >> 4;
  for (int i0 = 0; i0 < nvec; i0 += 8 * 64) {
    uint4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k * 64 + lane;
      v[k] = reinterpret_cast<const uint4*>(rec)[i < nvec ? i : nvec - 1];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) issued(v[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k * 64 + lane;
      if (i < nvec) reinterpret_cast<uint4*>(gw)[i] = v[k];
    }
  }
}

// An index a world-state launch skipped (mp_common.h: FAULT_STATE_INDEX); the next synchronising
// call reports it.
__device__ inline void report_state_index(const DevTables& t, int lane, int who, int index, int what) {
  if (lane == 0) {
    t.fault[FAULT_STATE_INDEX + 1] = (uint32_t)index;
    t.fault[FAULT_STATE_INDEX + 2] = (uint32_t)what;
    t.fault[FAULT_STATE_INDEX] = (uint32_t)who + 1u;
  }
}

// STEP_MODE_LOAD for the world of `wd`, whose own record is in LDS (wd.rec): what a stepping
// launch runs instead of step_world.  Wave-level, like step_world; the caller publishes the
// record to the renderers and writes LAYER from it.
template <class Tables>
__device__ inline void load_world(const DevTables& t, const Tables& c, const World& wd,
                                  const StepArgs& args) {
  const int lane = wd.lane, w = wd.w, P = t.P;
  const int r = __builtin_amdgcn_readfirstlane(args.src[w]);
  if (r == -1) return;   // as a masked reset leaves a world outside its mask
  if (r < -1 || r >= args.bank_rows) {   // never dereferenced: reported, the world left alone
    report_state_index(t, lane, w, r, kFaultLoadSrc);
    return;
  }
  uint8_t* rec = wd.rec;
  WorldTail* tail = reinterpret_cast<WorldTail*>(rec + t.grid_pad);
  // the destination's counters (WorldTail::ctr[], reward_fx) stay its own
  uint32_t keep = 0;
  if (lane < 8) keep = tail->ctr[lane];
  else if (lane == 8) keep = (uint32_t)tail->reward_fx;
  wsync();
  load_record(t, rec, args.bank + (size_t)r * t.world_stride, lane);
  wsync();
  if (lane < 8) tail->ctr[lane] = keep;
  else if (lane == 8) tail->reward_fx = (int32_t)keep;
  wsync();
  const StepOutputs& out = args.out;
  const LoadRules lr = load_rules(c);
  const bool done = __builtin_amdgcn_readfirstlane(tail->done) != 0;
  // (A) what the record says
  if (lane < P) {
    const size_t o = (size_t)w * P + lane;
    const int alive = tail->aalive[lane];
    const double v = 1.0 - (double)tail->ztimer[lane] / (double)lr.ready_cooldown;
    out.ready[o] = alive ? (v > 0.0 ? v : 0.0) : 0.0;
    out.position[o * 2 + 0] = tail->ax[lane];
    out.position[o * 2 + 1] = tail->ay[lane];
    out.orientation[o] = tail->aori[lane];
    // (B) as a reset writes them
    out.reward[o] = 0.0;
    out.aux0[o] = 0.0;
    if (lr.zeroes_dbg)
      for (int k = 0; k < 4; ++k)
        if (out.dbg[k]) out.dbg[k][o] = 0.0;
  }
  if (lr.zeroes_zap_matrix && out.zap_matrix)
    for (int i = lane; i < P * P; i += 64) out.zap_matrix[(size_t)w * P * P + i] = 0.0;
  load_level_obs(t, c, rec, out, w, lane);
  int4* rows = reinterpret_cast<int4*>(out.events) + (size_t)w * MP_EVENT_ROWS;
  if (lane == 0) {
    out.collective[w] = 0.0;
    out.step_type[w] = done ? 2 : 0;
    out.discount[w] = 0.0;
    const int n = done ? 0 : (lr.sanction_events ? 2 * P : P);
    rows[0] = int4{n, 0, 0, 0};
  }
  if (!done && lane < P) {
    rows[1 + lane] = int4{MP_EVENT_AVATAR_STARTED, 0, 0, 0};
    if (lr.sanction_events) rows[1 + P + lane] = int4{MP_EVENT_SET_SANCTIONING_LEVEL, lane + 1, 1, 0};
  }
  store_record(t, rec, wd.gw, lane);
}

// ---- registered episode starts (include/mp_episode_starts.h: MpEpisodeStarts) ------------------
// A start the launch skipped (the world took the level's own reset): words of their own, which
// the next synchronising call reports — word 32 = world + 1 (ONE world of a launch claims it, a
// compare-and-swap from 0, and writes the other three), 33 = rows[world], 34 = the rule of the
// row's verdict (0: the index is neither -1 nor a row of the bank), 35 = its offset word
// (mp_common.h: kFaultStartWorld).
__device__ inline void report_start(const DevTables& t, int lane, int w, int index, int rule, int offset) {
  if (lane == 0 && atomicCAS(&t.fault[kFaultStartWorld], 0u, (uint32_t)w + 1u) == 0u) {
    t.fault[kFaultStartWorld + 1] = (uint32_t)index;
    t.fault[kFaultStartWorld + 2] = (uint32_t)rule;
    t.fault[kFaultStartWorld + 3] = (uint32_t)offset;
  }
}

// Does this step start the world's next episode?  dispatch()'s own test for returning 1 in
// STEP_MODE_STEP / STEP_MODE_FIELDS (wave-uniform), asked BEFORE the step runs.
__device__ inline bool starts_here(const WorldTail* tail, const StepArgs& args) {
  if (args.mode & 1) return false;   // (RESET, LOAD: an explicit reset or load is not an episode start)
  return __builtin_amdgcn_readfirstlane((int)(tail->started && tail->done)) != 0 && args.auto_reset != 0;
}

// The row world `w` starts from, or -1 for the level's own reset: rows[w], read now; an index
// outside [-1, bank_rows) or a row whose verdict is not (0, 0) is reported and never read.
__device__ inline int start_row(const DevTables& t, const StartArgs& st, int w, int lane) {
  const int r = __builtin_amdgcn_readfirstlane(st.rows[w]);
  if (r == -1) return -1;
  if (r < -1 || r >= st.bank_rows) {
    report_start(t, lane, w, r, 0, 0);
    return -1;
  }
  if (st.verdicts) {
    const int rule = __builtin_amdgcn_readfirstlane(st.verdicts[2 * (size_t)r]);
    const int offset = __builtin_amdgcn_readfirstlane(st.verdicts[2 * (size_t)r + 1]);
    if (rule != 0 || offset != 0) {
      report_start(t, lane, w, r, rule, offset);
      return -1;
    }
  }
  return r;
}

// The episode start of the world of `wd`, whose rows[w] start_row() has just accepted, run BEHIND
// the level's own reset of the same step.  The reset has done what an episode start does to the
// world's own words (episode + 1, MP_CTR_EPISODES + 1) and has written every kind a reset writes;
// this is load_world itself on top of it, with the registration's bank and rows as the load's bank
// and src — so a step with a registration leaves exactly what step() and then MP_STATES_LOAD
// leave, and load_world is the text it was.  With `fresh` the seed and the episode count the
// reset left are put back into the loaded record (the orders the row cached were drawn under the
// row's: orders_step 0 has them drawn again) and the record is written back once more.
template <class Tables>
__device__ inline void start_world(const DevTables& t, const Tables& c, const World& wd,
                                   const StepArgs& args, const StartArgs& st) {
  const int lane = wd.lane;
  WorldTail* tail = reinterpret_cast<WorldTail*>(wd.rec + t.grid_pad);
  wsync();   // the reset's finish() has read the record for its write-back
  uint32_t keep = 0;   // lane 0, 1: the seed's halves; lane 2: the episode count
  if (lane < 2) keep = (uint32_t)(tail->seed >> (32 * lane));
  else if (lane == 2) keep = tail->episode;
  StepArgs la = args;
  la.bank = st.bank; la.src = st.rows; la.bank_rows = st.bank_rows;
  load_world(t, c, wd, la);
  if (st.fresh) {
    const uint32_t lo = (uint32_t)rdlane((int)keep, 0), hi = (uint32_t)rdlane((int)keep, 1);
    const uint32_t ep = (uint32_t)rdlane((int)keep, 2);
    if (lane == 0) {
      tail->seed = ((uint64_t)hi << 32) | lo;
      tail->episode = ep;
      tail->orders_step = 0u;
    }
    wsync();
    store_record(t, wd.rec, wd.gw, lane);
  }
}

// A stepping launch's work for one world: STEP_MODE_LOAD's, or the level's step / reset — and,
// in the families of the registered episode starts (kStarts), the start behind an auto-reset.
template <bool kStarts = false, class Tables, class Sites>
__device__ inline void step_or_load(const DevTables& t, const Tables& c, const Sites& sites,
                                    const World& wd, const Action& act, const StepArgs& args,
                                    const StartArgs* st = nullptr) {
  if (args.mode == STEP_MODE_LOAD) {
    load_world(t, c, wd, args);
  } else if constexpr (kStarts) {
    const WorldTail* tail = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
    const int r = starts_here(tail, args) ? start_row(t, *st, wd.w, wd.lane) : -1;
    step_world(t, c, sites, wd, act, args);
    if (r >= 0) start_world(t, c, wd, args, *st);
  } else {
    step_world(t, c, sites, wd, act, args);
  }
}

}  // namespace stepk

#endif  // MP_STEP_LOAD_H_
