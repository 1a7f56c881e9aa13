// step_masked.h — the one body of the K-step kernels under a device mask (MpStepActive,
// step_active.hip: Until = false), of those with stop conditions besides (MpStepUntil,
// step_until.hip: Until = true) and of those of a world list (MpStepListed, step_listed.hip:
// Until and Listed).  Each of the three units instantiates it for its own kernel family, one
// caller of each level's step in a unit (step_starts.hip says why).
#ifndef MP_STEP_MASKED_H_
#define MP_STEP_MASKED_H_

#include "step_listed.h"
#include "step_rows.h"

namespace stepk {

// An entry the launch skips; one of a launch's is named (state_view.hip reports the same way).
__device__ inline void report_entry(const DevTables& t, int lane, int i, int value, uint32_t what) {
  if (lane == 0 && atomicCAS(&t.fault[FAULT_STATE_INDEX], 0u, (uint32_t)i + 1u) == 0u) {
    t.fault[FAULT_STATE_INDEX + 1] = (uint32_t)value;
    t.fault[FAULT_STATE_INDEX + 2] = what;
  }
}

// run_many (step_many.hip; step_rows.h documents the rows, the carry rule and the fences) under a
// mask, and with a stop state where Until.  ONE family for every request: which rows are asked for
// (m.row[i], r.fin[i], r.layer, r.n_level, sp.row, hp.row), whether episode starts are registered
// (st.bank), and with Until which conditions stop a world (um->stop) and which of stopped / ran /
// returns are asked for are runtime, wave-uniform tests.
//
// The mask.  The wave reads its world's column ONCE, in front of the record: lane l loads the bytes
// of steps l, l + 64, ... (K <= 4096: 64 loads a lane at most) and keeps them as the bits of one
// 64-bit value, so step k's byte is bit k / 64 of lane k % 64 — a v_readlane with a wave-uniform
// lane, and no memory access in the loop.  (With one row for every step, or K = 1, it is the one
// byte.)  The loop does NOT fetch step k + 1's byte beside step k + 1's action ids: that load's
// s_waitcnt vmcnt(0) behind a step that may have been skipped also waits for the record's write-back
// of a step that ran — stores "nobody waits for" (step_rows.h) — and cost 1 us a step on clean_up
// (profiles/r21_step_active.md).  The same loads say whether the world has an active step at all.
// Without Until there is always a mask; with it am.active may be NULL: every bit is set.
//  * an active step is run_many's step: frozen carry, step_world, a registered start behind an
//    auto-reset, the post-step rows.
//  * a skipped step runs no level code and writes nothing of the world's: neither the record nor
//    an in-place buffer.  Where rows are asked for, row k of the five kinds and of r.fin is copied
//    from `prev` (row k - 1, or the in-place buffer for k = 0) — the carry rule, by the lanes that
//    stored the elements — and the level kinds, LAYER, the state row and the hash row come out of
//    the same post-step block as ever, which reads the unchanged in-place buffers and the
//    unchanged record in LDS.  A world never reset writes nothing.
//  * a world with no active step in the whole request is known BEFORE the record is requested:
//    for K = 1 (or one row for every step) that is the byte itself, otherwise a ballot over the
//    lanes' bits of the column.  Such a wave neither loads nor stores its record: it takes part in
//    load_tables and the barrier like a wave with w >= num_worlds and returns — after writing its
//    rows where rows are asked for, all of them carried from the in-place buffers (`started` is
//    then the one word of the record it reads).  Only rows that are functions of the record
//    (LAYER, the state row, the hash row) make it load the record (and never store it).  This is
//    what makes a sparse mask cheap.
//
// The stop state (Until) is the wave's: `halted` (an SGPR) holds the reason bits, and step k runs
// where the mask's bit is set and halted == 0.  A world whose `stopped` byte is non-zero on entry
// is a world with no active step: it takes the early path above, writes ran = 0 and returns = 0
// and leaves its byte alone.
//  * LAST is read from the record's tail in LDS behind a step that ran: done.  That is exactly
//    when the step left STEP_TYPE 2 — a level's step stores done and hands finish() done ? 2 : 1,
//    a reset clears done and hands it 0, the frozen step (dispatch()) leaves done set and writes
//    2, and load_world (a registered start) writes done ? 2 : 0 of the record it loaded.  Every one
//    of them writes the tail in front of a wsync() of its own, so no fence is added here.
//  * REWARD: player p's reward of the step is stored by lane p (finish(), dispatch()'s frozen
//    path, load_world), so lane p loads its own element of the step's row back, in program order.
//    With MP_STOP_REWARD the value is needed at once — a ballot of r != 0 — and that load's
//    s_waitcnt vmcnt(0) also waits for the record's write-back (see the mask for what that
//    costs).  Without it the value is only summed: it is consumed one step late, beside the next
//    step's action ids, where the loop waits for memory anyway.
//  * returns: g = 1; for each step that ran: ret += g * r; g *= gamma — every multiply and add
//    rounded on its own (__dmul_rn, __dadd_rn: no FMA), each lane its player's sum.
//  * a stopped world with no rows asked for leaves the loop: nothing more is written for it.
// ran counts the steps of a started world (a world never reset runs nothing and never stops).
//
// The list (Listed, always with Until) gives the wave TWO indices where the others have one:
//  * the world w = worlds[i], a wave-uniform load in front of everything, for the record, the
//    in-place buffers, next_orders, `stopped` and the registration's rows[];
//  * the column i, the wave's own number, for the actions, the mask, the per-step rows, ran and
//    returns.  The rows of the five kinds and of r.fin are reached through bases shifted by
//    d = i - w worlds (row_of, step_rows.h), the level kinds, LAYER, the state row and the hash row
//    by i itself.
// A wave whose entry is no world, or whose world's claim word holds another entry's tag
// (listed_tag, mp_common.h; k_claim_listed, step_listed.hip, ran in front of this launch), is a
// wave past the end of the list: it takes part in load_tables and the barrier and returns, having
// written nothing but the report (report_entry).  Without Listed w is i, d is 0, and a wave is live
// where w < num_worlds.
template <class Tables, class Sites, bool Until, bool Listed = false>
__device__ inline void run_many_masked(const DevTables& t, const Tables& c, const StepArgs& args0,
                                       const ManyArgs& m, const StepRows& r, int extra,
                                       const StateRows& sp, const HashRows& hp, const StartArgs& st,
                                       const ActiveArgs& am, const UntilArgs* um = nullptr,
                                       const ListArgs* la = nullptr) {
  static_assert(Until || !Listed, "a world list comes with the stop state (MpStepListed)");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int i = blockIdx.x * ((int)blockDim.x >> 6) + wave;
  uint8_t* tables = smem;
  const int per_world = t.world_stride + scratch_bytes(t) + extra;
  uint8_t* mine = smem + tables_bytes(t) + wave * per_world;
  bool live;
  int w;
  if constexpr (Listed) {
    live = i < la->count;
    w = 0;
    if (live) {
      w = __builtin_amdgcn_readfirstlane(la->worlds[i]);
      if (w < 0 || w >= args0.num_worlds) {
        report_entry(t, lane, i, w, kFaultListedWorld);
        live = false;
        w = 0;
      } else {
        const unsigned long long tag = listed_tag(la->generation, i);
        const unsigned long long own = la->claim[w];
        const uint32_t own_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)own);
        const uint32_t own_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(own >> 32));
        if ((((unsigned long long)own_hi << 32) | own_lo) != tag) {
          report_entry(t, lane, i, w, kFaultListedRepeat);
          live = false;
          w = 0;
        }
      }
    }
  } else {
    w = i;
    live = w < args0.num_worlds;
  }
  const long long d = Listed ? (long long)i - (long long)w : 0;
  World wd = make_world(t, mine, tables, mine + t.world_stride, args0.state, (Listed || live) ? w : 0, lane);
  wd.next_orders = args0.next_orders;
  const int K = m.steps;
  const bool record_rows = r.layer || sp.row || hp.row;
  const bool any_rows = record_rows || r.n_level || m.row[0] || m.row[1] || m.row[2] || m.row[3] || m.row[4] ||
                        r.fin[0] || r.fin[1] || r.fin[2] || r.fin[3];
  int act_id = 0;
  const bool column = (!Until || am.active) && K > 1 && am.step != 0;   // (otherwise one byte, or none, says it for every step)
  unsigned long long bits = 0;   // column: bit j = the byte of step lane + 64 j; otherwise: the one byte
  bool any = false;              // is there an active step at all?
  Sites sites = Sites();
  if (live) {
    act_id = fetch_action_id(t, args0.actions, args0.mode, i, lane);
    if (column) {
      for (int j = 0, k = lane; k < K; ++j, k += 64)
        bits |= (unsigned long long)(am.active[(long long)k * am.step + i] != 0) << j;
    } else {
      bits = (!Until || am.active) ? am.active[i] != 0 : 1;
    }
    if constexpr (Until)   // (stopped on entry: a world with no active step, whatever the mask says)
      if (um->stopped && __builtin_amdgcn_readfirstlane((int)um->stopped[w]) != 0) bits = 0;
    any = __ballot(bits != 0ull) != 0ull;
    if (any || record_rows) {
      sites = load_sites(c, lane);
      load_record(t, wd.rec, wd.gw, lane);
    }
  }
  load_tables(t, tables, (int)threadIdx.x, (int)blockDim.x);
  clear_marks(t, wd.mark, lane);
  begin_step(wd.sc, lane);
  __syncthreads();
  if (!live) return;
  if constexpr (Until) {
    if (!any) {   // (nothing runs: the counts are known now)
      if (um->ran && lane == 0) um->ran[i] = 0;
      if (um->returns && lane < t.P) um->returns[(size_t)i * t.P + lane] = 0.0;
    }
  }
  if (!any && !record_rows) {
    // no step to run and no row that needs the record: the rows, carried from the in-place buffers
    if (!any_rows) return;
    const WorldTail* gt = reinterpret_cast<const WorldTail*>(wd.gw + t.grid_pad);
    if (!__builtin_amdgcn_readfirstlane((int)gt->started)) return;
    for (int k = 0; k < K; ++k) {
      const StepOutputs to = outputs_of_row(args0.out, m, r, k, d, t.P);
      carry_five(t, m, to, args0.out, w, lane);
      carry_fin(t, r, to, args0.out, w, lane);
      copy_level_rows(r, k, w, i, lane);
    }
    return;
  }
  init_extra(t, c, wd.extra, lane);
  StepArgs args = args0;
  bool ran = false;   // did the step before this one run?
  // the stop state (without Until these keep their first values, and the compiler drops them)
  int halted = 0;     // the reason bits of the step that stopped this world (wave-uniform)
  int n_ran = 0;      // the steps it ran
  const bool sums = Until && um->returns != nullptr;
  const bool paid = Until && (um->stop & MP_STOP_REWARD) != 0;
  double ret = 0.0, g = 1.0, owed = 0.0;   // (lane p: player p's sum; owed: a reward not summed yet)
  bool owing = false;
  for (int k = 0; k < K; ++k) {
    int next_id = 0;
    if (k + 1 < K)
      next_id = fetch_action_id(t, args0.actions + (long long)(k + 1) * m.actions_step, args0.mode, i, lane);
    if constexpr (Until) {
      if (owing) {   // the step before's reward, loaded behind that step
        ret = __dadd_rn(ret, __dmul_rn(g, owed));
        g = __dmul_rn(g, um->gamma);
        owing = false;
      }
    }
    bool on = any && halted == 0;
    if (column) {
      const unsigned lo = (unsigned)rdlane((int)(unsigned)bits, k & 63);
      const unsigned hi = (unsigned)rdlane((int)(unsigned)(bits >> 32), k & 63);
      on = halted == 0 && (((((unsigned long long)hi << 32) | lo) >> (k >> 6)) & 1ull) != 0ull;
    }
    if (k) {
      wsync();   // finish() has read the record for its write-back; the row copies have read theirs
      if (ran) begin_step(wd.sc, lane);
      wsync();
    }
    // (one step's code is one step's: see run_many)
    int lane_k = lane;
    asm volatile("" : "+v"(lane_k));
    wd.lane = lane_k;
    const WorldTail* tl = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
    const StepOutputs prev = args.out;   // row k - 1, or the in-place buffers
    args.out = outputs_of_row(args0.out, m, r, k, d, t.P);
    if (on) {
      // (dispatch()'s frozen path, which this step is going to take)
      const bool frozen = __builtin_amdgcn_readfirstlane((int)(tl->started && tl->done)) && !args0.auto_reset;
      if (frozen) carry_fin(t, r, args.out, prev, w, lane_k);
      const Action act = lookup_action(t, wd, act_id, args0.mode);
      // (step_or_load<true>, step_load.h, with the registration as a runtime test)
      const int row = st.bank && starts_here(tl, args) ? start_row(t, st, w, lane_k) : -1;
      const bool started = Until && __builtin_amdgcn_readfirstlane((int)tl->started) != 0;
      step_world(t, c, sites, wd, act, args);
      if (row >= 0) start_world(t, c, wd, args, st);
      if constexpr (Until) {
        if (started) {   // (a world never reset ran nothing)
          ++n_ran;
          if ((um->stop & MP_STOP_LAST) && __builtin_amdgcn_readfirstlane((int)tl->done)) halted |= MP_STOP_LAST;
          if (sums || paid) {
            const double rw = lane_k < t.P ? args.out.reward[(size_t)w * t.P + lane_k] : 0.0;
            if (paid) {
              if (__ballot(rw != 0.0) != 0ull) halted |= MP_STOP_REWARD;
              ret = __dadd_rn(ret, __dmul_rn(g, rw));
              g = __dmul_rn(g, um->gamma);
            } else {
              owed = rw;
              owing = true;
            }
          }
        }
      }
    } else if (__builtin_amdgcn_readfirstlane((int)tl->started)) {
      carry_five(t, m, args.out, prev, w, lane_k);
      carry_fin(t, r, args.out, prev, w, lane_k);
    }
    ran = on;
    act_id = next_id;
    if (sp.row || hp.row || r.layer || r.n_level) {
      wsync();   // the record in LDS is final; the step's stores to the level kinds come before the loads below
      if (__builtin_amdgcn_readfirstlane((int)tl->started)) {
        copy_level_rows(r, k, w, i, lane_k);
        if (r.layer) {
          StepOutputs lo = args0.out;
          lo.layer = reinterpret_cast<int32_t*>(r.layer + (long long)k * r.layer_bytes);
          lo.layer_lut = r.layer_lut;
          write_layer(t, wd.rec, lo, i, lane_k);
        }
        if (sp.row)
          store_record(t, wd.rec, sp.row + (long long)k * sp.bytes + (size_t)i * t.world_stride, lane_k);
        if (hp.row) {
          const uint64_t sum =
              state_hash::wave_sum(state_hash::hash_share(hp.mask, wd.rec, t.world_stride >> 4, lane_k, 64));
          if (lane_k == 0)
            reinterpret_cast<uint64_t*>(hp.row + (long long)k * hp.bytes)[i] = state_hash::fmix64(sum);
        }
      }
    }
    if (Until && halted != 0 && !any_rows) break;   // (stopped, and no row left to carry)
  }
  if (!any) return;   // (only the rows wanted the record: the in-place buffers are what they were)
  if constexpr (Until) {
    if (owing) ret = __dadd_rn(ret, __dmul_rn(g, owed));
    if (um->ran && lane == 0) um->ran[i] = n_ran;
    if (um->returns && lane < t.P) um->returns[(size_t)i * t.P + lane] = ret;
    if (um->stopped && halted != 0 && lane == 0) um->stopped[w] = (uint8_t)halted;
  }
  wsync();
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
  // row K - 1 of every kind that has rows, in place too (a world never reset wrote nothing)
  if (__builtin_amdgcn_readfirstlane((int)tail->started)) {
    carry_five(t, m, args0.out, args.out, w, lane);
    carry_fin(t, r, args0.out, args.out, w, lane);
  }
  if (args0.out.layer) write_layer(t, wd.rec, args0.out, w, lane);
}

}  // namespace stepk

#endif  // MP_STEP_MASKED_H_
