// step_until.hip — the K-step kernels with stop conditions (MpStepUntil, include/mp_engine.h): the
// masked request of step_active.hip in which a world that ends its episode, or is paid, stops
// there for the rest of the launch, and which hands back how many steps each world ran and the
// discounted sum of its rewards over them.  A unit of its own, with its own copy of
// run_many_active's body (step_active.hip): the families of step_many.hip, step_active.hip,
// step_kernels.hip and step_starts.hip are compiled from exactly what they were compiled from
// before, one caller of each level's step in their unit (step_starts.hip says why).
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
#include "step_until.h"
#include "state_hash.h"

namespace {

using namespace stepk;

constexpr int kWorldsPerGroup = 4;   // (step_kernels.hip)

template <class T>
__device__ inline T* row_of(uint8_t* base, long long bytes, int k, T* in_place) {
  return base ? reinterpret_cast<T*>(base + (long long)k * bytes) : in_place;
}

// The outputs of step k: row k of every kind of the five and of r.fin that is asked for, the
// in-place buffer of the others.
__device__ inline StepOutputs outputs_of_row(const StepOutputs& in_place, const ManyArgs& m, const StepRows& r, int k) {
  StepOutputs o = in_place;
  o.reward = row_of(m.row[0], m.row_bytes[0], k, in_place.reward);
  o.collective = row_of(m.row[1], m.row_bytes[1], k, in_place.collective);
  o.step_type = row_of(m.row[2], m.row_bytes[2], k, in_place.step_type);
  o.discount = row_of(m.row[3], m.row_bytes[3], k, in_place.discount);
  o.events = row_of(m.row[4], m.row_bytes[4], k, in_place.events);
  o.ready = row_of(r.fin[0], r.fin_bytes[0], k, in_place.ready);
  o.aux0 = row_of(r.fin[1], r.fin_bytes[1], k, in_place.aux0);
  o.position = row_of(r.fin[2], r.fin_bytes[2], k, in_place.position);
  o.orientation = row_of(r.fin[3], r.fin_bytes[3], k, in_place.orientation);
  return o;
}

// READY_TO_SHOOT, AUX0, POSITION and ORIENTATION of world w, where asked for as rows: `from` ->
// `to`, each lane its own element (what run_many does in front of a frozen step).
__device__ inline void carry_fin(const DevTables& t, const StepRows& r, const StepOutputs& to,
                                 const StepOutputs& from, int w, int lane) {
  if (lane >= t.P) return;
  const size_t o = (size_t)w * t.P + lane;
  if (r.fin[0]) to.ready[o] = from.ready[o];
  if (r.fin[1]) to.aux0[o] = from.aux0[o];
  if (r.fin[2]) {
    to.position[o * 2 + 0] = from.position[o * 2 + 0];
    to.position[o * 2 + 1] = from.position[o * 2 + 1];
  }
  if (r.fin[3]) to.orientation[o] = from.orientation[o];
}

// REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT and EVENTS (the header row and the rows it
// counts) of world w, where asked for as rows: `from` -> `to` (what run_many does from row K - 1
// to the in-place buffers in the end).
__device__ inline void carry_five(const DevTables& t, const ManyArgs& m, const StepOutputs& to,
                                  const StepOutputs& from, int w, int lane) {
  const size_t o = (size_t)w * t.P + lane;
  if (m.row[0] && lane < t.P) to.reward[o] = from.reward[o];
  if (lane == 0) {
    if (m.row[1]) to.collective[w] = from.collective[w];
    if (m.row[2]) to.step_type[w] = from.step_type[w];
    if (m.row[3]) to.discount[w] = from.discount[w];
  }
  if (m.row[4]) {
    const int4* src = reinterpret_cast<const int4*>(from.events) + (size_t)w * MP_EVENT_ROWS;
    int4* dst = reinterpret_cast<int4*>(to.events) + (size_t)w * MP_EVENT_ROWS;
    int n = 0;
    if (lane == 0) { const int4 h = src[0]; dst[0] = h; n = h.x; }
    n = __builtin_amdgcn_readfirstlane(n);
    n = n < 0 ? 0 : n > MP_EVENT_ROWS - 1 ? MP_EVENT_ROWS - 1 : n;
    for (int i = lane; i < n; i += 64) dst[1 + i] = src[1 + i];
  }
}

// The level kinds of world w (StepRows::level): the in-place buffer -> row k.
__device__ inline void copy_level_rows(const StepRows& r, int k, int w, int lane) {
  for (int i = 0; i < r.n_level; ++i) {
    const long long n = r.level[i].count;
    const double* src = r.level[i].src + (size_t)w * n;
    double* dst = reinterpret_cast<double*>(r.level[i].row + (long long)k * r.level[i].bytes) + (size_t)w * n;
    for (int j = lane; j < n; j += 64) dst[j] = src[j];
  }
}

// run_many_active (step_active.hip, whose text on the mask, the skipped step and the no-step early
// path follows as it stands there) with a stop state.  ONE family for every request: which rows
// are asked for (m.row[i], r.fin[i], r.layer, r.n_level, sp.row, hp.row), whether episode starts
// are registered (st.bank), which conditions stop a world (um.stop) and which of stopped / ran /
// returns are asked for are runtime, wave-uniform tests.
//
// The stop state is the wave's: `halted` (an SGPR) holds the reason bits, and step k runs where
// the mask's bit is set and halted == 0.  A world whose `stopped` byte is non-zero on entry is a
// world with no active step: it takes the early path below (neither loads nor stores its record),
// writes ran = 0 and returns = 0 and leaves its byte alone.  Without a mask (am.active == NULL)
// every bit is set.
//  * LAST is read from the record's tail in LDS behind a step that ran: done.  That is exactly
//    when the step left STEP_TYPE 2 — a level's step stores done and hands finish() done ? 2 : 1,
//    a reset clears done and hands it 0, the frozen step (dispatch()) leaves done set and writes
//    2, and load_world (a registered start) writes done ? 2 : 0 of the record it loaded.  Every one
//    of them writes the tail in front of a wsync() of its own, so no fence is added here.
//  * REWARD: player p's reward of the step is stored by lane p (finish(), dispatch()'s frozen
//    path, load_world), so lane p loads its own element of the step's row back, in program order.
//    With MP_STOP_REWARD the value is needed at once — a ballot of r != 0 — and that load's
//    s_waitcnt vmcnt(0) also waits for the record's write-back (step_active.hip says what that
//    costs).  Without it the value is only summed: it is consumed one step late, beside the next
//    step's action ids, where the loop waits for memory anyway.
//  * returns: g = 1; for each step that ran: ret += g * r; g *= gamma — every multiply and add
//    rounded on its own (__dmul_rn, __dadd_rn: no FMA), each lane its player's sum.
//  * a stopped world with no rows asked for leaves the loop: nothing more is written for it.
// ran counts the steps of a started world (a world never reset runs nothing and never stops).
//
// The mask.  The wave reads its world's column ONCE, in front of the record: lane l loads the bytes
// of steps l, l + 64, ... (K <= 4096: 64 loads a lane at most) and keeps them as the bits of one
// 64-bit value, so step k's byte is bit k / 64 of lane k % 64 — a v_readlane with a wave-uniform
// lane, and no memory access in the loop.  (With one row for every step, or K = 1, it is the one
// byte.)  The loop does NOT fetch step k + 1's byte beside step k + 1's action ids: that load's
// s_waitcnt vmcnt(0) behind a step that may have been skipped also waits for the record's write-back
// of a step that ran — stores "nobody waits for" (run_many) — and cost 1 us a step on clean_up
// (profiles/r21_step_active.md).  The same loads say whether the world has an active step at all.
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
//    rows where rows are asked for, all of
//    them carried from the in-place buffers (`started` is then the one word of the record it
//    reads).  Only rows that are functions of the record (LAYER, the state row, the hash row)
//    make it load the record (and never store it).  This is what makes a sparse mask cheap.
template <class Tables, class Sites>
__device__ inline void run_many_until(const DevTables& t, const Tables& c, const StepArgs& args0,
                                       const ManyArgs& m, const StepRows& r, int extra,
                                      const StateRows& sp, const HashRows& hp, const StartArgs& st,
                                      const ActiveArgs& am, const UntilArgs& um) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int w = blockIdx.x * ((int)blockDim.x >> 6) + wave;
  uint8_t* tables = smem;
  const int per_world = t.world_stride + scratch_bytes(t) + extra;
  uint8_t* mine = smem + tables_bytes(t) + wave * per_world;
  const bool live = w < args0.num_worlds;
  World wd = make_world(t, mine, tables, mine + t.world_stride, args0.state, live ? w : 0, lane);
  wd.next_orders = args0.next_orders;
  const int K = m.steps;
  const bool record_rows = r.layer || sp.row || hp.row;
  const bool any_rows = record_rows || r.n_level || m.row[0] || m.row[1] || m.row[2] || m.row[3] || m.row[4] ||
                        r.fin[0] || r.fin[1] || r.fin[2] || r.fin[3];
  int act_id = 0;
  const bool column = am.active && K > 1 && am.step != 0;   // (otherwise one byte, or none, says it for every step)
  unsigned long long bits = 0;   // column: bit j = the byte of step lane + 64 j; otherwise: the one byte
  bool any = false;              // is there an active step at all?
  Sites sites = Sites();
  if (live) {
    act_id = fetch_action_id(t, args0.actions, args0.mode, w, lane);
    if (column) {
      for (int j = 0, k = lane; k < K; ++j, k += 64)
        bits |= (unsigned long long)(am.active[(long long)k * am.step + w] != 0) << j;
    } else {
      bits = am.active ? am.active[w] != 0 : 1;
    }
    // (stopped on entry: a world with no active step, whatever the mask says)
    if (um.stopped && __builtin_amdgcn_readfirstlane((int)um.stopped[w]) != 0) bits = 0;
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
  if (!any) {   // (nothing runs: the counts are known now)
    if (um.ran && lane == 0) um.ran[w] = 0;
    if (um.returns && lane < t.P) um.returns[(size_t)w * t.P + lane] = 0.0;
  }
  if (!any && !record_rows) {
    // no step to run and no row that needs the record: the rows, carried from the in-place buffers
    if (!any_rows) return;
    const WorldTail* gt = reinterpret_cast<const WorldTail*>(wd.gw + t.grid_pad);
    if (!__builtin_amdgcn_readfirstlane((int)gt->started)) return;
    for (int k = 0; k < K; ++k) {
      const StepOutputs to = outputs_of_row(args0.out, m, r, k);
      carry_five(t, m, to, args0.out, w, lane);
      carry_fin(t, r, to, args0.out, w, lane);
      copy_level_rows(r, k, w, lane);
    }
    return;
  }
  init_extra(t, c, wd.extra, lane);
  StepArgs args = args0;
  bool ran = false;   // did the step before this one run?
  int halted = 0;     // the reason bits of the step that stopped this world (wave-uniform)
  int n_ran = 0;      // the steps it ran
  const bool sums = um.returns != nullptr;
  const bool paid = (um.stop & MP_STOP_REWARD) != 0;
  double ret = 0.0, g = 1.0, owed = 0.0;   // (lane p: player p's sum; owed: a reward not summed yet)
  bool owing = false;
  for (int k = 0; k < K; ++k) {
    int next_id = 0;
    if (k + 1 < K)
      next_id = fetch_action_id(t, args0.actions + (long long)(k + 1) * m.actions_step, args0.mode, w, lane);
    if (owing) {   // the step before's reward, loaded behind that step
      ret = __dadd_rn(ret, __dmul_rn(g, owed));
      g = __dmul_rn(g, um.gamma);
      owing = false;
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
    args.out = outputs_of_row(args0.out, m, r, k);
    if (on) {
      // (dispatch()'s frozen path, which this step is going to take)
      const bool frozen = __builtin_amdgcn_readfirstlane((int)(tl->started && tl->done)) && !args0.auto_reset;
      if (frozen) carry_fin(t, r, args.out, prev, w, lane_k);
      const Action act = lookup_action(t, wd, act_id, args0.mode);
      // (step_or_load<true>, step_load.h, with the registration as a runtime test)
      const int row = st.bank && starts_here(tl, args) ? start_row(t, st, w, lane_k) : -1;
      const bool started = __builtin_amdgcn_readfirstlane((int)tl->started) != 0;
      step_world(t, c, sites, wd, act, args);
      if (row >= 0) start_world(t, c, wd, args, st);
      if (started) {   // (a world never reset ran nothing)
        ++n_ran;
        if ((um.stop & MP_STOP_LAST) && __builtin_amdgcn_readfirstlane((int)tl->done)) halted |= MP_STOP_LAST;
        if (sums || paid) {
          const double rw = lane_k < t.P ? args.out.reward[(size_t)w * t.P + lane_k] : 0.0;
          if (paid) {
            if (__ballot(rw != 0.0) != 0ull) halted |= MP_STOP_REWARD;
            ret = __dadd_rn(ret, __dmul_rn(g, rw));
            g = __dmul_rn(g, um.gamma);
          } else {
            owed = rw;
            owing = true;
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
        copy_level_rows(r, k, w, lane_k);
        if (r.layer) {
          StepOutputs lo = args0.out;
          lo.layer = reinterpret_cast<int32_t*>(r.layer + (long long)k * r.layer_bytes);
          lo.layer_lut = r.layer_lut;
          write_layer(t, wd.rec, lo, w, lane_k);
        }
        if (sp.row)
          store_record(t, wd.rec, sp.row + (long long)k * sp.bytes + (size_t)w * t.world_stride, lane_k);
        if (hp.row) {
          const uint64_t sum =
              state_hash::wave_sum(state_hash::hash_share(hp.mask, wd.rec, t.world_stride >> 4, lane_k, 64));
          if (lane_k == 0)
            reinterpret_cast<uint64_t*>(hp.row + (long long)k * hp.bytes)[w] = state_hash::fmix64(sum);
        }
      }
    }
    if (halted != 0 && !any_rows) break;   // (stopped, and no row left to carry)
  }
  if (!any) return;   // (only the rows wanted the record: the in-place buffers are what they were)
  if (owing) ret = __dadd_rn(ret, __dmul_rn(g, owed));
  if (um.ran && lane == 0) um.ran[w] = n_ran;
  if (um.returns && lane < t.P) um.returns[(size_t)w * t.P + lane] = ret;
  if (um.stopped && halted != 0 && lane == 0) um.stopped[w] = (uint8_t)halted;
  wsync();
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
  // row K - 1 of every kind that has rows, in place too (a world never reset wrote nothing)
  if (__builtin_amdgcn_readfirstlane((int)tail->started)) {
    carry_five(t, m, args0.out, args.out, w, lane);
    carry_fin(t, r, args0.out, args.out, w, lane);
  }
  if (args0.out.layer) write_layer(t, wd.rec, args0.out, w, lane);
}

// (`waves`: the waves a SIMD is to hold, 0 for the compiler's choice.  coop's loop needs 132 VGPRs with
// the sum's six, one band above k_many_active_coop's 124: at 4096 worlds a CU then held 12 waves
// instead of 16 and a 64-step request took 1.24 of the masked one's time
// (profiles/r22_step_until.md).  Asked to keep four waves a SIMD the compiler fits it into 128.)
#define MP_WAVES_0
#define MP_WAVES_4 __attribute__((amdgpu_waves_per_eu(4, 4)))
#define MP_MANY_UNTIL_KERNEL(name, TablesT, SitesT, extra, waves)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) MP_WAVES_##waves void name(DevTables t, TablesT c, StepArgs args, \
                                                               ManyArgs m, StepRows r, StateRows s,  \
                                                               HashRows h, StartArgs st, ActiveArgs am, \
                                                               UntilArgs um) {                       \
    run_many_until<TablesT, SitesT>(t, c, args, m, r, extra, s, h, st, am, um);                      \
  }
MP_MANY_UNTIL_KERNEL(k_many_until_clean_up, CleanUpTables, CleanUpSites, 0, 0)
MP_MANY_UNTIL_KERNEL(k_many_until_commons, CommonsTables, CommonsSites, 0, 0)
MP_MANY_UNTIL_KERNEL(k_many_until_coins, CoinsTables, CoinsSites, 0, 0)
MP_MANY_UNTIL_KERNEL(k_many_until_coop, CoopTables, CoopSites, 0, 4)
MP_MANY_UNTIL_KERNEL(k_many_until_gift, GiftTables, GiftSites, 0, 0)
MP_MANY_UNTIL_KERNEL(k_many_until_cook, CookTables, CookSites, 0, 0)
MP_MANY_UNTIL_KERNEL(k_many_until_mushroom, MushroomTables, MushroomSites, extra_bytes(c), 0)
MP_MANY_UNTIL_KERNEL(k_many_until_matrix, MatrixTables, MatrixSites, 0, 0)
MP_MANY_UNTIL_KERNEL(k_many_until_territory, TerritoryTables, TerritorySites, extra_bytes(c), 0)
#undef MP_MANY_UNTIL_KERNEL
#undef MP_WAVES_0
#undef MP_WAVES_4

}  // namespace

// These kernels may take all 160 KB of a CU's LDS, like the ones they stand in for.
int prepare_step_until() {
  const void* k[9] = {
      reinterpret_cast<const void*>(&k_many_until_clean_up), reinterpret_cast<const void*>(&k_many_until_commons),
      reinterpret_cast<const void*>(&k_many_until_coins), reinterpret_cast<const void*>(&k_many_until_territory),
      reinterpret_cast<const void*>(&k_many_until_matrix), reinterpret_cast<const void*>(&k_many_until_coop),
      reinterpret_cast<const void*>(&k_many_until_gift), reinterpret_cast<const void*>(&k_many_until_cook),
      reinterpret_cast<const void*>(&k_many_until_mushroom)};
  for (const void* f : k)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return 1;
  return 0;
}

// launch_step_active (step_active.hip) with the stop state `u`: the same geometry, one family.
void launch_step_until(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                       const StepManyLaunch& l, const UntilArgs& u, hipStream_t stream) {
  const int wpg = step_worlds_per_group(t, s);
  const size_t lds = (size_t)step_lds_bytes(t, s, wpg);
  const dim3 grid((args.num_worlds + wpg - 1) / wpg), block(wpg * 64);
  StepRows r = l.rows;   // (the level kinds' sources: this submission's buffers)
  for (int i = 0; i < r.n_level; ++i) r.level[i].src = level_source(args.out, r.level[i].which);
  const stepk::StartArgs st = l.starts ? *l.starts : stepk::StartArgs{};
#define MP_LAUNCH(level, tables)                                                                  \
  hipLaunchKernelGGL(k_many_until_##level, grid, block, lds, stream, t, tables, args, l.many, r, l.state, l.hash, st, l.active, u); \
  break;
  switch (s.substrate) {
    case MPK_SUBSTRATE_CLEAN_UP: MP_LAUNCH(clean_up, s.cu)
    case MPK_SUBSTRATE_COMMONS_HARVEST: MP_LAUNCH(commons, s.ch)
    case MPK_SUBSTRATE_COINS: MP_LAUNCH(coins, s.co)
    case MPK_SUBSTRATE_TERRITORY: MP_LAUNCH(territory, s.tr)
    case MPK_SUBSTRATE_THE_MATRIX: MP_LAUNCH(matrix, s.mx)
    case MPK_SUBSTRATE_COOP_MINING: MP_LAUNCH(coop, s.cm)
    case MPK_SUBSTRATE_GIFT_REFINEMENTS: MP_LAUNCH(gift, s.gr)
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING: MP_LAUNCH(cook, s.cc)
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS: MP_LAUNCH(mushroom, s.em)
  }
#undef MP_LAUNCH
}
