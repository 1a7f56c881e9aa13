// step_many.hip — the K-step form of the stand-alone step kernels (MpStepMany,
// include/mp_engine.h): one wavefront per world as in step_kernels.hip, with the world's record
// resident in LDS across K steps of one launch.  A unit of its own: the single-step kernels and
// k_frame are compiled from exactly what they were compiled from before.
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
#include "state_hash.h"

namespace {

using namespace stepk;

constexpr int kWorldsPerGroup = 4;   // (step_kernels.hip)

template <class T>
__device__ inline T* row_of(uint8_t* base, long long bytes, int k, T* in_place) {
  return base ? reinterpret_cast<T*>(base + (long long)k * bytes) : in_place;
}

// The K-step form of run_one_world: the tables, the site lists and the record are loaded once,
// the marks and the level's extras set up once (as a feeder of k_frame does for the worlds it
// steps one after the other on one scratch), and per step only the event scratch is cleared, the
// action looked up and the level's step run on the record in LDS.  Step k + 1's action ids are
// requested before step k's work.  finish() still stores the record after every step: those are
// stores nobody waits for, and the next step works on the LDS copy; the record HBM holds in the
// end is step K's.  The five per-step kinds go to row k of the caller's buffers where given; the
// wave then copies row K - 1 to the in-place buffers, every lane reading back exactly the words
// it stored itself (program order of one thread: no fence, no second launch).
//
// Rows (an MpStepTrajectory request, `r`): per-step rows of the other non-pixel kinds, row k =
// what the in-place buffer of the kind holds after step k of the loop of single steps.  That
// buffer KEEPS its value where a step does not write the kind, so the rows carry it:
//  * r.fin (READY_TO_SHOOT, AUX0, POSITION, ORIENTATION) are retargeted to row k like the five.
//    finish() writes them on every path but the frozen one (dispatch(): done without
//    auto-reset), element w * P + lane from lane `lane` (the_matrix's second store of READY
//    too).  Before a frozen step each lane copies its own element from row k - 1 (k = 0: from
//    the in-place buffer, stored by an earlier launch) to row k: it loads what it stored
//    itself, by finish() or by this copy one step earlier, so program order of one thread
//    covers it, and a step that is not frozen pays nothing.  Row K - 1 goes to the in-place
//    buffers in the end, lane by lane, as for the five.
//  * r.level: a level writes these where and when its rules say (INTERACTION_REWARDS from the
//    two lanes of an interaction, the zap matrix from the lane of the beam cell that hit), so
//    the step keeps writing the in-place buffer and the wave copies the world's slice of it to
//    row k after the step.  Here a lane does load words that OTHER lanes of its wave stored
//    during the step.  wsync() between the step and the loads orders them: a release and an
//    acquire fence at workgroup scope around a wave barrier.  Workgroup scope is enough, since
//    the stores and the loads come from one wave on one CU, and on gfx950 it costs no
//    instruction: outside threadgroup-split mode the compiler lowers these fences to a wait for
//    LDS only, because a CU's write-through vector L1 performs the vector memory instructions
//    of a wave in the order they were issued, so a load issued behind a store of the same CU
//    sees it (no L1 invalidate, no L2 write-back: nothing another CU could observe, tens of
//    cycles where the agent-scope forms cost microseconds).  The fences are still needed: they
//    are what keeps the compiler from moving the loads.  What the copy does cost is its own
//    s_waitcnt before the stores to row k: vmcnt counts loads and stores in one order, so the
//    loaded words arrive behind the record's write-back of finish().  Only a request that names
//    one of these kinds pays that.  The loop-top wsync() keeps the next step's stores to the
//    in-place buffer behind these loads.
//  * r.layer: write_layer() on row k from the record in LDS after every step of a started
//    world, a frozen one included (the same bytes again).
//  * the state rows (MP_STEP_ROW_STATE, `sp`, States = true: the k_step_states_* family):
//    store_record() of the record in LDS to row k after every step of a started world — the
//    bytes finish() has just written back to the world's own record, so what MP_STATES_SAVE
//    would copy from there.  It reads the LDS record behind the same wsync() as the layer row;
//    the loop-top wsync() keeps the next step's writes behind it.  A family of its own: with the
//    row as one more runtime branch of k_step_rows_*, that family's LAYER rows cost 9 % more on
//    clean_up (profiles/r16_observe_states.md); this way its code is what it was.
//  * the hash rows (MP_STEP_ROW_HASH, `hp`, Hashes = true: the k_step_hashes_* family): the hash
//    of the record in LDS (state_hash.h: every lane's share of the masked words, a wave-wide
//    sum, 8 bytes from lane 0) to element w of row k, behind the same wsync() and under the same
//    `started` test as the state row — so row k is the hash of what the state row's row k holds.
//    The mask's lines come from device memory (L2 after the first wave).  A request that names
//    both rows runs this family too: whether the record is stored as well is a runtime test
//    here and nowhere else (`sp->row`), and the three families above are what they were.
// Which kinds are asked for is wave-uniform: every branch on it is a scalar one.
//  * registered episode starts (MpEpisodeStarts, `st`, Starts = true: the k_many_starts_* family): a
//    step in which a world auto-resets runs start_world() behind the level's reset (step_load.h),
//    with the outputs of row k — so row k of every kind a start writes holds the start's values,
//    the level kinds are copied from the in-place buffer the start wrote, and LAYER, the state row
//    and the hash row come from the started record in LDS.  ONE family for every combination of
//    rows: which rows are asked for is a runtime test here (r.fin[i], r.layer, sp->row, hp->row),
//    as the state row is in k_step_hashes_*, and the four families above are what they were.
template <bool Rows, bool States, class Tables, class Sites, bool Hashes = false, bool Starts = false>
__device__ inline void run_many(const DevTables& t, const Tables& c, const StepArgs& args0,
                                const ManyArgs& m, const StepRows* rp, int extra,
                                const StateRows* sp = nullptr, const HashRows* hp = nullptr,
                                const StartArgs* st = nullptr) {
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
  int act_id = 0;
  Sites sites = Sites();
  if (live) {
    act_id = fetch_action_id(t, args0.actions, args0.mode, w, lane);
    sites = load_sites(c, lane);
    load_record(t, wd.rec, wd.gw, lane);
  }
  load_tables(t, tables, (int)threadIdx.x, (int)blockDim.x);
  clear_marks(t, wd.mark, lane);
  begin_step(wd.sc, lane);
  __syncthreads();
  if (!live) return;
  init_extra(t, c, wd.extra, lane);
  StepArgs args = args0;
  const int K = m.steps;
  for (int k = 0; k < K; ++k) {
    int next_id = 0;
    if (k + 1 < K)
      next_id = fetch_action_id(t, args0.actions + (long long)(k + 1) * m.actions_step, args0.mode, w, lane);
    if (k) {
      wsync();   // finish() has read the record for its write-back
      begin_step(wd.sc, lane);
      wsync();
    }
    // (one step's code is one step's: a lane index the compiler cannot see through keeps it from
    // hoisting every step-invariant value out of the loop and holding them all in registers)
    int lane_k = lane;
    asm volatile("" : "+v"(lane_k));
    wd.lane = lane_k;
    if constexpr (Rows) {
      const StepRows& r = *rp;
      const WorldTail* tl = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
      // (dispatch()'s frozen path, which this step is going to take)
      const bool frozen = __builtin_amdgcn_readfirstlane((int)(tl->started && tl->done)) && !args0.auto_reset;
      const StepOutputs prev = args.out;   // row k - 1, or the in-place buffers
      args.out.ready = row_of(r.fin[0], r.fin_bytes[0], k, args0.out.ready);
      args.out.aux0 = row_of(r.fin[1], r.fin_bytes[1], k, args0.out.aux0);
      args.out.position = row_of(r.fin[2], r.fin_bytes[2], k, args0.out.position);
      args.out.orientation = row_of(r.fin[3], r.fin_bytes[3], k, args0.out.orientation);
      if (frozen && lane_k < t.P) {
        const size_t o = (size_t)w * t.P + lane_k;
        if (r.fin[0]) args.out.ready[o] = prev.ready[o];
        if (r.fin[1]) args.out.aux0[o] = prev.aux0[o];
        if (r.fin[2]) {
          args.out.position[o * 2 + 0] = prev.position[o * 2 + 0];
          args.out.position[o * 2 + 1] = prev.position[o * 2 + 1];
        }
        if (r.fin[3]) args.out.orientation[o] = prev.orientation[o];
      }
    }
    args.out.reward = row_of(m.row[0], m.row_bytes[0], k, args0.out.reward);
    args.out.collective = row_of(m.row[1], m.row_bytes[1], k, args0.out.collective);
    args.out.step_type = row_of(m.row[2], m.row_bytes[2], k, args0.out.step_type);
    args.out.discount = row_of(m.row[3], m.row_bytes[3], k, args0.out.discount);
    args.out.events = row_of(m.row[4], m.row_bytes[4], k, args0.out.events);
    const Action act = lookup_action(t, wd, act_id, args0.mode);
    if constexpr (Starts) step_or_load<true>(t, c, sites, wd, act, args, st);
    else step_world(t, c, sites, wd, act, args);
    act_id = next_id;
    if constexpr (Rows) {
      const StepRows& r = *rp;
      if (States || (Hashes && !Starts) || (Starts && (sp->row || hp->row)) || r.layer || r.n_level) {
        wsync();   // the record in LDS is final; the step's stores to the level kinds come before the loads below
        const WorldTail* tl = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
        if (__builtin_amdgcn_readfirstlane((int)tl->started)) {
          for (int i = 0; i < r.n_level; ++i) {
            const long long n = r.level[i].count;
            const double* src = r.level[i].src + (size_t)w * n;
            double* dst = reinterpret_cast<double*>(r.level[i].row + (long long)k * r.level[i].bytes) + (size_t)w * n;
            for (int j = lane_k; j < n; j += 64) dst[j] = src[j];
          }
          if (r.layer) {
            StepOutputs lo = args0.out;
            lo.layer = reinterpret_cast<int32_t*>(r.layer + (long long)k * r.layer_bytes);
            lo.layer_lut = r.layer_lut;
            write_layer(t, wd.rec, lo, w, lane_k);
          }
          if constexpr (States)
            store_record(t, wd.rec, sp->row + (long long)k * sp->bytes + (size_t)w * t.world_stride, lane_k);
          if constexpr (Hashes) {
            if (sp->row)
              store_record(t, wd.rec, sp->row + (long long)k * sp->bytes + (size_t)w * t.world_stride, lane_k);
            if (!Starts || hp->row) {
            const uint64_t sum =
                state_hash::wave_sum(state_hash::hash_share(hp->mask, wd.rec, t.world_stride >> 4, lane_k, 64));
            if (lane_k == 0)
              reinterpret_cast<uint64_t*>(hp->row + (long long)k * hp->bytes)[w] = state_hash::fmix64(sum);
            }
          }
        }
      }
    }
  }
  wsync();
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(wd.rec + t.grid_pad);
  // step K's values of the five kinds, in place too (a world never reset wrote nothing)
  if (__builtin_amdgcn_readfirstlane((int)tail->started)) {
    const size_t o = (size_t)w * t.P + lane;
    if (m.row[0] && lane < t.P) args0.out.reward[o] = args.out.reward[o];
    if (lane == 0) {
      if (m.row[1]) args0.out.collective[w] = args.out.collective[w];
      if (m.row[2]) args0.out.step_type[w] = args.out.step_type[w];
      if (m.row[3]) args0.out.discount[w] = args.out.discount[w];
    }
    if (m.row[4]) {
      const int4* src = reinterpret_cast<const int4*>(args.out.events) + (size_t)w * MP_EVENT_ROWS;
      int4* dst = reinterpret_cast<int4*>(args0.out.events) + (size_t)w * MP_EVENT_ROWS;
      int n = 0;
      if (lane == 0) { const int4 h = src[0]; dst[0] = h; n = h.x; }
      n = __builtin_amdgcn_readfirstlane(n);
      n = n < 0 ? 0 : n > MP_EVENT_ROWS - 1 ? MP_EVENT_ROWS - 1 : n;
      for (int i = lane; i < n; i += 64) dst[1 + i] = src[1 + i];   // (row 1 + i: lane i % 64's own store)
    }
    if constexpr (Rows) {
      const StepRows& r = *rp;
      if (lane < t.P) {   // (element o: this lane's own store, by finish() or by the frozen steps' copy)
        if (r.fin[0]) args0.out.ready[o] = args.out.ready[o];
        if (r.fin[1]) args0.out.aux0[o] = args.out.aux0[o];
        if (r.fin[2]) {
          args0.out.position[o * 2 + 0] = args.out.position[o * 2 + 0];
          args0.out.position[o * 2 + 1] = args.out.position[o * 2 + 1];
        }
        if (r.fin[3]) args0.out.orientation[o] = args.out.orientation[o];
      }
    }
  }
  if (args0.out.layer) write_layer(t, wd.rec, args0.out, w, lane);
}

#define MP_STEP_MANY_KERNEL(name, TablesT, SitesT, extra)                                            \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void name(DevTables t, TablesT c, StepArgs args, \
                                                               ManyArgs m) {                         \
    run_many<false, false, TablesT, SitesT>(t, c, args, m, nullptr, extra);                          \
  }
MP_STEP_MANY_KERNEL(k_step_many_clean_up, CleanUpTables, CleanUpSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_commons, CommonsTables, CommonsSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_coins, CoinsTables, CoinsSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_coop, CoopTables, CoopSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_gift, GiftTables, GiftSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_cook, CookTables, CookSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_mushroom, MushroomTables, MushroomSites, extra_bytes(c))
MP_STEP_MANY_KERNEL(k_step_many_matrix, MatrixTables, MatrixSites, 0)
MP_STEP_MANY_KERNEL(k_step_many_territory, TerritoryTables, TerritorySites, extra_bytes(c))
#undef MP_STEP_MANY_KERNEL

// The same with the rows of an MpStepTrajectory request: a second family, so that an MpStepMany
// request runs exactly the code it ran before there was one.
#define MP_STEP_ROWS_KERNEL(name, TablesT, SitesT, extra)                                            \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void name(DevTables t, TablesT c, StepArgs args, \
                                                               ManyArgs m, StepRows r) {             \
    run_many<true, false, TablesT, SitesT>(t, c, args, m, &r, extra);                                \
  }
MP_STEP_ROWS_KERNEL(k_step_rows_clean_up, CleanUpTables, CleanUpSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_commons, CommonsTables, CommonsSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_coins, CoinsTables, CoinsSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_coop, CoopTables, CoopSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_gift, GiftTables, GiftSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_cook, CookTables, CookSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_mushroom, MushroomTables, MushroomSites, extra_bytes(c))
MP_STEP_ROWS_KERNEL(k_step_rows_matrix, MatrixTables, MatrixSites, 0)
MP_STEP_ROWS_KERNEL(k_step_rows_territory, TerritoryTables, TerritorySites, extra_bytes(c))
#undef MP_STEP_ROWS_KERNEL

// ... and with the per-step world states (MP_STEP_ROW_STATE) beside whatever other rows are asked
// for: a third family, so that the two above run exactly the code they ran before there was one.
#define MP_STEP_STATES_KERNEL(name, TablesT, SitesT, extra)                                          \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void name(DevTables t, TablesT c, StepArgs args, \
                                                               ManyArgs m, StepRows r, StateRows s) { \
    run_many<true, true, TablesT, SitesT>(t, c, args, m, &r, extra, &s);                             \
  }
MP_STEP_STATES_KERNEL(k_step_states_clean_up, CleanUpTables, CleanUpSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_commons, CommonsTables, CommonsSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_coins, CoinsTables, CoinsSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_coop, CoopTables, CoopSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_gift, GiftTables, GiftSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_cook, CookTables, CookSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_mushroom, MushroomTables, MushroomSites, extra_bytes(c))
MP_STEP_STATES_KERNEL(k_step_states_matrix, MatrixTables, MatrixSites, 0)
MP_STEP_STATES_KERNEL(k_step_states_territory, TerritoryTables, TerritorySites, extra_bytes(c))
#undef MP_STEP_STATES_KERNEL

// ... and with the per-step state hashes (MP_STEP_ROW_HASH), beside the state rows where the
// request names both: a fourth family, so that the three above run exactly the code they ran before
// there was one.
#define MP_STEP_HASHES_KERNEL(name, TablesT, SitesT, extra)                                          \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void name(DevTables t, TablesT c, StepArgs args, \
                                                               ManyArgs m, StepRows r, StateRows s,  \
                                                               HashRows h) {                         \
    run_many<true, false, TablesT, SitesT, true>(t, c, args, m, &r, extra, &s, &h);                  \
  }
MP_STEP_HASHES_KERNEL(k_step_hashes_clean_up, CleanUpTables, CleanUpSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_commons, CommonsTables, CommonsSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_coins, CoinsTables, CoinsSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_coop, CoopTables, CoopSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_gift, GiftTables, GiftSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_cook, CookTables, CookSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_mushroom, MushroomTables, MushroomSites, extra_bytes(c))
MP_STEP_HASHES_KERNEL(k_step_hashes_matrix, MatrixTables, MatrixSites, 0)
MP_STEP_HASHES_KERNEL(k_step_hashes_territory, TerritoryTables, TerritorySites, extra_bytes(c))
#undef MP_STEP_HASHES_KERNEL

// ... and with registered episode starts (MpEpisodeStarts), whatever rows the request names: a fifth
// family, so that the four above run exactly the code they ran before there was one.
#define MP_MANY_STARTS_KERNEL(name, TablesT, SitesT, extra)                                          \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void name(DevTables t, TablesT c, StepArgs args, \
                                                               ManyArgs m, StepRows r, StateRows s,  \
                                                               HashRows h, StartArgs st) {           \
    run_many<true, false, TablesT, SitesT, true, true>(t, c, args, m, &r, extra, &s, &h, &st);       \
  }
MP_MANY_STARTS_KERNEL(k_many_starts_clean_up, CleanUpTables, CleanUpSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_commons, CommonsTables, CommonsSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_coins, CoinsTables, CoinsSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_coop, CoopTables, CoopSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_gift, GiftTables, GiftSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_cook, CookTables, CookSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_mushroom, MushroomTables, MushroomSites, extra_bytes(c))
MP_MANY_STARTS_KERNEL(k_many_starts_matrix, MatrixTables, MatrixSites, 0)
MP_MANY_STARTS_KERNEL(k_many_starts_territory, TerritoryTables, TerritorySites, extra_bytes(c))
#undef MP_MANY_STARTS_KERNEL

}  // namespace

// The K-step kernels may take all 160 KB of a CU's LDS, like the single-step ones.
int prepare_step_many() {
  const void* km[45] = {
#define MP_BOTH(level)                                                                             \
  reinterpret_cast<const void*>(&k_step_many_##level), reinterpret_cast<const void*>(&k_step_rows_##level), \
      reinterpret_cast<const void*>(&k_step_states_##level), reinterpret_cast<const void*>(&k_step_hashes_##level), \
      reinterpret_cast<const void*>(&k_many_starts_##level)
      MP_BOTH(clean_up), MP_BOTH(commons), MP_BOTH(coins), MP_BOTH(territory), MP_BOTH(matrix),
      MP_BOTH(coop), MP_BOTH(gift), MP_BOTH(cook), MP_BOTH(mushroom)};
#undef MP_BOTH
  for (const void* f : km)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return 1;
  return 0;
}

// K steps of every world in one launch (MpStepMany, MpStepTrajectory): the geometry of
// launch_step.  l.any_rows == false: only rows of the five kinds, which runs k_step_many_*;
// l.state.row: the state rows, which runs k_step_states_*; l.hash.row: the hash rows (with or
// without the state rows), which runs k_step_hashes_*; l.starts: the engine's registered episode
// starts, which runs k_many_starts_* whatever the rows.
void launch_step_many(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                      const StepManyLaunch& l, hipStream_t stream) {
  const ManyArgs& m = l.many;
  const bool more = l.any_rows;
  const int wpg = step_worlds_per_group(t, s);
  const size_t lds = (size_t)step_lds_bytes(t, s, wpg);
  const dim3 grid((args.num_worlds + wpg - 1) / wpg), block(wpg * 64);
  StepRows r = l.rows;   // (the level kinds' sources: this submission's buffers)
  for (int i = 0; i < r.n_level; ++i) r.level[i].src = level_source(args.out, r.level[i].which);
#define MP_LAUNCH(level, tables)                                                                  \
  if (l.starts)                                                                                   \
    hipLaunchKernelGGL(k_many_starts_##level, grid, block, lds, stream, t, tables, args, m, r, l.state, l.hash, *l.starts); \
  else if (l.hash.row)                                                                                 \
    hipLaunchKernelGGL(k_step_hashes_##level, grid, block, lds, stream, t, tables, args, m, r, l.state, l.hash); \
  else if (l.state.row)                                                                           \
    hipLaunchKernelGGL(k_step_states_##level, grid, block, lds, stream, t, tables, args, m, r, l.state); \
  else if (more) hipLaunchKernelGGL(k_step_rows_##level, grid, block, lds, stream, t, tables, args, m, r); \
  else hipLaunchKernelGGL(k_step_many_##level, grid, block, lds, stream, t, tables, args, m);    \
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
