// step_many.hip — the K-step form of the stand-alone step kernels (MpStepMany,
// include/mp_engine.h): one wavefront per world as in step_kernels.hip, with the world's record
// resident in LDS across K steps of one launch.  A unit of its own: the single-step kernels and
// k_frame are compiled from exactly what they were compiled from before.
#include "step_levels.h"
#include "step_rows.h"

namespace {

using namespace stepk;

// K steps of one world (step_rows.h documents the loop, the rows, the carry rule and the fences).
// Five kernel families, each added so that the ones before it run exactly the code they ran:
//  * k_step_many_* (Rows = false): rows of the five kinds only, an MpStepMany request.
//  * k_step_rows_* (Rows): the rows of an MpStepTrajectory request, `rp`.
//  * k_step_states_* (States): the state rows too, always.  With the row as one more runtime
//    branch of k_step_rows_*, that family's LAYER rows cost 9 % more on clean_up
//    (profiles/r16_observe_states.md).
//  * k_step_hashes_* (Hashes): the hash rows, always; a request that names both rows runs this
//    family too: whether the record is stored as well is a runtime test (sp->row).
//  * k_many_starts_* (Starts, with Hashes): registered episode starts (MpEpisodeStarts, `st`).  A
//    step in which a world auto-resets runs start_world() behind the level's reset (step_load.h),
//    with the outputs of row k — so row k of every kind a start writes holds the start's values,
//    the level kinds are copied from the in-place buffer the start wrote, and LAYER, the state row
//    and the hash row come from the started record in LDS.  ONE family for every combination of
//    rows: which rows are asked for is a runtime test (r.fin[i], r.layer, sp->row, hp->row).
// The frozen carry, the level copy and the final copy are carry_fin, carry_five and copy_level_rows
// of step_rows.h written out: with the calls the four row families were scheduled differently and
// k_step_rows_clean_up's LAYER rows took 0.5 % longer (profiles/r23_kstep_refactor.md), so a change
// to the carry rule is made there AND here.
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

#define MP_STEP_MANY_KERNEL(level, TablesT, SitesT, sub, member)                                     \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_many_##level(DevTables t, TablesT c, \
                                                                             StepArgs args, ManyArgs m) { \
    run_many<false, false, TablesT, SitesT>(t, c, args, m, nullptr, extra_bytes(c));                 \
  }
MP_STEP_LEVELS(MP_STEP_MANY_KERNEL)
#undef MP_STEP_MANY_KERNEL

#define MP_STEP_ROWS_KERNEL(level, TablesT, SitesT, sub, member)                                     \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_rows_##level(                       \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r) {                               \
    run_many<true, false, TablesT, SitesT>(t, c, args, m, &r, extra_bytes(c));                       \
  }
MP_STEP_LEVELS(MP_STEP_ROWS_KERNEL)
#undef MP_STEP_ROWS_KERNEL

#define MP_STEP_STATES_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_states_##level(                     \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s) {                  \
    run_many<true, true, TablesT, SitesT>(t, c, args, m, &r, extra_bytes(c), &s);                    \
  }
MP_STEP_LEVELS(MP_STEP_STATES_KERNEL)
#undef MP_STEP_STATES_KERNEL

#define MP_STEP_HASHES_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_step_hashes_##level(                     \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s, HashRows h) {      \
    run_many<true, false, TablesT, SitesT, true>(t, c, args, m, &r, extra_bytes(c), &s, &h);         \
  }
MP_STEP_LEVELS(MP_STEP_HASHES_KERNEL)
#undef MP_STEP_HASHES_KERNEL

#define MP_MANY_STARTS_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_many_starts_##level(                     \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s, HashRows h, StartArgs st) { \
    run_many<true, false, TablesT, SitesT, true, true>(t, c, args, m, &r, extra_bytes(c), &s, &h, &st); \
  }
MP_STEP_LEVELS(MP_MANY_STARTS_KERNEL)
#undef MP_MANY_STARTS_KERNEL

}  // namespace

int prepare_step_many() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member)                                              \
  reinterpret_cast<const void*>(&k_step_many_##level), reinterpret_cast<const void*>(&k_step_rows_##level), \
      reinterpret_cast<const void*>(&k_step_states_##level), reinterpret_cast<const void*>(&k_step_hashes_##level), \
      reinterpret_cast<const void*>(&k_many_starts_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

// K steps of every world in one launch (MpStepMany, MpStepTrajectory): the geometry of
// launch_step.  l.any_rows == false: only rows of the five kinds, which runs k_step_many_*;
// l.state.row: the state rows, which runs k_step_states_*; l.hash.row: the hash rows (with or
// without the state rows), which runs k_step_hashes_*; l.starts: the engine's registered episode
// starts, which runs k_many_starts_* whatever the rows.
void launch_step_many(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                      const StepManyLaunch& l, hipStream_t stream) {
  const ManyArgs& m = l.many;
  const StepGeometry g = step_geometry(t, s, args.num_worlds);
  const StepRows r = step_rows_of(l, args.out);
#define MP_LAUNCH(kernel, ...) hipLaunchKernelGGL(kernel, g.grid, g.block, g.lds, stream, t, tables, args, __VA_ARGS__)
#define MP_LEVEL(level, TablesT, SitesT, sub, member)                                              \
  case sub: {                                                                                      \
    const TablesT& tables = s.member;                                                              \
    if (l.starts) MP_LAUNCH(k_many_starts_##level, m, r, l.state, l.hash, *l.starts);              \
    else if (l.hash.row) MP_LAUNCH(k_step_hashes_##level, m, r, l.state, l.hash);                  \
    else if (l.state.row) MP_LAUNCH(k_step_states_##level, m, r, l.state);                         \
    else if (l.any_rows) MP_LAUNCH(k_step_rows_##level, m, r);                                     \
    else MP_LAUNCH(k_step_many_##level, m);                                                        \
    break;                                                                                         \
  }
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
#undef MP_LAUNCH
}
