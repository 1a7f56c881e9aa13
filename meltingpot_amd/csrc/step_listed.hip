// step_listed.hip — the K-step kernels of a world list (MpStepListed, include/mp_engine.h): the
// request of step_until.hip launched with one wave per ENTRY of a device index list instead of one
// per world of the engine, so count entries are ceil(count / 4) workgroups whatever N is, the
// running worlds sit four to a workgroup, and the actions, the mask and every per-call tensor have
// count columns.  In front of it the claim kernel, which decides which entry owns a world.  A unit
// of its own with its own copy of the body (run_many_masked, step_masked.h, is the text it was, and
// so is every kernel that is built from it: step_starts.hip says why a family keeps its own caller
// of each level's step).
#include "step_levels.h"
#include "step_listed.h"
#include "step_rows.h"

namespace {

using namespace stepk;

// One thread an entry: the entry's tag into its world's word, the maximum wins.  A value that is
// no world is never an index (the step kernel reports it).
__global__ __launch_bounds__(256) void k_claim_listed(const int32_t* __restrict__ worlds, int count,
                                                      int num_worlds, unsigned long long* claim,
                                                      uint32_t generation) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= count) return;
  const int w = worlds[i];
  if (w < 0 || w >= num_worlds) return;
  atomicMax(&claim[w], ((unsigned long long)generation << 32) | (unsigned long long)(~(uint32_t)i));
}

// Row k of a kind for the wave of entry i and world w: the level code (step_world, finish(),
// load_world) and the carry helpers of step_rows.h index every output by w, so the row's base is
// moved by (i - w) worlds' elements — `shift` bytes — and element w of it is column i.  The
// in-place buffers stay by world.
template <class T>
__device__ inline T* entry_row(uint8_t* base, long long bytes, int k, long long shift, T* in_place) {
  return base ? reinterpret_cast<T*>(base + (long long)k * bytes + shift) : in_place;
}

// outputs_of_row (step_rows.h) with the rows moved from world w to column i: d = i - w.
__device__ inline StepOutputs outputs_of_entry(const StepOutputs& in_place, const ManyArgs& m, const StepRows& r,
                                               int k, long long d, int P) {
  StepOutputs o = in_place;
  o.reward = entry_row(m.row[0], m.row_bytes[0], k, d * P * 8, in_place.reward);
  o.collective = entry_row(m.row[1], m.row_bytes[1], k, d * 8, in_place.collective);
  o.step_type = entry_row(m.row[2], m.row_bytes[2], k, d * 4, in_place.step_type);
  o.discount = entry_row(m.row[3], m.row_bytes[3], k, d * 8, in_place.discount);
  o.events = entry_row(m.row[4], m.row_bytes[4], k, d * (MP_EVENT_ROWS * 16), in_place.events);
  o.ready = entry_row(r.fin[0], r.fin_bytes[0], k, d * P * 8, in_place.ready);
  o.aux0 = entry_row(r.fin[1], r.fin_bytes[1], k, d * P * 8, in_place.aux0);
  o.position = entry_row(r.fin[2], r.fin_bytes[2], k, d * P * 8, in_place.position);
  o.orientation = entry_row(r.fin[3], r.fin_bytes[3], k, d * P * 4, in_place.orientation);
  return o;
}

// copy_level_rows (step_rows.h): world w's slice of the in-place buffer -> column i of row k.
__device__ inline void copy_level_entry(const StepRows& r, int k, int w, int i, int lane) {
  for (int l = 0; l < r.n_level; ++l) {
    const long long n = r.level[l].count;
    const double* src = r.level[l].src + (size_t)w * n;
    double* dst = reinterpret_cast<double*>(r.level[l].row + (long long)k * r.level[l].bytes) + (size_t)i * n;
    for (int j = lane; j < n; j += 64) dst[j] = src[j];
  }
}

// An entry the launch skips; one of a launch's is named (state_view.hip reports the same way).
__device__ inline void report_entry(const DevTables& t, int lane, int i, int value, uint32_t what) {
  if (lane == 0 && atomicCAS(&t.fault[FAULT_STATE_INDEX], 0u, (uint32_t)i + 1u) == 0u) {
    t.fault[FAULT_STATE_INDEX + 1] = (uint32_t)value;
    t.fault[FAULT_STATE_INDEX + 2] = what;
  }
}

// run_many_masked<.., Until = true> (step_masked.h documents the mask, the stop state, the rows and
// every fence) with TWO indices where that has one:
//  * the world w = worlds[i], a wave-uniform load in front of everything, for the record, the
//    in-place buffers, next_orders, `stopped` and the registration's rows[];
//  * the column i, the wave's own number, for the actions, the mask, the per-step rows, ran and
//    returns.
// A wave whose entry is no world, or whose world's claim word holds another entry's tag, is a wave
// past the end of the list: it takes part in load_tables and the barrier and returns, having
// written nothing but the report.  Everything else is that body's text.
template <class Tables, class Sites>
__device__ inline void run_many_listed(const DevTables& t, const Tables& c, const StepArgs& args0,
                                       const ManyArgs& m, const StepRows& r, int extra,
                                       const StateRows& sp, const HashRows& hp, const StartArgs& st,
                                       const ActiveArgs& am, const UntilArgs& um, const ListArgs& la) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int i = blockIdx.x * ((int)blockDim.x >> 6) + wave;
  uint8_t* tables = smem;
  const int per_world = t.world_stride + scratch_bytes(t) + extra;
  uint8_t* mine = smem + tables_bytes(t) + wave * per_world;
  bool live = i < la.count;
  int w = 0;
  if (live) {
    w = __builtin_amdgcn_readfirstlane(la.worlds[i]);
    if (w < 0 || w >= args0.num_worlds) {
      report_entry(t, lane, i, w, kFaultListedWorld);
      live = false;
      w = 0;
    } else {
      const unsigned long long tag = ((unsigned long long)la.generation << 32) | (unsigned long long)(~(uint32_t)i);
      const unsigned long long own = la.claim[w];
      const uint32_t own_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)own);
      const uint32_t own_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(own >> 32));
      if ((((unsigned long long)own_hi << 32) | own_lo) != tag) {
        report_entry(t, lane, i, w, kFaultListedRepeat);
        live = false;
        w = 0;
      }
    }
  }
  const long long d = (long long)i - (long long)w;
  World wd = make_world(t, mine, tables, mine + t.world_stride, args0.state, w, lane);
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
    act_id = fetch_action_id(t, args0.actions, args0.mode, i, lane);
    if (column) {
      for (int j = 0, k = lane; k < K; ++j, k += 64)
        bits |= (unsigned long long)(am.active[(long long)k * am.step + i] != 0) << j;
    } else {
      bits = am.active ? am.active[i] != 0 : 1;
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
    if (um.ran && lane == 0) um.ran[i] = 0;
    if (um.returns && lane < t.P) um.returns[(size_t)i * t.P + lane] = 0.0;
  }
  if (!any && !record_rows) {
    // no step to run and no row that needs the record: the rows, carried from the in-place buffers
    if (!any_rows) return;
    const WorldTail* gt = reinterpret_cast<const WorldTail*>(wd.gw + t.grid_pad);
    if (!__builtin_amdgcn_readfirstlane((int)gt->started)) return;
    for (int k = 0; k < K; ++k) {
      const StepOutputs to = outputs_of_entry(args0.out, m, r, k, d, t.P);
      carry_five(t, m, to, args0.out, w, lane);
      carry_fin(t, r, to, args0.out, w, lane);
      copy_level_entry(r, k, w, i, lane);
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
      next_id = fetch_action_id(t, args0.actions + (long long)(k + 1) * m.actions_step, args0.mode, i, lane);
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
    args.out = outputs_of_entry(args0.out, m, r, k, d, t.P);
    if (on) {
      // (dispatch()'s frozen path, which this step is going to take)
      const bool frozen = __builtin_amdgcn_readfirstlane((int)(tl->started && tl->done)) && !args0.auto_reset;
      if (frozen) carry_fin(t, r, args.out, prev, w, lane_k);
      const Action act = lookup_action(t, wd, act_id, args0.mode);
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
        copy_level_entry(r, k, w, i, lane_k);
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
    if (halted != 0 && !any_rows) break;   // (stopped, and no row left to carry)
  }
  if (!any) return;   // (only the rows wanted the record: the in-place buffers are what they were)
  if (owing) ret = __dadd_rn(ret, __dmul_rn(g, owed));
  if (um.ran && lane == 0) um.ran[i] = n_ran;
  if (um.returns && lane < t.P) um.returns[(size_t)i * t.P + lane] = ret;
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

// (coop's loop needs 130 VGPRs here, one band above k_many_active_coop's 124, as
// k_many_until_coop's did: asked to keep four waves a SIMD the compiler fits it into 128 — see
// step_until.hip.  The definition below inherits the attribute from this declaration.)
__global__ __attribute__((amdgpu_waves_per_eu(4, 4))) void k_many_listed_coop(
    DevTables, CoopTables, StepArgs, ManyArgs, StepRows, StateRows, HashRows, StartArgs, ActiveArgs, UntilArgs,
    ListArgs);

#define MP_MANY_LISTED_KERNEL(level, TablesT, SitesT, sub, member)                                   \
  __global__ __launch_bounds__(kWorldsPerGroup * 64) void k_many_listed_##level(                     \
      DevTables t, TablesT c, StepArgs args, ManyArgs m, StepRows r, StateRows s, HashRows h,        \
      StartArgs st, ActiveArgs am, UntilArgs um, ListArgs la) {                                      \
    run_many_listed<TablesT, SitesT>(t, c, args, m, r, extra_bytes(c), s, h, st, am, um, la);        \
  }
MP_STEP_LEVELS(MP_MANY_LISTED_KERNEL)
#undef MP_MANY_LISTED_KERNEL
// (a parameter list above that differs from the macro's would declare an overload without the attribute)
static_assert(&k_many_listed_coop != nullptr, "k_many_listed_coop: one declaration, one definition");

}  // namespace

int prepare_step_listed() {
#define MP_LEVEL(level, TablesT, SitesT, sub, member) reinterpret_cast<const void*>(&k_many_listed_##level),
  const void* const k[] = {MP_STEP_LEVELS(MP_LEVEL)};
#undef MP_LEVEL
  return step_take_all_lds(k);
}

// The claim launch, then launch_step_until's launch (step_until.hip) with the geometry of
// list.count worlds: one family.
void launch_step_listed(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const StepManyLaunch& l, const UntilArgs& u, const ListArgs& list,
                        hipStream_t stream) {
  hipLaunchKernelGGL(k_claim_listed, dim3((list.count + 255) / 256), dim3(256), 0, stream, list.worlds,
                     list.count, args.num_worlds, list.claim, list.generation);
  const StepGeometry g = step_geometry(t, s, list.count);
  const StepRows r = step_rows_of(l, args.out);
  const stepk::StartArgs st = l.starts ? *l.starts : stepk::StartArgs{};
#define MP_LEVEL(level, TablesT, SitesT, sub, member)                                              \
  case sub:                                                                                        \
    hipLaunchKernelGGL(k_many_listed_##level, g.grid, g.block, g.lds, stream, t, s.member, args,   \
                       l.many, r, l.state, l.hash, st, l.active, u, list);                         \
    break;
  switch (s.substrate) { MP_STEP_LEVELS(MP_LEVEL) }
#undef MP_LEVEL
}
