// step_one.h — one world of a stand-alone step launch: what every kernel of step_kernels.hip and
// of step_starts.hip runs (one wavefront per world, up to four worlds per workgroup).  Included by
// those two units only, inside their anonymous namespace, behind `using namespace stepk`.
#ifndef MP_STEP_ONE_H_
#define MP_STEP_ONE_H_

template <class Tables, class Sites, bool kStarts = false>
__device__ inline void run_one_world(const DevTables& t, const Tables& c, const StepArgs& args,
                                     int extra, const StartArgs* st = nullptr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  // (fewer waves than kWorldsPerGroup when the records of four do not fit: step_worlds_per_group)
  const int w = blockIdx.x * ((int)blockDim.x >> 6) + wave;
  // LDS: [tables][wave 0: record, scratch, marks, extra][wave 1: ...]...
  uint8_t* tables = smem;
  const int per_world = t.world_stride + scratch_bytes(t) + extra;
  uint8_t* mine = smem + tables_bytes(t) + wave * per_world;
  const bool live = w < args.num_worlds;
#ifdef MP_STEP_TIMING
  const unsigned long long t_entry = __builtin_readcyclecounter();
#endif
  World wd = make_world(t, mine, tables, mine + t.world_stride, args.state, live ? w : 0, lane);
  wd.next_orders = args.next_orders;
  // every global read of the step is issued here, before the first wait: the
  // action id, the site lists, the record, the tables — one trip to memory
  int act_id = 0;
  Sites sites = Sites();
  if (live) {
    act_id = fetch_action_id(t, args.actions, args.mode, w, lane);
    sites = load_sites(c, lane);
    load_record(t, wd.rec, wd.gw, lane);
  }
  load_tables(t, tables, (int)threadIdx.x, (int)blockDim.x);
  clear_marks(t, wd.mark, lane);
  begin_step(wd.sc, lane);
  __syncthreads();   // the tables are the one thing the waves of a group share
  if (!live) return;
#ifdef MP_STEP_TIMING
  if (lane == 0 && (w == 7 || w == 2000) && args.mode == STEP_MODE_STEP)
    printf("w %d: entry -> record in LDS %llu cycles\n", w, __builtin_readcyclecounter() - t_entry);
#endif
  const Action act = lookup_action(t, wd, act_id, args.mode);
  init_extra(t, c, wd.extra, lane);
  step_or_load<kStarts>(t, c, sites, wd, act, args, st);   // (mp_load_worlds, episode starts: step_load.h)
  // "N.LAYER", when bound: from the record while it is in LDS (frozen and masked-out worlds
  // included: their record is the one in HBM)
  if (args.out.layer) {
    wsync();
    write_layer(t, wd.rec, args.out, w, lane);
  }
}

#endif  // MP_STEP_ONE_H_
