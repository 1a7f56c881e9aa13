// mp_engine.hip — C ABI of libmp_engine.so (declared in include/mp_engine.h).
//
// Host side of the boundary that replaces dmlab2d.Lab2d / dmlab2d.Environment
// (reference: meltingpot/utils/substrates/builder.py:179-187,
// wrappers/base.py:38-84).  No CPU execution path exists here: every call that
// would compute needs a HIP device and fails loudly without one.
#include <chrono>
#include <cmath>
#include <map>
#include <mutex>
#include "../../include/mp_engine.h"

#include <stdarg.h>
#include <stddef.h>
#include <sys/types.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pack_decode.h"
#include "stock.h"
#include "step_common.h"
#include "step_many.h"
#include "step_until.h"
#include "step_listed.h"
#include "state_obs.h"
#include "state_view.h"
#include "state_check.h"
#include "state_hash.h"
#include "episode_stats.h"
#include "ego_layer.h"
#include "view_hash.h"
#include "ego_planes.h"
#include "avatar_ids.h"

// frame.hip
constexpr int kFaultWords = 64 + 4 * 16 * 64 * 2;   // fault words + the timeline build's log
// views: 0 = per-agent RGB, 1 = WORLD.RGB, 2 = both in one launch
FramePlan plan_frame(const DevTables& t, const SubstrateTables& s, int num_worlds,
                     bool with_step, int views, int num_cus, const MpDevOptions* dev,
                     int pool_k = 1,    // pool_k: the per-agent view pooled by 2, 4, 8 (1: full)
                     int world_k = 1);  // world_k: WORLD.RGB pooled by 2, 4, 8 (1: full)
// (views: what the plan draws, 0 / 1 / 2 as plan_frame's; a factor enters only with its view)
int frame_lds_bytes(const DevTables& t, const FramePlan& p, int pool_k = 1, int world_k = 1,
                    int views = 2);
int render_blob_bytes(const DevTables& t);
int prepare_frame();
void build_render_blob(const DevTables& t, const uint8_t* images, const uint16_t* img_slot,
                       const uint32_t* pair_table, const int32_t* state_sprite,
                       const int8_t* state_player, const int32_t* view_sprite_map,
                       const uint8_t* sprite_flags8, const int32_t* state_orient,
                       uint8_t* blob);
uint32_t render_visible_layers(const DevTables& t, const uint8_t* blob, const int32_t* state_layer);
void launch_frame(const DevTables& t, const SubstrateTables* s, const stepk::StepArgs& args,
                  uint8_t* out_a, uint8_t* out_w, const FramePlan& p, hipStream_t stream,
                  int pool_k = 1, int world_k = 1);

thread_local std::string g_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                       \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess)                                                   \
      return fail(MP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct MpEngine {
  int device = 0;
  int N = 0;
  int auto_reset = 0;
  hipStream_t stream = nullptr;
  int substrate = 0;
  DevTables t{};
  SubstrateTables sub{};
  // resource / token classes of "N.INVENTORY" (0: the level has no such observation)
  int inventory_types() const {
    return substrate == MPK_SUBSTRATE_THE_MATRIX ? sub.mx.R
           : substrate == MPK_SUBSTRATE_GIFT_REFINEMENTS ? sub.gr.ntypes : 0;
  }
  std::vector<uint8_t> pack;       // host copy
  uint8_t* d_pack = nullptr;       // device copy of the pack
  uint8_t* d_extra = nullptr;      // derived tables (opaque flags, state->player)
  uint8_t* d_stepblob = nullptr;   // the step kernels' LDS tables (step_common.h)
  uint8_t* d_debug = nullptr;      // engine-owned debug observations (MpConfig.debug_observations)
  uint32_t* h_fault = nullptr;     // DevTables::fault: pinned, device-mapped host memory [64]
  uint8_t* d_state = nullptr;      // [N][world_stride]
  uint8_t* d_scalars = nullptr;    // engine-owned scalar outputs
  size_t scalars_bytes = 0, debug_bytes = 0;   // of d_scalars / d_debug (mp_tune saves them)
  StepOutputs own{};               // views into d_scalars
  void* bound[MP_OBS_KINDS] = {};
  // The rollout ring (mp_bind_output_ring): submission t since the ring was bound writes
  // slot t % ring_slots of every ring-bound kind.  Between submissions bound[kind] of a ring
  // kind is the slot written LAST (what mp_observe reads); before anything was submitted,
  // slot 0.
  struct RingKind { uint8_t* base = nullptr; uint64_t stride = 0; };
  RingKind ring[MP_OBS_KINDS];
  int ring_slots = 0;              // 0: no kind is ring-bound
  uint64_t ring_cursor = 0;        // submissions since the ring was bound
  bool ring_hold = false;          // mp_tune: submissions stay on the slot it pointed at
  bool layer_hold = false;         // mp_tune: submissions leave a bound "N.LAYER" alone
  std::vector<FramePlan> ring_plan[3];   // [views]: the plan mp_tune kept for each slot (empty: plan[1][views])
  void point_ring(int slot, bool pixels_only = false) {
    for (int k = 0; k < MP_OBS_KINDS; ++k)
      if (ring[k].base && (!pixels_only || is_pixel_kind(k)))
        bound[k] = ring[k].base + (uint64_t)slot * ring[k].stride;
  }
  bool ring_has_pixels() const {
    for (int k = 0; k < MP_OBS_KINDS; ++k)
      if (ring[k].base && is_pixel_kind(k)) return true;
    return false;
  }
  // The per-agent view: MP_OBS_RGB or one of the pooled kinds (at most one of them is bound,
  // mp_bind_output) — what the frame launch draws into its out_a, pooled by pool_k()
  static int pool_of(int kind) {
    return kind == MP_OBS_RGB_POOL2 ? 2 : kind == MP_OBS_RGB_POOL4 ? 4 : kind == MP_OBS_RGB_POOL8 ? 8 : 1;
  }
  static bool is_pixel_kind(int kind) {
    return kind == MP_OBS_RGB || kind == MP_OBS_WORLD_RGB || pool_of(kind) > 1;
  }
  int agent_kind() const {
    for (int k : {MP_OBS_RGB_POOL2, MP_OBS_RGB_POOL4, MP_OBS_RGB_POOL8})
      if (bound[k]) return k;
    return MP_OBS_RGB;
  }
  uint8_t* agent_view() const { return (uint8_t*)bound[agent_kind()]; }
  int pool_k() const { return pool_of(agent_kind()); }
  // MpConfig.world_pool: MP_OBS_WORLD_RGB is pooled by this factor (2, 4, 8) everywhere, 1 = full.
  // A property of the engine: its plans (plan, pool_plan, ring_plan) are made for it.
  int world_pool = 1;
  // [k = 2, 4, 8][drawing only, stepping + drawing][agents, -, both]: the plans of the pooled views
  // (pool_ok: the pack's pooled atlas and span staging fit the LDS beside a ring of records)
  FramePlan pool_plan[3][2][3] = {};
  bool pool_ok[3] = {};
  static int pool_index(int k) { return k == 2 ? 0 : k == 4 ? 1 : 2; }
  FramePlan& frame_plan(int stepping, int views, int k) {
    return k > 1 ? pool_plan[pool_index(k)][stepping][views] : plan[stepping][views];
  }
  int32_t* d_actions = nullptr;    // staging for mp_step_host
  int32_t* d_fields = nullptr;     // staging for mp_step_fields_host
  uint8_t* d_mask = nullptr;       // staging for mp_reset
  uint64_t* d_seeds = nullptr;
  unsigned long long* d_ctr = nullptr;  // mp_counters accumulator
  // mp_step_host: ring of pinned, device-mapped action buffers
  static constexpr int kHostSlots = 4;
  int32_t* h_actions[kHostSlots] = {};
  hipEvent_t h_copied[kHostSlots] = {};
  uint64_t host_steps = 0;
  FramePlan plan[2][3] = {};       // frame kernel geometry [drawing only, stepping + drawing][agents, world view, both]
  int frame_launches = 0;          // parity of DevTables::claim's counters (FramePlan::parity)
  uint32_t* d_claim = nullptr;     // DevTables::claim
  int num_cus = 0;
  int next_orders = 1;             // StepArgs::next_orders (MpDevOptions.no_next_orders turns it off)
  bool has_dev = false;            // MpConfig.dev given: the plans are the caller's, mp_tune keeps them
  bool touched = false;            // reset / stepped / restored since creation (mp_tune: may it really step?)
  bool has_state = false;          // reset, restored or loaded since creation (MP_STATES_SAVE)
  uint64_t fingerprint = 0;        // MP_STATES_FINGERPRINT: what a record's layout and meaning depend on
  int unfused = 0;                 // MpConfig.unfused: 0 the engine's choice, 1 two launches, 2 one
  // The registered episode starts (an MpEpisodeStarts request; step_load.h: start_world): while set,
  // a stepping submission runs the k_step_starts_* / k_many_starts_* families and draws the bound
  // views in launches of their own.  starts_hold: mp_tune's probes step without it.
  stepk::StartArgs starts{};
  bool has_starts = false, starts_hold = false;
  bool starting() const { return has_starts && !starts_hold; }
  // The registered episode statistics (an MpEpisodeStats request; episode_stats.h): while set, every
  // submission is followed by one launch of k_episode_stats.  stats_hold: mp_tune's probes are not folded.
  episode_stats::Columns stats_cols{};
  episode_stats::Banks stats{};
  bool has_stats = false, stats_hold = false;
  bool folding() const { return has_stats && !stats_hold; }
  // A registered tensor of every viewer's window: while `dst` is set, every submission is followed
  // by one launch that rewrites it from the records the submission left.  slots > 0: a ring, slot
  // s at dst + s * stride bytes.  mask, classes (the caller's device table), num_classes, facing:
  // what the unit has of them.
  struct ViewRegistration {
    void* dst = nullptr;
    uint64_t stride = 0, mask = 0;
    int slots = 0;
    const int32_t* classes = nullptr;
    int32_t num_classes = 0, facing = 0;
    void* slot(int s) const { return slots > 0 ? (uint8_t*)dst + (uint64_t)(s % slots) * stride : dst; }
  };
  // ego: the EGO_LAYER leaf, int32 [N][P][VH][VW][L] (an MpEgoLayer request; ego_layer.h); vh: the
  // view hashes, u64 [N][P] (MpViewHash; view_hash.h); ep: the class and facing planes, uint8
  // [N][P][C'][VH][VW] (MpEgoPlanes; ego_planes.h); av and avz: AVATAR_IDS_IN_VIEW and
  // AVATAR_IDS_IN_RANGE_TO_ZAP, int32 [N][P][P] each, written by one launch (MpAvatarIds;
  // avatar_ids.h).  mp_tune's probes write none of them (ring_hold, layer_hold).
  ViewRegistration ego, vh, ep, av, avz;
  int32_t num_layer_ids = 0;   // 1 + the largest id of d_layer_lut: the length of a class table
  bool viewing(const ViewRegistration& v) const { return v.dst && !ring_hold && !layer_hold; }
  // The engine's choice (MpConfig.unfused = 0): one launch, always.  (Round 2 drew
  // views under 64 KB a world — the two-player games — in a second launch: a CU
  // then has 64 worlds to step for 2 us of drawing each, and with 4-8 feeders the
  // fused form lost, 160 vs 113 us.  With batches of 8, 8 feeders (coins: 4) and the
  // round-3 kernel it wins: prisoners_dilemma repeated 102 vs 114 us, coins 156 vs
  // 190; plan_frame, tools/gpu_small_views.sh.)
  bool fuse(bool world_view) const {
    (void)world_view;
    return unfused != 1;
  }
  uint8_t* d_atlas = nullptr;      // de-duplicated atlas + image slots
  // An MpStatesObserve request's own memory (grown on demand, freed by mp_destroy): the rows a
  // pixel kind gathers for the draw-only launch, and the stash of state_obs.h
  uint8_t* d_obs_rows = nullptr;
  uint64_t obs_rows_bytes = 0;
  uint8_t* d_obs_stash = nullptr;
  uint64_t obs_stash_bytes = 0;
  int32_t* d_layer_lut = nullptr;  // StepOutputs::layer_lut [P][kLayerLutRow]
  // An MpStatesCheck request's view of the pack (state_check.h): built by mp_create's host stage,
  // and its copy in device memory for k_check_states
  state_check::CheckTables check = {};
  state_check::CheckTables* d_check = nullptr;
  // An MpStatesHash request's byte masks as u32 [world_stride / 4] in device memory (state_hash.h):
  // the default spec's from creation (MP_STEP_ROW_HASH reads it too), and the most recent custom
  // spec's, replaced behind a wait for the stream when a request brings another
  uint32_t* d_hash_mask = nullptr;
  uint32_t* d_hash_custom = nullptr;
  // An MpStepListed request's claim table (step_listed.h), u64 [N], allocated and zeroed by the
  // first such request, and the generation of the most recent one
  unsigned long long* d_listed_claim = nullptr;
  uint32_t listed_generation = 0;
  state_hash::Spec hash_custom = {};   // (custom == 0: none yet)
  state_hash::Layout hash_layout() const {
    return state_hash::layout_of(check, substrate == MPK_SUBSTRATE_THE_MATRIX ? sub.mx.player_block : -1);
  }
  StepOutputs outputs() const {
    StepOutputs o = own;
    if (bound[MP_OBS_REWARD]) o.reward = (double*)bound[MP_OBS_REWARD];
    if (bound[MP_OBS_READY_TO_SHOOT]) o.ready = (double*)bound[MP_OBS_READY_TO_SHOOT];
    if (bound[MP_OBS_AUX0]) o.aux0 = (double*)bound[MP_OBS_AUX0];
    if (bound[MP_OBS_STEP_TYPE]) o.step_type = (int32_t*)bound[MP_OBS_STEP_TYPE];
    if (bound[MP_OBS_DISCOUNT]) o.discount = (double*)bound[MP_OBS_DISCOUNT];
    if (bound[MP_OBS_COLLECTIVE_REWARD]) o.collective = (double*)bound[MP_OBS_COLLECTIVE_REWARD];
    if (bound[MP_OBS_POSITION]) o.position = (int32_t*)bound[MP_OBS_POSITION];
    if (bound[MP_OBS_ORIENTATION]) o.orientation = (int32_t*)bound[MP_OBS_ORIENTATION];
    if (bound[MP_OBS_EVENTS]) o.events = (int32_t*)bound[MP_OBS_EVENTS];
    for (int k = 0; k < 4; ++k)
      if (bound[MP_OBS_AUX1 + k]) o.dbg[k] = (double*)bound[MP_OBS_AUX1 + k];
    if (bound[MP_OBS_ZAP_MATRIX]) o.zap_matrix = (double*)bound[MP_OBS_ZAP_MATRIX];
    if (bound[MP_OBS_INVENTORY]) o.inventory = (double*)bound[MP_OBS_INVENTORY];
    if (bound[MP_OBS_INTERACTION_INVENTORIES])
      o.interaction = (double*)bound[MP_OBS_INTERACTION_INVENTORIES];
    if (bound[MP_OBS_MATRIX_CUMULANTS]) o.cumulants = (double*)bound[MP_OBS_MATRIX_CUMULANTS];
    if (bound[MP_OBS_INTERACTION_REWARDS])
      o.interaction_rewards = (double*)bound[MP_OBS_INTERACTION_REWARDS];
    if (bound[MP_OBS_LAYER] && !layer_hold) { o.layer = (int32_t*)bound[MP_OBS_LAYER]; o.layer_lut = d_layer_lut; }
    return o;
  }
};

namespace {

// mp_tune's probe actions: uniform over the ACTION_SET, a hash of the index (what a
// random policy — and bench.py — sends; NOOP steps cost 5 % less than real ones)
// mp_box_fill's store loop: the frame launch's store FORM (persistent workgroups, whole spans
// per wave from an LDS ticket counter, 16-byte lane-contiguous non-temporal stores: 1 KiB per
// wave instruction) with nothing but the stores — what the memory system takes from this
// write order on this buffer.  order 0: workgroup g owns bytes [g * own, (g + 1) * own) and
// walks them in spans of `span`; order 1: one chip-wide front, turn t of workgroup g is span
// t * G + g of the whole view.
__global__ __launch_bounds__(1024) void k_box_fill(uint8_t* out, uint64_t bytes, uint64_t own,
                                                   uint32_t span, int order) {
  __shared__ uint32_t next;
  if (threadIdx.x == 0) next = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t g = blockIdx.x, G = gridDim.x;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&next, 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    uint64_t begin, end;
    if (order == 0) {
      uint64_t lim = (g + 1) * own;
      if (lim > bytes) lim = bytes;
      begin = g * own + (uint64_t)t * span;
      if (begin >= lim) break;
      end = begin + span < lim ? begin + span : lim;
    } else {
      begin = ((uint64_t)t * G + g) * span;
      if (begin >= bytes) break;
      end = begin + span < bytes ? begin + span : bytes;
    }
    const uint64_t sp = reinterpret_cast<uint64_t>(out + begin);
    uint8_t* base = reinterpret_cast<uint8_t*>(
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(sp >> 32)) << 32) |
        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)sp));
    const uint32_t n = (uint32_t)(end - begin);
    for (uint32_t off = lane * 16u; off < n; off += 1024u)
      asm volatile("global_store_dwordx4 %0, %1, %2 nt" :: "v"(off), "v"(u32x4{t, off, 2u, 3u}), "s"(base));
  }
}

__global__ void k_probe_actions(int32_t* actions, int n, int nact, uint32_t salt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x = (uint32_t)i * 2654435761u + salt;
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  actions[i] = (int32_t)(x % (uint32_t)nact);
}

__global__ void k_set_seeds(uint8_t* state, int stride, int grid_pad, int n,
                            const uint64_t* seeds, const uint8_t* mask) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n || (mask && !mask[w])) return;
  WorldTail* tail = reinterpret_cast<WorldTail*>(state + (size_t)w * stride + grid_pad);
  tail->seed = seeds[w];
  tail->episode = 0;
  tail->orders_step = 0;   // (the orders finish() left were drawn under the old seed)
}

// Sums the per-world event counters (WorldTail::ctr, reward_fx) over the shard.
__global__ void k_sum_counters(const uint8_t* state, int stride, int grid_pad, int n,
                               unsigned long long* out) {
  unsigned long long acc[MP_CTR_COUNT];
  for (int k = 0; k < MP_CTR_COUNT; ++k) acc[k] = 0;
  for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < n; w += gridDim.x * blockDim.x) {
    const WorldTail* tail = reinterpret_cast<const WorldTail*>(state + (size_t)w * stride + grid_pad);
    for (int k = 0; k < MP_CTR_COUNT; ++k) acc[k] += tail->ctr[k];
    acc[MP_CTR_REWARD_SUM] += (unsigned long long)(long long)tail->reward_fx;  // signed
  }
  for (int k = 0; k < MP_CTR_COUNT; ++k) {
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if ((threadIdx.x & 63) == 0 && acc[k]) atomicAdd(&out[k], acc[k]);
  }
}

// MP_STATES_SAVE: row i of `dst` = the record of world worlds[i] (NULL: world i), one wave per row,
// in 16-byte lines with eight lines of a lane in flight.  A world index outside [0, n) is reported
// through the fault words and its row left as it was.
__global__ __launch_bounds__(256) void k_save_worlds(DevTables t, const uint8_t* __restrict__ state, int n,
                                                     const int32_t* __restrict__ worlds, int count,
                                                     uint8_t* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (row >= count) return;
  const int w = worlds ? __builtin_amdgcn_readfirstlane(worlds[row]) : row;
  if (w < 0 || w >= n) {
    if (lane == 0) {   // (the words of step_load.h: report_state_index)
      t.fault[FAULT_STATE_INDEX + 1] = (uint32_t)w;
      t.fault[FAULT_STATE_INDEX + 2] = 2u;
      t.fault[FAULT_STATE_INDEX] = (uint32_t)row + 1u;
    }
    return;
  }
  const int nvec = t.world_stride >> 4;
  const uint4* src = reinterpret_cast<const uint4*>(state + (size_t)w * t.world_stride);
  uint4* out = reinterpret_cast<uint4*>(dst + (size_t)row * t.world_stride);
  for (int i0 = 0; i0 < nvec; i0 += 8 * 64) {
    uint4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k * 64 + lane;
      v[k] = src[i < nvec ? i : nvec - 1];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) stepk::issued(v[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k * 64 + lane;
      if (i < nvec) out[i] = v[k];
    }
  }
}

// Waits for the engine's stream and reports a frame kernel that gave up on its
// pipeline (frame.hip: report_stall) — an engine bug, surfaced instead of hung on.
int sync_and_check(MpEngine* e, const char* who) {
  HIP_TRY(hipStreamSynchronize(e->stream));
  const volatile uint32_t* f = e->h_fault;
  if (f[0] != 0)
    return fail(MP_ERR_HIP,
                "%s: the frame kernel's pipeline stalled (site %u, workgroup %u, wave %u, batch %u, "
                "seen %u, wanted %u); its outputs are incomplete",
                who, f[0], f[1], f[2], f[3], f[4], f[5]);
  if (f[8] != 0) {
    const uint32_t world = f[8] - 1;
    e->h_fault[8] = 0;   // reported once; the engine stays usable
    return fail(MP_ERR_HIP,
                "%s: world %u paid an interaction reward outside every resultIndicatorColorInterval "
                "(the reference asserts there, the_matrix/components.lua:282-290); the indicator "
                "shows the first colour", who, world);
  }
  if (f[kFaultCheckWorld] != 0) {
    // a row a checked load refused (state_check.h): words of its own, which the load that follows
    // the filter cannot overwrite with an index it reports itself
    const uint32_t world = f[kFaultCheckWorld] - 1, row = f[kFaultCheckWorld + 1], rule = f[kFaultCheckWorld + 2],
                   offset_word = f[kFaultCheckWorld + 3];
    e->h_fault[kFaultCheckWorld] = 0;   // reported once; the engine stays usable
    if ((f[FAULT_STATE_INDEX + 2] & 255u) == kFaultCheckRefused) e->h_fault[FAULT_STATE_INDEX] = 0;
    return fail(MP_ERR_INVALID,
                "%s: checked MP_STATES_LOAD: row %d, which src[%u] names, is not a well-formed record "
                "(rule %u, offset word 0x%x); world %u was left as it was", who, (int)row, world, rule,
                offset_word, world);
  }
  if (f[kFaultStartWorld] != 0) {
    // a registered episode start a stepping launch skipped (step_load.h: report_start)
    const uint32_t world = f[kFaultStartWorld] - 1, index = f[kFaultStartWorld + 1], rule = f[kFaultStartWorld + 2],
                   offset_word = f[kFaultStartWorld + 3];
    e->h_fault[kFaultStartWorld] = 0;   // reported once; the engine stays usable
    if (rule == 0 && offset_word == 0)
      return fail(MP_ERR_INVALID,
                  "%s: MpEpisodeStarts: rows[%u] = %d is neither -1 nor a row of the bank; world %u took the "
                  "level's own reset", who, world, (int)index, world);
    return fail(MP_ERR_INVALID,
                "%s: MpEpisodeStarts: row %d, which rows[%u] names, is not a well-formed record (rule %u, "
                "offset word 0x%x); world %u took the level's own reset", who, (int)index, world, rule,
                offset_word, world);
  }
  if (f[FAULT_STATE_INDEX] != 0) {
    const uint32_t at = f[FAULT_STATE_INDEX] - 1, index = f[FAULT_STATE_INDEX + 1];
    const bool load = f[FAULT_STATE_INDEX + 2] == 1;
    const bool observe = f[FAULT_STATE_INDEX + 2] == kFaultObserveRow;
    const uint32_t what = f[FAULT_STATE_INDEX + 2];
    e->h_fault[FAULT_STATE_INDEX] = 0;   // reported once; the engine stays usable
    if (what == kFaultViewRow || what == kFaultViewPlayer)
      return fail(MP_ERR_INVALID,
                  "%s: MpStatesView: %s[%u] = %d is %s; element %u of the destination was left as it was",
                  who, what == kFaultViewRow ? "rows" : "players", at, (int)index,
                  what == kFaultViewRow ? "not a row of the bank" : "not a player of this engine", at);
    if (what == kFaultEgoRow || what == kFaultEgoPlayer)
      return fail(MP_ERR_INVALID,
                  "%s: MpEgoLayer: %s[%u] = %d is %s; element %u of the destination was left as it was",
                  who, what == kFaultEgoRow ? "rows" : "players", at, (int)index,
                  what == kFaultEgoRow ? "not a row of the bank (with no bank: no world of this engine)"
                                       : "not a player of this engine", at);
    if (what == kFaultViewHashRow || what == kFaultViewHashPlayer)
      return fail(MP_ERR_INVALID,
                  "%s: MpViewHash: %s[%u] = %d is %s; element %u of the destination was left as it was",
                  who, what == kFaultViewHashRow ? "rows" : "players", at, (int)index,
                  what == kFaultViewHashRow ? "not a row of the bank (with no bank: no world of this engine)"
                                            : "not a player of this engine", at);
    if (what == kFaultEgoPlanesRow || what == kFaultEgoPlanesPlayer)
      return fail(MP_ERR_INVALID,
                  "%s: MpEgoPlanes: %s[%u] = %d is %s; element %u of the destination was left as it was",
                  who, what == kFaultEgoPlanesRow ? "rows" : "players", at, (int)index,
                  what == kFaultEgoPlanesRow ? "not a row of the bank (with no bank: no world of this engine)"
                                             : "not a player of this engine", at);
    if (what == kFaultEgoPlanesClass)
      return fail(MP_ERR_INVALID,
                  "%s: MpEgoPlanes: classes[%u] = %d is outside [-1, num_classes); the entry counted as -1",
                  who, at, (int)index);
    if (what == kFaultAvatarIdsRow || what == kFaultAvatarIdsPlayer)
      return fail(MP_ERR_INVALID,
                  "%s: MpAvatarIds: %s[%u] = %d is %s; element %u of the destination was left as it was",
                  who, what == kFaultAvatarIdsRow ? "rows" : "players", at, (int)index,
                  what == kFaultAvatarIdsRow ? "not a row of the bank (with no bank: no world of this engine)"
                                             : "not a player of this engine", at);
    if (what == kFaultListedWorld || what == kFaultListedRepeat)
      return fail(MP_ERR_INVALID,
                  "%s: MpStepListed: worlds[%u] = %d %s; the entry ran nothing and element %u of every per-call "
                  "tensor was left as it was", who, at, (int)index,
                  what == kFaultListedWorld ? "is not a world of this engine" : "repeats an earlier entry's world", at);
    if (what == kFaultHashRow)
      return fail(MP_ERR_INVALID,
                  "%s: MpStatesHash: rows[%u] = %d is not a row of the bank (MP_HASH_WORLDS: no world of this "
                  "engine); element %u of out was left as it was", who, at, (int)index, at);
    if (what == kFaultCheckRow)
      return fail(MP_ERR_INVALID,
                  "%s: MpStatesCheck: rows[%u] = %d is not a row of the bank; element %u of out is (-1, %d)",
                  who, at, (int)index, at, (int)index);
    if (observe)
      return fail(MP_ERR_INVALID,
                  "%s: MpStatesObserve: rows[%u] = %d is not a row of the bank; element %u of the "
                  "destination was left as it was", who, at, (int)index, at);
    return load ? fail(MP_ERR_INVALID,
                       "%s: MP_STATES_LOAD: src[%u] = %d is neither -1 nor a row of the bank; world %u "
                       "was left as it was", who, at, (int)index, at)
                : fail(MP_ERR_INVALID,
                       "%s: MP_STATES_SAVE: worlds[%u] = %d is not a world of this engine; row %u was "
                       "left as it was", who, at, (int)index, at);
  }
  return MP_OK;
}

// The level's Zapper (avatar_library.lua:570-763), NULL on a level without one, and the name of
// the level's family for the refusal.
const ZapRules* zap_rules_of(const SubstrateTables& sub) {
  switch (sub.substrate) {
    case MPK_SUBSTRATE_CLEAN_UP: return &sub.cu.zap;
    case MPK_SUBSTRATE_COMMONS_HARVEST: return &sub.ch.zap;
    case MPK_SUBSTRATE_TERRITORY: return &sub.tr.zap;
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS: return &sub.em.zap;
    default: return nullptr;
  }
}
const char* family_name(const SubstrateTables& sub) {
  static const char* const kNames[] = {"?", "clean_up", "commons_harvest", "territory", "coins", "*_in_the_matrix",
                                       "coop_mining", "gift_refinements", "collaborative_cooking",
                                       "externality_mushrooms"};
  return sub.substrate >= 1 && sub.substrate <= 9 ? kNames[sub.substrate] : kNames[0];
}
// What an MpAvatarIds launch has of the pack: where the avatar_layer plane lies, and (with a
// Zapper) the footprint and the states' avatars (`sinfo`: the step tables' first 256 words).
void avatar_ids_tables(avatar_ids::Args* a, const DevTables& t, const ZapRules* zap, const uint32_t* sinfo) {
  a->plane_at = t.avatar_layer * t.H * t.W;
  a->sinfo = sinfo;
  if (zap) a->shape = zap->shape;
}

// Draw-only launch: the views of the records as they are.
// (pool_k > 1: `rgb` is the per-agent view pooled by pool_k)
void draw(MpEngine* e, uint8_t* rgb, uint8_t* wrgb, int pool_k = 1) {
  stepk::StepArgs args = {};
  args.state = e->d_state; args.num_worlds = e->N;
  FramePlan p = e->frame_plan(0, rgb && wrgb ? 2 : wrgb ? 1 : 0, rgb ? pool_k : 1);
  p.parity = e->frame_launches++ & 1;
  launch_frame(e->t, nullptr, args, rgb, wrgb, p, e->stream, rgb ? pool_k : 1, e->world_pool);
}

// (`many`: a K-step request, checked by step_request — K steps by the K-step kernels, then the
// draw-only launches of the unfused path; NULL: a single step)
int submit(MpEngine* e, int mode, const int32_t* actions, const uint8_t* mask,
           const uint8_t* bank = nullptr, const int32_t* src = nullptr, int bank_rows = 0,
           const StepManyLaunch* many = nullptr, const UntilArgs* until = nullptr,
           const ListArgs* list = nullptr) {
  stepk::StepArgs args;
  args.state = e->d_state; args.actions = actions; args.reset_mask = mask;
  args.bank = bank; args.src = src; args.bank_rows = bank_rows;
  args.mode = mode; args.auto_reset = e->auto_reset; args.num_worlds = e->N;
  args.next_orders = e->next_orders;
  // the rollout ring: this submission's slot (a pointer store per ring-bound kind)
  const bool ringing = e->ring_slots > 0 && !e->ring_hold;
  const int slot = e->ring_slots > 0 ? (int)(e->ring_cursor % (uint64_t)e->ring_slots) : 0;
  if (ringing) { e->point_ring(slot); ++e->ring_cursor; }
  args.out = e->outputs();
  // One persistent launch steps the worlds and renders the bound views — one or
  // both — from the records while they are in LDS (frame.hip).  A bound "N.LAYER" is
  // written by the launch that steps (args.out.layer): its feeders, or the step kernels.
  // (the per-agent view is MP_OBS_RGB or a pooled kind: pool_k)
  uint8_t* rgb = e->agent_view();
  uint8_t* wrgb = (uint8_t*)e->bound[MP_OBS_WORLD_RGB];
  const int pk = rgb ? e->pool_k() : 1;
  const int views = rgb && wrgb ? 2 : wrgb ? 1 : 0;
  // (registered episode starts: the step kernels' own family, then the draw-only launches)
  const stepk::StartArgs* starts =
      e->starting() && (mode == STEP_MODE_STEP || mode == STEP_MODE_FIELDS) ? &e->starts : nullptr;
  if (many || starts || (!rgb && !wrgb) || !e->fuse(rgb == nullptr)) {
    if (many) {
      StepManyLaunch l = *many;
      l.starts = starts;
      if (list) launch_step_listed(e->t, e->sub, args, l, *until, *list, e->stream);   // (MpStepListed)
      else if (until) launch_step_until(e->t, e->sub, args, l, *until, e->stream);   // (MpStepUntil)
      else if (l.active.active) launch_step_active(e->t, e->sub, args, l, e->stream);   // (MpStepActive)
      else launch_step_many(e->t, e->sub, args, l, e->stream);
    } else if (starts) {
      launch_step_starts(e->t, e->sub, args, *starts, e->stream);
    } else {
      launch_step(e->t, e->sub, args, e->stream);
    }
    if (rgb) draw(e, rgb, nullptr, pk);
    if (wrgb) draw(e, nullptr, wrgb);
  } else {
    // (the plan follows the buffer: a ring remembers one per slot, mp_tune)
    FramePlan p = ringing && e->ring_plan[views].size() == (size_t)e->ring_slots
                      ? e->ring_plan[views][(size_t)slot] : e->frame_plan(1, views, pk);
    p.parity = e->frame_launches++ & 1;
    launch_frame(e->t, &e->sub, args, rgb, wrgb, p, e->stream, pk, e->world_pool);
  }
  HIP_TRY(hipGetLastError());
  if (e->folding()) {
    // the statistics launch: what this submission wrote, folded into the caller's tensors
    episode_stats::Rows r = {};
    r.P = e->t.P;
    r.num_worlds = e->N;
    r.started = e->d_state + e->t.grid_pad + offsetof(WorldTail, started);
    r.started_stride = e->t.world_stride;
    if (many) {   // (step_request has checked that the rows and `ran` are there)
      const ManyArgs& m = many->many;
      r.columns = list ? list->count : e->N;
      r.K = m.steps;
      r.reward = (const double*)m.row[0]; r.reward_bytes = m.row_bytes[0];
      r.step_type = (const int32_t*)m.row[2]; r.step_type_bytes = m.row_bytes[2];
      r.events = (const int32_t*)m.row[4]; r.events_bytes = m.row_bytes[4];
      r.active = many->active.active; r.active_bytes = m.steps > 1 ? many->active.step : 0;
      if (until) r.ran = until->ran;
      if (list) { r.worlds = list->worlds; r.claim = list->claim; r.generation = list->generation; }
    } else {      // K = 1: the in-place buffers (bound ones, the ring slot just written)
      r.columns = e->N;
      r.K = 1;
      r.reward = args.out.reward; r.step_type = args.out.step_type; r.events = args.out.events;
      if (mode == STEP_MODE_RESET) r.sel8 = mask;
      if (mode == STEP_MODE_LOAD) { r.sel32 = src; r.sel_rows = bank_rows; }
    }
    launch_episode_stats(e->stats_cols, e->stats, r, false, e->stream);
    HIP_TRY(hipGetLastError());
  }
  // the registered views: every world's, rewritten from the records this submission left
  if (!e->viewing(e->ego) && !e->viewing(e->vh) && !e->viewing(e->ep) && !e->viewing(e->av) && !e->viewing(e->avz))
    return MP_OK;
  const ego_layer::Window g = ego_layer::window_of(e->t);
  auto worlds = [&](auto* a, const MpEngine::ViewRegistration& v) {   // what the three launches share
    a->g = g;
    a->src = e->d_state; a->src_rows = e->N; a->count = e->N;
    a->stride = e->t.world_stride; a->grid_pad = e->t.grid_pad;
    a->dst = static_cast<decltype(a->dst)>(v.slot(slot));
    a->lut = e->d_layer_lut; a->fault = e->t.fault;
  };
  if (e->viewing(e->ego)) {   // EGO_LAYER
    ego_layer::Args a = {};
    worlds(&a, e->ego);
    ego_layer::launch(a, ego_layer::plan_of(g, e->N, e->num_cus), e->stream);
    HIP_TRY(hipGetLastError());
  }
  if (e->viewing(e->vh)) {   // every viewer's hash
    view_hash::Args a = {};
    worlds(&a, e->vh);
    a.layer_mask = e->vh.mask;
    a.classes = e->vh.classes; a.num_classes = e->vh.classes ? e->num_layer_ids : 0;
    view_hash::launch(a, view_hash::plan_of(g, e->N, e->num_cus), e->stream);
    HIP_TRY(hipGetLastError());
  }
  if (e->viewing(e->ep)) {   // every viewer's class and facing planes
    ego_planes::Args a = {};
    worlds(&a, e->ep);
    a.layer_mask = e->ep.mask;
    a.classes = e->ep.classes; a.num_ids = e->num_layer_ids;
    a.num_classes = e->ep.num_classes; a.facing = e->ep.facing;
    ego_planes::launch(a, ego_planes::plan_of(g, ego_planes::planes_of(a), e->N, e->num_cus), e->stream);
    HIP_TRY(hipGetLastError());
  }
  if (e->viewing(e->av) || e->viewing(e->avz)) {   // whom every viewer sees and could zap
    avatar_ids::Args a = {};
    worlds(&a, e->av);
    a.dst = (int32_t*)(e->av.dst ? e->av.slot(slot) : nullptr);
    a.dst_zap = (int32_t*)(e->avz.dst ? e->avz.slot(slot) : nullptr);
    avatar_ids_tables(&a, e->t, zap_rules_of(e->sub), (const uint32_t*)e->t.step_blob);
    avatar_ids::launch(a, avatar_ids::plan_of(g, a.plane_at, e->N, e->num_cus), e->stream);
    HIP_TRY(hipGetLastError());
  }
  return MP_OK;
}

void retired_va(int64_t* bytes, int64_t* limit);   // (mapped views, below)
bool in_mapped_view(const void* p);

// A bank of world-state rows (MP_STATES_SAVE / MP_STATES_LOAD): device memory of the engine's
// device, [ptr, ptr + bytes) inside one allocation.
int check_bank(MpEngine* e, const void* ptr, uint64_t bytes, const char* who);

// A bound buffer is written by every launch from then on: a pointer the device cannot
// write (a host array, a stale tensor) would fault the GPU in the middle of a step — it is
// refused here instead.  Memory this library mapped itself is known by range (the runtime's
// pointer query does not know virtual-memory mappings).
int check_device_pointer(MpEngine* e, const void* ptr, const char* who) {
  if (in_mapped_view(ptr)) return MP_OK;
  hipPointerAttribute_t attr = {};
  const hipError_t rc = hipPointerGetAttributes(&attr, ptr);
  if (rc != hipSuccess) {
    (void)hipGetLastError();
    // The pointer query does not know virtual-memory mappings: a range ANOTHER library mapped
    // (torch's expandable segments, somebody's own hipMemMap) fails it although the device
    // writes it fine.  Such a range does answer hipMemGetAddressRange; only a pointer neither
    // query knows is refused.
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) == hipSuccess && base && size) return MP_OK;
    (void)hipGetLastError();
    return fail(MP_ERR_INVALID, "%s: %p is not memory the device can write (%s); bind a device buffer",
                who, ptr, hipGetErrorString(rc));
  }
  if (attr.type == hipMemoryTypeUnregistered)
    return fail(MP_ERR_INVALID, "%s: %p is plain host memory; bind a device buffer", who, ptr);
  if ((attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeArray) && attr.device != e->device)
    return fail(MP_ERR_INVALID, "%s: %p lives on device %d, the engine on device %d", who, ptr,
                attr.device, e->device);
  return MP_OK;
}

int check_bank(MpEngine* e, const void* ptr, uint64_t bytes, const char* who) {
  if (int rc = check_device_pointer(e, ptr, who)) return rc;
  if (in_mapped_view(ptr)) {
    if (!in_mapped_view((const char*)ptr + bytes - 1))
      return fail(MP_ERR_INVALID, "%s: [%p, +%llu bytes) leaves the mapped view it starts in", who, ptr,
                  (unsigned long long)bytes);
    return MP_OK;
  }
  hipPointerAttribute_t attr = {};
  const hipError_t rc = hipPointerGetAttributes(&attr, ptr);
  (void)hipGetLastError();
  if (rc == hipSuccess && attr.type == hipMemoryTypeHost)
    return fail(MP_ERR_INVALID, "%s: %p is host memory; world states live in device memory", who, ptr);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess || !base) {
    (void)hipGetLastError();
    return fail(MP_ERR_INVALID, "%s: %p is not in a device allocation the runtime knows", who, ptr);
  }
  if ((uint64_t)((const char*)ptr - (const char*)base) + bytes > (uint64_t)size)
    return fail(MP_ERR_INVALID, "%s: [%p, +%llu bytes) runs past the end of its allocation (%p, %zu bytes)",
                who, ptr, (unsigned long long)bytes, base, size);
  return MP_OK;
}

// The front of the requests that read rows of saved world states (MpStatesObserve, MpStatesView,
// MpStatesCheck, MpStatesHash, MpEpisodeStarts, MP_STATES_SAVE / MP_STATES_LOAD and the three view
// requests): each rule and its message once; a request calls them in its own order.
// `bounded`: the rows come from a bank (or from the engine's worlds in its place), which has a row.
int check_counts(const char* who, int32_t count, int32_t src_rows, bool bounded = true) {
  if (count < 1 || (bounded && src_rows < 1))
    return fail(MP_ERR_INVALID, "%s: count %d, bank_rows %d: both must be at least 1", who, count, src_rows);
  return MP_OK;
}

// Without a row list a request reads rows 0 .. count - 1.  `verb`: what it does to them; `bank`:
// "the bank has" so many, else "there are"; `needs_list` and `tail`: MP_CHECK_FILTER's own.
int check_row_list(const char* who, const int32_t* rows, int32_t count, int32_t src_rows, const char* verb,
                   bool bank = true, bool needs_list = false, const char* tail = "") {
  if (rows || (!needs_list && count <= src_rows)) return MP_OK;
  return fail(MP_ERR_INVALID, "%s: without a row list rows 0 .. count - 1 are %s (count %d, %s %d rows)%s", who,
              verb, count, bank ? "the bank has" : "there are", src_rows, tail);
}

// `whose`: "engine's" or "pack's".
int check_fingerprint(const char* who, uint64_t rows, uint64_t own, const char* whose) {
  if (rows == own) return MP_OK;
  return fail(MP_ERR_INVALID, "%s: the rows' state fingerprint %016llx is not this %s (%016llx): they were "
              "saved by an engine of another pack, player count or record layout", who, (unsigned long long)rows,
              whose, (unsigned long long)own);
}

// *need: the bytes `count` elements of `each` bytes take of dst.
int check_dst_bytes(const char* who, int32_t count, uint64_t each, uint64_t dst_bytes, uint64_t* need) {
  *need = (uint64_t)count * each;
  if (dst_bytes >= *need) return MP_OK;
  return fail(MP_ERR_INVALID, "%s: %d elements of %llu bytes need %llu bytes, dst has %llu", who, count,
              (unsigned long long)each, (unsigned long long)*need, (unsigned long long)dst_bytes);
}

int check_aligned(const char* who, const char* what, const void* at, uint64_t align) {
  if ((uintptr_t)at % align == 0) return MP_OK;
  return fail(MP_ERR_INVALID, "%s: %s %p is not %llu-byte aligned", who, what, at, (unsigned long long)align);
}

// A request's device memory: each extent (NULL: absent) aligned and inside one allocation of the
// engine's device, one after the other.  check_bank's name is "who (what)", or `who` alone.
struct Extent { const char* what; const void* at; uint64_t bytes; uint64_t align; };
int check_extents(MpEngine* e, const char* who, const Extent* all, size_t n) {
  HIP_TRY(hipSetDevice(e->device));
  char name[64];
  for (const Extent* x = all; x != all + n; ++x) {
    if (!x->at) continue;
    if (int rc = check_aligned(who, x->what, x->at, x->align)) return rc;
    if (x->what) snprintf(name, sizeof name, "%s (%s)", who, x->what);
    if (int rc = check_bank(e, x->at, x->bytes, x->what ? name : who)) return rc;
  }
  return MP_OK;
}
int check_extents(MpEngine* e, const char* who, std::initializer_list<Extent> all) {
  return check_extents(e, who, all.begin(), all.size());
}

// One per-agent view at a time: MP_OBS_RGB or one pooled kind (the frame launch draws one of them
// beside WORLD.RGB); a pooled view's buffer is 16-byte aligned (its span is staged by lines).
int check_agent_view(MpEngine* e, int kind, const void* ptr, const char* who) {
  if (kind != MP_OBS_RGB && MpEngine::pool_of(kind) == 1) return MP_OK;
  for (int k : {MP_OBS_RGB, MP_OBS_RGB_POOL2, MP_OBS_RGB_POOL4, MP_OBS_RGB_POOL8})
    if (k != kind && e->bound[k])
      return fail(MP_ERR_INVALID, "%s: kind %d is bound; one per-agent view (MP_OBS_RGB or one "
                  "MP_OBS_RGB_POOL*) at a time — unbind it first", who, k);
  if (MpEngine::pool_of(kind) > 1 && ((uintptr_t)ptr & 15) != 0)
    return fail(MP_ERR_INVALID, "%s: a pooled view's buffer must be 16-byte aligned (%p)", who, ptr);
  return MP_OK;
}

// A pooled WORLD.RGB (MpConfig.world_pool) is staged by 16-byte lines too.
int check_world_view(MpEngine* e, int kind, const void* ptr, const char* who) {
  if (kind == MP_OBS_WORLD_RGB && e->world_pool > 1 && ((uintptr_t)ptr & 15) != 0)
    return fail(MP_ERR_INVALID, "%s: a pooled WORLD.RGB buffer (MpConfig.world_pool = %d) must be "
                "16-byte aligned (%p)", who, e->world_pool, ptr);
  return MP_OK;
}

// mp_bind_output on a kind that was bound as a ring: the kind leaves the ring
void drop_ring_kind(MpEngine* e, int kind) {
  if (!e->ring[kind].base) return;
  e->ring[kind] = MpEngine::RingKind();
  for (auto& v : e->ring_plan) v.clear();
  bool any = false;
  for (int k = 0; k < MP_OBS_KINDS; ++k) any = any || e->ring[k].base;
  if (!any) { e->ring_slots = 0; e->ring_cursor = 0; }
}

// MP_STATES_FINGERPRINT: FNV-1a over what decides a record's layout and meaning — the pack as the
// engine runs it (roles applied), the player count, the record's geometry (grid_pad, world_stride:
// MpDevOptions.record_pad included) and MP_RECORD_LAYOUT_VERSION.
uint64_t state_fingerprint(const std::vector<uint8_t>& pack, const DevTables& t) {
  uint64_t h = 0xcbf29ce484222325ull;
  auto mix = [&](const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 0x100000001b3ull; }
  };
  const uint32_t words[4] = {MP_RECORD_LAYOUT_VERSION, (uint32_t)t.P, (uint32_t)t.grid_pad,
                             (uint32_t)t.world_stride};
  mix(words, sizeof(words));
  const uint64_t n = pack.size();
  mix(&n, sizeof(n));
  mix(pack.data(), pack.size());
  return h;
}

// ---- mp_create's device stage: runs on a pack decode_pack has accepted
#define DEV_ALLOC(ptr, bytes) HIP_TRY(hipMalloc((void**)&(ptr), (bytes)))

// The pack and its two derived blobs on the device; the tables: the pack decoded against it.
int upload_pack(MpEngine* e, const MpConfig& cfg, DecodedPack* d) {
  DEV_ALLOC(e->d_pack, e->pack.size());
  if (int rc = decode_pack(e->pack, cfg, e->d_pack, d)) return rc;   // (the host copy's verdict)
  HIP_TRY(hipMemcpy(e->d_pack, e->pack.data(), e->pack.size(), hipMemcpyHostToDevice));
  DEV_ALLOC(e->d_extra, d->extra.size());
  HIP_TRY(hipMemcpy(e->d_extra, d->extra.data(), d->extra.size(), hipMemcpyHostToDevice));
  DEV_ALLOC(e->d_stepblob, d->step_blob.size());
  HIP_TRY(hipMemcpy(e->d_stepblob, d->step_blob.data(), d->step_blob.size(), hipMemcpyHostToDevice));
  e->t = d->t;
  e->sub = d->sub;
  e->substrate = d->sub.substrate;
  e->t.sprite_flags8 = e->d_extra;
  e->t.step_blob = e->d_stepblob;
  return MP_OK;
}

// DevTables::fault in host memory (readable without a HIP call, i.e. while a kernel is stuck:
// 64 fault words + the -DMP_FRAME_TIMELINE build's log); DevTables::claim (+ -DMP_FRAME_ENDS stamps).
int alloc_fault_words(MpEngine* e) {
  HIP_TRY(hipHostMalloc((void**)&e->h_fault, kFaultWords * sizeof(uint32_t), hipHostMallocMapped));
  memset(e->h_fault, 0, kFaultWords * sizeof(uint32_t));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->t.fault, e->h_fault, 0));
  DEV_ALLOC(e->d_claim, (2 + 2 * 1024) * sizeof(uint32_t));
  HIP_TRY(hipMemset(e->d_claim, 0, (2 + 2 * 1024) * sizeof(uint32_t)));
  e->t.claim = e->d_claim;
  return MP_OK;
}

// The world records, zero but for their seeds.
int init_state(MpEngine* e, const MpConfig& cfg) {
  const DevTables& t = e->t;
  const size_t state_bytes = (size_t)e->N * t.world_stride;
  DEV_ALLOC(e->d_state, state_bytes);
  std::vector<uint8_t> init(state_bytes, 0);
  for (int w = 0; w < e->N; ++w) {
    WorldTail* tail = reinterpret_cast<WorldTail*>(init.data() + (size_t)w * t.world_stride + t.grid_pad);
    const uint64_t gw = cfg.world_offset + (uint64_t)w;
    tail->seed = (cfg.base_seed || cfg.literal_base_seed) ? cfg.base_seed + gw
                                                          : 0x9E3779B97F4A7C15ull * (gw + 1);
  }
  HIP_TRY(hipMemcpy(e->d_state, init.data(), state_bytes, hipMemcpyHostToDevice));
  return MP_OK;
}

// The engine-owned outputs (scalars, debug observations) and the staging buffers.
int alloc_outputs(MpEngine* e, const MpConfig& cfg) {
  const DevTables& t = e->t;
  const size_t NP = (size_t)e->N * t.P, N = (size_t)e->N;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_reward = take(NP * 8), o_ready = take(NP * 8), o_aux = take(NP * 8),
               o_disc = take(N * 8), o_coll = take(N * 8), o_type = take(N * 4),
               o_pos = take(NP * 8), o_ori = take(NP * 4),
               o_ev = take(N * MP_EVENT_ROWS * 16);
  const bool matrix = e->substrate == MPK_SUBSTRATE_THE_MATRIX;
  const size_t o_inv = take(NP * e->inventory_types() * 8),
               o_int = take(matrix ? NP * 2 * e->sub.mx.R * 8 : 0),
               o_irw = take(matrix ? NP * 2 * 8 : 0);
  DEV_ALLOC(e->d_scalars, off);
  e->scalars_bytes = off;
  HIP_TRY(hipMemset(e->d_scalars, 0, off));
  e->own.reward = (double*)(e->d_scalars + o_reward);
  e->own.ready = (double*)(e->d_scalars + o_ready);
  e->own.aux0 = (double*)(e->d_scalars + o_aux);
  e->own.discount = (double*)(e->d_scalars + o_disc);
  e->own.collective = (double*)(e->d_scalars + o_coll);
  e->own.step_type = (int32_t*)(e->d_scalars + o_type);
  e->own.position = (int32_t*)(e->d_scalars + o_pos);
  e->own.orientation = (int32_t*)(e->d_scalars + o_ori);
  e->own.events = (int32_t*)(e->d_scalars + o_ev);
  if (e->inventory_types() > 0) e->own.inventory = (double*)(e->d_scalars + o_inv);
  if (matrix) {
    e->own.interaction = (double*)(e->d_scalars + o_int);
    e->own.interaction_rewards = (double*)(e->d_scalars + o_irw);
  }
  if (cfg.debug_observations) {
    size_t doff = 0;
    auto dtake = [&](size_t bytes) { size_t o = doff; doff += (bytes + 255) & ~(size_t)255; return o; };
    size_t o_dbg[4];
    for (int k = 0; k < 4; ++k) o_dbg[k] = dtake(NP * 8);
    const size_t o_zm = dtake(NP * t.P * 8);
    const size_t o_cum = dtake(matrix ? NP * (1 + 3 * e->sub.mx.R) * 8 : 0);
    DEV_ALLOC(e->d_debug, doff);
    e->debug_bytes = doff;
    HIP_TRY(hipMemset(e->d_debug, 0, doff));
    if (mp_obs_bytes(e, MP_OBS_AUX1))   // (the substrates that have them: mp_obs_bytes)
      for (int k = 0; k < 4; ++k) e->own.dbg[k] = (double*)(e->d_debug + o_dbg[k]);
    if (mp_obs_bytes(e, MP_OBS_ZAP_MATRIX))
      e->own.zap_matrix = (double*)(e->d_debug + o_zm);
    if (matrix) e->own.cumulants = (double*)(e->d_debug + o_cum);
  }
  DEV_ALLOC(e->d_actions, NP * 4);
  DEV_ALLOC(e->d_mask, N);
  DEV_ALLOC(e->d_seeds, N * 8);
  DEV_ALLOC(e->d_ctr, MP_CTR_COUNT * 8);
  return MP_OK;
}
#undef DEV_ALLOC

// The renderer's images: the de-duplicated sprite atlas (noRotate sprites and solid colours
// have four identical facings), then the composite cache's and its (base, overlay) table.
struct Atlas {
  std::vector<uint8_t> images = std::vector<uint8_t>(256, 0);   // image 0: unused padding
  std::vector<uint16_t> slots;                                  // (sprite, facing) -> image
  std::vector<uint32_t> pair_table = std::vector<uint32_t>(kPairSlots, 0xffffffffu);
  int count = 1, pair_probe = 0, n_composites = 0, used_slots = 0;

  int add_image(const uint8_t* img, int from) {
    for (int k = from; k < count; ++k)
      if (memcmp(images.data() + (size_t)k * 256, img, 256) == 0) return k;
    images.insert(images.end(), img, img + 256);
    return count++;
  }
  void add_sprites(const uint8_t* rgba, const int32_t* flags, int nimg) {
    slots.assign((size_t)nimg, 0);
    for (int i = 0; i < nimg; ++i) {
      uint8_t img[256];
      memcpy(img, rgba + (size_t)i * 256, 256);
      if (flags[i >> 2] & MPK_SPRITE_OPAQUE) {
        // opaque images are only ever copied: store them pre-packed, 8 rows of
        // 24 B RGB followed by 8 B of padding
        uint8_t packed[256] = {0};
        for (int py = 0; py < 8; ++py)
          for (int px = 0; px < 8; ++px)
            for (int ch = 0; ch < 3; ++ch)
              packed[py * 32 + px * 3 + ch] = img[(py * 8 + px) * 4 + ch];
        memcpy(img, packed, 256);
      }
      slots[(size_t)i] = (uint16_t)add_image(img, 1);
    }
  }
  int lookup(uint32_t a, uint32_t b) const {
    for (uint32_t h = pair_hash(a, b), k = 0; k < (uint32_t)kPairSlots; ++k) {
      const uint32_t ent = pair_table[(h + k) & (kPairSlots - 1)];
      if (ent == 0xffffffffu) return -1;
      if ((ent >> 10) == ((a << 10) | b)) return (int)(ent & 1023u);
    }
    return -1;
  }
  void insert(uint32_t a, uint32_t b, uint32_t c) {
    for (uint32_t h = pair_hash(a, b), k = 0; k < (uint32_t)kPairSlots; ++k) {
      uint32_t& ent = pair_table[(h + k) & (kPairSlots - 1)];
      if (ent == 0xffffffffu) {
        ent = (a << 20) | (b << 10) | c;
        if ((int)k + 1 > pair_probe) pair_probe = (int)k + 1;
        return;
      }
    }
  }
  // one overlay image blended onto a packed opaque image, exactly as
  // render.hip does it (A7: (s*a + d*(255-a) + 127) / 255; binary sprites
  // replace where alpha > 0)
  void blend(int base_img, int ov_img, bool partial, uint8_t* out) const {
    memcpy(out, images.data() + (size_t)base_img * 256, 256);
    const uint8_t* ov = images.data() + (size_t)ov_img * 256;
    for (int py = 0; py < 8; ++py)
      for (int px = 0; px < 8; ++px) {
        const uint8_t* s = ov + (py * 8 + px) * 4;
        uint8_t* d = out + py * 32 + px * 3;
        const unsigned a = s[3];
        for (int ch = 0; ch < 3; ++ch) {
          if (partial) d[ch] = (uint8_t)((s[ch] * a + d[ch] * (255u - a) + 127u) / 255u);
          else if (a) d[ch] = s[ch];
        }
      }
  }
};

// An opaque look, then up to two non-opaque looks on higher layers; `cells` that can show it.
struct Look { int layer, sprite, orient; };
struct Stack { int n; Look l[3]; long cells; };

Stack& count_stack(std::vector<Stack>& stacks, const Look* l, int n) {
  for (auto& sk : stacks) {
    bool eq = sk.n == n;
    for (int k = 0; eq && k < n; ++k) eq = sk.l[k].sprite == l[k].sprite && sk.l[k].orient == l[k].orient;
    if (eq) { sk.cells++; return sk; }
  }
  Stack sk; sk.n = n; sk.cells = 1;
  for (int k = 0; k < n; ++k) sk.l[k] = l[k];
  stacks.push_back(sk);
  return stacks.back();
}

// Composite cache (render.hip phase 1): the (opaque base, overlay) stacks that the
// map's static pieces can form — dirt on water, shadows on sand, claimed-resource
// paint on its texture ... — so such cells become plain copies.  A piece's possible
// looks are all sprite-bearing states of its prefab ("prefab.state" names); avatars,
// their markings and beams move, so they are never part of a cached stack.
std::vector<Stack> collect_stacks(const MpEngine* e, const int32_t* flags) {
  const DevTables& t = e->t;
  const void* hp = e->pack.data();
  uint64_t names_len = 0;
  const char* names = table<char>(hp, "state_names", &names_len);
  const int32_t* objs = table<int32_t>(hp, "objects");
  const int32_t* st_layer = table<int32_t>(hp, "state_layer");
  const int32_t* st_sprite = table<int32_t>(hp, "state_sprite");
  const int32_t* st_orient = table<int32_t>(hp, "state_orient");
  const int nobj = table<int32_t>(hp, "hdr")[MPK_HDR_NOBJ];
  std::vector<std::string> prefab((size_t)t.nstates);
  for (uint64_t s = 0, off = 0; s < (uint64_t)t.nstates && off < names_len; ++s) {
    const std::string nm(names + off);
    off += nm.size() + 1;
    prefab[s] = nm.substr(0, nm.find('.'));
  }
  std::vector<std::vector<Look>> cell_looks((size_t)t.H * t.W);
  for (int i = 0; i < nobj; ++i) {
    const int32_t* ob = objs + 4 * i;
    if (ob[0] == MPK_KIND_SCENE || ob[0] == MPK_KIND_AVATAR || ob[0] == MPK_KIND_MARKING) continue;
    for (int s = 1; s < t.nstates; ++s)
      if (prefab[(size_t)s] == prefab[(size_t)ob[3]] && st_sprite[s] >= 0 && st_layer[s] >= 0)
        cell_looks[(size_t)ob[2] * t.W + ob[1]].push_back({st_layer[s], st_sprite[s], st_orient[s]});
  }
  std::vector<Stack> stacks;
  auto overlay = [&](const Look& l) { return !(flags[l.sprite] & (MPK_SPRITE_OPAQUE | MPK_SPRITE_EMPTY)); };
  for (const auto& looks : cell_looks) {
    // (sprite -1: no opaque piece below — the renderer starts from image 0,
    // black; the *_in_the_matrix maps have no floor under their resources)
    std::vector<Look> bases;
    for (const Look& a : looks)
      if (flags[a.sprite] & MPK_SPRITE_OPAQUE) bases.push_back(a);
    if (bases.empty()) bases.push_back({-1, -1, 0});   // a cell no piece can cover
    for (const Look& a : bases)
      for (const Look& b : looks) {
        if (b.layer <= a.layer || !overlay(b)) continue;
        const Look ab[3] = {a, b, b};
        count_stack(stacks, ab, 2);
        for (const Look& c : looks) {
          if (c.layer <= b.layer || !overlay(c)) continue;
          const Look abc[3] = {a, b, c};
          count_stack(stacks, abc, 3);
        }
      }
  }
  // stacks the lowering knows to be the common ones (territory: texture + wet +
  // dry paint of the SAME player, 9 of 81 combinations): first in their class
  uint64_t nh = 0;
  const int32_t* hints = table<int32_t>(hp, "composite_hints", &nh);
  for (uint64_t i = 0; hints && i + 2 < nh; i += 3) {
    Look l[3]; int n = 0; bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const int st = hints[i + k];
      if (st == 0 && k > 0) break;
      if (st <= 0 || st >= t.nstates || st_sprite[st] < 0 || st_layer[st] < 0) { ok = false; break; }
      l[n++] = {st_layer[st], st_sprite[st], st_orient[st]};
    }
    if (!ok || n < 2 || !(flags[l[0].sprite] & MPK_SPRITE_OPAQUE)) continue;
    for (int m = 2; m <= n; ++m) count_stack(stacks, l, m).cells = 1L << 40;
  }
  std::sort(stacks.begin(), stacks.end(), [](const Stack& x, const Stack& y) {
    return x.n != y.n ? x.n < y.n : x.cells > y.cells;   // all pairs before triples
  });
  return stacks;
}

// The composite cache's images, most common stacks first, in the LDS the renderer's preferred
// geometry leaves (more images must not cost worlds per workgroup: tools/sweep_env.sh).
void fill_composites(MpEngine* e, const MpDevOptions* dev, const int32_t* flags,
                     const std::vector<Stack>& stacks, Atlas& a) {
  DevTables& t = e->t;
  t.n_images = a.count;
  int max_composites = kPairSlots;
  for (int v = 0; v < 6; ++v) {
    const FramePlan p0 = plan_frame(t, e->sub, e->N, (v & 1) != 0, v >> 1, e->num_cus, dev, 1, e->world_pool);
    max_composites = std::min(max_composites,
                              (160 * 1024 - frame_lds_bytes(t, p0, 1, e->world_pool, v >> 1)) / 272);
  }
  max_composites = std::max(0, std::min(max_composites, kPairSlots / 2));
  if (dev && dev->max_composites >= 0) max_composites = std::min(max_composites, (int)dev->max_composites);
  for (const Stack& sk : stacks)
    for (int f = 0; f < 4; ++f) {
      int base = sk.l[0].sprite < 0 ? 0 : a.slots[(size_t)sk.l[0].sprite * 4 + ((f + sk.l[0].orient) & 3)];
      for (int k = 1; k < sk.n; ++k) {
        const int ov = a.slots[(size_t)sk.l[k].sprite * 4 + ((f + sk.l[k].orient) & 3)];
        int comp = a.lookup((uint32_t)base, (uint32_t)ov);
        if (comp < 0) {
          // (a triple extends a cached pair; it is skipped if its pair was)
          if (k < sk.n - 1 || a.n_composites >= max_composites || a.used_slots >= kPairSlots / 2 ||
              a.count >= 1023)
            break;
          uint8_t img[256];
          a.blend(base, ov, (flags[sk.l[k].sprite] & MPK_SPRITE_PARTIAL) != 0, img);
          const int before = a.count;
          comp = a.add_image(img, 0);
          a.n_composites += a.count - before;
          a.insert((uint32_t)base, (uint32_t)ov, (uint32_t)comp);
          ++a.used_slots;
        }
        base = comp;
      }
    }
}

// The renderer's atlas, composite cache and render blob.  (On the device side only
// because the composite budget comes from plan_frame, which needs the CU count.)
int build_atlas(MpEngine* e, const MpDevOptions* dev, const DecodedPack& d) {
  DevTables& t = e->t;
  const int32_t* flags = table<int32_t>(e->pack.data(), "sprite_flags");
  Atlas a;
  a.add_sprites(table<uint8_t>(e->pack.data(), "sprite_rgba"), flags, t.nsprites * 4);
  t.scratch_cells = (dev && dev->scratch_cells > 0) ? dev->scratch_cells : 8;
  if (!(dev && dev->no_composite_cache)) fill_composites(e, dev, flags, collect_stacks(e, flags), a);
  if (a.count > 1023) return fail(MP_ERR_PACK, "mp_create: %d distinct sprite images", a.count);
  t.n_images = a.count;
  t.pair_probe = a.pair_probe;
  // the atlas and the render blob (what every render workgroup stages besides its worlds,
  // already in LDS layout), uploaded in one buffer
  const void* hp = e->pack.data();
  const int nimg = t.nsprites * 4;
  const size_t img_bytes = (size_t)a.count * 256, slot_bytes = ((size_t)nimg * 2 + 15) & ~(size_t)15,
               pair_bytes = (size_t)kPairSlots * 4, blob_bytes = (size_t)render_blob_bytes(t);
  std::vector<uint8_t> flags8((size_t)t.nsprites);
  for (int s = 0; s < t.nsprites; ++s)
    flags8[(size_t)s] = (uint8_t)(((flags[s] & MPK_SPRITE_OPAQUE) ? 1 : 0) |
                                  ((flags[s] & MPK_SPRITE_PARTIAL) ? 2 : 0) |
                                  ((flags[s] & MPK_SPRITE_EMPTY) ? 4 : 0));
  const int8_t* splayer = reinterpret_cast<const int8_t*>(d.extra.data() + 256);   // state -> player
  // viewers 0 .. P-1, then the world view (row P_pack of the pack's table)
  const int32_t* vmap = table<int32_t>(hp, "view_sprite_map");
  std::vector<int32_t> vmap_p((size_t)(t.P + 1) * t.nsprites);
  for (int v = 0; v <= t.P; ++v)
    memcpy(vmap_p.data() + (size_t)v * t.nsprites,
           vmap + (size_t)(v < t.P ? v : t.P_pack) * t.nsprites, (size_t)t.nsprites * 4);
  std::vector<uint8_t> buf(img_bytes + slot_bytes + pair_bytes + blob_bytes, 0);
  memcpy(buf.data(), a.images.data(), img_bytes);
  memcpy(buf.data() + img_bytes, a.slots.data(), (size_t)nimg * 2);
  memcpy(buf.data() + img_bytes + slot_bytes, a.pair_table.data(), pair_bytes);
  uint8_t* blob = buf.data() + img_bytes + slot_bytes + pair_bytes;
  build_render_blob(t, a.images.data(), a.slots.data(), a.pair_table.data(),
                    table<int32_t>(hp, "state_sprite"), splayer, vmap_p.data(), flags8.data(),
                    table<int32_t>(hp, "state_orient"), blob);
  t.vis_layers = render_visible_layers(t, blob, table<int32_t>(hp, "state_layer"));
  HIP_TRY(hipMalloc((void**)&e->d_atlas, buf.size()));
  HIP_TRY(hipMemcpy(e->d_atlas, buf.data(), buf.size(), hipMemcpyHostToDevice));
  t.atlas_compact = e->d_atlas;
  t.img_slot = reinterpret_cast<const uint16_t*>(e->d_atlas + img_bytes);
  t.pair_table = reinterpret_cast<const uint32_t*>(e->d_atlas + img_bytes + slot_bytes);
  t.render_blob = e->d_atlas + img_bytes + slot_bytes + pair_bytes;
  if (dev && dev->verbose)
    fprintf(stderr, "mp_engine: composite cache: %d images, %d table entries, probe %d\n",
            a.n_composites, a.used_slots, a.pair_probe);
  return MP_OK;
}

// "N.LAYER"'s value of every (viewer, record byte) — what k_layer_view looks up per dword:
// 1 + the viewer's remapped sprite of the state, 0 for state 0 and states without a sprite
// (and bytes no state has); [256]: OutOfBounds (sprite 0), what an off-grid viewer sees.
std::vector<int32_t> layer_lut_rows(const void* pack, const DevTables& t) {
  const int32_t* ssprite = table<int32_t>(pack, "state_sprite");
  const int32_t* vmap = table<int32_t>(pack, "view_sprite_map");
  std::vector<int32_t> lut((size_t)t.P * kLayerLutRow, 0);
  for (int p = 0; p < t.P; ++p) {
    const int32_t* remap = vmap + (size_t)p * t.nsprites;
    int32_t* row = lut.data() + (size_t)p * kLayerLutRow;
    for (int s = 1; s < t.nstates && s < 256; ++s)
      row[s] = ssprite[s] >= 0 ? 1 + remap[ssprite[s]] : 0;
    row[256] = 1 + remap[0];
  }
  return lut;
}

int upload_layer_lut(MpEngine* e) {
  const DevTables& t = e->t;
  const std::vector<int32_t> lut = layer_lut_rows(e->pack.data(), t);
  e->num_layer_ids = view_hash::num_ids(lut.data(), t.P);
  HIP_TRY(hipMalloc((void**)&e->d_layer_lut, lut.size() * 4));
  HIP_TRY(hipMemcpy(e->d_layer_lut, lut.data(), lut.size() * 4, hipMemcpyHostToDevice));
  return MP_OK;
}

// FNV-1a of a pack's bytes (stock.h: MP_STOCK_*_PACK_HASH).
uint64_t pack_hash(const std::vector<uint8_t>& pack) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint8_t b : pack) { h ^= b; h *= 0x100000001b3ull; }
  return h;
}

// Which frame kernels an engine on this decoded pack runs (MpKernelVariant): the stock ones only
// if the pack is the committed one byte for byte and every folded field equals the header's.
int select_kernels(const std::vector<uint8_t>& pack, const DecodedPack& d, const MpDevOptions* dev) {
  if (dev && dev->generic_kernel) return MP_KERNEL_GENERIC;
  if (d.sub.substrate == MPK_SUBSTRATE_CLEAN_UP && pack_hash(pack) == MP_STOCK_CLEAN_UP_PACK_HASH &&
      StockCleanUp::matches(d.t, d.sub.cu))
    return MP_KERNEL_STOCK;
  return MP_KERNEL_GENERIC;
}

// The frame launches' plans, plain and pooled.
int plan_views(MpEngine* e, const MpDevOptions* dev) {
  const DevTables& t = e->t;
  for (int v = 0; v < 6; ++v) {
    FramePlan& pl = e->plan[v & 1][v >> 1];
    pl = plan_frame(t, e->sub, e->N, (v & 1) != 0, v >> 1, e->num_cus, dev);
    // (the one refusal of a pack that needs the device: the plans follow its CU count)
    if (frame_lds_bytes(t, pl) > 160 * 1024)
      return fail(MP_ERR_PACK, "mp_create: renderer needs %d B of LDS", frame_lds_bytes(t, pl));
  }
  // a pooled WORLD.RGB (MpConfig.world_pool): the plans that draw it, with its pooled atlas and span
  // staging in LDS; a pack where they do not fit beside a ring of records does not offer it
  if (e->world_pool > 1)
    for (int v = 2; v < 6; ++v) {
      FramePlan& pl = e->plan[v & 1][v >> 1];
      pl = plan_frame(t, e->sub, e->N, (v & 1) != 0, v >> 1, e->num_cus, dev, 1, e->world_pool);
      const int need = frame_lds_bytes(t, pl, 1, e->world_pool, v >> 1);
      if (need > 160 * 1024)
        return fail(MP_ERR_UNSUPPORTED, "mp_create: WORLD.RGB pooled by %d (MpConfig.world_pool) needs "
                    "%d B of LDS", e->world_pool, need);
    }
  // the pooled per-agent views (MP_OBS_RGB_POOL*): their plans, sized for the bytes they write;
  // a pack whose pooled atlas does not fit beside a ring of records does not offer them
  // (8 x 8 sprites only: the pooled image of a cell is 8/k pixels square)
  for (int i = 0; i < 3; ++i) {
    const int k = 2 << i;
    e->pool_ok[i] = t.sprite_size == 8;
    for (int v = 0; v < 6 && e->pool_ok[i]; ++v) {
      if ((v >> 1) == 1) continue;   // (WORLD.RGB alone has no per-agent view)
      FramePlan& pl = e->pool_plan[i][v & 1][v >> 1];
      pl = plan_frame(t, e->sub, e->N, (v & 1) != 0, v >> 1, e->num_cus, dev, k, e->world_pool);
      if (frame_lds_bytes(t, pl, k, e->world_pool, v >> 1) > 160 * 1024) e->pool_ok[i] = false;
    }
  }
  // (the stand-alone step launch: no view bound, LAYER alone, the two-launch form)
  if (step_worlds_per_group(t, e->sub) < 1)
    return fail(MP_ERR_PACK, "mp_create: the step kernels need %d B of LDS", step_lds_bytes(t, e->sub, 1));
  if (int rc = prepare_frame())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) failed: %d", rc);
  if (int rc = prepare_step())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the step kernels failed: %d", rc);
  if (int rc = prepare_step_many())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the K-step kernels failed: %d", rc);
  if (int rc = prepare_state_view())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the sampled-view kernels failed: %d", rc);
  if (int rc = ego_layer::prepare())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the EGO_LAYER kernels failed: %d", rc);
  if (int rc = view_hash::prepare())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the view-hash kernels failed: %d", rc);
  if (int rc = avatar_ids::prepare())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the avatar-ids kernels failed: %d", rc);
  if (int rc = ego_planes::prepare())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the ego-planes kernels failed: %d", rc);
  if (int rc = prepare_step_starts())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the episode-start kernels failed: %d", rc);
  if (int rc = prepare_step_active())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the masked K-step kernels failed: %d", rc);
  if (int rc = prepare_step_listed())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the listed K-step kernels failed: %d", rc);
  if (int rc = prepare_step_until())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the stopping K-step kernels failed: %d", rc);
  if (dev && dev->verbose)
    for (int v = 0; v < 6; ++v) {
      const FramePlan& pl = e->plan[v & 1][v >> 1];
      fprintf(stderr, "mp_engine: %d sprite images; frame plan %s, %s: %d buffers x %d worlds, %d of %d waves feed"
              " (%d draw the world view), %d groups own %d batches each + %d pooled, %d B LDS\n",
              t.n_images, (v & 1) ? "stepping + drawing" : "drawing",
              (v >> 1) == 0 ? "agents view" : (v >> 1) == 1 ? "world view" : "both views",
              pl.NB, pl.B, pl.feeders, pl.nwaves, pl.world_waves, pl.groups, pl.ks, pl.pool,
              frame_lds_bytes(t, pl, 1, e->world_pool, v >> 1));
    }
  return MP_OK;
}

int create_on_device(MpEngine* e, const MpConfig& cfg, DecodedPack* d) {
  const MpDevOptions* dev = cfg.dev;   // tests / tools only (include/mp_engine.h)
  e->has_dev = dev != nullptr;
  e->next_orders = !(dev && dev->no_next_orders);
  e->device = cfg.device;
  e->N = cfg.num_worlds;
  e->auto_reset = cfg.auto_reset;
  e->stream = (hipStream_t)cfg.stream;
  e->unfused = cfg.unfused;   // 0 is resolved once the pack is read
  e->world_pool = cfg.world_pool > 1 ? cfg.world_pool : 1;   // (mp_create checked it)
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg.device) != hipSuccess ||
      cus <= 0)
    return fail(MP_ERR_NO_DEVICE, "mp_create: device %d does not report its compute units", cfg.device);
  e->num_cus = cus;
  int rc;
  if ((rc = upload_pack(e, cfg, d))) return rc;
  e->sub.stock = select_kernels(e->pack, *d, dev);   // (host values only: the verdict of an MpKernelVariant request without an engine)
  if ((rc = alloc_fault_words(e)) || (rc = init_state(e, cfg)) ||
      (rc = alloc_outputs(e, cfg)) || (rc = build_atlas(e, dev, *d)) || (rc = upload_layer_lut(e)))
    return rc;
  return plan_views(e, dev);
}

// The rules' tables of an MpStatesCheck request where k_check_states reads them.
int upload_check_tables(MpEngine* e) {
  HIP_TRY(hipMalloc((void**)&e->d_check, sizeof(state_check::CheckTables)));
  HIP_TRY(hipMemcpy(e->d_check, &e->check, sizeof(state_check::CheckTables), hipMemcpyHostToDevice));
  return MP_OK;
}

// The default spec's byte mask of an MpStatesHash request where k_hash_rows and the K-step kernels
// read it.
int upload_hash_mask(MpEngine* e) {
  const state_hash::Layout l = e->hash_layout();
  std::vector<uint32_t> words((size_t)l.world_stride / 4);
  state_hash::build_byte_mask(l, state_hash::Spec{}, reinterpret_cast<uint8_t*>(words.data()));
  HIP_TRY(hipMalloc((void**)&e->d_hash_mask, (size_t)l.world_stride));
  HIP_TRY(hipMemcpy(e->d_hash_mask, words.data(), (size_t)l.world_stride, hipMemcpyHostToDevice));
  return MP_OK;
}

// mp_create's host stage: the config checked and copied (older, shorter layouts of MpConfig and
// MpDevOptions completed), the pack copied, roles applied, decoded and checked.  No HIP call.
struct HostStage {
  MpConfig cfg = {};
  MpDevOptions dev = {};
  std::vector<uint8_t> pack;
  DecodedPack d;
};

int host_stage(const void* pack, uint64_t pack_len, const MpConfig* cfg, HostStage* h) {
  // (an MpConfig of the ABI-8 layout, which ends before world_pool, reads as world_pool = 1)
  if (!cfg || (cfg->struct_size != sizeof(MpConfig) && cfg->struct_size != offsetof(MpConfig, world_pool)))
    return fail(MP_ERR_INVALID, "mp_create: bad MpConfig (struct_size)");
  memcpy(&h->cfg, cfg, cfg->struct_size);
  if (cfg->struct_size < sizeof(MpConfig)) h->cfg.world_pool = 1;
  cfg = &h->cfg;
  if (cfg->dev) {
    // (MpDevOptions before generic_kernel was appended reads as generic_kernel = 0)
    if (cfg->dev->struct_size != sizeof(MpDevOptions) &&
        cfg->dev->struct_size != offsetof(MpDevOptions, generic_kernel))
      return fail(MP_ERR_INVALID, "mp_create: bad MpDevOptions (struct_size)");
    memcpy(&h->dev, cfg->dev, cfg->dev->struct_size);
    h->dev.struct_size = sizeof(MpDevOptions);
    h->cfg.dev = &h->dev;
  }
  if (cfg->num_worlds <= 0)
    return fail(MP_ERR_INVALID, "mp_create: num_worlds must be positive");
  if (cfg->unfused < 0 || cfg->unfused > 2)
    return fail(MP_ERR_INVALID, "mp_create: MpConfig.unfused must be 0, 1 or 2 (got %d)", cfg->unfused);
  if (cfg->world_pool != 0 && cfg->world_pool != 1 && cfg->world_pool != 2 && cfg->world_pool != 4 &&
      cfg->world_pool != 8)
    return fail(MP_ERR_INVALID, "mp_create: MpConfig.world_pool must be 0, 1, 2, 4 or 8 (got %d)",
                cfg->world_pool);
  // the whole pack is decoded and checked on the host (pack_decode.hip) before a device is touched
  const int32_t* hdr = nullptr;
  if (int rc = check_header(pack, pack_len, *cfg, &hdr)) return rc;
  h->pack.assign((const uint8_t*)pack, (const uint8_t*)pack + pack_len);
  if (int rc = apply_roles(h->pack, *cfg)) return rc;
  if (int rc = decode_pack(h->pack, *cfg, h->pack.data(), &h->d)) return rc;
  if (cfg->world_pool > 1 && h->d.t.sprite_size != 8)   // (the pooled image of a cell is 8/k pixels square)
    return fail(MP_ERR_UNSUPPORTED, "mp_create: MpConfig.world_pool needs 8 x 8 sprites (the pack's are %d x %d)",
                h->d.t.sprite_size, h->d.t.sprite_size);
  return MP_OK;
}

// MpKernelVariant::fields: the C literal of a folded member's value, by its type.
void literal(std::string* out, int32_t v) { *out += std::to_string(v); }
void literal(std::string* out, uint32_t v) { *out += std::to_string(v) + "u"; }
void literal(std::string* out, uint64_t v) {
  char b[32];
  snprintf(b, sizeof b, "0x%llxull", (unsigned long long)v);
  *out += b;
}
void literal(std::string* out, double v) {
  char b[48];
  snprintf(b, sizeof b, "%a", v);   // (hexadecimal: exact)
  *out += b;
}

}  // namespace

extern "C" {

int mp_abi_version(void) { return MP_ABI_VERSION; }

const char* mp_last_error(void) { return g_error.c_str(); }

uint64_t mp_obs_bytes(const MpEngine* e, MpObsKind kind) {
  if (!e) return 0;
  const uint64_t N = (uint64_t)e->N, P = (uint64_t)e->t.P, S = (uint64_t)e->t.sprite_size;
  switch (kind) {
    case MP_OBS_RGB:
      return N * P * (e->t.vf + e->t.vb + 1) * S * (e->t.vl + e->t.vr + 1) * S * 3;
    case MP_OBS_WORLD_RGB: {
      const uint64_t k = (uint64_t)e->world_pool;   // (MpConfig.world_pool; 1 = the full image)
      return N * (e->t.H * S / k) * (e->t.W * S / k) * 3;
    }
    case MP_OBS_RGB_POOL2: case MP_OBS_RGB_POOL4: case MP_OBS_RGB_POOL8: {
      const uint64_t k = (uint64_t)MpEngine::pool_of(kind);
      if (!e->pool_ok[MpEngine::pool_index((int)k)]) return 0;
      return N * P * ((e->t.vf + e->t.vb + 1) * S / k) * ((e->t.vl + e->t.vr + 1) * S / k) * 3;
    }
    case MP_OBS_REWARD: case MP_OBS_READY_TO_SHOOT: case MP_OBS_AUX0: return N * P * 8;
    case MP_OBS_STEP_TYPE: return N * 4;
    case MP_OBS_DISCOUNT: case MP_OBS_COLLECTIVE_REWARD: return N * 8;
    case MP_OBS_POSITION: return N * P * 8;
    case MP_OBS_ORIENTATION: return N * P * 4;
    case MP_OBS_EVENTS: return N * MP_EVENT_ROWS * 16;
    case MP_OBS_AUX1: case MP_OBS_AUX2: case MP_OBS_AUX3: case MP_OBS_AUX4:
      return e->substrate == MPK_SUBSTRATE_CLEAN_UP ? N * P * 8 : 0;
    case MP_OBS_ZAP_MATRIX:
      return (e->substrate == MPK_SUBSTRATE_CLEAN_UP ||
              e->substrate == MPK_SUBSTRATE_COMMONS_HARVEST) ? N * P * P * 8 : 0;
    case MP_OBS_LAYER:
      return N * P * (e->t.vf + e->t.vb + 1) * (e->t.vl + e->t.vr + 1) * e->t.L * 4;
    case MP_OBS_INVENTORY:
      return N * P * e->inventory_types() * 8;
    case MP_OBS_INTERACTION_INVENTORIES:
      return e->substrate == MPK_SUBSTRATE_THE_MATRIX ? N * P * 2 * e->sub.mx.R * 8 : 0;
    case MP_OBS_MATRIX_CUMULANTS:
      return e->substrate == MPK_SUBSTRATE_THE_MATRIX ? N * P * (1 + 3 * e->sub.mx.R) * 8 : 0;
    case MP_OBS_INTERACTION_REWARDS:
      return e->substrate == MPK_SUBSTRATE_THE_MATRIX ? N * P * 2 * 8 : 0;
    default: return 0;
  }
}

int mp_create(const void* pack, uint64_t pack_len, const MpConfig* cfg,
              MpEngine** out) {
  if (!out) return fail(MP_ERR_INVALID, "mp_create: out is NULL");
  *out = nullptr;
  HostStage h;
  if (int rc = host_stage(pack, pack_len, cfg, &h)) return rc;
  cfg = &h.cfg;
  std::vector<uint8_t>& copy = h.pack;
  DecodedPack& d = h.d;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MP_ERR_NO_DEVICE,
                "mp_create: no HIP device; the engine has no CPU path");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(MP_ERR_INVALID, "mp_create: device %d out of range (%d devices)",
                cfg->device, ndev);
  HIP_TRY(hipSetDevice(cfg->device));

  MpEngine* e = new MpEngine();
  build_check_tables(d, &e->check);   // (of the host decode: create_on_device decodes against the device copy)
  e->pack = std::move(copy);
  int rc = create_on_device(e, *cfg, &d);
  if (rc == MP_OK) rc = upload_check_tables(e);
  if (rc == MP_OK) rc = upload_hash_mask(e);
  if (rc != MP_OK) {
    mp_destroy(e);
    return rc;
  }
  e->fingerprint = state_fingerprint(e->pack, e->t);
  *out = e;
  return MP_OK;
}

void mp_destroy(MpEngine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  if (e->h_fault) (void)hipHostFree(e->h_fault);
  void* bufs[] = {e->d_pack, e->d_extra, e->d_stepblob, e->d_debug, e->d_state, e->d_scalars,
                  e->d_actions, e->d_fields, e->d_mask, e->d_seeds, e->d_atlas, e->d_ctr, e->d_claim,
                  e->d_layer_lut, e->d_obs_rows, e->d_obs_stash, e->d_check, e->d_hash_mask,
                  e->d_hash_custom, e->d_listed_claim};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (int i = 0; i < MpEngine::kHostSlots; ++i)
    if (e->h_actions[i]) { (void)hipHostFree(e->h_actions[i]); (void)hipEventDestroy(e->h_copied[i]); }
  delete e;
}

int mp_info(const MpEngine* e, MpInfo* out) {
  if (!e || !out) return fail(MP_ERR_INVALID, "mp_info: NULL argument");
  memset(out, 0, sizeof *out);
  out->abi_version = MP_ABI_VERSION;
  out->substrate = e->substrate;
  out->num_worlds = e->N; out->num_players = e->t.P; out->num_actions = e->t.nact;
  out->map_h = e->t.H; out->map_w = e->t.W; out->num_layers = e->t.L;
  out->sprite_size = e->t.sprite_size;
  out->view_h = e->t.vf + e->t.vb + 1; out->view_w = e->t.vl + e->t.vr + 1;
  out->max_frames = e->t.max_frames;
  out->world_state_bytes = e->t.world_stride;
  // the launch form of a step with the views bound right now (the per-agent view
  // if none is)
  out->fused = !e->has_starts && e->fuse(!e->agent_view() && e->bound[MP_OBS_WORLD_RGB]) ? 1 : 0;
  out->num_resources = e->inventory_types();
  out->num_action_fields = e->t.nfields;
  {
    const bool a = e->agent_view() != nullptr, w = e->bound[MP_OBS_WORLD_RGB] != nullptr;
    const int views = a && w ? 2 : w ? 1 : 0;
    // (with a tuned ring: the plan of the slot the next submission writes)
    const FramePlan& p = e->ring_slots > 0 && e->ring_plan[views].size() == (size_t)e->ring_slots
                             ? e->ring_plan[views][(size_t)(e->ring_cursor % (uint64_t)e->ring_slots)]
                             : const_cast<MpEngine*>(e)->frame_plan(1, views, a ? e->pool_k() : 1);
    out->plan_batch_worlds = p.B; out->plan_ring_batches = p.NB; out->plan_owned_batches = p.ks;
    out->plan_pooled_batches = p.pool; out->plan_groups = p.groups;
    out->plan_store_sc1 = p.store_sc1;
    out->plan_feeders = p.feeders; out->plan_waves = p.nwaves;
    out->plan_pace = p.pace;
    out->plan_team = p.team;
    out->plan_late_priority = p.late_prio;
  }
  out->visible_layers = (int32_t)(e->t.vis_layers & 0xffffu);
  out->ring_slots = e->ring_slots;
  out->ring_next = e->ring_slots > 0 ? (int32_t)(e->ring_cursor % (uint64_t)e->ring_slots) : 0;
  retired_va(&out->retired_va_bytes, &out->retired_va_limit);
  return MP_OK;
}

int mp_set_stream(MpEngine* e, void* stream) {
  if (!e) return fail(MP_ERR_INVALID, "mp_set_stream: NULL engine");
  if ((hipStream_t)stream == e->stream) return MP_OK;
  // work already enqueued on the old stream is ordered before what follows on
  // the new one
  HIP_TRY(hipSetDevice(e->device));
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t rc = hipEventRecord(ev, e->stream);
  if (rc == hipSuccess) rc = hipStreamWaitEvent((hipStream_t)stream, ev, 0);
  (void)hipEventDestroy(ev);
  HIP_TRY(rc);
  e->stream = (hipStream_t)stream;
  return MP_OK;
}

int mp_bind_output(MpEngine* e, MpObsKind kind, void* device_ptr) {
  if (!e || kind < 0 || kind >= MP_OBS_KINDS)
    return fail(MP_ERR_INVALID, "mp_bind_output: bad argument");
  if (device_ptr && mp_obs_bytes(e, kind) == 0)
    return fail(MP_ERR_UNSUPPORTED, "mp_bind_output: this substrate has no observation %d", (int)kind);
  if (device_ptr)
    if (int rc = check_agent_view(e, kind, device_ptr, "mp_bind_output")) return rc;
  if (device_ptr)
    if (int rc = check_world_view(e, kind, device_ptr, "mp_bind_output")) return rc;
  if (device_ptr)
    if (int rc = check_device_pointer(e, device_ptr, "mp_bind_output")) return rc;
  // (a ring's tuned plans were sized for the per-agent view bound then: full and pooled views
  // lay LDS out differently, so a change of that kind drops them — mp_tune makes new ones)
  if ((kind == MP_OBS_RGB || MpEngine::pool_of(kind) > 1) && e->bound[kind] != device_ptr)
    for (auto& v : e->ring_plan) v.clear();
  e->bound[kind] = device_ptr;
  drop_ring_kind(e, kind);
  return MP_OK;
}

int mp_bind_output_ring(MpEngine* e, MpObsKind kind, void* base, uint64_t slot_stride_bytes,
                        int32_t slots) {
  if (!e || kind < 0 || kind >= MP_OBS_KINDS)
    return fail(MP_ERR_INVALID, "mp_bind_output_ring: bad argument");
  if (!base) return mp_bind_output(e, kind, nullptr);
  const uint64_t bytes = mp_obs_bytes(e, kind);
  if (bytes == 0)
    return fail(MP_ERR_UNSUPPORTED, "mp_bind_output_ring: this substrate has no observation %d", (int)kind);
  if (slots < 1 || slots > (1 << 20))
    return fail(MP_ERR_INVALID, "mp_bind_output_ring: %d slots", (int)slots);
  if (slot_stride_bytes < bytes || (slot_stride_bytes & 255) != 0)
    return fail(MP_ERR_INVALID, "mp_bind_output_ring: a slot stride of %llu bytes for an observation of %llu "
                "(must hold it and be a multiple of 256)", (unsigned long long)slot_stride_bytes,
                (unsigned long long)bytes);
  if (int rc = check_agent_view(e, kind, base, "mp_bind_output_ring")) return rc;
  if (int rc = check_world_view(e, kind, base, "mp_bind_output_ring")) return rc;
  if (int rc = check_device_pointer(e, base, "mp_bind_output_ring")) return rc;
  if (int rc = check_device_pointer(e, (const char*)base + (uint64_t)(slots - 1) * slot_stride_bytes + bytes - 1,
                                    "mp_bind_output_ring (last byte of the last slot)")) return rc;
  bool others = false;
  for (int k = 0; k < MP_OBS_KINDS; ++k) others = others || (k != (int)kind && e->ring[k].base);
  if (others && slots != e->ring_slots)
    return fail(MP_ERR_INVALID, "mp_bind_output_ring: %d slots, but the kinds already bound as rings have %d "
                "(one position for all of them)", (int)slots, e->ring_slots);
  if (!others) { e->ring_slots = slots; e->ring_cursor = 0; }
  e->ring[kind].base = (uint8_t*)base;
  e->ring[kind].stride = slot_stride_bytes;
  for (auto& v : e->ring_plan) v.clear();   // plans belong to the buffers they were timed on
  // between submissions a ring kind points at the slot written last (slot 0 before the first)
  const uint64_t last = e->ring_cursor ? (e->ring_cursor - 1) % (uint64_t)e->ring_slots : 0;
  e->bound[kind] = e->ring[kind].base + last * slot_stride_bytes;
  return MP_OK;
}

int mp_reset(MpEngine* e, const uint64_t* seeds, const uint8_t* mask) {
  if (!e) return fail(MP_ERR_INVALID, "mp_reset: NULL engine");
  e->touched = true;
  e->has_state = true;
  HIP_TRY(hipSetDevice(e->device));
  const uint8_t* dmask = nullptr;
  if (mask) {
    HIP_TRY(hipMemcpyAsync(e->d_mask, mask, (size_t)e->N, hipMemcpyHostToDevice, e->stream));
    dmask = e->d_mask;
  }
  if (seeds) {
    HIP_TRY(hipMemcpyAsync(e->d_seeds, seeds, (size_t)e->N * 8, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_set_seeds, dim3((e->N + 255) / 256), dim3(256), 0, e->stream,
                       e->d_state, e->t.world_stride, e->t.grid_pad, e->N,
                       (const uint64_t*)e->d_seeds, dmask);
  }
  if (mask || seeds) HIP_TRY(hipStreamSynchronize(e->stream));  // host buffers are the caller's
  if (!mask && e->h_fault[0] != 0) {
    // a reported pipeline stall stays reported (every synchronising call fails)
    // until ALL worlds are reset: that makes the state whole again
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 9; ++i) e->h_fault[i] = 0;
  }
  return submit(e, STEP_MODE_RESET, nullptr, dmask);
}

int mp_step(MpEngine* e, const int32_t* actions_device) {
  if (!e || !actions_device) return fail(MP_ERR_INVALID, "mp_step: NULL argument");
  e->touched = true;
  HIP_TRY(hipSetDevice(e->device));
  return submit(e, STEP_MODE_STEP, actions_device, nullptr);
}

int mp_step_host(MpEngine* e, const int32_t* actions_host) {
  if (!e || !actions_host) return fail(MP_ERR_INVALID, "mp_step_host: NULL argument");
  e->touched = true;
  const size_t NP = (size_t)e->N * e->t.P;
  for (size_t i = 0; i < NP; ++i)
    if (actions_host[i] < 0 || actions_host[i] >= e->t.nact)
      return fail(MP_ERR_INVALID,
                  "mp_step_host: action %d of player %zu in world %zu is outside [0, %d)",
                  actions_host[i], i % e->t.P, i / e->t.P, e->t.nact);
  HIP_TRY(hipSetDevice(e->device));
  // The step kernel reads the actions straight from pinned, device-mapped host
  // memory (28 B per wave, fetched before — and hidden behind — its record load):
  // no copy engine, no stream synchronisation, the host runs ahead of the GPU.
  const int slot = (int)(e->host_steps++ % MpEngine::kHostSlots);
  if (!e->h_actions[slot]) {
    HIP_TRY(hipHostMalloc((void**)&e->h_actions[slot], NP * 4, hipHostMallocMapped));
    HIP_TRY(hipEventCreateWithFlags(&e->h_copied[slot], hipEventDisableTiming));
  } else {
    HIP_TRY(hipEventSynchronize(e->h_copied[slot]));  // the step that read this slot, 4 steps ago
  }
  memcpy(e->h_actions[slot], actions_host, NP * 4);
  int32_t* dev_view = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void**)&dev_view, e->h_actions[slot], 0));
  const int rc = submit(e, STEP_MODE_STEP, dev_view, nullptr);
  HIP_TRY(hipEventRecord(e->h_copied[slot], e->stream));
  return rc;
}

int mp_step_fields(MpEngine* e, const int32_t* fields_device) {
  if (!e || !fields_device) return fail(MP_ERR_INVALID, "mp_step_fields: NULL argument");
  e->touched = true;
  HIP_TRY(hipSetDevice(e->device));
  return submit(e, STEP_MODE_FIELDS, fields_device, nullptr);
}

int mp_step_fields_host(MpEngine* e, const int32_t* fields_host) {
  if (!e || !fields_host) return fail(MP_ERR_INVALID, "mp_step_fields_host: NULL argument");
  e->touched = true;
  const size_t A = (size_t)e->t.nfields, NP = (size_t)e->N * e->t.P;
  for (size_t i = 0; i < NP * A; ++i) {
    const int a = (int)(i % A);
    const int lo = (int)(int8_t)(e->t.field_lo >> (8 * a)), hi = (int)(int8_t)(e->t.field_hi >> (8 * a));
    if (fields_host[i] < lo || fields_host[i] > hi)
      return fail(MP_ERR_INVALID,
                  "mp_step_fields_host: field %d of player %zu in world %zu is %d, outside [%d, %d]",
                  a, (i / A) % e->t.P, i / A / e->t.P, fields_host[i], lo, hi);
  }
  HIP_TRY(hipSetDevice(e->device));
  // (not a hot path: staged through the engine's own device buffer)
  if (!e->d_fields) HIP_TRY(hipMalloc((void**)&e->d_fields, NP * 4 * 4));
  HIP_TRY(hipMemcpyAsync(e->d_fields, fields_host, NP * A * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // the host array is the caller's
  return submit(e, STEP_MODE_FIELDS, e->d_fields, nullptr);
}

int mp_observe(MpEngine* e, MpObsKind kind, void* dst) {
  if (!e || !dst) return fail(MP_ERR_INVALID, "mp_observe: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  const StepOutputs o = e->outputs();
  const void* src = nullptr;
  switch (kind) {
    case MP_OBS_RGB:
      draw(e, (uint8_t*)dst, nullptr);
      HIP_TRY(hipGetLastError());
      return MP_OK;
    case MP_OBS_WORLD_RGB:
      if (int rc = check_world_view(e, kind, dst, "mp_observe")) return rc;
      draw(e, nullptr, (uint8_t*)dst);
      HIP_TRY(hipGetLastError());
      return MP_OK;
    case MP_OBS_RGB_POOL2: case MP_OBS_RGB_POOL4: case MP_OBS_RGB_POOL8:
      if (mp_obs_bytes(e, kind) == 0)
        return fail(MP_ERR_UNSUPPORTED, "mp_observe: this substrate has no observation %d", (int)kind);
      if (((uintptr_t)dst & 15) != 0)
        return fail(MP_ERR_INVALID, "mp_observe: a pooled view's buffer must be 16-byte aligned (%p)", dst);
      draw(e, (uint8_t*)dst, nullptr, MpEngine::pool_of(kind));
      HIP_TRY(hipGetLastError());
      return MP_OK;
    case MP_OBS_LAYER:
      launch_layer_view(e->t, e->d_state, (int32_t*)dst, e->N, e->stream);
      HIP_TRY(hipGetLastError());
      return MP_OK;
    case MP_OBS_REWARD: src = o.reward; break;
    case MP_OBS_READY_TO_SHOOT: src = o.ready; break;
    case MP_OBS_AUX0: src = o.aux0; break;
    case MP_OBS_STEP_TYPE: src = o.step_type; break;
    case MP_OBS_DISCOUNT: src = o.discount; break;
    case MP_OBS_COLLECTIVE_REWARD: src = o.collective; break;
    case MP_OBS_POSITION: src = o.position; break;
    case MP_OBS_ORIENTATION: src = o.orientation; break;
    case MP_OBS_EVENTS: src = o.events; break;
    case MP_OBS_AUX1: case MP_OBS_AUX2: case MP_OBS_AUX3: case MP_OBS_AUX4:
      src = o.dbg[kind - MP_OBS_AUX1];
      break;
    case MP_OBS_ZAP_MATRIX: src = o.zap_matrix; break;
    case MP_OBS_INVENTORY: src = o.inventory; break;
    case MP_OBS_INTERACTION_INVENTORIES: src = o.interaction; break;
    case MP_OBS_MATRIX_CUMULANTS: src = o.cumulants; break;
    case MP_OBS_INTERACTION_REWARDS: src = o.interaction_rewards; break;
    default: return fail(MP_ERR_UNSUPPORTED, "mp_observe: unknown observation kind %d", (int)kind);
  }
  if (!src)
    return fail(MP_ERR_UNSUPPORTED,
                "mp_observe: debug observation %d is not produced (bind it before the step, or "
                "create the engine with debug_observations; or the substrate has none)", (int)kind);
  if (src != dst)
    HIP_TRY(hipMemcpyAsync(dst, src, mp_obs_bytes(e, kind), hipMemcpyDeviceToDevice, e->stream));
  return MP_OK;
}

int mp_dump(MpEngine* e, uint8_t* grid, int32_t* avat, int32_t* glob) {
  if (!e || !grid || !avat || !glob) return fail(MP_ERR_INVALID, "mp_dump: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = sync_and_check(e, "mp_dump")) return rc;
  const DevTables& t = e->t;
  std::vector<uint8_t> host((size_t)e->N * t.world_stride);
  HIP_TRY(hipMemcpy(host.data(), e->d_state, host.size(), hipMemcpyDeviceToHost));
  for (int w = 0; w < e->N; ++w) {
    const uint8_t* rec = host.data() + (size_t)w * t.world_stride;
    const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
    const size_t render_bytes = (size_t)t.L * t.H * t.W;
    memcpy(grid + (size_t)w * render_bytes, rec, render_bytes);
    for (int p = 0; p < t.P; ++p) {
      int32_t* a = avat + ((size_t)w * t.P + p) * 8;
      a[0] = tail->ax[p]; a[1] = tail->ay[p]; a[2] = tail->aori[p];
      a[3] = tail->aalive[p]; a[4] = tail->ztimer[p]; a[5] = tail->ctimer[p];
      a[6] = tail->frame - tail->achange[p]; a[7] = 0;
    }
    int32_t* g = glob + (size_t)w * 8;
    g[0] = tail->step; g[1] = tail->done; g[2] = tail->frame; g[3] = tail->aux_count;
    g[4] = (int32_t)tail->episode; g[5] = g[6] = g[7] = 0;
    if (e->substrate == MPK_SUBSTRATE_COOP_MINING) {
      // the ores' Lua-side variables, packed as oracle/coop_mining.c:coop_dump packs them:
      // the sum of the live countdowns, a position-weighted sum of the miner sets
      const CoopTables& c = e->sub.cm;
      const int32_t* cells = table<int32_t>(e->pack.data(), "ore_cells");
      const uint8_t* M = rec + (size_t)c.plane_m * t.H * t.W;
      const uint8_t* C = rec + (size_t)c.plane_c * t.H * t.W;
      uint32_t cd = 0, ms = 0;
      for (int i = 0; i < c.n_ore; ++i) {
        cd += C[cells[i]];
        ms += (uint32_t)M[cells[i]] * (uint32_t)(i + 1);
      }
      g[5] = (int32_t)cd; g[6] = (int32_t)(ms & 0x7fffffffu);
    }
    if (e->substrate == MPK_SUBSTRATE_COLLABORATIVE_COOKING) {
      // the pots' cooking times, summed as oracle/collaborative_cooking.c:cook_dump sums them
      const CookTables& c = e->sub.cc;
      const int32_t* pots = table<int32_t>(e->pack.data(), "cc_pot_cells");
      const uint8_t* T = rec + (size_t)c.plane_t * t.H * t.W;
      uint32_t times = 0;
      for (int k = 0; k < c.n_pot; ++k) times += (uint32_t)(T[pots[k]] & 31) * (uint32_t)(k + 1);
      g[3] = 0; g[5] = (int32_t)times;
    }
    if (e->substrate == MPK_SUBSTRATE_GIFT_REFINEMENTS) {
      // the inventories, packed as oracle/gift_refinements.c:gift_dump packs them
      for (int p = 0; p < t.P; ++p)
        avat[((size_t)w * t.P + p) * 8 + 7] = tail->flag0[p] | (tail->flag1[p] << 4) | (tail->level[p] << 8);
    }
    if (e->substrate == MPK_SUBSTRATE_THE_MATRIX) {
      // extra parity fields, same packing as oracle/the_matrix.c:matrix_dump
      const MatrixTables& c = e->sub.mx;
      for (int p = 0; p < t.P; ++p) {
        int32_t* a = avat + ((size_t)w * t.P + p) * 8;
        const int f1 = tail->flag1[p];
        a[5] = tail->level[p] | ((f1 & 7) << 8) | (((f1 >> 3) & 1) << 12) |
               ((tail->aflags[p] & 1) << 13) | (tail->freeze[p] << 16);
        const int m = tail->flag0[p];
        a[7] = m ? (1 | (tail->ctimer[p] << 1) | (tail->nozap[p] << 9) |
                    ((int)((c.s_mark_packed >> (8 * (m - 1))) & 255ull) << 17))
                 : 0;
      }
      const uint8_t* A = rec + (size_t)c.plane_a * t.H * t.W;
      for (int cell = 0; cell < t.H * t.W; ++cell)
        if ((A[cell] >> 4) & 1) g[5] += A[cell] & 3;
    }
    if (e->substrate == MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS) {
      // extra parity fields, same packing as oracle/externality_mushrooms.c:mushroom_dump
      const MushroomTables& c = e->sub.em;
      for (int p = 0; p < t.P; ++p) {
        avat[((size_t)w * t.P + p) * 8 + 5] = 0;   // (ctimer holds the marking's x here, not a timer)
        avat[((size_t)w * t.P + p) * 8 + 7] =
            tail->level[p] | (tail->freeze[p] << 4) | (tail->removal[p] << 12) |
            (tail->nozap[p] << 16) | ((tail->aflags[p] & 1) << 24) |
            (((tail->aflags[p] >> 1) & 1) << 25);
      }
      const int32_t* cells = table<int32_t>(e->pack.data(), "mushroom_cells");
      const uint8_t* S = rec + (size_t)c.live_layer * t.H * t.W;
      const uint8_t* A = rec + (size_t)c.plane_age * t.H * t.W;
      int live = 0, ages = 0;
      for (int i = 0; i < c.n_site; ++i)
        if (S[cells[i]] != 0) { live++; ages += (S[cells[i]] - c.s_type0 + 1) * A[cells[i]]; }
      g[3] = live; g[5] = ages; g[6] = tail->aux_count - c.n_live_init + 1000; g[7] = tail->aux_count;
    }
    if (e->substrate == MPK_SUBSTRATE_TERRITORY) {
      // extra parity fields, same packing as oracle/territory.c:territory_dump
      for (int p = 0; p < t.P; ++p)
        avat[((size_t)w * t.P + p) * 8 + 7] =
            tail->level[p] | (tail->freeze[p] << 4) | (tail->removal[p] << 12) |
            (tail->nozap[p] << 16) | ((tail->aflags[p] & 1) << 24) |
            (((tail->aflags[p] >> 1) & 1) << 25);
      const uint8_t* A = rec + (size_t)e->sub.tr.plane_a * t.H * t.W;
      std::vector<int32_t> cells((size_t)e->sub.tr.n_res);
      memcpy(cells.data(), table<int32_t>(e->pack.data(), "resource_cells"),
             cells.size() * sizeof(int32_t));
      for (int32_t cell : cells) {
        g[5] += A[cell] & 3; g[6] += (A[cell] >> 2) & 1; g[7] += A[cell] >> 3;
      }
    }
  }
  return MP_OK;
}

// An MpWorldStates request (include/mp_engine.h): what mp_snapshot / mp_restore do when `bytes` is
// sizeof(MpWorldStates) — no engine's snapshot is that small (a record is >= 448 bytes).
static int save_worlds(MpEngine* e, const int32_t* worlds, int32_t count, void* dst, uint64_t dst_bytes);
static int load_worlds(MpEngine* e, const void* bank, int32_t bank_rows, const int32_t* src,
                       uint64_t fingerprint);
static int world_states(MpEngine* e, MpWorldStates* r, bool restore) {
  if (r->struct_size != sizeof(MpWorldStates))
    return fail(MP_ERR_INVALID, "MpWorldStates: struct_size %u, expected %zu", r->struct_size,
                sizeof(MpWorldStates));
  if (restore != (r->op == MP_STATES_LOAD))
    return fail(MP_ERR_INVALID, "MpWorldStates: op %d goes to %s", r->op,
                r->op == MP_STATES_LOAD ? "mp_restore" : "mp_snapshot");
  switch (r->op) {
    case MP_STATES_FINGERPRINT: r->fingerprint = e->fingerprint; return MP_OK;
    case MP_STATES_SAVE: {
      const int rc = save_worlds(e, r->worlds, r->count, r->bank, r->bank_bytes);
      if (rc == MP_OK) r->fingerprint = e->fingerprint;
      return rc;
    }
    case MP_STATES_LOAD: return load_worlds(e, r->bank, r->bank_rows, r->src, r->fingerprint);
    default: return fail(MP_ERR_INVALID, "MpWorldStates: unknown op %d", r->op);
  }
}

// A K-step request (include/mp_engine.h: MpStepMany, MpStepTrajectory, MpStepActive, MpStepUntil),
// whichever struct it came in: `r` names the rows it wants, `who` is the request's own name in the
// messages, `mask` (MpStepActive, MpStepUntil) the device mask and the distance between two of its
// rows, `until` (MpStepUntil, MpStepListed, whose mask may be NULL) the stop state, `list`
// (MpStepListed only) the world list: the actions, the mask, the rows, ran and returns then have
// list->count columns where the others have N (`stopped` stays by world).  Everything is checked
// here, against kStepRowKinds (step_many.h) and mp_obs_bytes, before the one submission.
static int step_request(MpEngine* e, const char* who, const MpStepTrajectory& r,
                        const ActiveArgs* mask = nullptr, const UntilArgs* until = nullptr,
                        ListArgs* list = nullptr) {
  if (!e || !r.actions) return fail(MP_ERR_INVALID, "%s: NULL engine or actions", who);
  if (r.steps < 1 || r.steps > MP_STEP_MANY_MAX)
    return fail(MP_ERR_INVALID, "%s: steps %d is outside [1, %d]", who, r.steps, MP_STEP_MANY_MAX);
  if (r.fields != 0 && r.fields != 1)
    return fail(MP_ERR_INVALID, "%s: fields %d is neither 0 (discrete ids) nor 1 (raw fields)", who, r.fields);
  if (!e->has_state)
    return fail(MP_ERR_INVALID, "%s: the engine has never been reset; there is nothing to step", who);
  const uint64_t K = (uint64_t)r.steps, N = (uint64_t)e->N, P = (uint64_t)e->t.P;
  if (list) {
    if (!list->worlds) return fail(MP_ERR_INVALID, "%s: NULL worlds", who);
    if (list->count < 1 || (uint64_t)list->count > N)
      return fail(MP_ERR_INVALID, "%s: count %d is outside [1, %llu] (more entries than worlds must repeat one)", who,
                  list->count, (unsigned long long)N);
    if ((uintptr_t)list->worlds & 3)
      return fail(MP_ERR_INVALID, "%s: worlds %p is not 4-byte aligned", who, (const void*)list->worlds);
  }
  const uint64_t C = list ? (uint64_t)list->count : N;   // the columns of every per-call tensor
  const uint64_t ablock = C * P * (r.fields ? (uint64_t)e->t.nfields : 1u) * 4u;
  if (r.actions_step_bytes != 0 && (r.actions_step_bytes < ablock || r.actions_step_bytes % 4))
    return fail(MP_ERR_INVALID, "%s: actions_step_bytes %llu is neither 0 nor a multiple of 4 that "
                "holds one step's block of %llu bytes", who, (unsigned long long)r.actions_step_bytes,
                (unsigned long long)ablock);
  if ((uintptr_t)r.actions & 3)
    return fail(MP_ERR_INVALID, "%s: actions %p is not 4-byte aligned", who, (const void*)r.actions);
  // (the limit has not grown with MP_STEP_ROW_HASH: the pixel kinds are never rows, so a request that
  // names every kind it can, once, and both extra rows stays below it)
  if (r.num_rows < 0 || r.num_rows > MP_OBS_KINDS + 1 || (r.num_rows > 0 && !r.rows))
    return fail(MP_ERR_INVALID, "%s: num_rows %d with rows %p; every kind may be named once", who,
                r.num_rows, (const void*)r.rows);
  HIP_TRY(hipSetDevice(e->device));
  char name[64];
  snprintf(name, sizeof name, "%s (actions)", who);
  if (int rc = check_bank(e, r.actions, (K - 1) * r.actions_step_bytes + ablock, name)) return rc;
  snprintf(name, sizeof name, "%s (worlds)", who);
  if (list)
    if (int rc = check_bank(e, list->worlds, C * 4u, name)) return rc;
  StepManyLaunch l = {};
  if (mask) {
    if (!mask->active && !until) return fail(MP_ERR_INVALID, "%s: NULL active", who);
    if (!mask->active && mask->step != 0)
      return fail(MP_ERR_INVALID, "%s: active_step_bytes %llu with a NULL active", who, (unsigned long long)mask->step);
    if (mask->step != 0 && (uint64_t)mask->step < C)
      return fail(MP_ERR_INVALID, "%s: active_step_bytes %llu is neither 0 nor at least one step's row of %llu "
                  "bytes", who, (unsigned long long)mask->step, (unsigned long long)C);
    snprintf(name, sizeof name, "%s (active)", who);
    if (mask->active)
      if (int rc = check_bank(e, mask->active, (K - 1) * (uint64_t)mask->step + C, name)) return rc;
    if (until) {
      // (stopped, ran, returns: written by the launch — device memory, whole extents)
      if ((uintptr_t)until->ran & 3)
        return fail(MP_ERR_INVALID, "%s: ran %p is not 4-byte aligned", who, (const void*)until->ran);
      if ((uintptr_t)until->returns & 7)
        return fail(MP_ERR_INVALID, "%s: returns %p is not 8-byte aligned", who, (const void*)until->returns);
      snprintf(name, sizeof name, "%s (stopped)", who);
      if (until->stopped)
        if (int rc = check_bank(e, until->stopped, N, name)) return rc;
      snprintf(name, sizeof name, "%s (ran)", who);
      if (until->ran)
        if (int rc = check_bank(e, until->ran, C * 4u, name)) return rc;
      snprintf(name, sizeof name, "%s (returns)", who);
      if (until->returns)
        if (int rc = check_bank(e, until->returns, C * P * 8u, name)) return rc;
    }
    // (a slot row of a skipped world has no defined content)
    if (e->ring_slots > 0)
      return fail(MP_ERR_UNSUPPORTED, "%s: a rollout ring is bound (mp_bind_output_ring); a masked step "
                  "writes no ring slot — unbind the ring first", who);
    if (e->unfused == 2 && (e->agent_view() || e->bound[MP_OBS_WORLD_RGB]))
      return fail(MP_ERR_UNSUPPORTED, "%s: the engine was created with MpConfig.unfused = 2 (one launch a "
                  "step) and has a pixel view bound; a masked step is the step kernels and a draw per view", who);
    l.active = *mask;
  }
  l.many.steps = r.steps;
  l.many.actions_step = (long long)(r.actions_step_bytes / 4);
  l.rows.layer_lut = e->d_layer_lut;
  const StepOutputs o = e->outputs();
  bool seen[kStepRowCount] = {};
  for (int i = 0; i < r.num_rows; ++i) {
    const MpStepRow& row = r.rows[i];
    const int kind = row.kind, index = step_row_index(kind);
    if (index < 0)
      return fail(MP_ERR_INVALID, "%s: rows[%d] names kind %d, which is no observation kind", who, i, kind);
    if (MpEngine::is_pixel_kind(kind))
      return fail(MP_ERR_INVALID, "%s: rows[%d] names pixel kind %d; a K-step launch draws no frames — "
                  "intermediate frames are what mp_step with a rollout ring (mp_bind_output_ring) writes",
                  who, i, kind);
    const StepRowKind& k = kStepRowKinds.of[index];
    if (!k.name) return fail(MP_ERR_INVALID, "%s: kind %d has no per-step rows", who, kind);
    if (seen[index]) return fail(MP_ERR_INVALID, "%s: %s (kind %d) is named twice", who, k.name, kind);
    seen[index] = true;
    // (MP_STEP_ROW_STATE: a row is the N records; MP_STEP_ROW_HASH: their N hashes)
    // (every kind's block is N equal parts: with a list a row holds C of them)
    const uint64_t block = (k.place == kRowState ? mp_snapshot_bytes(e)
                            : k.place == kRowHash ? N * 8u : mp_obs_bytes(e, (MpObsKind)kind)) / N * C;
    const uint64_t elem = (uint64_t)k.elem;
    if (block == 0)
      return fail(MP_ERR_UNSUPPORTED, "%s: this substrate has no observation %s (kind %d)", who, k.name, kind);
    if (!row.rows) return fail(MP_ERR_INVALID, "%s: rows[%d] (%s) has no buffer", who, i, k.name);
    // (produced or not does not depend on the ring slot: a ring-bound kind is bound in every slot)
    if (k.place == kRowLevel && !level_source(o, kind))
      return fail(MP_ERR_UNSUPPORTED,
                  "%s: observation %s (kind %d) is not produced (a debug observation: bind it, or create "
                  "the engine with debug_observations)", who, k.name, kind);
    if (row.step_bytes < block || row.step_bytes % elem)
      return fail(MP_ERR_INVALID, "%s: step_bytes of %s is %llu; it must be a multiple of %llu that "
                  "holds one step's rows of %llu bytes", who, k.name, (unsigned long long)row.step_bytes,
                  (unsigned long long)elem, (unsigned long long)block);
    if ((uintptr_t)row.rows % elem)
      return fail(MP_ERR_INVALID, "%s: the %s buffer %p is not %llu-byte aligned", who, k.name, row.rows,
                  (unsigned long long)elem);
    snprintf(name, sizeof name, "%s (%s)", who, k.name);
    if (int rc = check_bank(e, row.rows, (K - 1) * row.step_bytes + block, name)) return rc;
    uint8_t* const base = (uint8_t*)row.rows;
    const long long bytes = (long long)row.step_bytes;
    l.any_rows = l.any_rows || k.place != kRowFive;
    switch (k.place) {
      case kRowFive: l.many.row[k.slot] = base; l.many.row_bytes[k.slot] = bytes; break;
      case kRowFin: l.rows.fin[k.slot] = base; l.rows.fin_bytes[k.slot] = bytes; break;
      case kRowLayer: l.rows.layer = base; l.rows.layer_bytes = bytes; break;
      case kRowState: l.state.row = base; l.state.bytes = bytes; break;
      case kRowHash: l.hash.row = base; l.hash.bytes = bytes; l.hash.mask = e->d_hash_mask; break;
      default: {
        StepRows::Level& lv = l.rows.level[l.rows.n_level++];
        lv.which = kind;   // (launch_step_many resolves the buffer: a rollout ring moves it per submission)
        lv.row = base;
        lv.bytes = bytes;
        lv.count = (long long)(block / 8 / C);
      }
    }
  }
  if (until) {
    // stopped, ran and returns are written while other waves still read the actions, the mask and
    // `stopped`, and write the rows: none of the three may overlap anything else the request names
    struct Range { const char* what; uintptr_t at; uint64_t bytes; };
    std::vector<Range> all = {{"actions", (uintptr_t)r.actions, (K - 1) * r.actions_step_bytes + ablock}};
    if (mask && mask->active) all.push_back({"active", (uintptr_t)mask->active, (K - 1) * (uint64_t)mask->step + C});
    for (int i = 0; i < r.num_rows; ++i) {
      const int index = step_row_index(r.rows[i].kind);
      const StepRowKind& k = kStepRowKinds.of[index];
      const uint64_t block = (k.place == kRowState ? mp_snapshot_bytes(e)
                              : k.place == kRowHash ? N * 8u : mp_obs_bytes(e, (MpObsKind)r.rows[i].kind)) / N * C;
      all.push_back({k.name, (uintptr_t)r.rows[i].rows, (K - 1) * r.rows[i].step_bytes + block});
      // (the list is read by every wave while the rows are written)
      if (list && (uintptr_t)list->worlds < all.back().at + all.back().bytes &&
          all.back().at < (uintptr_t)list->worlds + C * 4u)
        return fail(MP_ERR_INVALID, "%s: worlds overlaps the %s buffer, which the request writes", who, k.name);
    }
    if (list) all.push_back({"worlds", (uintptr_t)list->worlds, C * 4u});
    const size_t first = all.size();
    if (until->stopped) all.push_back({"stopped", (uintptr_t)until->stopped, N});
    if (until->ran) all.push_back({"ran", (uintptr_t)until->ran, C * 4u});
    if (until->returns) all.push_back({"returns", (uintptr_t)until->returns, C * P * 8u});
    for (size_t i = first; i < all.size(); ++i)
      for (size_t j = 0; j < i; ++j)
        if (all[i].at < all[j].at + all[j].bytes && all[j].at < all[i].at + all[i].bytes)
          return fail(MP_ERR_INVALID, "%s: %s overlaps %s; stopped, ran and returns must not overlap each other "
                      "or any other buffer of the request", who, all[i].what, all[j].what);
  }
  if (e->folding()) {
    // registered episode statistics (MpEpisodeStats): the launch behind this one reads these
    if (!l.many.row[0] || !l.many.row[2])
      return fail(MP_ERR_INVALID, "%s: episode statistics are registered (MpEpisodeStats); the request must name "
                  "the REWARD and STEP_TYPE rows", who);
    if (!l.many.row[4] && e->stats_cols.C + e->stats_cols.C2 > 0)
      return fail(MP_ERR_INVALID, "%s: episode statistics with event columns are registered (MpEpisodeStats); "
                  "the request must name the EVENTS row", who);
    if (until && !until->ran)
      return fail(MP_ERR_INVALID, "%s: episode statistics are registered (MpEpisodeStats); the request must "
                  "name ran (which steps ran is read from it)", who);
  }
  if (list) {
    // the claim table: the first listed request's allocation (zeroed: generation 0 is nobody's)
    if (!e->d_listed_claim) {
      HIP_TRY(hipMalloc((void**)&e->d_listed_claim, N * 8u));
      HIP_TRY(hipMemsetAsync(e->d_listed_claim, 0, N * 8u, e->stream));
    }
    if (++e->listed_generation == 0) {   // (2^32 requests later: start over from a cleared table)
      HIP_TRY(hipMemsetAsync(e->d_listed_claim, 0, N * 8u, e->stream));
      e->listed_generation = 1;
    }
    list->claim = e->d_listed_claim;
    list->generation = e->listed_generation;
  }
  e->touched = true;
  return submit(e, r.fields ? STEP_MODE_FIELDS : STEP_MODE_STEP, r.actions, nullptr, nullptr, nullptr, 0, &l, until,
                list);
}

// What mp_restore does when `bytes` is sizeof(MpStepMany): every non-NULL per_step[i] is one row
// of the i-th of the five kinds.
static int many_request(MpEngine* e, const MpStepMany& r) {
  static const char kWho[] = "MpStepMany";
  if (r.struct_size != sizeof(MpStepMany))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStepMany));
  MpStepRow rows[5];
  MpStepTrajectory t = {sizeof t, r.steps, r.fields, 0, r.actions, r.actions_step_bytes, rows};
  for (int kind = 0; kind < MP_OBS_KINDS; ++kind) {
    const StepRowKind& k = kStepRowKinds.of[kind];
    if (k.place == kRowFive && r.per_step[k.slot])
      rows[t.num_rows++] = {kind, 0, r.per_step[k.slot], r.per_step_bytes[k.slot]};
  }
  return step_request(e, kWho, t);
}

// ... and when it is sizeof(MpStepTrajectory): the request as it stands.
static int trajectory_request(MpEngine* e, const MpStepTrajectory& r) {
  static const char kWho[] = "MpStepTrajectory";
  if (r.struct_size != sizeof(MpStepTrajectory))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStepTrajectory));
  return step_request(e, kWho, r);
}

// ... and when it is sizeof(MpStepActive): the same request under a device mask.
static int active_request(MpEngine* e, const MpStepActive& r) {
  static const char kWho[] = "MpStepActive";
  if (r.struct_size != sizeof(MpStepActive))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStepActive));
  for (uint64_t word : r.reserved)
    if (word != 0) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", kWho);
  if (r.active_step_bytes > (1ull << 40))
    return fail(MP_ERR_INVALID, "%s: active_step_bytes %llu", kWho, (unsigned long long)r.active_step_bytes);
  const MpStepTrajectory t = {sizeof t, r.steps, r.fields, r.num_rows, r.actions, r.actions_step_bytes, r.rows};
  const ActiveArgs mask = {r.active, (long long)r.active_step_bytes};
  return step_request(e, kWho, t, &mask);
}

// ... and when it is sizeof(MpStepUntil): the masked request with a stop state.
static int until_request(MpEngine* e, const MpStepUntil& r) {
  static const char kWho[] = "MpStepUntil";
  if (r.struct_size != sizeof(MpStepUntil))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStepUntil));
  if (r.pad != 0) return fail(MP_ERR_INVALID, "%s: pad must be 0", kWho);
  for (uint64_t word : r.reserved)
    if (word != 0) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", kWho);
  if (r.stop & ~(uint32_t)(MP_STOP_LAST | MP_STOP_REWARD))
    return fail(MP_ERR_INVALID, "%s: stop %u has bits beyond MP_STOP_LAST | MP_STOP_REWARD", kWho, r.stop);
  if (!std::isfinite(r.gamma)) return fail(MP_ERR_INVALID, "%s: gamma %g is not finite", kWho, r.gamma);
  if (r.active_step_bytes > (1ull << 40))
    return fail(MP_ERR_INVALID, "%s: active_step_bytes %llu", kWho, (unsigned long long)r.active_step_bytes);
  const MpStepTrajectory t = {sizeof t, r.steps, r.fields, r.num_rows, r.actions, r.actions_step_bytes, r.rows};
  const ActiveArgs mask = {r.active, (long long)r.active_step_bytes};
  const UntilArgs until = {r.stop, r.stopped, r.ran, r.returns, r.gamma};
  return step_request(e, kWho, t, &mask, &until);
}

// ... and when it is sizeof(MpStepListed): the stopping request of the worlds a device list names.
static int listed_request(MpEngine* e, const MpStepListed& r) {
  static const char kWho[] = "MpStepListed";
  if (r.struct_size != sizeof(MpStepListed))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStepListed));
  if (r.pad != 0 || r.reserved2 != 0) return fail(MP_ERR_INVALID, "%s: pad and reserved2 must be 0", kWho);
  for (uint64_t word : r.reserved)
    if (word != 0) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", kWho);
  for (uint64_t word : r.reserved3)
    if (word != 0) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", kWho);
  if (r.stop & ~(uint32_t)(MP_STOP_LAST | MP_STOP_REWARD))
    return fail(MP_ERR_INVALID, "%s: stop %u has bits beyond MP_STOP_LAST | MP_STOP_REWARD", kWho, r.stop);
  if (!std::isfinite(r.gamma)) return fail(MP_ERR_INVALID, "%s: gamma %g is not finite", kWho, r.gamma);
  if (r.active_step_bytes > (1ull << 40))
    return fail(MP_ERR_INVALID, "%s: active_step_bytes %llu", kWho, (unsigned long long)r.active_step_bytes);
  const MpStepTrajectory t = {sizeof t, r.steps, r.fields, r.num_rows, r.actions, r.actions_step_bytes, r.rows};
  const ActiveArgs mask = {r.active, (long long)r.active_step_bytes};
  const UntilArgs until = {r.stop, r.stopped, r.ran, r.returns, r.gamma};
  ListArgs list = {r.worlds, r.count, nullptr, 0u};
  return step_request(e, kWho, t, &mask, &until, &list);
}

// An MpStatesObserve request (include/mp_engine.h; carried by mp_snapshot): observations of rows
// of a bank, enqueued on the engine's stream.  Everything is checked before the first launch, and
// nothing of the engine's is written but its own scratch and the parity of the claim counters
// (which a draw-only launch of mp_observe moves on in the same way).
static int grow_obs_buffer(uint8_t** buf, uint64_t* have, uint64_t need) {
  if (*have >= need) return MP_OK;
  // (hipFree waits for the launches that may still read the old one)
  if (*buf) { HIP_TRY(hipFree(*buf)); *buf = nullptr; *have = 0; }
  HIP_TRY(hipMalloc((void**)buf, need));
  *have = need;
  return MP_OK;
}

// What MpStatesObserve and MpStatesView check before they launch; the first is read as the second
// without players.  `per_player`: MpStatesView's own rules (players, no MP_OBS_WORLD_RGB, and dst
// of a pixel kind on any byte); else MpStatesObserve's (mp_observe's: a pooled span is staged by
// 16-byte lines).  `size`: the request's own.
struct StatesDraw {
  bool pixel;
  uint64_t per, need;   // bytes of an element, of dst
};
static int states_front(MpEngine* e, const char* kWho, const MpStatesView& r, size_t size, bool per_player,
                        StatesDraw* d) {
  if (!e) return fail(MP_ERR_INVALID, "%s: NULL engine", kWho);
  if (r.struct_size != size)
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, size);
  if (r.reserved[0] || r.reserved[1]) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", kWho);
  if (!r.bank || !r.dst) return fail(MP_ERR_INVALID, "%s: NULL bank or dst", kWho);
  if (per_player && !r.players) return fail(MP_ERR_INVALID, "%s: NULL players", kWho);
  if (int rc = check_counts(kWho, r.count, r.bank_rows)) return rc;
  if (int rc = check_row_list(kWho, r.rows, r.count, r.bank_rows, "drawn")) return rc;
  if (int rc = check_fingerprint(kWho, r.fingerprint, e->fingerprint, "engine's")) return rc;
  const int kind = r.kind;
  if (kind < 0 || kind >= MP_OBS_KINDS)
    return fail(MP_ERR_INVALID, "%s: kind %d is no observation kind", kWho, kind);
  if (per_player && kind == MP_OBS_WORLD_RGB)
    return fail(MP_ERR_INVALID, "%s: MP_OBS_WORLD_RGB is not a per-player kind (MpStatesObserve draws it)", kWho);
  d->pixel = MpEngine::is_pixel_kind(kind);
  uint64_t elem = 1;   // what dst is aligned to
  switch (kind) {
    case MP_OBS_LAYER: case MP_OBS_POSITION: case MP_OBS_ORIENTATION: elem = 4; break;
    case MP_OBS_READY_TO_SHOOT: case MP_OBS_INVENTORY: elem = 8; break;
    default:
      if (!d->pixel)
        return fail(MP_ERR_INVALID, "%s: kind %d is not a function of the record (a transition kind: what a "
                    "step or a reset reports, which no saved state holds)", kWho, kind);
  }
  const bool pooled =
      !per_player && (MpEngine::pool_of(kind) > 1 || (kind == MP_OBS_WORLD_RGB && e->world_pool > 1));
  if (pooled) elem = 16;
  d->per = mp_obs_bytes(e, (MpObsKind)kind) / ((uint64_t)e->N * (per_player ? (uint64_t)e->t.P : 1u));
  if (d->per == 0)
    return fail(MP_ERR_UNSUPPORTED, "%s: this substrate has no observation %d", kWho, kind);
  if (int rc = check_dst_bytes(kWho, r.count, d->per, r.dst_bytes, &d->need)) return rc;
  if ((uintptr_t)r.dst % elem)
    return fail(MP_ERR_INVALID, "%s: dst %p is not %llu-byte aligned%s", kWho, r.dst, (unsigned long long)elem,
                pooled ? " (a pooled view's buffer)" : "");
  if (int rc = check_aligned(kWho, "rows", r.rows, 4)) return rc;
  if (int rc = check_aligned(kWho, "players", r.players, 4)) return rc;
  const uint64_t count = (uint64_t)r.count;   // (records are read in 16-byte lines)
  return check_extents(e, kWho, {{"bank", r.bank, (uint64_t)r.bank_rows * (uint64_t)e->t.world_stride, 16},
                                 {"rows", r.rows, count * 4, 1},
                                 {"players", r.players, count * 4, 1},
                                 {"dst", r.dst, d->need, 1}});
}

static int states_observe(MpEngine* e, const MpStatesObserve& r) {
  static const char kWho[] = "MpStatesObserve";
  const MpStatesView q = {r.struct_size, r.kind, r.fingerprint, r.bank, r.rows, nullptr, r.dst, r.dst_bytes,
                          r.bank_rows, r.count, {0, 0}};
  StatesDraw d;
  if (int rc = states_front(e, kWho, q, sizeof r, false, &d)) return rc;
  const int kind = r.kind;
  const bool pixel = d.pixel;
  const uint64_t per = d.per, count = (uint64_t)r.count, S = (uint64_t)e->t.world_stride;
  const uint8_t* bank = (const uint8_t*)r.bank;
  if (!pixel && kind != MP_OBS_LAYER) {
    launch_state_obs(e->t, e->sub, kind, bank, r.bank_rows, r.rows, r.count, r.dst, e->stream);
    HIP_TRY(hipGetLastError());
    return MP_OK;
  }
  // LAYER and the pixel kinds are drawn by launches that take contiguous records: k_layer_view and
  // the draw-only frame launch.  The engine's own draw plan serves N worlds; another count gets a
  // plan of its own, which must fit the LDS beside the composite cache (sized at mp_create for
  // the engine's plans; plan_frame shrinks its ring down to two single-world batches to fit).
  const bool agents = kind != MP_OBS_WORLD_RGB;
  const int views = agents ? 0 : 1, pk = agents ? MpEngine::pool_of(kind) : 1;
  FramePlan p = {};
  if (pixel) {
    p = r.count == e->N ? e->frame_plan(0, views, pk)
                        : plan_frame(e->t, e->sub, r.count, false, views, e->num_cus, nullptr, pk, e->world_pool);
    const int lds = frame_lds_bytes(e->t, p, pk, e->world_pool, views);
    if (lds > 160 * 1024)
      return fail(MP_ERR_UNSUPPORTED, "%s: a draw plan for %d rows of kind %d needs %d B of LDS beside this "
                  "engine's composite cache", kWho, r.count, kind, lds);
  }
  // With a row list: the rows copied next to each other into the engine's scratch first.
  const uint8_t* state = bank;
  if (r.rows) {
    if (int rc = grow_obs_buffer(&e->d_obs_rows, &e->obs_rows_bytes, count * S)) return rc;
    const uint64_t stash = 64 + (uint64_t)kObsStashSlots * per;
    if (e->obs_stash_bytes < stash) {
      if (int rc = grow_obs_buffer(&e->d_obs_stash, &e->obs_stash_bytes, stash)) return rc;
      HIP_TRY(hipMemsetAsync(e->d_obs_stash, 0, 64, e->stream));
    }
    launch_gather_rows(e->t, bank, r.bank_rows, r.rows, r.count, e->d_obs_rows, (const uint8_t*)r.dst, per,
                       e->d_obs_stash, e->stream);
    state = e->d_obs_rows;
  }
  if (pixel) {
    stepk::StepArgs args = {};
    args.state = const_cast<uint8_t*>(state);
    args.num_worlds = r.count;
    p.parity = e->frame_launches++ & 1;
    uint8_t* out = (uint8_t*)r.dst;
    launch_frame(e->t, nullptr, args, agents ? out : nullptr, agents ? nullptr : out, p, e->stream, pk,
                 e->world_pool);
  } else {
    launch_layer_view(e->t, state, (int32_t*)r.dst, r.count, e->stream);
  }
  if (r.rows) launch_restore_stash((uint8_t*)r.dst, per, e->d_obs_stash, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// An MpStatesView request (include/mp_engine.h; carried by mp_snapshot): one player's view of each
// sampled row, enqueued on the engine's stream.  Everything is checked before the launch; nothing
// of the engine's is written and no device memory is allocated or freed.
static int states_view(MpEngine* e, const MpStatesView& r) {
  static const char kWho[] = "MpStatesView";
  StatesDraw d;
  if (int rc = states_front(e, kWho, r, sizeof r, true, &d)) return rc;
  const int kind = r.kind;
  const uint64_t per = d.per;
  const uint8_t* bank = (const uint8_t*)r.bank;
  if (!d.pixel && kind != MP_OBS_LAYER) {
    launch_state_view_scalar(e->t, e->sub, kind, bank, r.bank_rows, r.rows, r.players, r.count, r.dst, e->stream);
    HIP_TRY(hipGetLastError());
    return MP_OK;
  }
  const StateViewPlan p = state_view_plan(e->t, kind, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's record and row of view cells need %d B of LDS beside the "
                "renderer's tables", kWho, p.lds);
  if ((uint64_t)p.view_bytes != per)   // (the launch's stride through dst is the one dst_bytes was checked with)
    return fail(MP_ERR_HIP, "%s: a view of kind %d is %llu bytes to the engine and %u to the kernel", kWho, kind,
                (unsigned long long)per, p.view_bytes);
  launch_state_view(e->t, p, kind, bank, r.bank_rows, r.rows, r.players, r.count, r.dst, e->d_layer_lut, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

uint64_t mp_snapshot_bytes(const MpEngine* e) {
  return e ? (uint64_t)e->N * e->t.world_stride : 0;
}

// An MpStateLayout request (include/mp_engine.h; carried by mp_snapshot; `e` may be NULL: the
// host-only question).  The tail's fields are state_check.h's list of WorldTail's members.
static int state_layout(const MpEngine* e, MpStateLayout* r) {
  static const char kWho[] = "MpStateLayout";
  if (r->struct_size != sizeof(MpStateLayout))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r->struct_size, sizeof(MpStateLayout));
  MpStateField* fields = r->fields;
  const int32_t cap = r->fields_cap;
  state_check::CheckTables ck;
  uint64_t fingerprint;
  int player_block = -1;
  if (e) {
    ck = e->check;
    fingerprint = e->fingerprint;
    if (e->substrate == MPK_SUBSTRATE_THE_MATRIX) player_block = e->sub.mx.player_block;
  } else {
    HostStage h;
    if (int rc = host_stage(r->pack, r->pack_len, r->cfg, &h)) return rc;
    build_check_tables(h.d, &ck);
    fingerprint = state_fingerprint(h.pack, h.d.t);
    if (h.d.sub.substrate == MPK_SUBSTRATE_THE_MATRIX) player_block = h.d.sub.mx.player_block;
  }
  if (fields && cap < state_check::kNumTailFields)
    return fail(MP_ERR_INVALID, "%s: fields_cap %d, the tail has %d fields", kWho, cap, state_check::kNumTailFields);
  r->layout_version = MP_RECORD_LAYOUT_VERSION;
  r->map_h = ck.H; r->map_w = ck.W; r->num_layers = ck.L; r->num_players = ck.P; r->num_states = ck.nstates;
  r->grid_planes = ck.grid_planes; r->grid_bytes = ck.grid_bytes; r->grid_pad = ck.grid_pad;
  r->world_stride = ck.world_stride; r->tail_bytes = (int32_t)sizeof(WorldTail);
  r->max_frames = ck.max_frames; r->avatar_layer = ck.avatar_layer; r->substrate = ck.substrate;
  r->player_block = player_block;
  r->reserved[0] = r->reserved[1] = 0;
  r->fingerprint = fingerprint;
  r->num_fields = state_check::kNumTailFields;
  for (int i = 0; fields && i < state_check::kNumTailFields; ++i) {
    const state_check::TailField& f = state_check::kTailFields[i];
    memset(&fields[i], 0, sizeof fields[i]);
    snprintf(fields[i].name, sizeof fields[i].name, "%s", f.name);
    fields[i].offset = f.offset; fields[i].elem_bytes = f.elem; fields[i].count = f.count;
  }
  return MP_OK;
}

// An MpStatesCheck request (include/mp_engine.h; carried by mp_snapshot).  Everything is checked
// before the one launch; the launch writes `out` and, for a refused row or a bad index, the
// fault words — nothing else of the engine's.
static int states_check(MpEngine* e, const MpStatesCheck& r) {
  static const char kWho[] = "MpStatesCheck";
  if (r.struct_size != sizeof(MpStatesCheck))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStatesCheck));
  if (r.op != MP_CHECK_ROWS && r.op != MP_CHECK_HOST && r.op != MP_CHECK_FILTER)
    return fail(MP_ERR_INVALID, "%s: unknown op %d", kWho, r.op);
  if ((r.op == MP_CHECK_HOST) != (e == nullptr))
    return fail(MP_ERR_INVALID, "%s: MP_CHECK_HOST goes without an engine, the other forms with one", kWho);
  if (!r.bank || !r.out) return fail(MP_ERR_INVALID, "%s: NULL bank or out", kWho);
  if (int rc = check_counts(kWho, r.count, r.bank_rows)) return rc;
  if (int rc = check_row_list(kWho, r.rows, r.count, r.bank_rows, "judged", true, r.op == MP_CHECK_FILTER,
                              "; a filter needs its src"))
    return rc;
  const uint64_t count = (uint64_t)r.count, need = count * (r.op == MP_CHECK_FILTER ? 4u : 8u);
  if (r.out_bytes < need)
    return fail(MP_ERR_INVALID, "%s: %d verdicts need %llu bytes, out has %llu", kWho, r.count,
                (unsigned long long)need, (unsigned long long)r.out_bytes);
  if (((uintptr_t)r.out & 3) || ((uintptr_t)r.rows & 3))
    return fail(MP_ERR_INVALID, "%s: rows %p and out %p must be 4-byte aligned", kWho, (const void*)r.rows, r.out);
  if (r.op == MP_CHECK_HOST) {
    HostStage h;
    if (int rc = host_stage(r.pack, r.pack_len, r.cfg, &h)) return rc;
    const uint64_t fingerprint = state_fingerprint(h.pack, h.d.t);
    if (r.fingerprint != fingerprint)
      return fail(MP_ERR_INVALID, "%s: the rows' state fingerprint %016llx is not this pack's (%016llx)", kWho,
                  (unsigned long long)r.fingerprint, (unsigned long long)fingerprint);
    state_check::CheckTables ck;
    build_check_tables(h.d, &ck);
    check_rows_host(ck, (const uint8_t*)r.bank, r.bank_rows, r.rows, r.count, (int32_t*)r.out);
    return MP_OK;
  }
  if (int rc = check_fingerprint(kWho, r.fingerprint, e->fingerprint, "engine's")) return rc;
  if (r.op == MP_CHECK_FILTER && r.count != e->N)
    return fail(MP_ERR_INVALID, "%s: a filter takes the src of a load, one entry per world (count %d, the "
                "engine has %d worlds)", kWho, r.count, e->N);
  // (records are read in 16-byte lines)
  if (int rc = check_extents(e, kWho, {{"bank", r.bank, (uint64_t)r.bank_rows * (uint64_t)e->t.world_stride, 16},
                                       {"rows", r.rows, count * 4, 1},
                                       {"out", r.out, need, 1}}))
    return rc;
  if (r.op == MP_CHECK_FILTER)
    launch_filter_states(e->d_check, (const uint8_t*)r.bank, r.bank_rows, r.rows, r.count, (int32_t*)r.out,
                         e->t.fault, e->stream);
  else
    launch_check_states(e->d_check, (const uint8_t*)r.bank, r.bank_rows, r.rows, r.count, (int32_t*)r.out,
                        e->t.fault, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// An MpStatesHash request (include/mp_engine.h; carried by mp_snapshot; `e` is NULL for the host
// form).  Everything is checked before the one launch; the launch writes `out` and, for a bad
// index, the fault words — nothing else of the engine's, and `touched` stays what it was.
static int states_hash(MpEngine* e, const MpStatesHash& r) {
  static const char kWho[] = "MpStatesHash";
  if (r.struct_size != sizeof(MpStatesHash))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpStatesHash));
  if (r.op != MP_HASH_ROWS && r.op != MP_HASH_WORLDS && r.op != MP_HASH_HOST && r.op != MP_HASH_MASK)
    return fail(MP_ERR_INVALID, "%s: unknown op %d", kWho, r.op);
  if ((r.op == MP_HASH_HOST && e) || ((r.op == MP_HASH_ROWS || r.op == MP_HASH_WORLDS) && !e))
    return fail(MP_ERR_INVALID, "%s: MP_HASH_HOST goes without an engine, MP_HASH_ROWS and MP_HASH_WORLDS with one", kWho);
  if ((r.flags & ~(MP_HASH_CUSTOM | MP_HASH_PLAYER_BLOCK)) != 0 ||
      (!(r.flags & MP_HASH_CUSTOM) && (r.flags != 0 || r.plane_mask != 0 || r.field_mask != 0)))
    return fail(MP_ERR_INVALID, "%s: flags %d with plane_mask %llx and field_mask %x: the default spec is all "
                "zeros, a custom one has MP_HASH_CUSTOM", kWho, r.flags, (unsigned long long)r.plane_mask, r.field_mask);
  if (!r.out) return fail(MP_ERR_INVALID, "%s: NULL out", kWho);
  const state_hash::Spec spec = {r.plane_mask, r.field_mask, r.flags & MP_HASH_CUSTOM ? 1 : 0,
                                 r.flags & MP_HASH_PLAYER_BLOCK ? 1 : 0};
  const bool rows_op = r.op == MP_HASH_ROWS || r.op == MP_HASH_HOST;
  if (rows_op && !r.bank) return fail(MP_ERR_INVALID, "%s: NULL bank", kWho);
  if (r.op != MP_HASH_MASK) {
    if (int rc = check_counts(kWho, r.count, r.bank_rows, rows_op)) return rc;
    if (rows_op)
      if (int rc = check_row_list(kWho, r.rows, r.count, r.bank_rows, "hashed")) return rc;
    if (r.op == MP_HASH_WORLDS && !r.rows && r.count != e->N)
      return fail(MP_ERR_INVALID, "%s: without a world list every world is hashed (count %d, the engine has %d)",
                  kWho, r.count, e->N);
    if (r.out_bytes < (uint64_t)r.count * 8u)
      return fail(MP_ERR_INVALID, "%s: %d hashes need %llu bytes, out has %llu", kWho, r.count,
                  (unsigned long long)r.count * 8u, (unsigned long long)r.out_bytes);
    if (((uintptr_t)r.out & 7) || ((uintptr_t)r.rows & 3))
      return fail(MP_ERR_INVALID, "%s: out %p must be 8-byte aligned, rows %p 4-byte aligned", kWho, r.out,
                  (const void*)r.rows);
  }
  // the layout and the fingerprint: the engine's, or the pack's by the host stage
  state_hash::Layout lay;
  uint64_t fingerprint;
  if (e) {
    lay = e->hash_layout();
    fingerprint = e->fingerprint;
  } else {
    HostStage h;
    if (int rc = host_stage(r.pack, r.pack_len, r.cfg, &h)) return rc;
    lay = hash_layout_of(h.d);
    fingerprint = state_fingerprint(h.pack, h.d.t);
  }
  if (const char* why = state_hash::spec_error(lay, spec))
    return fail(MP_ERR_INVALID, "%s: %s (plane_mask %llx over %d planes, field_mask %x over %d fields)", kWho, why,
                (unsigned long long)r.plane_mask, lay.grid_planes, r.field_mask, state_hash::TF_COUNT);
  const uint64_t S = (uint64_t)lay.world_stride;
  if (r.op == MP_HASH_MASK) {
    if (r.out_bytes < S)
      return fail(MP_ERR_INVALID, "%s: the mask of a row is %llu bytes, out has %llu", kWho,
                  (unsigned long long)S, (unsigned long long)r.out_bytes);
    state_hash::build_byte_mask(lay, spec, (uint8_t*)r.out);
    return MP_OK;
  }
  if (rows_op)
    if (int rc = check_fingerprint(kWho, r.fingerprint, fingerprint, e ? "engine's" : "pack's")) return rc;
  if (r.op == MP_HASH_HOST) {
    std::vector<uint32_t> words((size_t)S / 4);
    state_hash::build_byte_mask(lay, spec, reinterpret_cast<uint8_t*>(words.data()));
    const int bad = hash_rows_host(words.data(), (const uint8_t*)r.bank, r.bank_rows, (int)S, r.rows, r.count,
                                   (uint64_t*)r.out);
    if (bad >= 0)
      return fail(MP_ERR_INVALID, "%s: rows[%d] = %d is not a row of the bank; element %d of out was left as it "
                  "was", kWho, bad, r.rows ? r.rows[bad] : bad, bad);
    return MP_OK;
  }
  if (r.op == MP_HASH_WORLDS && !e->has_state)
    return fail(MP_ERR_INVALID, "%s: the engine has never been reset; there is no state to hash", kWho);
  const uint64_t count = (uint64_t)r.count;   // (records are read in 16-byte lines)
  if (int rc = check_extents(e, kWho, {{"bank", rows_op ? r.bank : nullptr, (uint64_t)r.bank_rows * S, 16},
                                       {"rows", r.rows, count * 4, 1},
                                       {"out", r.out, count * 8, 1}}))
    return rc;
  const uint32_t* mask = e->d_hash_mask;
  if (spec.custom) {
    if (!state_hash::same_spec(spec, e->hash_custom)) {
      // another custom spec: its mask replaces the last one's, which launches in flight may still
      // read — behind a wait for the stream (the request's one synchronisation, once per new spec)
      std::vector<uint32_t> words((size_t)S / 4);
      state_hash::build_byte_mask(lay, spec, reinterpret_cast<uint8_t*>(words.data()));
      if (!e->d_hash_custom) HIP_TRY(hipMalloc((void**)&e->d_hash_custom, (size_t)S));
      HIP_TRY(hipStreamSynchronize(e->stream));
      e->hash_custom = state_hash::Spec{};
      HIP_TRY(hipMemcpy(e->d_hash_custom, words.data(), (size_t)S, hipMemcpyHostToDevice));
      e->hash_custom = spec;
    }
    mask = e->d_hash_custom;
  }
  if (rows_op)
    launch_hash_rows(mask, (const uint8_t*)r.bank, r.bank_rows, (int)S, r.rows, r.count, (uint64_t*)r.out,
                     e->t.fault, e->stream);
  else
    launch_hash_rows(mask, (const uint8_t*)e->d_state, e->N, (int)S, r.rows, r.count, (uint64_t*)r.out,
                     e->t.fault, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// An MpEpisodeStarts request (include/mp_engine.h; carried by mp_restore): registers, replaces or
// clears the engine's episode starts.  No launch; everything is checked before anything changes.
static int episode_starts(MpEngine* e, const MpEpisodeStarts& r) {
  static const char kWho[] = "MpEpisodeStarts";
  if (!e) return fail(MP_ERR_INVALID, "%s: NULL engine", kWho);
  if (r.struct_size != sizeof(MpEpisodeStarts))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpEpisodeStarts));
  if (!r.bank) {   // clears the registration: the engine's launches are what they were
    e->has_starts = false;
    e->starts = stepk::StartArgs{};
    return MP_OK;
  }
  if (!e->auto_reset)
    return fail(MP_ERR_INVALID, "%s: the engine was created with auto_reset = 0: no world ever starts an "
                "episode by itself", kWho);
  if (e->unfused == 2)
    return fail(MP_ERR_UNSUPPORTED, "%s: the engine was created with MpConfig.unfused = 2 (one launch a step); "
                "a step with registered episode starts is the step kernels' launch and one per view", kWho);
  if (r.bank_rows <= 0) return fail(MP_ERR_INVALID, "%s: bank_rows %d: the bank has no rows", kWho, r.bank_rows);
  if (!r.rows) return fail(MP_ERR_INVALID, "%s: NULL rows", kWho);
  if (r.fresh != 0 && r.fresh != 1)
    return fail(MP_ERR_INVALID, "%s: fresh %d is neither 0 nor 1", kWho, r.fresh);
  if (int rc = check_fingerprint(kWho, r.fingerprint, e->fingerprint, "engine's")) return rc;
  if (int rc = check_aligned(kWho, "bank", r.bank, 16)) return rc;   // (records are read in 16-byte lines)
  if (((uintptr_t)r.rows & 3) || ((uintptr_t)r.verdicts & 3))
    return fail(MP_ERR_INVALID, "%s: rows %p and verdicts %p must be 4-byte aligned", kWho, (const void*)r.rows,
                (const void*)r.verdicts);
  if (int rc = check_extents(e, kWho, {{"bank", r.bank, (uint64_t)r.bank_rows * (uint64_t)e->t.world_stride, 1},
                                       {"rows", r.rows, (uint64_t)e->N * 4, 1},
                                       {"verdicts", r.verdicts, (uint64_t)r.bank_rows * 8, 1}}))
    return rc;
  e->starts.bank = (const uint8_t*)r.bank;
  e->starts.rows = r.rows;
  e->starts.verdicts = r.verdicts;
  e->starts.bank_rows = r.bank_rows;
  e->starts.fresh = r.fresh;
  e->has_starts = true;
  return MP_OK;
}

// An MpEpisodeStats request (include/mp_engine.h; carried by mp_restore): registers or clears the
// engine's episode statistics (no launch), tallies event rows on the device (one launch), or applies
// the rule to host rows (`e` may be NULL: no device is touched).  Everything is checked first.
static int episode_stats_request(MpEngine* e, const MpEpisodeStats& r) {
  static const char kWho[] = "MpEpisodeStats";
  if (r.struct_size != sizeof(MpEpisodeStats))
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", kWho, r.struct_size, sizeof(MpEpisodeStats));
  if (r.op < MP_STATS_REGISTER || r.op > MP_STATS_HOST) return fail(MP_ERR_INVALID, "%s: unknown op %d", kWho, r.op);
  if (r.op == MP_STATS_HOST ? e != nullptr : e == nullptr)
    return fail(MP_ERR_INVALID, "%s: %s", kWho, e ? "MP_STATS_HOST takes no engine" : "NULL engine");
  if (r.reserved != 0 || r.reserved2[0] != 0 || r.reserved2[1] != 0)
    return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", kWho);
  if (r.op == MP_STATS_CLEAR) {   // the engine's launches are what they were
    e->has_stats = false;
    e->stats = episode_stats::Banks{};
    e->stats_cols = episode_stats::Columns{};
    return MP_OK;
  }
  if (r.num_columns < 0 || r.num_columns > MP_STATS_MAX_COLUMNS)
    return fail(MP_ERR_INVALID, "%s: num_columns %d is outside [0, %d]", kWho, r.num_columns, MP_STATS_MAX_COLUMNS);
  if (r.num_pairs < 0 || r.num_pairs > MP_STATS_MAX_PAIRS)
    return fail(MP_ERR_INVALID, "%s: num_pairs %d is outside [0, %d]", kWho, r.num_pairs, MP_STATS_MAX_PAIRS);
  if ((r.num_columns > 0 && !r.columns) || (r.num_pairs > 0 && !r.pairs))
    return fail(MP_ERR_INVALID, "%s: NULL columns or pairs with a count above 0", kWho);
  episode_stats::Columns cols = {};
  cols.C = r.num_columns;
  cols.C2 = r.num_pairs;
  for (int i = 0; i < r.num_columns + r.num_pairs; ++i) {
    const bool pair = i >= r.num_columns;
    const MpEventColumn& c = pair ? r.pairs[i - r.num_columns] : r.columns[i];
    const char* what = pair ? "pairs" : "columns";
    const int at = pair ? i - r.num_columns : i;
    if (c.player_payload > 1 || c.filter_payload > 2)
      return fail(MP_ERR_INVALID, "%s: %s[%d] names a payload that is neither a nor b", kWho, what, at);
    if (c.player_shift > 31 || c.filter_shift > 31 || c.other_shift > 31)
      return fail(MP_ERR_INVALID, "%s: %s[%d] has a shift of 32 or more", kWho, what, at);
    if (c.reserved[0] || c.reserved[1] || c.reserved[2] || c.reserved2)
      return fail(MP_ERR_INVALID, "%s: %s[%d]: the reserved words must be 0", kWho, what, at);
    (pair ? cols.pair[at] : cols.col[at]) = c;
  }
  const bool events_needed = r.num_columns + r.num_pairs > 0;
  if (r.op == MP_STATS_TALLY || r.op == MP_STATS_HOST) {
    if (r.steps < 1 || r.count < 1)
      return fail(MP_ERR_INVALID, "%s: steps %d and count %d must be at least 1", kWho, r.steps, r.count);
    if (r.op == MP_STATS_TALLY ? !r.events : events_needed && !r.events)
      return fail(MP_ERR_INVALID, "%s: NULL events", kWho);
    if ((r.num_columns > 0 && !r.running.counts) || (r.num_pairs > 0 && !r.running.pairs))
      return fail(MP_ERR_INVALID, "%s: NULL counts or pairs for the columns named", kWho);
  }
  if (r.op == MP_STATS_HOST && (r.num_players < 1 || r.num_players > MP_MAX_PLAYERS))
    return fail(MP_ERR_INVALID, "%s: num_players %d is outside [1, %d]", kWho, r.num_players, MP_MAX_PLAYERS);
  const uint64_t P = r.op == MP_STATS_HOST ? (uint64_t)r.num_players : (uint64_t)e->t.P;
  const uint64_t CP = (uint64_t)r.num_columns * P, PP = (uint64_t)r.num_pairs * P * P;
  episode_stats::Banks b = {r.open, r.episodes, r.dropped, r.running, r.last, r.total};
  if (r.op == MP_STATS_REGISTER || r.op == MP_STATS_HOST) {
    const MpStatsBank* banks[3] = {&r.running, &r.last, &r.total};
    if (!r.open || !r.episodes || !r.dropped) return fail(MP_ERR_INVALID, "%s: NULL open, episodes or dropped", kWho);
    for (const MpStatsBank* k : banks)
      if (!k->returns || !k->length || (r.num_columns > 0 && !k->counts) || (r.num_pairs > 0 && !k->pairs))
        return fail(MP_ERR_INVALID, "%s: a bank (running, last, total) lacks a tensor", kWho);
  }
  if (r.op == MP_STATS_HOST) {
    if (!r.step_type || !r.reward) return fail(MP_ERR_INVALID, "%s: NULL step_type or reward", kWho);
    episode_stats::Rows rows = {};
    rows.columns = r.count; rows.K = r.steps; rows.P = (int)P;
    rows.step_type = r.step_type; rows.step_type_bytes = (long long)r.count * 4;
    rows.reward = r.reward; rows.reward_bytes = (long long)r.count * (long long)P * 8;
    rows.events = r.events; rows.events_bytes = (long long)r.count * MP_EVENT_ROWS * 16;
    rows.active = r.active; rows.active_bytes = r.count;
    rows.ran = r.ran;
    episode_stats_host(cols, b, rows);
    return MP_OK;
  }
  // every tensor: device memory of the engine's device, aligned, its whole extent in one allocation
  std::vector<Extent> all;
  if (r.op == MP_STATS_TALLY) {
    const uint64_t K = (uint64_t)r.steps, M = (uint64_t)r.count;
    all.push_back({"events", r.events, K * M * MP_EVENT_ROWS * 16u, 16});
    if (r.active) all.push_back({"active", r.active, K * M, 1});
    if (r.ran) all.push_back({"ran", r.ran, M * 4u, 4});
    if (CP) all.push_back({"counts", r.running.counts, M * CP * 4u, 4});
    if (PP) all.push_back({"pairs", r.running.pairs, M * PP * 4u, 4});
  } else {
    const uint64_t N = (uint64_t)e->N;
    all.push_back({"open", r.open, N, 1});
    all.push_back({"episodes", r.episodes, N * 4u, 4});
    all.push_back({"dropped", r.dropped, N * 4u, 4});
    const MpStatsBank* banks[3] = {&r.running, &r.last, &r.total};
    static const char* const names[3][4] = {{"running.returns", "running.length", "running.counts", "running.pairs"},
                                            {"last.returns", "last.length", "last.counts", "last.pairs"},
                                            {"total.returns", "total.length", "total.counts", "total.pairs"}};
    for (int k = 0; k < 3; ++k) {
      const uint64_t elem = k == 2 ? 8u : 4u;
      all.push_back({names[k][0], banks[k]->returns, N * P * 8u, 8});
      all.push_back({names[k][1], banks[k]->length, N * elem, elem});
      if (CP) all.push_back({names[k][2], banks[k]->counts, N * CP * elem, elem});
      if (PP) all.push_back({names[k][3], banks[k]->pairs, N * PP * elem, elem});
    }
  }
  if (int rc = check_extents(e, kWho, all.data(), all.size())) return rc;
  if (r.op == MP_STATS_TALLY) {
    episode_stats::Rows rows = {};
    rows.columns = r.count; rows.K = r.steps; rows.P = (int)P;
    rows.events = r.events; rows.events_bytes = (long long)r.count * MP_EVENT_ROWS * 16;
    rows.active = r.active; rows.active_bytes = r.count;
    rows.ran = r.ran;
    launch_episode_stats(cols, b, rows, true, e->stream);
    HIP_TRY(hipGetLastError());
    return MP_OK;
  }
  e->stats_cols = cols;
  e->stats = b;
  e->has_stats = true;
  return MP_OK;
}

// The requests about every viewer's window — MpEgoLayer, MpViewHash, MpEgoPlanes, MpAvatarIds
// (include/mp_engine.h; carried by mp_snapshot; `e` is NULL for the host form) — are one front and four tails.  Each
// draws from bank rows or from the engine's worlds (one launch), registers or clears the tensor
// behind every submission (no launch), or applies its function to host rows; everything is
// checked first.  Their structs begin alike, and the front reads them through that beginning:
struct ViewRequest {
  uint32_t struct_size;
  int32_t op;              // 1: draw, 2: register, 3: host (MP_EGO_*, MP_VIEWHASH_*, MP_EGOPLANES_*)
  uint64_t fingerprint;
  const void* bank;
  const int32_t* rows;
  const int32_t* players;
  void* dst;
  uint64_t dst_bytes;
  int32_t bank_rows, count;
  uint64_t slot_stride;
  int32_t slots;
  int32_t word76;          // MpEgoLayer: reserved; the other two: classes_len
  const void* pack;
  uint64_t pack_len;
  const MpConfig* cfg;
};
enum { VIEW_DRAW = 1, VIEW_REGISTER = 2, VIEW_HOST = 3 };
#define MP_VIEW_FIELD(T, f) (offsetof(T, f) == offsetof(ViewRequest, f))
#define MP_VIEW_PREFIX(T)                                                                                      \
  (MP_VIEW_FIELD(T, op) && MP_VIEW_FIELD(T, fingerprint) && MP_VIEW_FIELD(T, bank) && MP_VIEW_FIELD(T, rows) && \
   MP_VIEW_FIELD(T, players) && MP_VIEW_FIELD(T, dst) && MP_VIEW_FIELD(T, dst_bytes) &&                        \
   MP_VIEW_FIELD(T, bank_rows) && MP_VIEW_FIELD(T, count) && MP_VIEW_FIELD(T, slot_stride) &&                  \
   MP_VIEW_FIELD(T, slots) && MP_VIEW_FIELD(T, pack) && MP_VIEW_FIELD(T, pack_len) && MP_VIEW_FIELD(T, cfg) && \
   sizeof(T) >= sizeof(ViewRequest))
static_assert(MP_VIEW_PREFIX(MpEgoLayer) && MP_VIEW_PREFIX(MpViewHash) && MP_VIEW_PREFIX(MpEgoPlanes) &&
                  MP_VIEW_PREFIX(MpAvatarIds),
              "MpEgoLayer, MpViewHash, MpEgoPlanes and MpAvatarIds share their leading fields");
static_assert(MP_AVATARIDS_DRAW == VIEW_DRAW && MP_AVATARIDS_REGISTER == VIEW_REGISTER && MP_AVATARIDS_HOST == VIEW_HOST,
              "and MpAvatarIds the numbers of their ops");
static_assert(MP_EGO_DRAW == VIEW_DRAW && MP_VIEWHASH_DRAW == VIEW_DRAW && MP_EGOPLANES_DRAW == VIEW_DRAW &&
                  MP_EGO_REGISTER == VIEW_REGISTER && MP_VIEWHASH_REGISTER == VIEW_REGISTER &&
                  MP_EGOPLANES_REGISTER == VIEW_REGISTER && MP_EGO_HOST == VIEW_HOST &&
                  MP_VIEWHASH_HOST == VIEW_HOST && MP_EGOPLANES_HOST == VIEW_HOST,
              "and the numbers of their ops");
#undef MP_VIEW_PREFIX
#undef MP_VIEW_FIELD
static ViewRequest view_of(const void* request) {
  ViewRequest q;
  memcpy(&q, request, sizeof q);
  return q;
}

// The words that differ in the three requests' messages.
struct ViewWords {
  const char* who;       // "MpEgoLayer"
  const char* host_op;   // "MP_EGO_HOST"
  const char* thing;     // a registration: "the leaf" of N worlds
  const char* need;      // "needs" so many bytes
  const char* drawn;     // rows are "drawn"
  const char* draw;      // there is no state to "draw"
};

// The tables a request works with: the engine's, or the pack's by the host stage.
struct ViewTables {
  HostStage h;
  std::vector<int32_t> host_lut;   // (host form) the viewers' value tables
  const DevTables* t = nullptr;
  uint64_t fingerprint = 0;
  int32_t num_ids = 0;             // the length of a class table
};

// struct_size, op, engine, reserved words, pack: what is checked before the request is looked at.
static int view_prologue(const MpEngine* e, const ViewRequest& q, const ViewWords& w, size_t size, bool reserved_zero) {
  if (q.struct_size != size)
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", w.who, q.struct_size, size);
  if (q.op != VIEW_DRAW && q.op != VIEW_REGISTER && q.op != VIEW_HOST)
    return fail(MP_ERR_INVALID, "%s: unknown op %d", w.who, q.op);
  if (q.op == VIEW_HOST ? e != nullptr : e == nullptr) {
    if (e) return fail(MP_ERR_INVALID, "%s: %s takes no engine", w.who, w.host_op);
    return fail(MP_ERR_INVALID, "%s: NULL engine", w.who);
  }
  if (!reserved_zero) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", w.who);
  if (q.op == VIEW_HOST && (!q.pack || !q.cfg))
    return fail(MP_ERR_INVALID, "%s: %s needs the pack and its config (NULL pack or cfg)", w.who, w.host_op);
  return MP_OK;
}

static int view_tables(const MpEngine* e, const ViewRequest& q, ViewTables* v) {
  if (e) {
    v->t = &e->t;
    v->fingerprint = e->fingerprint;
    v->num_ids = e->num_layer_ids;
    return MP_OK;
  }
  if (int rc = host_stage(q.pack, q.pack_len, q.cfg, &v->h)) return rc;
  v->t = &v->h.d.t;
  v->fingerprint = state_fingerprint(v->h.pack, v->h.d.t);
  v->host_lut = layer_lut_rows(v->h.pack.data(), v->h.d.t);
  v->num_ids = view_hash::num_ids(v->host_lut.data(), v->t->P);
  return MP_OK;
}

// layer_mask as the kernels take it: 0 names every layer of the view.
static int view_layer_mask(const ViewWords& w, const ego_layer::Window& g, uint64_t asked, uint64_t* layer_mask) {
  if (g.L > 64) return fail(MP_ERR_UNSUPPORTED, "%s: %d layers; layer_mask names 64", w.who, g.L);
  const uint64_t every = g.L == 64 ? ~0ull : (1ull << g.L) - 1ull;
  if (asked & ~every)
    return fail(MP_ERR_INVALID, "%s: layer_mask %016llx has a bit that names no layer (the view has %d)", w.who,
                (unsigned long long)asked, g.L);
  *layer_mask = asked ? asked : every;
  return MP_OK;
}

static int view_record_lines(const ViewWords& w, const DevTables& t, const ego_layer::Window& g) {
  if ((t.grid_pad & 15) || (t.world_stride & 15) || (int64_t)g.L * g.HW > (int64_t)t.grid_pad)
    return fail(MP_ERR_UNSUPPORTED, "%s: a record of %d bytes with %d bytes of planes is not read in 16-byte lines",
                w.who, t.world_stride, t.grid_pad);
  return MP_OK;
}

// A registration's geometry: the ring, the bytes `dst` must hold (*need) with `world` bytes a world
// and slots `align`-byte aligned (1: anywhere), and `dst` itself.
static int view_register(MpEngine* e, const ViewRequest& q, const ViewWords& w, uint64_t world, unsigned align,
                         uint64_t* need) {
  const uint64_t block = (uint64_t)e->N * world;
  if (q.slots < 0) return fail(MP_ERR_INVALID, "%s: slots %d", w.who, q.slots);
  if (q.slots > 0 && q.slots != e->ring_slots)
    return fail(MP_ERR_INVALID, "%s: a ring of %d slots, the engine's ring has %d (mp_bind_output_ring; one "
                "position for all of them)", w.who, q.slots, e->ring_slots);
  if (q.slots > 0 && (q.slot_stride < block || (q.slot_stride & (align - 1)))) {
    char lie[48] = "";
    if (align > 1) snprintf(lie, sizeof lie, ", and slots lie %u-byte aligned", align);
    return fail(MP_ERR_INVALID, "%s: slot_stride %llu: a slot is %llu bytes%s", w.who,
                (unsigned long long)q.slot_stride, (unsigned long long)block, lie);
  }
  *need = q.slots > 0 ? (uint64_t)(q.slots - 1) * q.slot_stride + block : block;
  if (q.dst_bytes < *need)
    return fail(MP_ERR_INVALID, "%s: %s of %d worlds%s %s %llu bytes, dst has %llu", w.who, w.thing, e->N,
                q.slots > 0 ? " in every slot" : "", w.need, (unsigned long long)*need,
                (unsigned long long)q.dst_bytes);
  HIP_TRY(hipSetDevice(e->device));
  char name[48];
  snprintf(name, sizeof name, "%s (dst)", w.who);
  if (int rc = check_device_pointer(e, q.dst, name)) return rc;
  return check_bank(e, q.dst, *need, name);
}

static MpEngine::ViewRegistration registration_of(const ViewRequest& q) {
  MpEngine::ViewRegistration v;
  v.dst = q.dst;
  v.stride = q.slots > 0 ? q.slot_stride : 0;
  v.slots = q.slots;
  return v;
}

// What a draw or a host call reads and how much it writes: `view` bytes an element with players[],
// `world` without.
struct ViewSource {
  bool live;          // the engine's worlds
  int32_t src_rows;
  uint64_t need;      // bytes of dst
};
static int view_source(const MpEngine* e, const ViewRequest& q, const ViewWords& w, const ViewTables& v,
                       uint64_t view, uint64_t world, ViewSource* s) {
  s->live = q.op == VIEW_DRAW && !q.bank;
  if (q.op == VIEW_HOST && !q.bank) return fail(MP_ERR_INVALID, "%s: NULL bank", w.who);
  s->src_rows = s->live ? e->N : q.bank_rows;
  if (int rc = check_counts(w.who, q.count, s->src_rows)) return rc;
  if (int rc = check_row_list(w.who, q.rows, q.count, s->src_rows, w.drawn, false)) return rc;
  if (int rc = check_fingerprint(w.who, q.fingerprint, v.fingerprint, e ? "engine's" : "pack's")) return rc;
  if (int rc = check_dst_bytes(w.who, q.count, q.players ? view : world, q.dst_bytes, &s->need)) return rc;
  if (((uintptr_t)q.rows & 3) || ((uintptr_t)q.players & 3))
    return fail(MP_ERR_INVALID, "%s: rows %p and players %p must be 4-byte aligned", w.who, (const void*)q.rows,
                (const void*)q.players);
  return MP_OK;
}

// The fields every unit's Args has, of a draw or a host call.
extern "C++" {
template <class Args>
static void view_args(Args* a, const ego_layer::Window& g, const ViewRequest& q, const ViewTables& v,
                      const ViewSource& s) {
  a->g = g;
  a->rows = q.rows; a->players = q.players;
  a->src_rows = s.src_rows; a->count = q.count;
  a->stride = v.t->world_stride; a->grid_pad = v.t->grid_pad;
}
}

// The host twin met an index out of range at position `bad` (`row`: of rows[], else of players[]).
static int view_host_fault(const ViewRequest& q, const ViewWords& w, int bad, bool row) {
  return fail(MP_ERR_INVALID, "%s: %s[%d] = %d is %s; the elements from %d on were left as they were", w.who,
              row ? "rows" : "players", bad, row ? (q.rows ? q.rows[bad] : bad) : q.players[bad],
              row ? "not a row of the bank" : "not a player of this pack", bad);
}

// A draw's device memory: the state or the bank, rows, players, a class table, dst.
static int view_device_source(MpEngine* e, const ViewRequest& q, const ViewWords& w, const ViewSource& s,
                              const void* classes, uint64_t classes_bytes) {
  if (s.live && !e->has_state)
    return fail(MP_ERR_INVALID, "%s: the engine has never been reset; there is no state to %s", w.who, w.draw);
  const uint64_t count = (uint64_t)q.count, bank = (uint64_t)q.bank_rows * (uint64_t)e->t.world_stride;
  return check_extents(e, w.who, {{"bank", s.live ? nullptr : q.bank, bank, 16},   // (records are read in 16-byte lines)
                                  {"rows", q.rows, count * 4, 1},
                                  {"players", q.players, count * 4, 1},
                                  {"classes", classes, classes_bytes, 1},
                                  {"dst", q.dst, s.need, 1}});
}

static int ego_layer_request(MpEngine* e, const MpEgoLayer& r) {
  static const ViewWords w = {"MpEgoLayer", "MP_EGO_HOST", "the leaf", "needs", "drawn", "draw"};
  const char* const kWho = w.who;
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_EGO_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->ego = MpEngine::ViewRegistration{};
    return MP_OK;
  }
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  if ((uintptr_t)r.dst & 3) return fail(MP_ERR_INVALID, "%s: dst %p is not 4-byte aligned", kWho, r.dst);
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  const uint64_t view = (uint64_t)g.VH * (uint64_t)g.VW * (uint64_t)g.L * 4u, world = view * (uint64_t)g.P;
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  if (r.op == MP_EGO_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 4, &need)) return rc;
    const ego_layer::Plan p = ego_layer::plan_of(g, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes need %d B of LDS", kWho, p.lds);
    e->ego = registration_of(q);
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, view, world, &s)) return rc;
  ego_layer::Args a = {};
  view_args(&a, g, q, v, s);
  a.dst = (int32_t*)r.dst;
  if (r.op == MP_EGO_HOST) {
    a.src = (const uint8_t*)r.bank;
    a.lut = v.host_lut.data();
    uint32_t what = 0;
    const int bad = ego_layer::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultEgoRow) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, nullptr, 0)) return rc;
  const ego_layer::Plan p = ego_layer::plan_of(g, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes need %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.lut = e->d_layer_lut; a.fault = e->t.fault;
  ego_layer::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// (`out` is the caller's struct: num_ids is written back)
static int view_hash_request(MpEngine* e, MpViewHash* out) {
  static const ViewWords w = {"MpViewHash", "MP_VIEWHASH_HOST", "the hashes", "need", "hashed", "hash"};
  const char* const kWho = w.who;
  MpViewHash r;
  memcpy(&r, out, sizeof r);
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_VIEWHASH_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->vh = MpEngine::ViewRegistration{};
    out->num_ids = e->num_layer_ids;
    return MP_OK;
  }
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const int32_t num_ids = v.num_ids;
  if (num_ids < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the pack's view tables hold a negative id", kWho);
  out->num_ids = num_ids;
  if (r.op != MP_VIEWHASH_REGISTER && r.count == 0 && !r.dst) return MP_OK;   // the question alone
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  if ((uintptr_t)r.dst & 7) return fail(MP_ERR_INVALID, "%s: dst %p is not 8-byte aligned", kWho, r.dst);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  uint64_t layer_mask;
  if (int rc = view_layer_mask(w, g, r.layer_mask, &layer_mask)) return rc;
  if (r.classes ? r.classes_len != num_ids : r.classes_len != 0)
    return fail(MP_ERR_INVALID, "%s: classes_len %d: a class table has one entry per id, %d of them (0 without "
                "a table)", kWho, r.classes_len, num_ids);
  if ((uintptr_t)r.classes & 3)
    return fail(MP_ERR_INVALID, "%s: classes %p is not 4-byte aligned", kWho, (const void*)r.classes);
  const uint64_t world = (uint64_t)g.P * 8u;
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  const int num_classes = r.classes ? num_ids : 0;
  if (r.op == MP_VIEWHASH_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 8, &need)) return rc;
    if (r.classes)
      if (int rc = check_bank(e, r.classes, (uint64_t)num_classes * 4, "MpViewHash (classes)")) return rc;
    const view_hash::Plan p = view_hash::plan_of(g, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render planes need %d B of LDS", kWho, p.lds);
    e->vh = registration_of(q);
    e->vh.mask = layer_mask;
    e->vh.classes = r.classes;
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, 8u, world, &s)) return rc;
  view_hash::Args a = {};
  view_args(&a, g, q, v, s);
  a.dst = (uint64_t*)r.dst;
  a.layer_mask = layer_mask;
  a.classes = r.classes; a.num_classes = num_classes;
  if (r.op == MP_VIEWHASH_HOST) {
    a.src = (const uint8_t*)r.bank;
    a.lut = v.host_lut.data();
    uint32_t what = 0;
    const int bad = view_hash::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultViewHashRow) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, r.classes, (uint64_t)num_classes * 4)) return rc;
  const view_hash::Plan p = view_hash::plan_of(g, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render planes need %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.lut = e->d_layer_lut; a.fault = e->t.fault;
  view_hash::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// (`out` is the caller's struct: num_ids is written back)
static int ego_planes_request(MpEngine* e, MpEgoPlanes* out) {
  static const ViewWords w = {"MpEgoPlanes", "MP_EGOPLANES_HOST", "the planes", "need", "drawn", "draw"};
  const char* const kWho = w.who;
  MpEgoPlanes r;
  memcpy(&r, out, sizeof r);
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_EGOPLANES_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->ep = MpEngine::ViewRegistration{};
    out->num_ids = e->num_layer_ids;
    return MP_OK;
  }
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const int32_t num_ids = v.num_ids;
  if (num_ids < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the pack's view tables hold a negative id", kWho);
  out->num_ids = num_ids;
  if (r.op != MP_EGOPLANES_REGISTER && r.count == 0 && !r.dst) return MP_OK;   // the question alone
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  uint64_t layer_mask;
  if (int rc = view_layer_mask(w, g, r.layer_mask, &layer_mask)) return rc;
  if (!r.classes) return fail(MP_ERR_INVALID, "%s: NULL classes: the planes are those of a class table", kWho);
  if (r.classes_len != num_ids)
    return fail(MP_ERR_INVALID, "%s: classes_len %d: a class table has one entry per id, %d of them", kWho,
                r.classes_len, num_ids);
  if ((uintptr_t)r.classes & 3)
    return fail(MP_ERR_INVALID, "%s: classes %p is not 4-byte aligned", kWho, (const void*)r.classes);
  if (r.num_classes < 1 || r.num_classes > ego_planes::kMaxClasses)
    return fail(MP_ERR_INVALID, "%s: num_classes %d is outside [1, %d]", kWho, r.num_classes, ego_planes::kMaxClasses);
  if (r.facing != 0 && r.facing != 1) return fail(MP_ERR_INVALID, "%s: facing %d is neither 0 nor 1", kWho, r.facing);
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  const int num_planes = r.num_classes + (r.facing ? 4 : 0);
  const uint64_t view = (uint64_t)num_planes * (uint64_t)g.VH * (uint64_t)g.VW, world = (uint64_t)g.P * view;
  if (view * (uint64_t)g.VH * (uint64_t)g.VW >= (1ull << 32))   // (a byte's plane is found with one multiply)
    return fail(MP_ERR_UNSUPPORTED, "%s: a viewer's planes are %llu bytes", kWho, (unsigned long long)view);
  if (r.op == MP_EGOPLANES_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 1, &need)) return rc;
    if (int rc = check_bank(e, r.classes, (uint64_t)num_ids * 4, "MpEgoPlanes (classes)")) return rc;
    const ego_planes::Plan p = ego_planes::plan_of(g, num_planes, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render and bit planes need %d B of LDS",
                  kWho, p.lds);
    e->ep = registration_of(q);
    e->ep.mask = layer_mask;
    e->ep.classes = r.classes;
    e->ep.num_classes = r.num_classes;
    e->ep.facing = r.facing;
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, view, world, &s)) return rc;
  ego_planes::Args a = {};
  view_args(&a, g, q, v, s);
  a.dst = (uint8_t*)r.dst;
  a.layer_mask = layer_mask;
  a.classes = r.classes; a.num_ids = num_ids;
  a.num_classes = r.num_classes; a.facing = r.facing;
  if (r.op == MP_EGOPLANES_HOST) {
    for (int32_t id = 0; id < num_ids; ++id)
      if (r.classes[id] < -1 || r.classes[id] >= r.num_classes)
        return fail(MP_ERR_INVALID, "%s: classes[%d] = %d is outside [-1, num_classes = %d)", kWho, id,
                    r.classes[id], r.num_classes);
    a.src = (const uint8_t*)r.bank;
    a.lut = v.host_lut.data();
    uint32_t what = 0;
    const int bad = ego_planes::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultEgoPlanesRow) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, r.classes, (uint64_t)num_ids * 4)) return rc;
  const ego_planes::Plan p = ego_planes::plan_of(g, num_planes, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render and bit planes need %d B of LDS",
                kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.lut = e->d_layer_lut; a.fault = e->t.fault;
  ego_planes::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// Two destinations of one shape, either may be absent: the front's checks run once for each that
// is there, on a copy of the request's beginning that names it as `dst`.
static int avatar_ids_request(MpEngine* e, const MpAvatarIds& r) {
  static const ViewWords w = {"MpAvatarIds", "MP_AVATARIDS_HOST", "a leaf", "needs", "drawn", "draw"};
  const char* const kWho = w.who;
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_AVATARIDS_REGISTER && !r.dst && !r.dst_zap) {   // clears the registration: the engine's launches are what they were
    e->av = e->avz = MpEngine::ViewRegistration{};
    return MP_OK;
  }
  if (!r.dst && !r.dst_zap) return fail(MP_ERR_INVALID, "%s: NULL dst and NULL dst_zap", kWho);
  if (((uintptr_t)r.dst | (uintptr_t)r.dst_zap) & 3)
    return fail(MP_ERR_INVALID, "%s: dst %p and dst_zap %p must be 4-byte aligned", kWho, r.dst, r.dst_zap);
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const SubstrateTables& sub = e ? e->sub : v.h.d.sub;
  const ZapRules* zap = zap_rules_of(sub);
  if (r.dst_zap && !zap)
    return fail(MP_ERR_INVALID, "%s: %s has no Zapper: there is no AVATAR_IDS_IN_RANGE_TO_ZAP on this level "
                "(AVATAR_IDS_IN_VIEW works on every level)", kWho, family_name(sub));
  if (r.dst_zap && (zap->shape.n < 1 || zap->shape.n > 16))
    return fail(MP_ERR_UNSUPPORTED, "%s: a zap footprint of %d cells", kWho, zap->shape.n);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  const uint64_t view = (uint64_t)g.P * 4u, world = view * (uint64_t)g.P;
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  if (v.t->avatar_layer < 0 || v.t->avatar_layer >= g.L)
    return fail(MP_ERR_UNSUPPORTED, "%s: avatar_layer %d is no render plane", kWho, v.t->avatar_layer);
  ViewRequest qv = q, qz = q;   // the request as IN_VIEW's alone, as IN_RANGE's alone
  qz.dst = r.dst_zap; qz.dst_bytes = r.dst_zap_bytes;
  avatar_ids::Args a = {};
  avatar_ids_tables(&a, *v.t, r.dst_zap ? zap : nullptr,
                    e ? (const uint32_t*)e->t.step_blob : (const uint32_t*)v.h.d.step_blob.data());
  if (r.op == MP_AVATARIDS_REGISTER) {
    uint64_t need;
    if (r.dst) if (int rc = view_register(e, qv, w, world, 4, &need)) return rc;
    if (r.dst_zap) if (int rc = view_register(e, qz, w, world, 4, &need)) return rc;
    const avatar_ids::Plan p = avatar_ids::plan_of(g, a.plane_at, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: one wave's avatar plane needs %d B of LDS", kWho, p.lds);
    e->av = r.dst ? registration_of(qv) : MpEngine::ViewRegistration{};
    e->avz = r.dst_zap ? registration_of(qz) : MpEngine::ViewRegistration{};
    return MP_OK;
  }
  ViewSource s, sz;
  if (r.dst) if (int rc = view_source(e, qv, w, v, view, world, &s)) return rc;
  if (r.dst_zap) if (int rc = view_source(e, qz, w, v, view, world, &sz)) return rc;
  if (!r.dst) s = sz;
  view_args(&a, g, q, v, s);
  a.dst = (int32_t*)r.dst;
  a.dst_zap = (int32_t*)r.dst_zap;
  if (r.op == MP_AVATARIDS_HOST) {
    a.src = (const uint8_t*)r.bank;
    uint32_t what = 0;
    const int bad = avatar_ids::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultAvatarIdsRow) : MP_OK;
  }
  if (r.dst) if (int rc = view_device_source(e, qv, w, s, nullptr, 0)) return rc;
  if (r.dst_zap) if (int rc = view_device_source(e, qz, w, s, nullptr, 0)) return rc;
  const avatar_ids::Plan p = avatar_ids::plan_of(g, a.plane_at, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's avatar plane needs %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.fault = e->t.fault;
  avatar_ids::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// mp_snapshot / mp_restore tell their requests apart by size (a snapshot is >= 448 bytes): the 18.
constexpr size_t kRequestSizes[] = {
    sizeof(MpKernelVariant), sizeof(MpWorldStates), sizeof(MpStatesObserve), sizeof(MpStepMany),
    sizeof(MpStepTrajectory), sizeof(MpStateLayout), sizeof(MpStatesCheck), sizeof(MpStatesHash),
    sizeof(MpEpisodeStarts), sizeof(MpStatesView), sizeof(MpStepActive), sizeof(MpStepUntil),
    sizeof(MpStepListed), sizeof(MpEpisodeStats), sizeof(MpEgoLayer), sizeof(MpViewHash), sizeof(MpEgoPlanes),
    sizeof(MpAvatarIds)};
constexpr bool request_sizes_tell_apart() {
  for (size_t i = 0; i < sizeof kRequestSizes / sizeof kRequestSizes[0]; ++i) {
    if (kRequestSizes[i] >= 448) return false;
    for (size_t j = 0; j < i; ++j)
      if (kRequestSizes[i] == kRequestSizes[j]) return false;
  }
  return true;
}
static_assert(request_sizes_tell_apart(), "two requests of one size, or one the size of a snapshot");
static_assert(sizeof(MpAvatarIds) == 144 && sizeof(MpEgoPlanes) == 160 && sizeof(MpViewHash) == 152 && sizeof(MpEgoLayer) == 128 &&
                  sizeof(MpEpisodeStats) == 224 && sizeof(MpEventColumn) == 32 && sizeof(MpStatsBank) == 32 &&
                  sizeof(MpStatesObserve) == 64 && sizeof(MpStateLayout) == 120 && sizeof(MpStatesCheck) == 88 &&
                  sizeof(MpStateField) == 32 && sizeof(MpStatesHash) == 104 && sizeof(MpEpisodeStarts) == 72 &&
                  sizeof(MpStatesView) == 80 && sizeof(MpStepActive) == 96 && sizeof(MpStepUntil) == 136 &&
                  sizeof(MpStepListed) == 176,
              "the layouts include/mp_engine.h documents");
static_assert(offsetof(MpStepUntil, active_step_bytes) == offsetof(MpStepActive, active_step_bytes) &&
                  offsetof(MpStepUntil, stop) == offsetof(MpStepActive, reserved),
              "MpStepUntil's leading fields are MpStepActive's");
static_assert(offsetof(MpStepListed, gamma) == offsetof(MpStepUntil, gamma) &&
                  offsetof(MpStepListed, reserved) == offsetof(MpStepUntil, reserved) &&
                  offsetof(MpStepListed, worlds) == sizeof(MpStepUntil),
              "MpStepListed's leading fields are MpStepUntil's");
// An MpKernelVariant request (carried by mp_snapshot; `e` may be NULL: the host-only question).
static int kernel_variant(const MpEngine* e, MpKernelVariant* r) {
  if (r->struct_size != sizeof(MpKernelVariant))
    return fail(MP_ERR_INVALID, "MpKernelVariant: struct_size %u, expected %zu", r->struct_size, sizeof(MpKernelVariant));
  if (e) { r->variant = e->sub.stock; return MP_OK; }
  char* fields = r->fields;
  const uint64_t fields_cap = r->fields_cap;
  HostStage h;
  if (int rc = host_stage(r->pack, r->pack_len, r->cfg, &h)) return rc;
  if (fields) {
    if (h.d.sub.substrate != MPK_SUBSTRATE_CLEAN_UP)
      return fail(MP_ERR_UNSUPPORTED, "MpKernelVariant: no stock kernels for this level");
    std::string text;
#define MP_FIELD_T(f) text += "t " #f " "; literal(&text, h.d.t.f); text += "\n";
#define MP_FIELD_C(f) text += "c " #f " "; literal(&text, h.d.sub.cu.f); text += "\n";
    MP_STOCK_DEV_FIELDS(MP_FIELD_T)
    MP_STOCK_CLEAN_UP_FIELDS(MP_FIELD_C)
#undef MP_FIELD_T
#undef MP_FIELD_C
    text += "hash ";
    literal(&text, pack_hash(h.pack));
    text += "\n";
    if (text.size() + 1 > fields_cap)
      return fail(MP_ERR_INVALID, "MpKernelVariant: fields needs %zu bytes", text.size() + 1);
    memcpy(fields, text.c_str(), text.size() + 1);
  }
  r->variant = select_kernels(h.pack, h.d, h.cfg.dev);
  return MP_OK;
}

int mp_snapshot(MpEngine* e, void* buf, uint64_t bytes) {
  if (buf && bytes == sizeof(MpKernelVariant)) return kernel_variant(e, (MpKernelVariant*)buf);
  if (e && buf && bytes == sizeof(MpWorldStates)) return world_states(e, (MpWorldStates*)buf, false);
  if (buf && bytes == sizeof(MpStatesObserve)) {
    MpStatesObserve r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return states_observe(e, r);
  }
  if (buf && bytes == sizeof(MpStatesView)) {
    MpStatesView r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return states_view(e, r);
  }
  if (buf && bytes == sizeof(MpEgoLayer)) {
    MpEgoLayer r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return ego_layer_request(e, r);
  }
  if (buf && bytes == sizeof(MpViewHash)) return view_hash_request(e, (MpViewHash*)buf);   // (num_ids is written back)
  if (buf && bytes == sizeof(MpEgoPlanes)) return ego_planes_request(e, (MpEgoPlanes*)buf);   // (likewise)
  if (buf && bytes == sizeof(MpAvatarIds)) {
    MpAvatarIds r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return avatar_ids_request(e, r);
  }
  if (buf && bytes == sizeof(MpStateLayout)) return state_layout(e, (MpStateLayout*)buf);
  if (buf && bytes == sizeof(MpStatesCheck)) {
    MpStatesCheck r;   // (read only: the verdicts go to r.out)
    memcpy(&r, buf, sizeof r);
    return states_check(e, r);
  }
  if (buf && bytes == sizeof(MpStatesHash)) {
    MpStatesHash r;   // (read only: the hashes go to r.out)
    memcpy(&r, buf, sizeof r);
    return states_hash(e, r);
  }
  if (!e || !buf || bytes != mp_snapshot_bytes(e))
    return fail(MP_ERR_INVALID, "mp_snapshot: bad buffer");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = sync_and_check(e, "mp_snapshot")) return rc;
  HIP_TRY(hipMemcpy(buf, e->d_state, bytes, hipMemcpyDeviceToHost));
  return MP_OK;
}

int mp_restore(MpEngine* e, const void* buf, uint64_t bytes) {
  if (e && buf && bytes == sizeof(MpWorldStates)) {
    MpWorldStates r;   // (read only: a load writes nothing back)
    memcpy(&r, buf, sizeof r);
    return world_states(e, &r, true);
  }
  if (buf && bytes == sizeof(MpStepMany)) {
    MpStepMany r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return many_request(e, r);
  }
  if (buf && bytes == sizeof(MpStepTrajectory)) {
    MpStepTrajectory r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return trajectory_request(e, r);
  }
  if (buf && bytes == sizeof(MpEpisodeStarts)) {
    MpEpisodeStarts r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return episode_starts(e, r);
  }
  if (buf && bytes == sizeof(MpStepActive)) {
    MpStepActive r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return active_request(e, r);
  }
  if (buf && bytes == sizeof(MpStepUntil)) {
    MpStepUntil r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return until_request(e, r);
  }
  if (buf && bytes == sizeof(MpStepListed)) {
    MpStepListed r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return listed_request(e, r);
  }
  if (buf && bytes == sizeof(MpEpisodeStats)) {
    MpEpisodeStats r;   // (read only: nothing is written back)
    memcpy(&r, buf, sizeof r);
    return episode_stats_request(e, r);
  }
  if (!e || !buf || bytes != mp_snapshot_bytes(e))
    return fail(MP_ERR_INVALID, "mp_restore: bad buffer");
  HIP_TRY(hipSetDevice(e->device));
  e->touched = true;
  e->has_state = true;
  if (int rc = sync_and_check(e, "mp_restore")) return rc;
  HIP_TRY(hipMemcpy(e->d_state, buf, bytes, hipMemcpyHostToDevice));
  return MP_OK;
}

static int save_worlds(MpEngine* e, const int32_t* worlds, int32_t count, void* dst, uint64_t dst_bytes) {
  if (!e || !dst || count <= 0)
    return fail(MP_ERR_INVALID, "MP_STATES_SAVE: NULL engine or buffer, or no rows");
  if (!worlds && count != e->N)
    return fail(MP_ERR_INVALID, "MP_STATES_SAVE: without a world list every world is saved (count %d, "
                "the engine has %d)", count, e->N);
  const uint64_t stride = (uint64_t)e->t.world_stride, bytes = (uint64_t)count * stride;
  if (dst_bytes < bytes)
    return fail(MP_ERR_INVALID, "MP_STATES_SAVE: %d rows of %llu bytes need %llu bytes, the buffer has %llu",
                count, (unsigned long long)stride, (unsigned long long)bytes, (unsigned long long)dst_bytes);
  if (!e->has_state)
    return fail(MP_ERR_INVALID, "MP_STATES_SAVE: the engine has never been reset; there is no state to save");
  if (int rc = check_extents(e, "MP_STATES_SAVE", {{nullptr, dst, bytes, 1},
                                                   {"world list", worlds, (uint64_t)count * 4, 1}}))
    return rc;
  hipLaunchKernelGGL(k_save_worlds, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, e->stream, e->t,
                     (const uint8_t*)e->d_state, e->N, worlds, (int)count, (uint8_t*)dst);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

static int load_worlds(MpEngine* e, const void* bank, int32_t bank_rows, const int32_t* src,
                       uint64_t fingerprint) {
  if (!e || !bank || !src || bank_rows <= 0)
    return fail(MP_ERR_INVALID, "MP_STATES_LOAD: NULL engine, bank or src, or an empty bank");
  if (int rc = check_fingerprint("MP_STATES_LOAD", fingerprint, e->fingerprint, "engine's")) return rc;
  const uint64_t bytes = (uint64_t)bank_rows * (uint64_t)e->t.world_stride;
  if (int rc = check_extents(e, "MP_STATES_LOAD", {{nullptr, bank, bytes, 1}, {"src", src, (uint64_t)e->N * 4, 1}}))
    return rc;
  e->touched = true;
  e->has_state = true;
  return submit(e, STEP_MODE_LOAD, nullptr, nullptr, (const uint8_t*)bank, src, bank_rows);
}

int mp_counters(MpEngine* e, uint64_t out[MP_CTR_COUNT]) {
  if (!e || !out) return fail(MP_ERR_INVALID, "mp_counters: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemsetAsync(e->d_ctr, 0, MP_CTR_COUNT * 8, e->stream));
  hipLaunchKernelGGL(k_sum_counters, dim3(256), dim3(256), 0, e->stream, e->d_state,
                     e->t.world_stride, e->t.grid_pad, e->N, e->d_ctr);
  HIP_TRY(hipGetLastError());
  unsigned long long host[MP_CTR_COUNT];
  HIP_TRY(hipMemcpyAsync(host, e->d_ctr, sizeof(host), hipMemcpyDeviceToHost, e->stream));
  if (int rc = sync_and_check(e, "mp_counters")) return rc;
  for (int k = 0; k < MP_CTR_COUNT; ++k) out[k] = host[k];
  return MP_OK;
}

#if defined(MP_FRAME_TIMELINE) || defined(MP_FRAME_ENDS)
// developer build: the frame kernel's event log (frame.hip: FRAME_STAGE) / its per-workgroup stamps
__attribute__((visibility("default")))   // (not in the header: these builds only)
int mp_debug_timeline(MpEngine* e, uint32_t* out, int nwords) {
  if (!e || !out || nwords > kFaultWords - 64) return MP_ERR_INVALID;
#if defined(MP_FRAME_ENDS)
  if (nwords > 2 * 1024) return MP_ERR_INVALID;
  (void)hipStreamSynchronize(e->stream);
  (void)hipMemcpy(out, e->d_claim + 2, (size_t)nwords * 4, hipMemcpyDeviceToHost);
  (void)hipMemset(e->d_claim + 2, 0, 2 * 1024 * 4);
  return MP_OK;
#endif
  for (int i = 0; i < nwords; ++i) out[i] = ((const volatile uint32_t*)e->h_fault)[64 + i];
  memset((void*)(e->h_fault + 64), 0, (size_t)(kFaultWords - 64) * 4);
  return MP_OK;
}
#endif

// ---- memory for a bound view (include/mp_engine.h: mp_alloc_output)
}  // extern "C"
namespace {
struct MappedView { size_t bytes; size_t chunk; std::vector<hipMemGenericAllocationHandle_t> handles; };
std::map<void*, MappedView> g_mapped;   // views made of mapped chunks (plain ones are not listed)
std::mutex g_mapped_lock;
// Address space retired by released mapped views (free_output keeps their ranges reserved), and
// the bound beyond which nothing more is mapped: a process that places views for ever (a sweep
// that creates engine after engine) gets a clear error instead of an address space that silently
// fills up.  16 TiB: ~25,000 placed clean_up views.
int64_t g_retired_va = 0;
int64_t g_retired_va_limit = (int64_t)16 << 40;

void retired_va(int64_t* bytes, int64_t* limit) {
  std::lock_guard<std::mutex> g(g_mapped_lock);
  if (bytes) *bytes = g_retired_va;
  if (limit) *limit = g_retired_va_limit;
}

// is `p` inside a view this library mapped?  (hipPointerGetAttributes does not know them)
bool in_mapped_view(const void* p) {
  std::lock_guard<std::mutex> g(g_mapped_lock);
  auto it = g_mapped.upper_bound(const_cast<void*>(p));
  if (it == g_mapped.begin()) return false;
  --it;
  return (const char*)p < (const char*)it->first + it->second.bytes;
}

// undoes a partly built mapping (best effort) and reports `rc`
int mapped_failed(void* base, MappedView& v, size_t mapped, hipError_t rc, const char* what) {
  if (base) {
    if (mapped) (void)hipMemUnmap(base, mapped * v.chunk);
    (void)hipMemAddressFree(base, v.bytes);
  }
  for (auto h : v.handles) (void)hipMemRelease(h);
  (void)hipGetLastError();
  return fail(MP_ERR_HIP, "mp_alloc_output: %s failed: %s", what, hipGetErrorString(rc));
}
}  // namespace
extern "C" {

// One virtual range mapped onto separately created physical chunks: the view the frame launch
// writes evenly (a view whose physical pages lie next to each other — a contiguous extent,
// large pieces of a plain allocation — is written 25 - 45 % slower: profiles/r05_alloc_method.md;
// scattering the chunks FURTHER, pools and shuffles, added nothing there and is gone).
static int alloc_mapped(int device, uint64_t bytes, uint64_t chunk_bytes, void** out) {
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, chunk_bytes >= (2u << 20)
                                                           ? hipMemAllocationGranularityRecommended
                                                           : hipMemAllocationGranularityMinimum));
  if (gran == 0) gran = 4096;
  MappedView v;
  v.chunk = ((size_t)chunk_bytes + gran - 1) / gran * gran;
  const size_t n = ((size_t)bytes + v.chunk - 1) / v.chunk;
  if (n > (1u << 20)) return fail(MP_ERR_INVALID, "mp_alloc_output: %zu chunks", n);
  v.bytes = n * v.chunk;
  {
    int64_t retired = 0, limit = 0;
    retired_va(&retired, &limit);
    if (retired + (int64_t)v.bytes > limit)
      return fail(MP_ERR_HIP, "mp_alloc_output: this process has retired %lld bytes of address space with "
                  "released mapped views (their ranges are never reused: stale translations); mapping %zu "
                  "more would pass the bound of %lld (mp_set_retired_va_limit) — reuse views instead of "
                  "placing new ones", (long long)retired, v.bytes, (long long)limit);
  }
  void* base = nullptr;
  hipError_t rc = hipMemAddressReserve(&base, v.bytes, v.chunk < (2u << 20) ? (2u << 20) : v.chunk, nullptr, 0);
  if (rc != hipSuccess) return mapped_failed(nullptr, v, 0, rc, "hipMemAddressReserve");
  v.handles.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    hipMemGenericAllocationHandle_t h;
    rc = hipMemCreate(&h, v.chunk, &prop, 0);
    if (rc != hipSuccess) return mapped_failed(base, v, 0, rc, "hipMemCreate");
    v.handles.push_back(h);
  }
  for (size_t i = 0; i < n; ++i) {
    rc = hipMemMap((char*)base + i * v.chunk, v.chunk, 0, v.handles[i], 0);
    if (rc != hipSuccess) return mapped_failed(base, v, i, rc, "hipMemMap");
  }
  hipMemAccessDesc acc = {};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  rc = hipMemSetAccess(base, v.bytes, &acc, 1);
  if (rc != hipSuccess) return mapped_failed(base, v, n, rc, "hipMemSetAccess");
  {
    std::lock_guard<std::mutex> g(g_mapped_lock);
    g_mapped[base] = v;
  }
  *out = base;
  return MP_OK;
}

int mp_alloc_output(int device, uint64_t bytes, uint64_t chunk_bytes, void** out) {
  if (!out || bytes == 0) return fail(MP_ERR_INVALID, "mp_alloc_output: bad argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  if (chunk_bytes == 0) {
    const hipError_t rc = hipMalloc(out, (size_t)bytes);
    if (rc != hipSuccess) {
      (void)hipGetLastError();
      *out = nullptr;
      return fail(MP_ERR_HIP, "mp_alloc_output: hipMalloc of %llu bytes failed: %s",
                  (unsigned long long)bytes, hipGetErrorString(rc));
    }
    return MP_OK;
  }
  return alloc_mapped(device, bytes, chunk_bytes, out);
}

// The physical chunks go back to the driver; the VIRTUAL range stays reserved and is
// never handed out again (`keep_va`, always true in this library).  Measured on this
// stack (ROCm 7.2, gfx950): a range released with hipMemAddressFree is reused by the next
// hipMemAddressReserve, and kernels then write through translations of the OLD mapping —
// a second placed view came back with 267 - 1030 of 1030 worlds stale, no error anywhere
// (tools/gpu_r04_dbg_place.py).  Address space is not scarce (a placement retires
// ~12 x the view's size of it); correctness is.
static int free_output(int device, void* ptr, bool keep_va) {
  if (!ptr) return MP_OK;
  HIP_TRY(hipSetDevice(device));
  MappedView v;
  bool mapped = false;
  {
    std::lock_guard<std::mutex> g(g_mapped_lock);
    auto it = g_mapped.find(ptr);
    if (it != g_mapped.end()) { v = it->second; g_mapped.erase(it); mapped = true; }
  }
  if (!mapped) {
    HIP_TRY(hipFree(ptr));   // (waits for the device's work on the buffer)
    return MP_OK;
  }
  // best effort: whatever fails, the rest is still released
  hipError_t first = hipDeviceSynchronize(), rc = hipMemUnmap(ptr, v.bytes);
  if (first == hipSuccess) first = rc;
  for (auto h : v.handles) {
    rc = hipMemRelease(h);
    if (first == hipSuccess) first = rc;
  }
  if (!keep_va) {
    rc = hipMemAddressFree(ptr, v.bytes);
    if (first == hipSuccess) first = rc;
  } else {
    std::lock_guard<std::mutex> g(g_mapped_lock);
    g_retired_va += (int64_t)v.bytes;
  }
  if (first != hipSuccess) {
    (void)hipGetLastError();
    return fail(MP_ERR_HIP, "mp_free_output: %s", hipGetErrorString(first));
  }
  return MP_OK;
}

int mp_free_output(int device, void* ptr) { return free_output(device, ptr, true); }

// torch.cuda.memory.CUDAPluggableAllocator entry points (meltingpot_amd/memory.py): tensors a
// caller allocates inside `memory.mapped_allocations()` — a learner's own rollout buffers —
// come from scattered 2 MB chunks like the engine's own views (32 MB and up; below that an
// ordinary hipMalloc).  NULL on failure, as the allocator interface expects.
void* mp_torch_alloc(ssize_t size, int device, void* stream) {
  (void)stream;
  void* p = nullptr;
  if (size <= 0) return nullptr;
  if (mp_alloc_output(device, (uint64_t)size, size >= (ssize_t)(32 << 20) ? (2u << 20) : 0, &p) != MP_OK)
    return nullptr;
  return p;
}

void mp_torch_free(void* ptr, ssize_t size, int device, void* stream) {
  (void)size; (void)stream;
  (void)free_output(device, ptr, true);
}

int mp_set_retired_va_limit(int64_t bytes) {
  if (bytes < 0) return fail(MP_ERR_INVALID, "mp_set_retired_va_limit: %lld", (long long)bytes);
  std::lock_guard<std::mutex> g(g_mapped_lock);
  g_retired_va_limit = bytes;
  return MP_OK;
}

namespace {

// The launches mp_tune times, back to back (one pair of events around `reps` of them,
// two more in front: the device stays busy, the clocks where a training loop has them):
// dry — a reset whose mask names no world: nothing is stepped, no record written back,
// every bound view drawn exactly as a step draws it — or, on an engine nothing has been
// done with yet, REAL steps (uniformly random actions) behind a device-side copy of the state.
struct Events {   // RAII: a pair of timing events
  hipEvent_t a = nullptr, b = nullptr;
  int create() {
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    return MP_OK;
  }
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

int timed_launches_us(MpEngine* e, bool real, int reps, double* us) {
  // (a probe never starts a world from the registered bank: it times the engine's own launches)
  struct HoldStarts {
    MpEngine* e; bool was;
    explicit HoldStarts(MpEngine* eng) : e(eng), was(eng->starts_hold) { e->starts_hold = true; }
    ~HoldStarts() { e->starts_hold = was; }
  } hold(e);
  Events ev;
  if (int rc = ev.create()) return rc;
  int rc = MP_OK;
  auto one = [&]() {
    return real ? submit(e, STEP_MODE_STEP, e->d_actions, nullptr)
                : submit(e, STEP_MODE_RESET, nullptr, e->d_mask);
  };
  for (int r = 0; r < 2 && rc == MP_OK; ++r) rc = one();
  HIP_TRY(hipEventRecord(ev.a, e->stream));
  for (int r = 0; r < reps && rc == MP_OK; ++r) rc = one();
  HIP_TRY(hipEventRecord(ev.b, e->stream));
  if (hipEventSynchronize(ev.b) != hipSuccess) {
    (void)hipGetLastError();
    if (rc == MP_OK) rc = fail(MP_ERR_HIP, "mp_tune: a probe launch failed");
  }
  float ms = 0;
  if (rc == MP_OK) HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
  *us = (double)ms * 1e3 / (reps > 0 ? reps : 1);
  return rc;
}

// What a probe that really steps must put back, whatever happens in between (RAII: every
// exit path of mp_tune — and of mp_place_output, which calls it — leaves the engine the engine
// it was): the records, the counters and the engine's own scalar outputs are copied aside and
// copied back; the CALLER's scalar outputs are unbound for the duration (the probe's steps
// write the engine's own buffers instead), so that no memory of the caller's but the pixel
// views being timed is touched.
struct ProbeState {
  MpEngine* e;
  uint8_t* saved = nullptr;
  bool copied = false;
  bool held = false, was_held = false;
  void* rebind[MP_OBS_KINDS] = {};
  size_t parts[4] = {};
  explicit ProbeState(MpEngine* eng) : e(eng) {
    parts[0] = (size_t)e->N * e->t.world_stride;
    parts[1] = MP_CTR_COUNT * 8;
    parts[2] = e->scalars_bytes;
    parts[3] = e->d_debug ? e->debug_bytes : 0;
  }
  uint8_t* part(int k) const {
    return k == 0 ? e->d_state : k == 1 ? (uint8_t*)e->d_ctr : k == 2 ? e->d_scalars : e->d_debug;
  }
  // (and a bound "N.LAYER" is not written by the probe's launches: dry ones would put the records'
  // LAYER into whichever ring slot is being timed, stepping ones the probe's steps')
  bool was_stats = false;   // (the probe's launches are not folded into registered episode statistics)
  void hold_ring() {
    was_held = e->ring_hold; e->ring_hold = true; e->layer_hold = true; held = true;
    was_stats = e->stats_hold; e->stats_hold = true;
  }
  // MP_OK with copied == false: no room for the copy — the probe runs dry
  int save() {
    const size_t total = parts[0] + parts[1] + parts[2] + parts[3];
    if (hipMalloc((void**)&saved, total) != hipSuccess) {
      (void)hipGetLastError();
      saved = nullptr;
      return MP_OK;
    }
    size_t off = 0;
    for (int k = 0; k < 4; ++k) {
      if (parts[k]) {
        const hipError_t rc = hipMemcpyAsync(saved + off, part(k), parts[k], hipMemcpyDeviceToDevice, e->stream);
        if (rc != hipSuccess) {
          (void)hipGetLastError();
          (void)hipStreamSynchronize(e->stream);
          (void)hipFree(saved);
          saved = nullptr;
          return fail(MP_ERR_HIP, "mp_tune: saving the engine's state failed: %s", hipGetErrorString(rc));
        }
      }
      off += parts[k];
    }
    copied = true;
    for (int k = 0; k < MP_OBS_KINDS; ++k)
      if (!MpEngine::is_pixel_kind(k)) { rebind[k] = e->bound[k]; e->bound[k] = nullptr; }
    return MP_OK;
  }
  int restore() {
    int rc = MP_OK;
    if (copied) {
      size_t off = 0;
      hipError_t first = hipSuccess;
      for (int k = 0; k < 4; ++k) {
        if (parts[k]) {
          const hipError_t r = hipMemcpyAsync(part(k), saved + off, parts[k], hipMemcpyDeviceToDevice, e->stream);
          if (first == hipSuccess) first = r;
        }
        off += parts[k];
      }
      const hipError_t r = hipStreamSynchronize(e->stream);
      if (first == hipSuccess) first = r;
      for (int k = 0; k < MP_OBS_KINDS; ++k)
        if (!MpEngine::is_pixel_kind(k)) e->bound[k] = rebind[k];
      copied = false;
      if (first != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(MP_ERR_HIP, "mp_tune: putting the engine's state back failed: %s", hipGetErrorString(first));
      }
    }
    if (saved) { (void)hipFree(saved); saved = nullptr; }
    if (held) {
      e->ring_hold = was_held;
      e->layer_hold = false;
      e->stats_hold = was_stats;
      held = false;
      if (e->ring_slots > 0 && !e->ring_hold) {   // ring kinds point at the slot written last again
        const uint64_t last = e->ring_cursor ? (e->ring_cursor - 1) % (uint64_t)e->ring_slots : 0;
        e->point_ring((int)last);
      }
    }
    return rc;
  }
  ~ProbeState() { (void)restore(); }
};

}  // namespace

static int tune_impl(MpEngine* e, double* us_per_launch, bool* stepped, bool quick = false);

int mp_tune(MpEngine* e, double* us_per_launch) { return tune_impl(e, us_per_launch, nullptr); }

// (`stepped`: whether the probe really stepped — false when the engine is in use or there
// was no room for the copy of its state; `quick`: what mp_place_output asks of every candidate
// buffer — the stock plan and the team order, one group of launches each, no stages: buffers
// differ by 10 - 25 %, the winner gets the whole search afterwards)
static int tune_impl(MpEngine* e, double* us_per_launch, bool* stepped, bool quick) {
  if (!e) return fail(MP_ERR_INVALID, "mp_tune: NULL engine");
  HIP_TRY(hipSetDevice(e->device));
  if (stepped) *stepped = false;
  if (us_per_launch) *us_per_launch = 0.0;
  // a ring: every slot is its own buffer (its own physical pages), the plan follows each
  const int slots = e->ring_slots > 0 && e->ring_has_pixels() ? e->ring_slots : 1;
  uint8_t* rgb = e->agent_view();
  uint8_t* wrgb = (uint8_t*)e->bound[MP_OBS_WORLD_RGB];
  if ((!rgb && !wrgb) || !e->fuse(rgb == nullptr)) return MP_OK;
  const int views = rgb && wrgb ? 2 : wrgb ? 1 : 0;
  const int pk = rgb ? e->pool_k() : 1;   // (a pooled per-agent view has plans of its own)
  // (everything in flight finishes first: a tune between two steps sees whole records)
  if (int rc = sync_and_check(e, "mp_tune")) return rc;
  FramePlan& plan = e->frame_plan(1, views, pk);
  const FramePlan before = plan;
  const FramePlan stock = plan_frame(e->t, e->sub, e->N, true, views, e->num_cus, nullptr, pk, e->world_pool);
  // the candidates: the stock plan; the same ring cut into single worlds; that with
  // half of every workgroup's share pooled; the stock plan with sc1 stores.  (Same
  // number of LDS record slots: the composite cache was sized for the stock plan.)
  std::vector<FramePlan> cand;
  cand.push_back(e->has_dev ? plan : stock);
  if (!e->has_dev) {
    const int lds_slots = stock.NB * stock.B;
    for (int pct : {100, 50}) {
      if (quick) break;
      MpDevOptions d = {};
      d.struct_size = sizeof d;
      d.max_composites = -1;
      d.batch_worlds = 1;
      d.ring_batches = lds_slots;
      d.static_pct = pct;
      const FramePlan p = plan_frame(e->t, e->sub, e->N, true, views, e->num_cus, &d, pk, e->world_pool);
      if (frame_lds_bytes(e->t, p, pk, e->world_pool, views) <= frame_lds_bytes(e->t, stock, pk, e->world_pool, views) &&
          (p.B != stock.B || p.NB != stock.NB || p.pool != stock.pool))
        cand.push_back(p);
    }
    // ... the single-world ring dealt to XCD teams (round 6: each XCD writes one compact front; since
    // the launch is its own store loop that is 118 -> 109 us for WORLD.RGB on a view the memory side
    // serves unevenly, 94 -> 89 on one it serves evenly, and with a pause on top 100: profiles/r06_resolve.md)
    {
      MpDevOptions d = {};
      d.struct_size = sizeof d;
      d.max_composites = -1;
      d.batch_worlds = 1;
      d.ring_batches = lds_slots;
      d.team = 1;
      const FramePlan p = plan_frame(e->t, e->sub, e->N, true, views, e->num_cus, &d, pk, e->world_pool);
      if (p.team && frame_lds_bytes(e->t, p, pk, e->world_pool, views) <= frame_lds_bytes(e->t, stock, pk, e->world_pool, views)) {
        cand.push_back(p);
        if (!quick && views != 1 && stock.feeders >= 4) {   // ... and with half the feeders (see below)
          d.feeders = stock.feeders / 2;
          const FramePlan h = plan_frame(e->t, e->sub, e->N, true, views, e->num_cus, &d, pk, e->world_pool);
          if (h.team && h.feeders != p.feeders && frame_lds_bytes(e->t, h, pk, e->world_pool, views) <= frame_lds_bytes(e->t, stock, pk, e->world_pool, views))
            cand.push_back(h);
        }
      }
    }
    // ... and the stock ring with sc1 pixel stores: 13 % faster for commons_harvest on
    // the buffers the memory side serves unevenly (341 -> 297 us), slower everywhere
    // else (profiles/r04_plans.md)
    // (per-agent views only: for WORLD.RGB it is slower on every buffer measured, by more
    // than a probe of NOOP steps resolves)
    if (views != 1 && !quick) {
      FramePlan q = stock;
      q.store_sc1 = 1;
      cand.push_back(q);
    }
    // ... and half the feeders (6 -> 3: three more drawing waves).  Where the memory side
    // serves a buffer evenly the per-agent drawing is issue-bound and the extra waves are
    // worth 8 - 13 % (clean_up, both views: 244 -> 205 - 213 us); where it does not, the
    // thirteenth wave starves and the launch is 4 % SLOWER (profiles/r04_head.md)
    if (views != 1 && stock.feeders >= 4 && !quick) {
      MpDevOptions d = {};
      d.struct_size = sizeof d;
      d.max_composites = -1;
      d.feeders = stock.feeders / 2;
      const FramePlan p = plan_frame(e->t, e->sub, e->N, true, views, e->num_cus, &d, pk, e->world_pool);
      if (frame_lds_bytes(e->t, p, pk, e->world_pool, views) <= frame_lds_bytes(e->t, stock, pk, e->world_pool, views) && p.feeders != stock.feeders)
        cand.push_back(p);
    }
  }
  if (cand.size() == 1 && !us_per_launch) return MP_OK;
  // An engine nothing has been done with yet (the usual moment to bind) is really
  // stepped: all worlds reset, uniformly random actions, behind a device-side copy of the records,
  // the counters and the engine's scalar outputs — what a plan costs when it steps is what is wanted, and a dry
  // launch ranks plans a few per cent apart wrongly (measured: the single-world ring
  // 96.5 us dry, 106.7 stepping, against 96.7 / 103.0 for the stock ring:
  // profiles/r04_plans.md).  An engine in use is timed dry, and a plan must then beat
  // the stock one by 6 % to replace it.
  ProbeState probe(e);   // (its destructor puts everything back on every path out of here)
  probe.hold_ring();
  if (!e->touched)
    if (int rc = probe.save()) return rc;
  const bool stepping = probe.copied;
  if (stepped) *stepped = stepping;
  if (e->ring_slots > 0) e->point_ring(0, stepping);
  int rc = MP_OK;
  if (stepping) {
    const int n = e->N * e->t.P;
    hipLaunchKernelGGL(k_probe_actions, dim3((n + 255) / 256), dim3(256), 0, e->stream,
                       e->d_actions, n, e->t.nact, 0x5eedu);
    rc = submit(e, STEP_MODE_RESET, nullptr, nullptr);
  } else {
    const hipError_t r = hipMemsetAsync(e->d_mask, 0, (size_t)e->N, e->stream);
    if (r != hipSuccess) { (void)hipGetLastError(); rc = fail(MP_ERR_HIP, "mp_tune: %s", hipGetErrorString(r)); }
  }
  // A device that has idled for a few ms runs its next ~150 launches 5 - 20 % slower
  // (clock ramp, profiles/r03_clock_ramp.md) — which would be charged to whichever plan
  // is timed first.  The first candidate runs untimed, in groups of eight, until five
  // groups in a row are within 1 % of the fastest group so far and none of them has
  // improved on it by 0.5 % (at most 40 groups, 32 ms): the ramp is not monotonic — 120 110
  // 117 118 116 114 112 111 110 110 108 107 107 107 us by tens of launches after 1 s of
  // idling — and two groups agreeing, round 3's rule, can be a plateau half way up.  The
  // clocks are then where a training loop, which never lets the device idle, has them —
  // for the candidates' timings and for whatever the caller launches next.
  plan = cand[0];
  {
    double best = 1e30;
    int steady = 0;
    for (int g = 0; g < 40 && rc == MP_OK && steady < 5; ++g) {
      double us = 0.0;
      rc = timed_launches_us(e, stepping, 6, &us);   // (2 + 6 launches)
      if (us < 0.995 * best) { best = us; steady = 0; }
      else if (us <= 1.01 * best) { ++steady; if (us < best) best = us; }
      else steady = 0;
    }
  }
  std::vector<FramePlan> kept((size_t)slots, cand[0]);
  double sum_us = 0;
  for (int sl = 0; sl < slots && rc == MP_OK; ++sl) {
    if (e->ring_slots > 0) e->point_ring(sl, stepping);
    double best_us = 1e30, stock_us = 0;
    int best = 0;
    std::vector<double> first_us(cand.size(), 1e30);
    for (size_t i = 0; i < cand.size() && rc == MP_OK; ++i) {
      plan = cand[i];
      rc = timed_launches_us(e, stepping, 6, &first_us[i]);
    }
    // A second look at whatever came within 6 % of the fastest, three times as long (round 6: with eight
    // candidates a few per cent apart — the team order is worth 3 - 5 % on an even buffer — one group of
    // six launches picked differently from run to run): the stock plan always, the others by their first
    // timing.  (A plan replaces the stock one only by a margin: the probe's steps are the first of an
    // episode, or no steps at all — 3 % stepping, 6 % dry.)
    {
      double fastest = 1e30;
      for (double us : first_us) fastest = std::min(fastest, us);
      for (size_t i = 0; i < cand.size() && rc == MP_OK; ++i) {
        if (i != 0 && first_us[i] > 1.06 * fastest) continue;
        plan = cand[i];
        double us = first_us[i];
        if (!quick) rc = timed_launches_us(e, stepping, 18, &us);
        if (i == 0) stock_us = us;
        if (rc == MP_OK && (i == 0 || us < std::min(best_us, (stepping ? 0.97 : 0.94) * stock_us))) {
          best_us = us; best = (int)i;
        }
      }
    }
    // ... and the pause of a renderer wave between two passes (FramePlan::pace, round 6).  Since the
    // renderers' resolve is two LDS round trips a pass instead of eighteen, the launch is its own store loop plus the head
    // on every buffer — 90 - 95 us for WORLD.RGB where the memory side takes the view's pages evenly, and
    // 113 - 119 where it does not: there a launch that writes FASTER finishes LATER (the old resolve's
    // 105 us on such a buffer were its pace), and a pause of two or three units gives the 104 back
    // (profiles/r06_resolve.md).  Searched on the plan just picked; the same margin as between plans.
    FramePlan chosen = cand[(size_t)best];
    // ... the feeders' wave priority once their first world is out (FramePlan::late_prio; round 6).  Under
    // the new resolve the renderers issue instructions where the old one waited on LDS, and a feeder at
    // their priority steps more slowly beside them: where the steps are the long pole (sixteen worlds
    // behind four feeders: externality_mushrooms, coop_mining, gift_refinements) priority 1 is 4 - 5 %
    // on every buffer, for commons_harvest 3 - 6 %; for clean_up's per-agent view it costs 4 % on an even
    // buffer (profiles/r06_resolve.md section 8) — so it is timed, on the plan just picked.
    // (only a probe that really steps can see it: in a dry launch the feeders load records and nothing else)
    if (rc == MP_OK && !e->has_dev && stepping && chosen.late_prio == 0 && !quick) {
      FramePlan q = chosen;
      q.late_prio = 1;
      plan = q;
      double us = 0;
      rc = timed_launches_us(e, stepping, 12, &us);
      if (rc == MP_OK && us < (stepping ? 0.97 : 0.94) * best_us) { best_us = us; chosen = q; }
    }
    if (rc == MP_OK && !e->has_dev && !quick) {
      // (all five: the response is not monotonic — clean_up's per-agent view on an uneven buffer 169.8 /
      // 169.7 / 166.2 / 154.7 / 166.0 us at 0 / 1 / 2 / 4 / 6 units, commons_harvest 345 / 341 / 329 / 310 / 337)
      const FramePlan base = chosen;
      const double unpaced_us = best_us;
      for (int pc : {1, 2, 3, 4, 6}) {
        if (rc != MP_OK) break;
        FramePlan q = base;
        q.pace = pc;
        plan = q;
        double us = 0;
        rc = timed_launches_us(e, stepping, 12, &us);
        // (3 % dry or stepping: what a pause changes is the renderers against the memory side, which a
        // dry launch has whole; the 6 % of a dry probe is for plans that move the FEEDERS' work)
        if (rc == MP_OK && us < std::min(best_us, 0.97 * unpaced_us)) { best_us = us; chosen = q; }
      }
    }
    if (rc == MP_OK) { kept[(size_t)sl] = chosen; sum_us += best_us; }
  }
  plan = rc == MP_OK ? kept[0] : before;
  if (rc == MP_OK && e->ring_slots > 0 && e->ring_has_pixels()) e->ring_plan[views] = kept;
  const int rc2 = probe.restore();   // ... and the engine is the engine it was
  if (rc != MP_OK) return rc;
  if (rc2 != MP_OK) return rc2;
  if (us_per_launch) *us_per_launch = sum_us / slots;
  return sync_and_check(e, "mp_tune");
}

int mp_place_output(MpEngine* e, MpObsKind kind, int32_t candidates, uint64_t max_bytes,
                    void** device_ptr, MpPlacement* report) {
  if (!e || !device_ptr) return fail(MP_ERR_INVALID, "mp_place_output: NULL argument");
  *device_ptr = nullptr;
  if (report) memset(report, 0, sizeof *report);
  if (!MpEngine::is_pixel_kind(kind))
    return fail(MP_ERR_INVALID, "mp_place_output: kind %d is not a pixel view", (int)kind);
  if (e->ring[kind].base)
    return fail(MP_ERR_INVALID, "mp_place_output: kind %d is bound as a ring; unbind it first", (int)kind);
  if (candidates < 1) candidates = 1;
  if (candidates > 32) candidates = 32;
  HIP_TRY(hipSetDevice(e->device));
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t bytes = mp_obs_bytes(e, kind);
  if (bytes == 0)
    return fail(MP_ERR_UNSUPPORTED, "mp_place_output: this substrate has no observation %d", (int)kind);
  if (max_bytes == 0) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    max_bytes = free_b / 4;
  }
  // candidates alive at a time: released chunks come straight back from the driver's
  // pool, so a round's buffers are held together to be different placements
  uint64_t alive = max_bytes / bytes;
  if (alive < 1)
    return fail(MP_ERR_INVALID, "mp_place_output: max_bytes %llu holds no view of %llu bytes",
                (unsigned long long)max_bytes, (unsigned long long)bytes);
  if (alive > 12) alive = 12;   // a round; another one only if no candidate of it stands out
  if (alive > (uint64_t)candidates) alive = (uint64_t)candidates;
  if (alive == 1) candidates = 1;   // nothing can be compared inside the caller's bound
  // RAII: whatever path leaves this function, every buffer but the one handed out is released
  // and the kind is bound to what it was bound to (or to the winner)
  struct Round {
    MpEngine* e; MpObsKind kind; void* previous; void* keep = nullptr;
    std::vector<void*> bufs;
    bool done = false;
    ~Round() {
      for (void* p : bufs)
        if (p != keep) (void)free_output(e->device, p, true);
      if (!done) {
        if (keep) (void)free_output(e->device, keep, true);
        e->bound[kind] = previous;
      }
    }
    void release_losers() {
      for (void* p : bufs)
        if (p != keep) (void)free_output(e->device, p, true);
      bufs.clear();
    }
  } round{e, kind, e->bound[kind]};
  MpPlacement rep = {};
  rep.requested = candidates;
  double best_us = 1e30;
  int rc = MP_OK;
  bool first = true, exhausted = false;
  while (rep.candidates < candidates && rc == MP_OK && !exhausted) {
    // a round: as many fresh buffers as fit next to the best one so far — the FIRST round
    // eight at most: where a box shows no spread between views mapped from scattered 2 MB
    // chunks (profiles/r05_alloc_method.md), eight that agree to 3 % settle it in half a
    // second; four were too few — on a box where every second candidate is the slow kind
    // (this round's per-agent view: 124 - 128 against 145 - 157 us) one first round in
    // sixteen is all slow, agrees with itself, and keeps a view 25 % slower than the next
    uint64_t room = alive - (round.keep && alive > 1 ? 1 : 0);
    if (rep.candidates == 0 && room > 8) room = 8;
    for (uint64_t i = 0; i < room && rep.candidates + (int)round.bufs.size() < candidates; ++i) {
      void* p = nullptr;
      // (every fourth candidate one plain allocation: views mapped from 2 MB chunks are the
      // evenly served kind on most boxes — profiles/r05_alloc_method.md — but on one box of
      // round 6 all three were the slow kind and one of two plain allocations the fast one,
      // 78 against 97 us in the bare loop: profiles/r06_fill_geometry.md)
      const int index = rep.candidates + (int)round.bufs.size();
      if (mp_alloc_output(e->device, bytes, index % 4 == 3 ? 0 : (2u << 20), &p) != MP_OK) {
        // out of memory (or of address space): the probe goes on with what there is, and says so
        ++rep.out_of_memory;
        exhausted = true;
        break;
      }
      round.bufs.push_back(p);
    }
    if (round.bufs.empty()) break;
    const int round_first = rep.candidates;
    for (void* p : round.bufs) {
      e->bound[kind] = p;
      double us = 0;
      bool stepped = false;
      rc = tune_impl(e, &us, &stepped, /*quick=*/true);
      if (rc != MP_OK) break;
      if (first) { rep.stepped = stepped ? 1 : 0; first = false; }
      rep.us[rep.candidates] = (float)us;
      if (us < best_us) {
        void* old = round.keep;
        best_us = us; round.keep = p; rep.picked = rep.candidates;
        if (old && std::find(round.bufs.begin(), round.bufs.end(), old) == round.bufs.end())
          (void)free_output(e->device, old, true);
      }
      ++rep.candidates;
    }
    if (rc != MP_OK) break;
    round.release_losers();
    if (rep.candidates - round_first >= 4) {
      // a round whose candidates all take the same time: there is no lottery to win for this
      // view on this box (WORLD.RGB mostly) — stop
      const float lo = *std::min_element(rep.us + round_first, rep.us + rep.candidates);
      const float hi = *std::max_element(rep.us + round_first, rep.us + rep.candidates);
      if (hi < 1.03f * lo) { rep.early_exit = 1; break; }
    }
    // an outlier among them (a fast placement is 8 % or more below the median)?  enough
    if (rep.candidates >= 4) {
      std::vector<float> v(rep.us, rep.us + rep.candidates);
      std::sort(v.begin(), v.end());
      if (v[0] < 0.92f * v[v.size() / 2]) { rep.early_exit = 2; break; }
    }
  }
  if (rc == MP_OK && !round.keep)
    rc = fail(MP_ERR_HIP, "mp_place_output: no buffer of %llu bytes could be mapped: %s",
              (unsigned long long)bytes, g_error.c_str());
  if (rc != MP_OK) return rc;   // (~Round releases everything and rebinds what was bound)
  e->bound[kind] = round.keep;
  rc = mp_tune(e, nullptr);   // the plan for the buffer that stays
  if (rc != MP_OK) return rc;
  round.done = true;
  *device_ptr = round.keep;
  rep.setup_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (report) *report = rep;
  return MP_OK;
}

int mp_box_fill(MpEngine* e, MpObsKind kind, int32_t reps, MpBoxFill* out) {
  if (!e || !out) return fail(MP_ERR_INVALID, "mp_box_fill: NULL argument");
  memset(out, 0, sizeof *out);
  if (kind != MP_OBS_RGB && kind != MP_OBS_WORLD_RGB)
    return fail(MP_ERR_INVALID, "mp_box_fill: kind %d is not a pixel view", (int)kind);
  if (kind == MP_OBS_WORLD_RGB && e->world_pool > 1)
    return fail(MP_ERR_INVALID, "mp_box_fill: WORLD.RGB is pooled by %d (MpConfig.world_pool)",
                e->world_pool);
  if (e->ring[kind].base || !e->bound[kind])
    return fail(MP_ERR_INVALID, "mp_box_fill: kind %d is not bound to one buffer", (int)kind);
  if (reps < 1) reps = 1;
  if (reps > 1000) reps = 1000;
  HIP_TRY(hipSetDevice(e->device));
  uint8_t* view = (uint8_t*)e->bound[kind];
  const uint64_t bytes = mp_obs_bytes(e, kind);
  if (bytes == 0 || bytes % 16)
    return fail(MP_ERR_UNSUPPORTED, "mp_box_fill: a view of %llu bytes", (unsigned long long)bytes);
  // the store loop's geometry = the frame launch's under the plan that is current for what is bound
  const bool both = e->bound[MP_OBS_RGB] && e->bound[MP_OBS_WORLD_RGB];
  const int views = both ? 2 : kind == MP_OBS_WORLD_RGB ? 1 : 0;
  const FramePlan& p = e->plan[1][views];
  int waves = p.nwaves - p.feeders;
  if (both) waves = kind == MP_OBS_WORLD_RGB ? p.world_waves : waves - p.world_waves;
  if (waves < 1) waves = 1;
  const int row_cells = kind == MP_OBS_WORLD_RGB ? e->t.W : e->t.vl + e->t.vr + 1;
  const int R = 64 / row_cells > 0 ? 64 / row_cells : 1;
  const uint32_t span = (uint32_t)R * 8u * (uint32_t)row_cells * 24u;   // one renderer pass
  const uint64_t per_world = bytes / (uint64_t)e->N;
  const uint64_t own = (uint64_t)p.ks * (uint64_t)p.B * per_world;       // a workgroup's worlds
  const int groups = p.groups > 0 ? p.groups : 1;
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  } ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  float us[3] = {0, 0, 0};
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() -> hipError_t {
      if (what == 0) return hipMemsetAsync(view, 0x5a, (size_t)bytes, e->stream);
      const uint64_t owned = what == 1 ? ((own + 15) & ~(uint64_t)15) : 0;
      // (a pooled plan owns less than the view: its rest is walked by the same workgroups)
      const uint64_t cover = what == 1 ? (bytes + (uint64_t)groups - 1) / (uint64_t)groups : 0;
      const uint64_t share = what == 1 ? (owned * (uint64_t)groups >= bytes ? owned : ((cover + 15) & ~(uint64_t)15)) : 0;
      hipLaunchKernelGGL(k_box_fill, dim3(groups), dim3(waves * 64), 0, e->stream, view, bytes, share,
                         what == 1 ? span : 4096u, what == 1 ? 0 : 1);
      return hipGetLastError();
    };
    HIP_TRY(launch());
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(ev.a, e->stream));
    for (int r = 0; r < reps; ++r) HIP_TRY(launch());
    HIP_TRY(hipEventRecord(ev.b, e->stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    us[what] = ms * 1e3f / (float)reps;
  }
  out->bytes = bytes;
  out->memset_us = us[0];
  out->product_order_us = us[1];
  out->front_4k_us = us[2];
  out->groups = groups;
  out->waves = waves;
  out->span_bytes = span;
  return sync_and_check(e, "mp_box_fill");
}

int mp_fault_words(const MpEngine* e, uint32_t out[64]) {
  if (!e || !out) return fail(MP_ERR_INVALID, "mp_fault_words: NULL argument");
  for (int i = 0; i < 64; ++i) out[i] = ((const volatile uint32_t*)e->h_fault)[i];
  return MP_OK;
}

int mp_sync(MpEngine* e) {
  if (!e) return fail(MP_ERR_INVALID, "mp_sync: NULL engine");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = sync_and_check(e, "mp_sync")) return rc;
  return MP_OK;
}

}  // extern "C"
