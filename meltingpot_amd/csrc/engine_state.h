// engine_state.h — what the units of the engine's host side share (mp_engine.hip, engine_atlas.hip,
// engine_requests.hip, engine_views.hip, engine_outputs.hip, mp_place.hip): the engine object, the
// error path, the frame launches' prototypes, the submission path and the checks of a request's
// memory.  Internal: nothing here is exported (-fvisibility=hidden, exports.map).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/mp_engine.h"
#include "pack_decode.h"
#include "step_common.h"
#include "step_many.h"
#include "step_until.h"
#include "step_listed.h"
#include "state_check.h"
#include "state_hash.h"
#include "episode_stats.h"
#include "avatar_ids.h"

// ---- errors (mp_engine.hip): the text mp_last_error returns, per thread
extern thread_local std::string g_error;
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                       \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess)                                                   \
      return fail(MP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// ---- frame.hip
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
  // wl: the WORLD.LAYER leaf, int32 [N][H][W][L]; wp: the world planes, uint8 [N][C'][H][W] (the
  // world ops of MpEgoLayer and MpEgoPlanes; world_view.h), written behind those.
  ViewRegistration ego, vh, ep, av, avz, wl, wp;
  int32_t num_layer_ids = 0;   // 1 + the largest id of d_layer_lut: the length of a class table
  int32_t num_world_ids = 0;   // 1 + the largest id of d_world_lut: the length of a world planes' class table
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
  int32_t* d_world_lut = nullptr;  // the world's value table [kLayerLutRow] (world_view.h)
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

// ---- mp_create's stages that other units call too (mp_engine.hip; build_atlas: engine_atlas.hip)
struct HostStage {
  MpConfig cfg = {};
  MpDevOptions dev = {};
  std::vector<uint8_t> pack;
  DecodedPack d;
};
int host_stage(const void* pack, uint64_t pack_len, const MpConfig* cfg, HostStage* h);
int build_atlas(MpEngine* e, const MpDevOptions* dev, const DecodedPack& d);
uint64_t state_fingerprint(const std::vector<uint8_t>& pack, const DevTables& t);
std::vector<int32_t> layer_lut_rows(const void* pack, const DevTables& t);
std::vector<int32_t> world_lut_row(const void* pack, const DevTables& t);
uint64_t pack_hash(const std::vector<uint8_t>& pack);
int select_kernels(const std::vector<uint8_t>& pack, const DecodedPack& d, const MpDevOptions* dev);
const ZapRules* zap_rules_of(const SubstrateTables& sub);
const char* family_name(const SubstrateTables& sub);
void avatar_ids_tables(avatar_ids::Args* a, const DevTables& t, const ZapRules* zap, const uint32_t* sinfo);

// ---- the submission path (mp_engine.hip)
int sync_and_check(MpEngine* e, const char* who);
void draw(MpEngine* e, uint8_t* rgb, uint8_t* wrgb, int pool_k = 1);
int submit(MpEngine* e, int mode, const int32_t* actions, const uint8_t* mask,
           const uint8_t* bank = nullptr, const int32_t* src = nullptr, int bank_rows = 0,
           const StepManyLaunch* many = nullptr, const UntilArgs* until = nullptr,
           const ListArgs* list = nullptr);

// ---- the checks of a request's counts and memory (mp_engine.hip), each rule and its message once
int check_bank(MpEngine* e, const void* ptr, uint64_t bytes, const char* who);
int check_device_pointer(MpEngine* e, const void* ptr, const char* who);
int check_counts(const char* who, int32_t count, int32_t src_rows, bool bounded = true);
int check_row_list(const char* who, const int32_t* rows, int32_t count, int32_t src_rows, const char* verb,
                   bool bank = true, bool needs_list = false, const char* tail = "");
int check_fingerprint(const char* who, uint64_t rows, uint64_t own, const char* whose);
int check_dst_bytes(const char* who, int32_t count, uint64_t each, uint64_t dst_bytes, uint64_t* need);
int check_aligned(const char* who, const char* what, const void* at, uint64_t align);
struct Extent { const char* what; const void* at; uint64_t bytes; uint64_t align; };
int check_extents(MpEngine* e, const char* who, const Extent* all, size_t n);
int check_extents(MpEngine* e, const char* who, std::initializer_list<Extent> all);
int check_agent_view(MpEngine* e, int kind, const void* ptr, const char* who);
int check_world_view(MpEngine* e, int kind, const void* ptr, const char* who);

// ---- the mapped views (engine_outputs.hip)
void retired_va(int64_t* bytes, int64_t* limit);
bool in_mapped_view(const void* p);
int free_output(int device, void* ptr, bool keep_va);

// ---- the four requests about every viewer's window (engine_views.hip; carried by mp_snapshot,
// engine_requests.hip)
int ego_layer_request(MpEngine* e, const MpEgoLayer& r);
int view_hash_request(MpEngine* e, MpViewHash* out);
int ego_planes_request(MpEngine* e, MpEgoPlanes* out);
int avatar_ids_request(MpEngine* e, const MpAvatarIds& r);
