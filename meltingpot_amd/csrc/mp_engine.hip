// mp_engine.hip — C ABI of libmp_engine.so (declared in include/mp_engine.h).
//
// Host side of the boundary that replaces dmlab2d.Lab2d / dmlab2d.Environment
// (reference: meltingpot/utils/substrates/builder.py:179-187,
// wrappers/base.py:38-84).  No CPU execution path exists here: every call that
// would compute needs a HIP device and fails loudly without one.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "engine_state.h"
#include "stock.h"
#include "state_view.h"
#include "ego_layer.h"
#include "view_hash.h"
#include "ego_planes.h"
#include "world_view.h"

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

namespace {

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

// The requests whose launches report a rows[] index and a players[] index (mp_common.h:
// IndexFault) tell them in one sentence: the request's name and what each index "is".
struct IndexPairReport {
  uint32_t row, player;
  const char* request;
  const char* row_is;
  const char* player_is;
};
constexpr char kNoRow[] = "not a row of the bank";
constexpr char kNoRowOrWorld[] = "not a row of the bank (with no bank: no world of this engine)";
constexpr char kNoPlayer[] = "not a player of this engine";
constexpr IndexPairReport kIndexPairReports[] = {
    {kFaultViewRow, kFaultViewPlayer, "MpStatesView", kNoRow, kNoPlayer},
    {kFaultEgoRow, kFaultEgoPlayer, "MpEgoLayer", kNoRowOrWorld, kNoPlayer},
    {kFaultViewHashRow, kFaultViewHashPlayer, "MpViewHash", kNoRowOrWorld, kNoPlayer},
    {kFaultEgoPlanesRow, kFaultEgoPlanesPlayer, "MpEgoPlanes", kNoRowOrWorld, kNoPlayer},
    {kFaultAvatarIdsRow, kFaultAvatarIdsPlayer, "MpAvatarIds", kNoRowOrWorld, kNoPlayer},
    // (the world ops take no players[]: one code each)
    {kFaultWorldLayerRow, kFaultWorldLayerRow, "MpEgoLayer (MP_EGO_WORLD_DRAW)", kNoRowOrWorld, kNoPlayer},
    {kFaultWorldPlanesRow, kFaultWorldPlanesRow, "MpEgoPlanes (MP_EGOPLANES_WORLD_DRAW)", kNoRowOrWorld, kNoPlayer},
};

}  // namespace

// Waits for the engine's stream and reports a frame kernel that gave up on its
// pipeline (frame.hip: report_stall) — an engine bug, surfaced instead of hung on — and then
// whatever a launch wrote into the fault words by design: each report once.
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
    const uint32_t what = f[FAULT_STATE_INDEX + 2];
    e->h_fault[FAULT_STATE_INDEX] = 0;   // reported once; the engine stays usable
    for (const IndexPairReport& p : kIndexPairReports)
      if (what == p.row || what == p.player)
        return fail(MP_ERR_INVALID,
                    "%s: %s: %s[%u] = %d is %s; element %u of the destination was left as it was",
                    who, p.request, what == p.row ? "rows" : "players", at, (int)index,
                    what == p.row ? p.row_is : p.player_is, at);
    switch (what) {
      case kFaultEgoPlanesClass:
        return fail(MP_ERR_INVALID,
                    "%s: MpEgoPlanes: classes[%u] = %d is outside [-1, num_classes); the entry counted as -1",
                    who, at, (int)index);
      case kFaultWorldPlanesClass:
        return fail(MP_ERR_INVALID,
                    "%s: MpEgoPlanes (MP_EGOPLANES_WORLD_DRAW): classes[%u] = %d is outside [-1, num_classes); the "
                    "entry counted as -1", who, at, (int)index);
      case kFaultListedWorld:
      case kFaultListedRepeat:
        return fail(MP_ERR_INVALID,
                    "%s: MpStepListed: worlds[%u] = %d %s; the entry ran nothing and element %u of every per-call "
                    "tensor was left as it was", who, at, (int)index,
                    what == kFaultListedWorld ? "is not a world of this engine" : "repeats an earlier entry's world", at);
      case kFaultHashRow:
        return fail(MP_ERR_INVALID,
                    "%s: MpStatesHash: rows[%u] = %d is not a row of the bank (MP_HASH_WORLDS: no world of this "
                    "engine); element %u of out was left as it was", who, at, (int)index, at);
      case kFaultCheckRow:
        return fail(MP_ERR_INVALID,
                    "%s: MpStatesCheck: rows[%u] = %d is not a row of the bank; element %u of out is (-1, %d)",
                    who, at, (int)index, at, (int)index);
      case kFaultObserveRow:
        return fail(MP_ERR_INVALID,
                    "%s: MpStatesObserve: rows[%u] = %d is not a row of the bank; element %u of the "
                    "destination was left as it was", who, at, (int)index, at);
      case kFaultLoadSrc:
        return fail(MP_ERR_INVALID,
                    "%s: MP_STATES_LOAD: src[%u] = %d is neither -1 nor a row of the bank; world %u "
                    "was left as it was", who, at, (int)index, at);
      case kFaultSaveWorld:
      default:   // (no launch writes another value)
        return fail(MP_ERR_INVALID,
                    "%s: MP_STATES_SAVE: worlds[%u] = %d is not a world of this engine; row %u was "
                    "left as it was", who, at, (int)index, at);
    }
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
void draw(MpEngine* e, uint8_t* rgb, uint8_t* wrgb, int pool_k) {
  stepk::StepArgs args = {};
  args.state = e->d_state; args.num_worlds = e->N;
  FramePlan p = e->frame_plan(0, rgb && wrgb ? 2 : wrgb ? 1 : 0, rgb ? pool_k : 1);
  p.parity = e->frame_launches++ & 1;
  launch_frame(e->t, nullptr, args, rgb, wrgb, p, e->stream, rgb ? pool_k : 1, e->world_pool);
}

// (`many`: a K-step request, checked by step_request — K steps by the K-step kernels, then the
// draw-only launches of the unfused path; NULL: a single step)
int submit(MpEngine* e, int mode, const int32_t* actions, const uint8_t* mask,
           const uint8_t* bank, const int32_t* src, int bank_rows, const StepManyLaunch* many,
           const UntilArgs* until, const ListArgs* list) {
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
  if (!e->viewing(e->ego) && !e->viewing(e->vh) && !e->viewing(e->ep) && !e->viewing(e->av) && !e->viewing(e->avz) &&
      !e->viewing(e->wl) && !e->viewing(e->wp))
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
  if (e->viewing(e->wl)) {   // WORLD.LAYER
    world_view::LayerArgs a = {};
    worlds(&a, e->wl);
    a.lut = e->d_world_lut;
    world_view::launch(a, world_view::layer_plan(g, e->N, e->num_cus), e->stream);
    HIP_TRY(hipGetLastError());
  }
  if (e->viewing(e->wp)) {   // the world's class and facing planes
    world_view::PlanesArgs a = {};
    worlds(&a, e->wp);
    a.lut = e->d_world_lut;
    a.layer_mask = e->wp.mask;
    a.classes = e->wp.classes; a.num_ids = e->num_world_ids;
    a.num_classes = e->wp.num_classes; a.facing = e->wp.facing;
    world_view::launch(a, world_view::planes_plan(g, a.num_classes, e->N, e->num_cus), e->stream);
    HIP_TRY(hipGetLastError());
  }
  return MP_OK;
}

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

// A bank of world-state rows (MP_STATES_SAVE / MP_STATES_LOAD): device memory of the engine's
// device, [ptr, ptr + bytes) inside one allocation.
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
int check_counts(const char* who, int32_t count, int32_t src_rows, bool bounded) {
  if (count < 1 || (bounded && src_rows < 1))
    return fail(MP_ERR_INVALID, "%s: count %d, bank_rows %d: both must be at least 1", who, count, src_rows);
  return MP_OK;
}

// Without a row list a request reads rows 0 .. count - 1.  `verb`: what it does to them; `bank`:
// "the bank has" so many, else "there are"; `needs_list` and `tail`: MP_CHECK_FILTER's own.
int check_row_list(const char* who, const int32_t* rows, int32_t count, int32_t src_rows, const char* verb,
                   bool bank, bool needs_list, const char* tail) {
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

namespace {

// mp_bind_output on a kind that was bound as a ring: the kind leaves the ring
void drop_ring_kind(MpEngine* e, int kind) {
  if (!e->ring[kind].base) return;
  e->ring[kind] = MpEngine::RingKind();
  for (auto& v : e->ring_plan) v.clear();
  bool any = false;
  for (int k = 0; k < MP_OBS_KINDS; ++k) any = any || e->ring[k].base;
  if (!any) { e->ring_slots = 0; e->ring_cursor = 0; }
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

}  // namespace

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

// The WORLD's value table (world_view.h): a viewer's row through row P of view_sprite_map, the map
// "WORLD.RGB" is rendered through (frame.hip: build_world_images).  [256] stays 0: no cell of the
// whole map is off it.
std::vector<int32_t> world_lut_row(const void* pack, const DevTables& t) {
  const int32_t* ssprite = table<int32_t>(pack, "state_sprite");
  const int32_t* remap = table<int32_t>(pack, "view_sprite_map") + (size_t)t.P * t.nsprites;
  std::vector<int32_t> row((size_t)kLayerLutRow, 0);
  for (int s = 1; s < t.nstates && s < 256; ++s)
    row[s] = ssprite[s] >= 0 ? 1 + remap[ssprite[s]] : 0;
  return row;
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

namespace {

int upload_layer_lut(MpEngine* e) {
  const DevTables& t = e->t;
  const std::vector<int32_t> lut = layer_lut_rows(e->pack.data(), t);
  e->num_layer_ids = view_hash::num_ids(lut.data(), t.P);
  HIP_TRY(hipMalloc((void**)&e->d_layer_lut, lut.size() * 4));
  HIP_TRY(hipMemcpy(e->d_layer_lut, lut.data(), lut.size() * 4, hipMemcpyHostToDevice));
  const std::vector<int32_t> wt = world_lut_row(e->pack.data(), t);
  e->num_world_ids = world_view::num_ids(wt.data());
  HIP_TRY(hipMalloc((void**)&e->d_world_lut, wt.size() * 4));
  HIP_TRY(hipMemcpy(e->d_world_lut, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
  return MP_OK;
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
  if (int rc = world_view::prepare())
    return fail(MP_ERR_HIP, "mp_create: hipFuncSetAttribute(max dynamic LDS) of the world-view kernels failed: %d", rc);
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

}  // namespace

// mp_create's host stage: the config checked and copied (older, shorter layouts of MpConfig and
// MpDevOptions completed), the pack copied, roles applied, decoded and checked.  No HIP call.
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
                  e->d_layer_lut, e->d_world_lut, e->d_obs_rows, e->d_obs_stash, e->d_check, e->d_hash_mask,
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
