// engine_requests.hip — the requests mp_snapshot and mp_restore carry (include/mp_engine.h): the
// saved world states (MpWorldStates, MpStatesObserve, MpStatesView, MpStateLayout, MpStatesCheck,
// MpStatesHash, MpEpisodeStarts, MpEpisodeStats), the K-step requests (MpStepMany, MpStepTrajectory,
// MpStepActive, MpStepUntil, MpStepListed) and MpKernelVariant, one handler each; the table that
// tells them apart (kRequests) with the two carriers; the four view requests' handlers are
// engine_views.hip's.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "engine_state.h"
#include "stock.h"
#include "state_obs.h"
#include "state_view.h"

namespace {

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
      t.fault[FAULT_STATE_INDEX + 2] = kFaultSaveWorld;
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

}  // extern "C"

namespace {

// What a carrier calls for a buffer of a request's size.  Copy-in: the handler reads a copy, and
// the caller's struct is never written.
template <class R, auto handler>
int copied(MpEngine* e, void* buf) {
  R r;
  memcpy(&r, buf, sizeof r);
  return handler(e, r);
}
// In place: the handler writes its answer into the caller's struct.
template <class R, auto handler>
int in_place(MpEngine* e, void* buf) {
  return handler(e, (R*)buf);
}
// MpWorldStates is a save through mp_snapshot (the fingerprint is written back) and a load through
// mp_restore (nothing is).
int save_states(MpEngine* e, MpWorldStates* r) { return world_states(e, r, false); }
int load_states(MpEngine* e, MpWorldStates& r) { return world_states(e, &r, true); }

// The 18 requests.  mp_snapshot and mp_restore tell them apart by size (a snapshot is >= 448
// bytes).  `snapshot`, `restore`: what the carrier calls, NULL where the size is no request of that
// carrier's — it then falls through to the carrier's own "bad buffer".  `null_engine`: whether the
// handler is reached without an engine (to refuse in its own words, or to answer its host form).
struct Request {
  size_t size;
  int (*snapshot)(MpEngine* e, void* buf);
  int (*restore)(MpEngine* e, void* buf);   // (always copy-in: mp_restore's buffer is const)
  bool null_engine;
};
constexpr Request kRequests[] = {
    {sizeof(MpKernelVariant), in_place<MpKernelVariant, kernel_variant>, nullptr, true},
    {sizeof(MpWorldStates), in_place<MpWorldStates, save_states>, copied<MpWorldStates, load_states>, false},
    {sizeof(MpStatesObserve), copied<MpStatesObserve, states_observe>, nullptr, true},
    {sizeof(MpStatesView), copied<MpStatesView, states_view>, nullptr, true},
    {sizeof(MpEgoLayer), copied<MpEgoLayer, ego_layer_request>, nullptr, true},
    {sizeof(MpViewHash), in_place<MpViewHash, view_hash_request>, nullptr, true},     // (num_ids is written back)
    {sizeof(MpEgoPlanes), in_place<MpEgoPlanes, ego_planes_request>, nullptr, true},   // (likewise)
    {sizeof(MpAvatarIds), copied<MpAvatarIds, avatar_ids_request>, nullptr, true},
    {sizeof(MpStateLayout), in_place<MpStateLayout, state_layout>, nullptr, true},
    {sizeof(MpStatesCheck), copied<MpStatesCheck, states_check>, nullptr, true},       // (the verdicts go to r.out)
    {sizeof(MpStatesHash), copied<MpStatesHash, states_hash>, nullptr, true},          // (the hashes go to r.out)
    {sizeof(MpStepMany), nullptr, copied<MpStepMany, many_request>, true},
    {sizeof(MpStepTrajectory), nullptr, copied<MpStepTrajectory, trajectory_request>, true},
    {sizeof(MpEpisodeStarts), nullptr, copied<MpEpisodeStarts, episode_starts>, true},
    {sizeof(MpStepActive), nullptr, copied<MpStepActive, active_request>, true},
    {sizeof(MpStepUntil), nullptr, copied<MpStepUntil, until_request>, true},
    {sizeof(MpStepListed), nullptr, copied<MpStepListed, listed_request>, true},
    {sizeof(MpEpisodeStats), nullptr, copied<MpEpisodeStats, episode_stats_request>, true},
};
constexpr bool request_sizes_tell_apart() {
  for (const Request& q : kRequests) {
    if (q.size >= 448) return false;
    for (const Request* p = kRequests; p != &q; ++p)
      if (p->size == q.size) return false;
  }
  return true;
}
static_assert(request_sizes_tell_apart(), "two requests of one size, or one the size of a snapshot");

const Request* request_of(const void* buf, uint64_t bytes) {
  if (!buf) return nullptr;
  for (const Request& q : kRequests)
    if (q.size == bytes) return &q;
  return nullptr;
}

}  // namespace

extern "C" {

int mp_snapshot(MpEngine* e, void* buf, uint64_t bytes) {
  const Request* q = request_of(buf, bytes);
  if (q && q->snapshot && (e || q->null_engine)) return q->snapshot(e, buf);
  if (!e || !buf || bytes != mp_snapshot_bytes(e))
    return fail(MP_ERR_INVALID, "mp_snapshot: bad buffer");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = sync_and_check(e, "mp_snapshot")) return rc;
  HIP_TRY(hipMemcpy(buf, e->d_state, bytes, hipMemcpyDeviceToHost));
  return MP_OK;
}

int mp_restore(MpEngine* e, const void* buf, uint64_t bytes) {
  const Request* q = request_of(buf, bytes);
  if (q && q->restore && (e || q->null_engine)) return q->restore(e, const_cast<void*>(buf));
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

}  // extern "C"
