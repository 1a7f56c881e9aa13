// mp_place.hip — where a bound view lies and how the frame launch is shaped for it: the tuner
// (mp_tune), the placement search (mp_place_output) and the store-order probe (mp_box_fill), with
// the two kernels only they launch.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "engine_state.h"

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

extern "C" {

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

}  // extern "C"
