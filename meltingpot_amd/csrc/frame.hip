// frame.hip — the observation kernels: layer views + tile renderer for N worlds,
// persistent, with the environment step fused in.
//
// Replaces the observation reads that follow every reference step
// (api:observation, lua/modules/api_factory.lua:73-75):
//   "N.RGB"      playerLayerView:observation -> playerView:render
//                (avatar_library.lua:225-277)   egocentric 11x11 cells, 88x88x3
//   "WORLD.RGB"  worldView:render(worldLayerView:observation)
//                (base_simulation.lua:347-368)  whole map, H*8 x W*8 x 3
// i.e. dmlab2d's `world:createView` + `tile.Scene:render` — and, in the fused
// form, api:advance itself (api_factory.lua:104-111; step_<substrate>.h).
// Semantics of the views (window, rotation, OutOfBounds, per-viewer spriteMap,
// relative facing, bottom->top 8-bit alpha compositing) are the ones the CPU
// restatement in oracle/render.c documents as assumptions A6-A9; this file is
// bit-exact with it.
//
// Execution shape (v12).  The kernel writes 192 B per output cell and reads
// ~9 B, so it is HBM-write bound by construction; what the store path charges
// for on MI355X is the NUMBER of vector store instructions a wave issues
// (profiles/r01_render_ablation.md), so the observation leaves as few, full,
// 16-byte-per-lane stores as possible.  Round 1 (v11) ran one launch per step
// for the rules (one wave per world, 25-90 us, latency-bound: SQ_WAIT_ANY 60 %)
// and one for the pixels whose workgroups each paid a 14-17 us prologue.  v12 is
// ONE persistent launch per bound view:
//   * grid = one workgroup per CU (all 160 KB of LDS; 12 waves for WORLD.RGB,
//     16 for the per-agent views: plan_frame); a workgroup owns a contiguous
//     range of worlds and walks it in batches of B worlds through two LDS
//     record buffers;
//   * the workgroup's prologue stages what never changes — the blob with the
//     de-duplicated sprite atlas, the composite cache and the lookup tables,
//     plus the step's tables — once per CU instead of once per 8 worlds;
//   * the last F waves are FEEDERS, the others RENDERERS (two code paths of one
//     kernel; the feeders run at raised wave priority: a step is a chain of
//     dependent instructions, the renderers always have independent work).
//     A feeder brings worlds of the next batch into the free buffer — record
//     HBM -> LDS, then (fused form) the whole environment step on it, in LDS,
//     by that one wave (step_<substrate>.h), and the stepped record streamed
//     back to HBM — while the renderers draw the current batch.  The step's
//     dependent-latency chain (~10 us of LDS round trips and scalar waits,
//     almost no issue slots) hides behind the store-bound rendering of the
//     previous batch; only the first batch of a workgroup is exposed;
//   * rendering is handed out as tickets (batch, pass) from one LDS counter; a
//     renderer with a ticket waits (s_sleep polling of LDS flags) until every
//     world of that batch has been fed, so there is no workgroup barrier after
//     the prologue; a feeder refills a buffer once every pass of its previous
//     batch has been counted done;
//   * work unit = a "strip": one row of output cells = 8 pixel rows, contiguous
//     in the output tensor in both views.  A pass = floor(64 / row_cells) whole
//     strips = one contiguous 64-byte-aligned span;
//   * phase 1, one lane per cell: resolve the cell's draw list from the LDS
//     planes — top -> bottom, stopping at the first fully opaque sprite.  Stacks
//     that static pieces of the map form (dirt on water, a shadow on sand,
//     claimed-resource paint on its texture) were pre-blended by mp_create: a
//     hash lookup replaces (base, overlay) by the composite image, so only
//     avatars, beams and rare combinations are left to composite.  Those cells
//     are listed densely (8-bit alpha ones first);
//   * phase 2b, eight lanes per listed cell (one per pixel row): binary-alpha
//     select or the 8-bit blend in registers, result staged in the wave's LDS
//     scratch as one more pre-packed image;
//   * phase 2a: the span leaves as 16-byte lane-contiguous chunks (1 KiB per
//     wave store, whole cache lines); each half chunk is an 8-byte LDS read from
//     the pre-packed image of the cell it falls in (atlas, composite or scratch);
//   * a pass with more composited cells than the scratch holds falls back to
//     per-row 12 + 12-byte stores (bit-identical, 16 instead of 12 stores).
// The main loop of a rendering wave issues NO global loads (loads and stores
// share vmcnt and the per-CU memory pipe is in-order); the feeders' loads are
// few (a record is 6 KB against the 121-372 KB of pixels it turns into).
#include "frame_kernel.h"

// Launch geometry.  One workgroup per CU (all 160 KB of LDS): the sprite
// atlas and tables are staged once per CU, every wave has its staging area for
// composited cells, and a ring of NB buffers of B worlds each takes the rest: enough
// slots that drawing the resident worlds (tens of us) covers the feeders' steps of
// the next ones (~10 us each, in parallel), few enough that they fit.
static int slot_scratch_bytes(const DevTables& t, const SubstrateTables& s) {
  int extra = 0;
  if (s.substrate == MPK_SUBSTRATE_TERRITORY) extra = stepk::extra_bytes(s.tr);
  if (s.substrate == MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS) extra = stepk::extra_bytes(s.em);
  return stepk::scratch_bytes(t) + extra;
}


// views: 0 = per-agent RGB, 1 = WORLD.RGB, 2 = both in one launch
// pool_k: the per-agent view is pooled by k (2, 4, 8: MP_OBS_RGB_POOL*), 1 = the full image.  The
// geometry is chosen as for the full view: a renderer's cost of a pooled pass is its per-cell
// resolve, which pooling does not shrink, so neither the batch / feeder choice nor the share of
// renderer waves between two views is scaled by the bytes written; pool_k only enters the LDS
// layout (pooled atlas, span staging) the ring is fitted beside.  world_k: the same for WORLD.RGB
// (MpConfig.world_pool), which enters only plans that draw it (views 1 and 2).
FramePlan plan_frame(const DevTables& t, const SubstrateTables& s, int num_worlds,
                     bool with_step, int views, int num_cus, const MpDevOptions* dev, int pool_k,
                     int world_k) {
  FramePlan p = {};
  const int lds_pool = pool_k > 1 && views != 1 ? pool_k : 0;   // (frame_lds_layout's arguments)
  const int lds_wpool = world_k > 1 && views != 0 ? world_k : 0;
  const bool world_view = views == 1;
  const int max_waves = ((with_step && s.substrate == MPK_SUBSTRATE_THE_MATRIX) ? kMatrixThreads
                                                                                : kDrawThreads) / 64;
  // Renderers: the drawing is the store path's business, and more waves are not
  // better — WORLD.RGB (720-byte rows) is drawn fastest by 8 waves (96 us; 110 us
  // with 12, 113 us with 10, same box), the per-agent views (264-byte rows) by
  // 12-13.  Feeders: a step takes 10-25 us of one wave (a chain of dependent LDS
  // and scalar round trips) and a CU's 16-32 worlds must be fed faster than they
  // are drawn: measured, fused clean_up 259 / 176 / 134 us with 1 / 2 / 4 feeders
  // (profiles/r02_frame_geometry.md, profiles/r02_frame_timeline.md)
  p.nwaves = world_view ? 12 : 16;
  p.feeders = 4;
  int B = 4, NB = 2;
  // per-agent views, fused: batches of three leave the composite cache more LDS
  // and draw faster whatever the box.  Feeders: since round 3 a feeder's later
  // steps run at the renderers' priority and its record reads hit the cache (nt
  // pixel stores); fewer feeders = more drawing waves.  commons_harvest: 313 us
  // with 6 feeders on every box; with 3 (13 drawing waves, four per SIMD) 266 us
  // on one box and 350 on three others — the per-agent drawing is then issue-bound
  // and the fourth wave of a SIMD starves (pass times 4.8 / 5.3 / 5.9 / 7.2 us by
  // wave on a fast CU, 5.6 / 6.5 / 9.5 / 12.6 on a slow one of the same launch):
  // 6 stays.  territory, whose step is 3 x longer: 366 us with 3, 434 with 2 or 6;
  // the matrix level 6 feeders at priority 3 (329 us; 362-397 with 3)
  // (tools/gpu_r03_call10.sh / call13.sh, profiles/r03_frame_plans.md)
  if (with_step && !world_view && max_waves == 16) {
    B = 3;
    p.feeders = s.substrate == MPK_SUBSTRATE_THE_MATRIX ? 6
                : s.substrate == MPK_SUBSTRATE_TERRITORY ? 3
                : 6;
    // small views (the two-player games: under 64 KB of pixels a world): a CU has
    // 64 worlds to step for a few us of drawing each, the stepping is the long
    // pole: batches of 8 and 8 feeders (matrix games: 102 us against 114 in two
    // launches, 125-139 with batches of 4-6, 152 with 4 feeders), 4 feeders for
    // coins' short step (156 us against 190 in two launches, 176 with 8)
    const long long view_bytes = (long long)t.P * (t.vf + t.vb + 1) * (t.vl + t.vr + 1) *
                                 t.sprite_size * t.sprite_size * 3;
    // (round 5: the 40 x 40 views of two players — collaborative_cooking's small kitchens,
    // 9.6 KB a world — leave the renderers next to nothing to do: 8 feeders 26.0 us, 4 feeders
    // 36.7; the nine-player kitchen, 43 KB a world, is indifferent, 60.7 / 61.1:
    // tools/history/gpu_r05_call17.sh)
    if (view_bytes < 64 * 1024 && views == 0) {
      B = 8;
      p.feeders = (s.substrate == MPK_SUBSTRATE_THE_MATRIX || view_bytes < 16 * 1024) ? 8 : 4;
    } else if (view_bytes < 150 * 1024 && views == 0 && s.substrate != MPK_SUBSTRATE_THE_MATRIX &&
               s.substrate != MPK_SUBSTRATE_TERRITORY) {
      // (round 5: five or six viewers of 88 x 88 — coop_mining, gift_refinements,
      // externality_mushrooms.  Batches of 4 with 4 feeders: 4096 worlds are then 256
      // workgroups x 4 batches, where batches of 3 are 228 x 6 and leave 28 CUs idle; same
      // buffers, tools/history/gpu_r05_call28.sh: 111.6 against 130.2 - 132.0 us, 112.8 against
      // 121.4 - 126.1, 104.7 against 114.6 - 115.8; clean_up's seven viewers: 146.6 against 145.1)
      B = 4;
      p.feeders = 4;
    }
  }
  // The same for what `substrate.build` binds on the small substrates (round 5, same buffers,
  // tools/history/gpu_r05_call20.sh): BOTH views with per-agent views under 45 KB a world —
  // batches of 8 and 8 feeders: collaborative_cooking cramped 45.5 -> 34.7 us, crowded 97.7 ->
  // 87.8, prisoners_dilemma repeated 106.4 -> 88.1 (coins, 46.5 KB: 93.2 -> 100.3, stays); and
  // WORLD.RGB alone under 16 KB a world (the two-player kitchens): 34.8 -> 26.2 (the matrix
  // games' and coins' world views are 66 KB and more: 74.9 -> 123, 53.3 -> 90 — they stay)
  if (with_step && max_waves == 16) {
    const long long agent_bytes = (long long)t.P * (t.vf + t.vb + 1) * (t.vl + t.vr + 1) *
                                  t.sprite_size * t.sprite_size * 3;
    const long long world_bytes = (long long)t.H * t.W * t.sprite_size * t.sprite_size * 3;
    if ((views == 2 && agent_bytes < 45 * 1024) || (views == 1 && world_bytes < 16 * 1024)) {
      B = 8;
      p.feeders = 8;
    } else if (views == 1 && world_bytes < 64 * 1024) {
      // WORLD.RGB alone, 16 - 64 KB a world (the two larger kitchens, externality_mushrooms):
      // still the stepping that takes the time — 16 waves, half of them feeders (same
      // buffers, tools/history/gpu_r05_call33.sh: crowded 54.6 -> 39.9 us, figure_eight
      // 48.2 -> 37.4 with batches of 8; externality_mushrooms, 62 KB, 73.9 -> 67.8 with 6)
      B = world_bytes < 32 * 1024 ? 8 : 6;
      p.feeders = B;
      p.nwaves = 16;
    }
  }
  if (p.nwaves > max_waves) p.nwaves = max_waves;
  p.slot_scratch = with_step ? slot_scratch_bytes(t, s) : 0;
  if (num_cus <= 0) num_cus = 1;
  // feeders after their first world: back to the renderers' priority, except for
  // the long steps (territory 433 us at priority 0, 371 us at 3; clean_up 119 -> 115,
  // commons 327 -> 309 the other way round)
  p.late_prio = (s.substrate == MPK_SUBSTRATE_TERRITORY || s.substrate == MPK_SUBSTRATE_THE_MATRIX) ? 3 : 0;
  int static_pct = 100;
  // test / development overrides (MpConfig.dev: test_frame_geometry_edge_cases,
  // tools/gpu_plan_sweep.sh); NULL in product paths
  if (dev) {
    if (dev->late_feeder_prio > 0) p.late_prio = dev->late_feeder_prio - 1;
    if (dev->batch_worlds > 0) B = dev->batch_worlds;
    if (dev->ring_batches > 0) NB = dev->ring_batches;
    if (dev->waves > 0) p.nwaves = dev->waves;
    if (dev->feeders > 0) p.feeders = dev->feeders;
    if (dev->max_groups > 0 && dev->max_groups < num_cus) num_cus = dev->max_groups;
    if (dev->static_pct > 0) static_pct = dev->static_pct > 100 ? 100 : dev->static_pct;
  }
  if (p.nwaves < (views == 2 ? 3 : 2)) p.nwaves = views == 2 ? 3 : 2;   // a feeder + a renderer per view
  if (p.nwaves > max_waves) p.nwaves = max_waves;
  if (B > kMaxBatch) B = kMaxBatch;
  if (B > num_worlds) B = num_worlds;
  if (NB < 2) NB = 2;
  while (NB * B > kMaxSlots && NB > 2) --NB;
  // F divides the ring (NB * B slots), leaves a wave to draw, and its claim chains
  // (A = F / gcd(F, B)) fit the buffers: a buffer serves ONE chain (A divides NB)
  auto fit_feeders = [&]() {
    if (p.feeders > NB * B) p.feeders = NB * B;
    if (p.feeders > p.nwaves - (views == 2 ? 2 : 1)) p.feeders = p.nwaves - (views == 2 ? 2 : 1);
    for (; p.feeders > 1; --p.feeders) {
      const int chains = p.feeders / gcd_int(p.feeders, B);
      if ((NB * B) % p.feeders == 0 && NB % chains == 0 && chains <= kMaxChains) break;
    }
  };
  fit_feeders();
  while (frame_lds_layout(t, NB * B, p.feeders, p.nwaves, p.slot_scratch, lds_pool, lds_wpool).total > 160 * 1024) {
    if (NB > 2) --NB;
    else if (B > 1) --B;
    else break;
    fit_feeders();
  }
  // (a developer override of the staging area can still be too big: fewer waves)
  while (p.nwaves > 4 &&
         frame_lds_layout(t, NB * B, p.feeders, p.nwaves, p.slot_scratch, lds_pool, lds_wpool).total > 160 * 1024) {
    --p.nwaves;
    fit_feeders();
  }
  p.B = B;
  p.NB = NB;
  p.store_sc1 = (dev && dev->store_sc1 > 0) ? 1 : 0;
  p.pace = (dev && dev->pace > 0) ? dev->pace - 1 : 0;
  p.team = 0;   // (set below, once the split is known)
  p.head = with_step ? kStockHead : 0;
  if (with_step && dev && dev->head > 0) p.head = (dev->head - 1) & 1;
  // two views: the renderer waves are shared out by the bytes each view writes
  p.world_waves = 0;
  if (views == 2) {
    const int renderers = p.nwaves - p.feeders;
    const long long wb = (long long)t.H * t.W, ab = (long long)t.P * (t.vf + t.vb + 1) * (t.vl + t.vr + 1);
    int ww = (int)((renderers * wb + (wb + ab) / 2) / (wb + ab));
    if (dev && dev->world_waves > 0) ww = dev->world_waves;
    if (ww < 1) ww = 1;
    if (ww > renderers - 1) ww = renderers - 1;
    p.world_waves = ww;   // (fit_feeders leaves two renderers: one per view at least)
  }
  // the worlds: an even split of whole batches over the workgroups (whole batches,
  // except in the last workgroup: territory 249 workgroups x 33 worlds rather than
  // 256 x 32 with a partial eleventh batch each: measured, 408 vs 414 us; filling all
  // 256 CUs instead — commons_harvest 256 x 16 with a ragged sixth batch rather than
  // 228 x 18 — is 6 % SLOWER over eight buffers, profiles/r03_buffer_placement.md) —
  // or (static_pct < 100) a smaller even split and the rest in the pool
  const int nbt = (num_worlds + B - 1) / B;
  int groups = nbt < num_cus ? nbt : num_cus;
  const int fair = (nbt + groups - 1) / groups;
  const int chains = p.feeders / gcd_int(p.feeders, B);
  int ks = fair;
  if (static_pct < 100) {
    ks = fair * static_pct / 100;
    if (ks < chains) ks = chains;   // a chain's first claim rides on an owned batch
  }
  if (ks >= fair) {
    p.ks = fair;
    p.groups = (nbt + fair - 1) / fair;
    p.pool = 0;
  } else {
    p.ks = ks;
    p.groups = groups;              // every CU: nbt >= groups * fair - (groups - 1) > groups * ks
    if ((long long)p.groups * ks > nbt) p.groups = nbt / ks;
    p.pool = nbt - p.groups * ks;
  }
  // XCD teams (MpDevOptions.team; mp_tune times it as a candidate): single-world batches, nothing
  // pooled (a pass then never spans two worlds of a batch that do not lie next to each other)
  if (dev && dev->team > 0 && p.B == 1 && p.pool == 0) p.team = 1;
  return p;
}

// (pool_k / world_k: as plan_frame's, for a plan of the view(s) that `views` names)
int frame_lds_bytes(const DevTables& t, const FramePlan& p, int pool_k, int world_k, int views) {
  return frame_lds_layout(t, p.NB * p.B, p.feeders, p.nwaves, p.slot_scratch,
                          pool_k > 1 && views != 1 ? pool_k : 0, world_k > 1 && views != 0 ? world_k : 0)
      .total;
}

// The world-independent part of a workgroup's LDS image (bytes [0, world) of
// frame_lds_layout), built once on the host.  `sprite_flags8`, `state_sprite`,
// `state_player`, `view_sprite_map`, `state_orient`, `img_slot`, `images` and
// `pair_table` are host copies of the tables of the same names.
int render_blob_bytes(const DevTables& t) { return frame_lds_layout(t, 1, 1, 1, 0).world; }

void build_render_blob(const DevTables& t, const uint8_t* images, const uint16_t* img_slot,
                       const uint32_t* pair_table, const int32_t* state_sprite,
                       const int8_t* state_player, const int32_t* view_sprite_map,
                       const uint8_t* sprite_flags8, const int32_t* state_orient,
                       uint8_t* blob) {
  const FrameLds lo = frame_lds_layout(t, 1, 1, 1, 0);
  memset(blob, 0, (size_t)lo.world);
  for (int i = 0; i < t.n_images; ++i)
    memcpy(blob + lo.atlas + (size_t)i * kSpriteStride, images + (size_t)i * 256, 256);
  uint16_t* sinfo = reinterpret_cast<uint16_t*>(blob + lo.sinfo);   // sprite | (player+1) << 8
  uint16_t* rinfo = reinterpret_cast<uint16_t*>(blob + lo.rinfo);   // remapped sprite | flags << 8
  uint16_t* slot = reinterpret_cast<uint16_t*>(blob + lo.slot);     // atlas image of (sprite, facing)
  uint16_t* stab = reinterpret_cast<uint16_t*>(blob + lo.stab);     // entry of (facing, state)
  uint32_t* pairs = reinterpret_cast<uint32_t*>(blob + lo.pairs);
  for (int s = 0; s < 256; ++s) {
    const int sp = s < t.nstates ? state_sprite[s] : -1;
    const int pl = s < t.nstates ? state_player[s] : -1;
    sinfo[s] = (uint16_t)((sp < 0 ? 0xff : sp) | ((pl + 1) << 8));
  }
  for (int i = 0; i < (t.P + 1) * t.nsprites; ++i) {
    const int sp = view_sprite_map[i];
    rinfo[i] = (uint16_t)(sp | ((sprite_flags8[sp] & 3) << 8));
  }
  for (int i = 0; i < t.nsprites * 4; ++i) slot[i] = img_slot[i];
  // state -> entry under the world sprite map, per relative facing; avatar
  // states are resolved per viewer (own orientation, Self remap) in phase 1
  for (int i = 0; i < 4 * 256; ++i) {
    const int f = i >> 8, st = i & 255;
    uint32_t e = 0;
    if (st < t.nstates && state_sprite[st] >= 0) {
      if (state_player[st] >= 0) {
        e = kAvatarBit | (uint32_t)st;
      } else {
        const int sp = view_sprite_map[t.P * t.nsprites + state_sprite[st]];
        // (a beam pseudo-state of an oriented sprite carries its own facing)
        e = ((uint32_t)(sprite_flags8[sp] & 3) << 10) | img_slot[sp * 4 + ((f + state_orient[st]) & 3)];
        // a sprite without a visible pixel (territory's level-1 marking) draws nothing
        if (sprite_flags8[sp] & 4) e = 0;
      }
    }
    stab[i] = (uint16_t)e;
  }
  for (int i = 0; i < kPairSlots; ++i) pairs[i] = pair_table[i];
  // what a cell beyond the map shows to viewer v: its OutOfBounds sprite (sprite 0 under its
  // sprite map), facing north — one look-up in phase 1 instead of two dependent ones
  uint16_t* oobimg = reinterpret_cast<uint16_t*>(blob + lo.oobimg);
  for (int v = 0; v <= t.P; ++v) oobimg[v] = slot[(rinfo[v * t.nsprites] & 255u) << 2];
}


// DevTables::vis_layers from the blob's state table: bit l = some state of render plane l has
// an entry (a sprite with a visible pixel, or an avatar's), bit 16 + l = some state of it is an
// avatar's.  `state_layer` is the host copy of the table of that name.
uint32_t render_visible_layers(const DevTables& t, const uint8_t* blob, const int32_t* state_layer) {
  const FrameLds lo = frame_lds_layout(t, 1, 1, 1, 0);
  const uint16_t* stab = reinterpret_cast<const uint16_t*>(blob + lo.stab);
  uint32_t vis = 0;
  for (int st = 0; st < t.nstates && st < 256; ++st) {
    const int l = state_layer[st];
    if (l < 0 || l >= t.L || l >= kMaxLayers) continue;
    for (int f = 0; f < 4; ++f) {
      const uint32_t e = stab[f * 256 + st];
      if (e != 0) vis |= 1u << l;
      if (e & kAvatarBit) vis |= 1u << (16 + l);
    }
  }
  return vis;
}

namespace {

template <class Tables, class Sites, int kPool>
void launch_pooled(const DevTables& t, const Tables& c, const stepk::StepArgs& args, uint8_t* out_a,
                   uint8_t* out_w, const FramePlan& p, hipStream_t stream) {
  FrameConsts K = frame_consts(t, p, args.num_worlds, !std::is_same<Tables, NoTables>::value, kPool);
  const size_t lds = (size_t)K.lo.total;
  if (out_w) {
    K.npb_all = K.npb[0] + K.npb[1];
    hipLaunchKernelGGL((k_frame<Tables, Sites, 2, kPool>), dim3(p.groups), dim3(p.nwaves * 64), lds,
                       stream, t, c, args, out_a, out_w, K);
  } else {
    K.npb_all = K.npb[0];
    hipLaunchKernelGGL((k_frame<Tables, Sites, 0, kPool>), dim3(p.groups), dim3(p.nwaves * 64), lds,
                       stream, t, c, args, out_a, out_w, K);
  }
}

// pool_k > 1: out_a is the per-agent view pooled by pool_k (MP_OBS_RGB_POOL*)
template <class Tables, class Sites>
void launch_one(const DevTables& t, const Tables& c, const stepk::StepArgs& args, uint8_t* out_a,
                uint8_t* out_w, const FramePlan& p, hipStream_t stream, int pool_k) {
  if (out_a && pool_k > 1) {
    if (pool_k == 2) launch_pooled<Tables, Sites, 2>(t, c, args, out_a, out_w, p, stream);
    else if (pool_k == 4) launch_pooled<Tables, Sites, 4>(t, c, args, out_a, out_w, p, stream);
    else launch_pooled<Tables, Sites, 8>(t, c, args, out_a, out_w, p, stream);
    return;
  }
  FrameConsts K = frame_consts(t, p, args.num_worlds, !std::is_same<Tables, NoTables>::value, 0);
  const size_t lds = (size_t)K.lo.total;
  if (out_a && out_w) {
    K.npb_all = K.npb[0] + K.npb[1];
    hipLaunchKernelGGL((k_frame<Tables, Sites, 2>), dim3(p.groups), dim3(p.nwaves * 64), lds,
                       stream, t, c, args, out_a, out_w, K);
  } else if (out_w) {
    K.npb_all = K.npb[1];
    hipLaunchKernelGGL((k_frame<Tables, Sites, 1>), dim3(p.groups), dim3(p.nwaves * 64), lds,
                       stream, t, c, args, out_a, out_w, K);
  } else {
    K.npb_all = K.npb[0];
    hipLaunchKernelGGL((k_frame<Tables, Sites, 0>), dim3(p.groups), dim3(p.nwaves * 64), lds,
                       stream, t, c, args, out_a, out_w, K);
  }
}

template <class Tables, class Sites>
int allow_lds() {
  const void* k[9] = {
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 0>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 1>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 0, 2>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 2>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 0, 4>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 4>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 0, 8>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 8>)};
  hipError_t r[9];
  for (int i = 0; i < 9; ++i)
    r[i] = hipFuncSetAttribute(k[i], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  for (hipError_t e : r)
    if (e != hipSuccess) return (int)e;
  return 0;
}

}  // namespace

// frame_stock.hip: the clean_up kernels with the committed pack's constants compiled in
int prepare_frame_stock();
void launch_frame_stock(const DevTables& t, const CleanUpTables& c, const stepk::StepArgs& args,
                        uint8_t* out_a, uint8_t* out_w, const FramePlan& p, hipStream_t stream);

// The frame kernels use up to 160 KB of dynamic LDS; declare it (a no-op where
// the runtime grants it anyway).  Called once per engine, with its device current.
int prepare_frame() {
  int rc = prepare_frame_wpool<2>();
  if (!rc) rc = prepare_frame_stock();
  if (!rc) rc = prepare_frame_wpool<4>();
  if (!rc) rc = prepare_frame_wpool<8>();
  if (!rc) rc = allow_lds<NoTables, NoSites>();
  if (!rc) rc = allow_lds<CleanUpTables, stepk::CleanUpSites>();
#if !defined(MP_FRAME_ISA_SUBSET)
  if (!rc) rc = allow_lds<CommonsTables, stepk::CommonsSites>();
  if (!rc) rc = allow_lds<TerritoryTables, stepk::TerritorySites>();
  if (!rc) rc = allow_lds<CoinsTables, stepk::CoinsSites>();
  if (!rc) rc = allow_lds<MatrixTables, stepk::MatrixSites>();
  if (!rc) rc = allow_lds<CoopTables, stepk::CoopSites>();
  if (!rc) rc = allow_lds<GiftTables, stepk::GiftSites>();
  if (!rc) rc = allow_lds<CookTables, stepk::CookSites>();
  if (!rc) rc = allow_lds<MushroomTables, stepk::MushroomSites>();
#endif
  return rc;
}

// One launch: the views `out_a` (per-agent RGB) and / or `out_w` (WORLD.RGB) of all
// worlds — from the records in HBM (s == NULL: mp_observe, views of a reset that
// names no world ...), or stepped first (one environment step or reset of all worlds
// + the views of the result).  `p` is the plan for exactly these views; p.parity
// alternates between consecutive frame launches of an engine (DevTables::claim).
// pool_k > 1: `out_a` is the per-agent view pooled by that factor (2, 4, 8); world_k > 1: `out_w`
// is WORLD.RGB pooled by that factor (the instantiations of frame_wpool<k>.hip).  The pooled
// views and the draw-only launch have no stock form.
void launch_frame(const DevTables& t, const SubstrateTables* s, const stepk::StepArgs& args,
                  uint8_t* out_a, uint8_t* out_w, const FramePlan& p, hipStream_t stream, int pool_k,
                  int world_k) {
  if (out_w && world_k > 1) {
    if (world_k == 2) launch_frame_wpool<2>(t, s, args, out_a, out_w, p, stream, pool_k);
    else if (world_k == 4) launch_frame_wpool<4>(t, s, args, out_a, out_w, p, stream, pool_k);
    else launch_frame_wpool<8>(t, s, args, out_a, out_w, p, stream, pool_k);
    return;
  }
  if (!s) {
    launch_one<NoTables, NoSites>(t, NoTables(), args, out_a, out_w, p, stream, pool_k);
    return;
  }
  // the committed pack (mp_create: SubstrateTables::stock), full views: its constants compiled in
  if (s->stock == MP_KERNEL_STOCK && s->substrate == MPK_SUBSTRATE_CLEAN_UP && !(out_a && pool_k > 1)) {
    launch_frame_stock(t, s->cu, args, out_a, out_w, p, stream);
    return;
  }
#if defined(MP_FRAME_ISA_SUBSET)
  // developer build (tools/isa_stats.sh quick): the draw-only and the clean_up kernels alone
  if (s->substrate == MPK_SUBSTRATE_CLEAN_UP)
    launch_one<CleanUpTables, stepk::CleanUpSites>(t, s->cu, args, out_a, out_w, p, stream, pool_k);
#else
  switch (s->substrate) {
    case MPK_SUBSTRATE_CLEAN_UP:
      launch_one<CleanUpTables, stepk::CleanUpSites>(t, s->cu, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COMMONS_HARVEST:
      launch_one<CommonsTables, stepk::CommonsSites>(t, s->ch, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_TERRITORY:
      launch_one<TerritoryTables, stepk::TerritorySites>(t, s->tr, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COINS:
      launch_one<CoinsTables, stepk::CoinsSites>(t, s->co, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_THE_MATRIX:
      launch_one<MatrixTables, stepk::MatrixSites>(t, s->mx, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COOP_MINING:
      launch_one<CoopTables, stepk::CoopSites>(t, s->cm, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_GIFT_REFINEMENTS:
      launch_one<GiftTables, stepk::GiftSites>(t, s->gr, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING:
      launch_one<CookTables, stepk::CookSites>(t, s->cc, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS:
      launch_one<MushroomTables, stepk::MushroomSites>(t, s->em, args, out_a, out_w, p, stream, pool_k);
      break;
  }
#endif
}
