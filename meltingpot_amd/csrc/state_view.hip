// state_view.hip — sampled (row, player) views of a bank of saved records (an MpStatesView
// request, include/mp_engine.h): element i of the destination is ONE player's view of ONE row,
// read from the row where it lies.  No world is loaded, no row is copied aside, nothing of the
// engine's is written.  A unit of its own: k_frame, the step kernels and state_obs.hip compile
// to exactly the assembly they compiled to before (profiles/r20_observe_views.md).
//
//   k_view_scalar   READY_TO_SHOOT, POSITION, ORIENTATION, INVENTORY: one thread per element, by
//                   k_state_obs's rules (state_obs_rules.h);
//   k_state_view    LAYER and the pixel kinds: one wave per view.  The wave stages what a view needs
//                   of its record in LDS — the render planes and the head of the tail (positions,
//                   orientations, who is alive), 16-byte loads, eight of a lane in flight — and
//                   draws the view strip by strip: a strip is one row of view cells (VW <= 64:
//                   lane = cell resolves the cell's draw list as k_frame's phase 1 does, from the
//                   same tables — DevTables::render_blob, staged once per workgroup), composed in
//                   the wave's LDS scratch (eight lanes a cell, one per pixel row, with k_frame's
//                   blend_row) and stored as the contiguous bytes it is: the 16-byte lines inside
//                   it lane-contiguous (1 KiB a wave store), the bytes before the first and behind
//                   the last line one byte a lane.  A pooled kind reduces every composited cell
//                   (k x k box average, rounded half up) before it is put into the strip; the
//                   composite cache (pair_table) is not consulted: a cell's overlays are blended
//                   where k_frame may take a pre-blended image, to the same pixels.
//                   Sprite look-ups are k_frame's: a piece that is no avatar shows the sprite the
//                   world's sprite map gives it, an avatar the one the VIEWER's map gives it.
// An index of rows[] outside the bank or of players[] outside [0, P) is never used as one: its
// element of the destination stays as it was — every such element — and ONE of them is reported
// through the fault words (FAULT_STATE_INDEX; the first to claim them, so position, value and
// kind of index belong together).
#include <stddef.h>

#include "frame_kernel.h"
#include "state_obs_rules.h"
#include "state_view.h"

namespace {

using namespace stepk;

constexpr int kViewLdsMax = 160 * 1024;
static_assert(offsetof(WorldTail, aalive) + MP_MAX_PLAYERS == kHeadBytes && offsetof(WorldTail, ax) == 0,
              "the staged head of the tail is ax, ay, aori, aalive");
constexpr int kViewMaxWaves = 16;

struct ViewArgs {
  const uint8_t* bank;
  const int32_t* rows;
  const int32_t* players;
  uint8_t* dst;
  const int32_t* layer_lut;
  int32_t bank_rows, count, waves;
  int32_t blob_bytes;               // the render blob in front of the waves' areas (0: LAYER)
  int32_t planes_vec;               // 16-byte vectors of the L render planes
  int32_t per_wave;                 // a wave's LDS: draw lists, record part, strip
  int32_t sinfo, rinfo, slot, stab, oobimg;   // frame_lds_layout's offsets inside the blob
  uint32_t view_bytes, strip_bytes;           // of one element, of one row of view cells
  int32_t nvis;                     // the render planes that can show anything, bottom -> top:
  uint32_t plane_off[6];            // each one's byte offset in a record, two u16 per word
};

__device__ inline void report_view_index(const DevTables& t, int lane, int at, int index, uint32_t what) {
  if (lane == 0 && atomicCAS(&t.fault[FAULT_STATE_INDEX], 0u, (uint32_t)at + 1u) == 0u) {
    t.fault[FAULT_STATE_INDEX + 1] = (uint32_t)index;
    t.fault[FAULT_STATE_INDEX + 2] = what;
  }
}

template <class Tables>
__global__ __launch_bounds__(256) void k_view_scalar(DevTables t, Tables c, int kind,
                                                     const uint8_t* __restrict__ bank, int bank_rows,
                                                     const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ players, int count,
                                                     void* __restrict__ dst) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= count) return;
  const int r = rows ? rows[i] : i, p = players[i];
  if (r < 0 || r >= bank_rows) { report_view_index(t, 0, i, r, kFaultViewRow); return; }
  if (p < 0 || p >= t.P) { report_view_index(t, 0, i, p, kFaultViewPlayer); return; }
  const uint8_t* rec = bank + (size_t)r * t.world_stride;
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
  const size_t o = (size_t)i;
  switch (kind) {
    case MP_OBS_READY_TO_SHOOT: static_cast<double*>(dst)[o] = ready_of(c, tail, p); break;
    case MP_OBS_POSITION:
      static_cast<int32_t*>(dst)[o * 2 + 0] = tail->ax[p];
      static_cast<int32_t*>(dst)[o * 2 + 1] = tail->ay[p];
      break;
    case MP_OBS_ORIENTATION: static_cast<int32_t*>(dst)[o] = tail->aori[p]; break;
    case MP_OBS_INVENTORY: {
      const int n = inventory_classes(c), held = inventory_held(c);
      for (int k = 0; k < held; ++k) static_cast<double*>(dst)[o * n + k] = inventory_of(t, c, rec, p, k);
      break;
    }
    default: break;
  }
}

// kPix pixels (0x00BBGGRR each) -> their 3 * kPix packed bytes as words, low byte first.
template <int kPix>
__device__ inline void pack_pixels(const uint32_t* px, uint32_t* w) {
#pragma unroll
  for (int j = 0; j < (kPix * 3 + 3) / 4; ++j) w[j] = 0u;
#pragma unroll
  for (int i = 0; i < kPix * 3; ++i) w[i >> 2] |= ((px[i / 3] >> (8 * (i % 3))) & 255u) << (8 * (i & 3));
}
// ... put at `d` in LDS, which is a multiple of kBytes past a 16-byte line + `al` (wave-uniform:
// the strip is staged at the offset inside a line that it has in the destination, and a view
// starts on any byte): words where that is 4-byte aligned, halves or bytes where it is not.
template <int kBytes>
__device__ inline void lds_put(uint8_t* d, const uint32_t* w, uint32_t al) {
  if (kBytes % 4 == 0 && (al & 3u) == 0u) {
#pragma unroll
    for (int j = 0; j < kBytes / 4; ++j) reinterpret_cast<uint32_t*>(d)[j] = w[j];
  } else if (kBytes % 2 == 0 && (al & 1u) == 0u) {
#pragma unroll
    for (int j = 0; j < kBytes / 2; ++j)
      reinterpret_cast<uint16_t*>(d)[j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
  } else {
#pragma unroll
    for (int j = 0; j < kBytes; ++j) d[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

// `len` bytes staged at `pst` (same offset inside a 16-byte line as g0) -> g0 .. g0 + len, and
// nothing outside: the neighbouring bytes are other views'.
__device__ inline void store_span(uint8_t* g0, const uint8_t* pst, uint32_t len, int lane) {
  const uint32_t lead = (16u - ((uint32_t)(uintptr_t)g0 & 15u)) & 15u;
  const uint32_t head = lead < len ? lead : len;
  const uint32_t nch = len > lead ? (len - lead) >> 4 : 0u;
  const uint32_t tail0 = lead + nch * 16u;
  uint4* gq = reinterpret_cast<uint4*>(g0 + lead);
  for (uint32_t q = (uint32_t)lane; q < nch; q += 64u)
    gq[q] = *reinterpret_cast<const uint4*>(pst + lead + q * 16u);
  const uint32_t tb = tail0 + (uint32_t)lane - 16u;
  if ((uint32_t)lane < head) g0[lane] = pst[lane];
  else if (lane >= 16 && lane < 32 && tb < len) g0[tb] = pst[tb];
}

template <int kMode>   // 0: LAYER; 1: RGB; 2, 4, 8: RGB pooled by that factor
__global__ __launch_bounds__(kViewMaxWaves * 64) void k_state_view(DevTables t, ViewArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = t.W, H = t.H, HW = t.H * t.W, P = t.P;
  const int VW = t.vl + t.vr + 1, VH = t.vf + t.vb + 1;

  if constexpr (kMode != 0) {
    // the tables, once per workgroup (eight loads in flight per thread, as k_frame copies them)
    const uint4* src = reinterpret_cast<const uint4*>(t.render_blob);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    const int n = a.blob_bytes >> 4, nthr = a.waves * 64;
    for (int i = tid; i < n; i += 8 * nthr) {
      uint4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = src[min(i + k * nthr, n - 1)];
#pragma unroll
      for (int k = 0; k < 8; ++k) issued(v[k]);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (i + k * nthr < n) dst[i + k * nthr] = v[k];
    }
    __syncthreads();
  }
  const uint8_t* atlas = smem;
  const uint16_t* sinfo = reinterpret_cast<const uint16_t*>(smem + a.sinfo);   // sprite | (player+1) << 8
  const uint16_t* rinfo = reinterpret_cast<const uint16_t*>(smem + a.rinfo);   // remapped sprite | flags << 8
  const uint16_t* slot = reinterpret_cast<const uint16_t*>(smem + a.slot);     // atlas image of (sprite, facing)
  const uint16_t* stab = reinterpret_cast<const uint16_t*>(smem + a.stab);     // entry of (facing, state)
  const uint16_t* oobimg = reinterpret_cast<const uint16_t*>(smem + a.oobimg);

  uint8_t* const wbase = smem + a.blob_bytes + wave * a.per_wave;
  CellRec* const recs = reinterpret_cast<CellRec*>(wbase);   // [64] draw lists of a strip's cells
  uint8_t* const grid = wbase + 64 * sizeof(CellRec);        // the render planes ...
  uint8_t* const head = grid + a.planes_vec * 16;            // ... ax[16] ay[16] aori[16] aalive[16]
  uint8_t* const strip = head + kHeadBytes;
  const int py = lane & 7, sub = lane >> 3;
  const uint32_t strip_bytes = a.strip_bytes;

  for (int i = (int)blockIdx.x * a.waves + wave; i < a.count; i += (int)gridDim.x * a.waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    const int p = __builtin_amdgcn_readfirstlane(a.players[i]);
    if (r < 0 || r >= a.bank_rows) { report_view_index(t, lane, i, r, kFaultViewRow); continue; }
    if (p < 0 || p >= P) { report_view_index(t, lane, i, p, kFaultViewPlayer); continue; }
    wsync();   // (the view before this one has left the wave's LDS)
    {
      const uint4* src = reinterpret_cast<const uint4*>(a.bank + (size_t)r * t.world_stride);
      uint4* out = reinterpret_cast<uint4*>(grid);
      const int nvec = a.planes_vec;
      const uint4 hv = lane < kHeadBytes / 16 ? src[(t.grid_pad >> 4) + lane] : uint4{0u, 0u, 0u, 0u};
      for (int i0 = 0; i0 < nvec; i0 += 8 * 64) {
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int j = i0 + k * 64 + lane;
          v[k] = src[j < nvec ? j : nvec - 1];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) issued(v[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int j = i0 + k * 64 + lane;
          if (j < nvec) out[j] = v[k];
        }
      }
      if (lane < kHeadBytes / 16) reinterpret_cast<uint4*>(head)[lane] = hv;
    }
    wsync();

    const bool on_grid = head[48 + p] != 0;   // A6: an off-grid viewer sees only OutOfBounds
    const int hx = head[p], hy = head[16 + p];
    uint8_t* const gview = a.dst + (size_t)i * a.view_bytes;
    const int cx = lane;
    const bool live = cx < VW;

    if constexpr (kMode == 0) {
      // "N.LAYER": the window is not turned with the avatar; write_layer's value function
      // (stepk::layer_value) for this one viewer.  Of the tail only its head is staged: the
      // positions and who is alive, which is all the function reads.
      const uint32_t L = (uint32_t)t.L;
      const LayerWindow g = layer_window(t);
      const WorldTail* tail = reinterpret_cast<const WorldTail*>(head);
      for (int cy = 0; cy < VH; ++cy) {
        uint8_t* const g0 = gview + (size_t)cy * strip_bytes;
        uint8_t* const pst = strip + ((uint32_t)(uintptr_t)g0 & 15u);
        if (live) {
          int32_t* d = reinterpret_cast<int32_t*>(pst) + (uint32_t)cx * L;
          for (uint32_t l = 0; l < L; ++l)
            d[l] = layer_value(t, g, grid, tail, a.layer_lut, (uint32_t)p, (uint32_t)cx, (uint32_t)cy, l);
        }
        wsync();
        store_span(g0, pst, strip_bytes, lane);
        wsync();
      }
    } else {
      constexpr int kPool = kMode;                 // (1: the full view)
      constexpr int kPN = 8 / kPool;               // pixels of a cell's row, rows of a cell
      constexpr int kRowBytes = kPN * 3;
      const uint32_t prow = (uint32_t)VW * (uint32_t)kRowBytes;   // one pixel row of the strip
      const uint32_t vo = on_grid ? (uint32_t)head[32 + p] : 0u;
      const uint32_t oob_img = oobimg[p];
      const uint16_t* rinfo_v = rinfo + p * t.nsprites;           // this viewer's sprite map
      const uint16_t* tf = stab + (((0u - vo) & 3u) << 8);        // pieces other than avatars face north
      const uint8_t* atlas_row = atlas + py * 32;
      for (int cy = 0; cy < VH; ++cy) {
        uint8_t* const g0 = gview + (size_t)cy * strip_bytes;
        const uint32_t al = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(uintptr_t)g0 & 15u));
        uint8_t* const pst = strip + al;
        // ---- lane = cell: the draw list, top -> bottom; a lane is done at its first opaque
        // sprite (everything below is hidden)
        {
          const int dx = cx - t.vl, dy = cy - t.vf;   // right, down in the view's frame
          const int ax = vo == 0u ? dx : vo == 1u ? -dy : vo == 2u ? -dx : dy;
          const int ay = vo == 0u ? dy : vo == 1u ? dx : vo == 2u ? -dy : -dx;
          int x = hx + ax, y = hy + ay;
          bool inside;
          if (t.topology == 1) {
            x = ((x % W) + W) % W;
            y = ((y % H) + H) % H;
            inside = true;
          } else {
            inside = x >= 0 && x < W && y >= 0 && y < H;
          }
          const int cell = live && on_grid && inside ? y * W + x : -1;
          const uint8_t* gp = grid + (cell >= 0 ? cell : 0);
          CellRec rc;
          rc.ov0 = 0; rc.ov1 = 0; rc.ov2 = 0;
          uint32_t base_e = cell < 0 ? oob_img : 0u;   // image 0 is black
          bool done = cell < 0;
          // (one plane after the other: fetching all plane bytes first and all table entries second,
          // as k_frame's resolve does, measured 1 - 3 us slower per launch here)
#pragma unroll
          for (int k = kMaxLayers - 1; k >= 0; --k) {
            if (k >= a.nvis) continue;                 // (wave-uniform)
            uint32_t e = tf[gp[(a.plane_off[k >> 1] >> (16 * (k & 1))) & 0xffffu]];   // tf[0] == 0
            if (e & kAvatarBit) {                      // avatars: own orientation, the viewer's sprite map
              const uint32_t si = sinfo[e & 255u];
              const uint32_t ori = head[32 + (si >> 8) - 1];
              const uint32_t rm = rinfo_v[si & 255u];
              e = ((rm >> 8) << 10) | slot[((rm & 255u) << 2) | ((ori - vo) & 3u)];
            }
            const bool opaque = (e & ((uint32_t)FLAG_OPAQUE << 10)) != 0u;
            base_e = (opaque && !done) ? e : base_e;
            done = done || opaque;
            if (e != 0u && !done) {                    // prepend: the list is kept bottom -> top
              rc.ov2 = (rc.ov2 << 12) | (rc.ov1 >> 20);
              rc.ov1 = (rc.ov1 << 12) | (rc.ov0 >> 20);
              rc.ov0 = (rc.ov0 << 12) | e;
            }
          }
          rc.base = (base_e & 1023u) * kSpriteStride;
          recs[lane] = rc;
        }
        wsync();
        // ---- eight lanes a cell, one per pixel row: the opaque base image's packed row, the
        // overlays blended onto it bottom -> top, the row (or its share of the pooled rows) into
        // the strip
        for (int c = sub; c < VW; c += 8) {
          const CellRec rc = recs[c];
          const uint8_t* row = atlas_row + rc.base;
          const uint4 lo4 = *reinterpret_cast<const uint4*>(row);
          const uint2 hi2 = *reinterpret_cast<const uint2*>(row + 16);
          uint32_t w[6] = {lo4.x, lo4.y, lo4.z, lo4.w, hi2.x, hi2.y};
          uint32_t o0 = rc.ov0, o1 = rc.ov1, o2 = rc.ov2;
          if (kPool != 1 || o0 != 0u) {
            uint32_t acc[8];
            unpack_row(w, acc);
            while (o0 != 0u) {
              const uint32_t e = o0 & 4095u;
              o0 = (o0 >> 12) | (o1 << 20);
              o1 = (o1 >> 12) | (o2 << 20);
              o2 >>= 12;
              const uint8_t* orow = atlas_row + (e & 1023u) * kSpriteStride;
              if ((e >> 10) & FLAG_PARTIAL) blend_row<2>(acc, orow);
              else blend_row<1>(acc, orow);
            }
            if constexpr (kPool == 1) {
              pack_row(acc, w);
            } else {
              // R and B summed in the two 16-bit halves of one word (64 x 255 < 2^16), G alone:
              // the row's groups of k pixels, then the k rows of a pooled row over their lanes
              constexpr uint32_t kHalf = (uint32_t)(kPool * kPool / 2);
              constexpr int kS2 = kPool == 2 ? 2 : kPool == 4 ? 4 : 6;   // / k^2
              uint32_t rb[kPN], gs[kPN];
#pragma unroll
              for (int j = 0; j < kPN; ++j) {
                rb[j] = 0u; gs[j] = 0u;
#pragma unroll
                for (int q = 0; q < kPool; ++q) {
                  rb[j] += acc[j * kPool + q] & 0xff00ffu;
                  gs[j] += (acc[j * kPool + q] >> 8) & 255u;
                }
              }
#pragma unroll
              for (int m = 1; m < kPool; m <<= 1)
#pragma unroll
                for (int j = 0; j < kPN; ++j) {
                  rb[j] += (uint32_t)__shfl_xor((int)rb[j], m);
                  gs[j] += (uint32_t)__shfl_xor((int)gs[j], m);
                }
              uint32_t px[kPN];
#pragma unroll
              for (int j = 0; j < kPN; ++j)
                px[j] = (((rb[j] & 0xffffu) + kHalf) >> kS2) | (((gs[j] + kHalf) >> kS2) << 8) |
                        ((((rb[j] >> 16) + kHalf) >> kS2) << 16);
              pack_pixels<kPN>(px, w);
            }
          }
          if ((py & (kPool - 1)) == 0)
            lds_put<kRowBytes>(pst + (uint32_t)(py / kPool) * prow + (uint32_t)c * (uint32_t)kRowBytes, w, al);
        }
        wsync();   // (the strip is whole in LDS)
        store_span(g0, pst, strip_bytes, lane);
        wsync();
      }
    }
  }
}

template <int kMode>
void launch_mode(const DevTables& t, const ViewArgs& a, int groups, int lds, hipStream_t stream) {
  hipLaunchKernelGGL(k_state_view<kMode>, dim3((unsigned)groups), dim3((unsigned)a.waves * 64u),
                     (size_t)lds, stream, t, a);
}

int mode_of(int kind) {
  return kind == MP_OBS_LAYER ? 0 : kind == MP_OBS_RGB_POOL2 ? 2 : kind == MP_OBS_RGB_POOL4 ? 4
         : kind == MP_OBS_RGB_POOL8 ? 8 : 1;
}

// A launch's arguments but for the request's pointers: the LDS layout and the visible planes.
ViewArgs view_args(const DevTables& t, int kind) {
  ViewArgs a = {};
  const int mode = mode_of(kind);
  const int VW = t.vl + t.vr + 1;
  const FrameLds lo = frame_lds_layout(t, 1, 1, 1, 0);
  a.blob_bytes = mode ? lo.world : 0;
  a.sinfo = lo.sinfo; a.rinfo = lo.rinfo; a.slot = lo.slot; a.stab = lo.stab; a.oobimg = lo.oobimg;
  a.planes_vec = (t.L * t.H * t.W + 15) >> 4;
  const int pn = mode ? 8 / mode : 0;
  a.strip_bytes = mode ? (uint32_t)(VW * pn * pn * 3) : (uint32_t)(VW * t.L * 4);
  a.view_bytes = a.strip_bytes * (uint32_t)(t.vf + t.vb + 1);
  // (the strip is staged at its destination's offset inside a 16-byte line)
  a.per_wave = 64 * (int)sizeof(CellRec) + a.planes_vec * 16 + kHeadBytes + (((int)a.strip_bytes + 16 + 15) & ~15);
  for (int l = 0; l < kMaxLayers && l < t.L; ++l) {
    if (!((t.vis_layers >> l) & 1u)) continue;
    a.plane_off[a.nvis >> 1] |= (uint32_t)(l * t.H * t.W) << (16 * (a.nvis & 1));   // (< 65536: mp_create)
    ++a.nvis;
  }
  return a;
}

}  // namespace

StateViewPlan state_view_plan(const DevTables& t, int kind, int count, int num_cus) {
  const ViewArgs a = view_args(t, kind);
  StateViewPlan p = {};
  p.view_bytes = a.view_bytes;
  int fit = (kViewLdsMax - a.blob_bytes) / a.per_wave;
  if (fit < 1) { p.lds = a.blob_bytes + a.per_wave; return p; }
  if (fit > kViewMaxWaves) fit = kViewMaxWaves;
  // every CU a workgroup before a workgroup gets more waves; four waves at least share one copy
  // of the tables where they fit
  const int cus = num_cus > 0 ? num_cus : 1;
  int waves = (count + cus - 1) / cus;
  if (waves < 4) waves = 4;
  if (waves > fit) waves = fit;
  if (waves > count) waves = count;
  p.waves = waves;
  p.groups = (count + waves - 1) / waves;
  if (p.groups > 2 * cus) p.groups = 2 * cus;   // (a wave then draws several views in turn)
  p.lds = a.blob_bytes + waves * a.per_wave;
  return p;
}

void launch_state_view(const DevTables& t, const StateViewPlan& plan, int kind, const uint8_t* bank,
                       int bank_rows, const int32_t* rows, const int32_t* players, int count,
                       void* dst, const int32_t* layer_lut, hipStream_t stream) {
  ViewArgs a = view_args(t, kind);
  a.bank = bank; a.rows = rows; a.players = players; a.dst = static_cast<uint8_t*>(dst);
  a.layer_lut = layer_lut;
  a.bank_rows = bank_rows; a.count = count; a.waves = plan.waves;
  switch (mode_of(kind)) {
    case 0: launch_mode<0>(t, a, plan.groups, plan.lds, stream); break;
    case 1: launch_mode<1>(t, a, plan.groups, plan.lds, stream); break;
    case 2: launch_mode<2>(t, a, plan.groups, plan.lds, stream); break;
    case 4: launch_mode<4>(t, a, plan.groups, plan.lds, stream); break;
    default: launch_mode<8>(t, a, plan.groups, plan.lds, stream); break;
  }
}

void launch_state_view_scalar(const DevTables& t, const SubstrateTables& s, int kind,
                              const uint8_t* bank, int bank_rows, const int32_t* rows,
                              const int32_t* players, int count, void* dst, hipStream_t stream) {
  const dim3 grid((unsigned)((count + 255) / 256)), block(256);
#define MP_LAUNCH(tables)                                                                          \
  hipLaunchKernelGGL(k_view_scalar, grid, block, 0, stream, t, tables, kind, bank, bank_rows, rows, \
                     players, count, dst);                                                          \
  break;
  switch (s.substrate) {
    case MPK_SUBSTRATE_CLEAN_UP: MP_LAUNCH(s.cu)
    case MPK_SUBSTRATE_COMMONS_HARVEST: MP_LAUNCH(s.ch)
    case MPK_SUBSTRATE_COINS: MP_LAUNCH(s.co)
    case MPK_SUBSTRATE_TERRITORY: MP_LAUNCH(s.tr)
    case MPK_SUBSTRATE_THE_MATRIX: MP_LAUNCH(s.mx)
    case MPK_SUBSTRATE_COOP_MINING: MP_LAUNCH(s.cm)
    case MPK_SUBSTRATE_GIFT_REFINEMENTS: MP_LAUNCH(s.gr)
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING: MP_LAUNCH(s.cc)
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS: MP_LAUNCH(s.em)
  }
#undef MP_LAUNCH
}

int prepare_state_view() {
  const void* k[5] = {reinterpret_cast<const void*>(&k_state_view<0>), reinterpret_cast<const void*>(&k_state_view<1>),
                      reinterpret_cast<const void*>(&k_state_view<2>), reinterpret_cast<const void*>(&k_state_view<4>),
                      reinterpret_cast<const void*>(&k_state_view<8>)};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kViewLdsMax);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
