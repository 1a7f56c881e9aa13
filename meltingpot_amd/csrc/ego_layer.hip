// ego_layer.hip — EGO_LAYER (an MpEgoLayer request, include/mp_engine.h): the layer view in the
// avatar's own frame, drawn from records where they lie — bank rows or the engine's worlds.  No
// world is loaded, nothing of the engine's is written.  A unit of its own: k_frame, the step
// kernels, state_obs.hip and state_view.hip compile to exactly what they compiled to before.
//
//   k_ego_layer_rows    every viewer of a row: one wave per row, the row's contiguous
//                       [P][VH][VW][L] block (the registered leaf; a draw without players);
//   k_ego_layer_views   one viewer of a row: one wave per (row, player), its [VH][VW][L] block.
// Both are one body.  The wave stages what the value function reads of its record in LDS — the
// render planes and the head of the tail (positions, orientations, who is alive), 16-byte loads,
// eight of a lane in flight (state_view.hip, step_load.h) — and writes its block with
// write_layer's store scheme (step_common.h): up to three dwords before the block's first 16-byte
// boundary, 16-byte lane-contiguous chunks with four of a lane's values worked out before the
// first store, then up to three dwords.  A dword's (viewer, window cell, layer) is split from its
// index with magic_of / div_by; its value is ego_layer::value (ego_layer.h).  The 1 KB-a-viewer
// value table is read from global memory and stays in the caches, as write_layer reads it.
// An index of rows[] that is no row or of players[] outside [0, P) is never used as one: its
// element of the destination stays as it was — every such element — and ONE of them is reported
// through the fault words (FAULT_STATE_INDEX; the first to claim them).
#include <stddef.h>

#include "step_common.h"
#include "ego_layer.h"

namespace ego_layer {

namespace {

using stepk::div_by;
using stepk::issued;
using stepk::magic_of;
using stepk::wsync;

constexpr int kLdsMax = 160 * 1024;
constexpr int kMaxWaves = 16;
constexpr int kHead = 4 * MP_MAX_PLAYERS;   // ax, ay, aori, aalive
static_assert(offsetof(WorldTail, ax) == 0 && offsetof(WorldTail, ay) == MP_MAX_PLAYERS &&
                  offsetof(WorldTail, aori) == 2 * MP_MAX_PLAYERS && offsetof(WorldTail, aalive) == 3 * MP_MAX_PLAYERS,
              "the staged head of the tail is ax, ay, aori, aalive");

// a wave's LDS: the render planes in whole 16-byte vectors, then the head
__host__ __device__ inline int planes_vec(const Window& g) { return (g.L * g.HW + 15) >> 4; }
__host__ __device__ inline int per_wave(const Window& g) { return planes_vec(g) * 16 + kHead; }

__device__ inline void report_index(uint32_t* fault, int lane, int at, int index, uint32_t what) {
  if (lane == 0 && atomicCAS(&fault[FAULT_STATE_INDEX], 0u, (uint32_t)at + 1u) == 0u) {
    fault[FAULT_STATE_INDEX + 1] = (uint32_t)index;
    fault[FAULT_STATE_INDEX + 2] = what;
  }
}

template <bool kAll>
__device__ inline void ego_body(const Args& a, uint8_t* smem) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const Window& g = a.g;
  const int nvec = planes_vec(g);
  uint8_t* const planes = smem + wave * per_wave(g);
  uint8_t* const head = planes + nvec * 16;
  const uint32_t L = (uint32_t)g.L, VW = (uint32_t)g.VW, VH = (uint32_t)g.VH;
  const uint32_t n = (kAll ? (uint32_t)g.P : 1u) * VH * VW * L;
  const uint32_t mL = magic_of(L), mVW = magic_of(VW), mVH = magic_of(VH);

  for (int i = (int)blockIdx.x * waves + wave; i < a.count; i += (int)gridDim.x * waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    if (r < 0 || r >= a.src_rows) { report_index(a.fault, lane, i, r, kFaultEgoRow); continue; }
    uint32_t p0 = 0u;
    if constexpr (!kAll) {
      const int p = __builtin_amdgcn_readfirstlane(a.players[i]);
      if (p < 0 || p >= g.P) { report_index(a.fault, lane, i, p, kFaultEgoPlayer); continue; }
      p0 = (uint32_t)p;
    }
    wsync();   // (the element before this one has left the wave's LDS)
    {
      const uint4* src = reinterpret_cast<const uint4*>(a.src + (size_t)r * (size_t)a.stride);
      uint4* out = reinterpret_cast<uint4*>(planes);
      const uint4 hv = lane < kHead / 16 ? src[(a.grid_pad >> 4) + lane] : uint4{0u, 0u, 0u, 0u};
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
      if (lane < kHead / 16) reinterpret_cast<uint4*>(head)[lane] = hv;
    }
    wsync();

    auto val = [&](uint32_t e) -> int32_t {
      const uint32_t cell = div_by(e, mL), l = e - cell * L;
      const uint32_t row = div_by(cell, mVW), vx = cell - row * VW;
      const uint32_t p = div_by(row, mVH), vy = row - p * VH;   // (one viewer: p == 0)
      return value(g, planes, head, a.lut, p0 + p, vx, vy, l);
    };
    int32_t* blk = a.dst + (size_t)i * n;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(blk) >> 2) & 3u;
    const uint32_t lead = ((4u - mis) & 3u) < n ? ((4u - mis) & 3u) : n;
    if ((uint32_t)lane < lead) blk[lane] = val((uint32_t)lane);
    const uint32_t nq = (n - lead) >> 2;
    int4* q = reinterpret_cast<int4*>(blk + lead);
    for (uint32_t c0 = 0; c0 < nq; c0 += 4 * 64) {
      int4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t c = c0 + (uint32_t)(k * 64 + lane);
        const uint32_t e = lead + 4u * (c < nq ? c : nq - 1u);
        v[k] = int4{val(e), val(e + 1), val(e + 2), val(e + 3)};
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t c = c0 + (uint32_t)(k * 64 + lane);
        if (c < nq) q[c] = v[k];
      }
    }
    const uint32_t rest = lead + 4u * nq + (uint32_t)lane;
    if (rest < n) blk[rest] = val(rest);
  }
}

}  // namespace

__global__ __launch_bounds__(kMaxWaves * 64) void k_ego_layer_rows(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  ego_body<true>(a, smem);
}

__global__ __launch_bounds__(kMaxWaves * 64) void k_ego_layer_views(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  ego_body<false>(a, smem);
}

Plan plan_of(const Window& g, int count, int num_cus) {
  Plan p = {};
  const int per = per_wave(g);
  int fit = kLdsMax / per;
  if (fit < 1) { p.lds = per; return p; }
  if (fit > kMaxWaves) fit = kMaxWaves;
  // every CU a workgroup before a workgroup gets more waves
  const int cus = num_cus > 0 ? num_cus : 1;
  int waves = (count + cus - 1) / cus;
  if (waves < 4) waves = 4;
  if (waves > fit) waves = fit;
  if (waves > count) waves = count;
  p.waves = waves;
  p.groups = (count + waves - 1) / waves;
  if (p.groups > 2 * cus) p.groups = 2 * cus;   // (a wave then draws several elements in turn)
  p.lds = waves * per;
  return p;
}

void launch(const Args& a, const Plan& p, hipStream_t stream) {
  if (a.players)
    hipLaunchKernelGGL(k_ego_layer_views, dim3((unsigned)p.groups), dim3((unsigned)p.waves * 64u), (size_t)p.lds,
                       stream, a);
  else
    hipLaunchKernelGGL(k_ego_layer_rows, dim3((unsigned)p.groups), dim3((unsigned)p.waves * 64u), (size_t)p.lds,
                       stream, a);
}

int prepare() {
  const void* k[2] = {reinterpret_cast<const void*>(&k_ego_layer_rows),
                      reinterpret_cast<const void*>(&k_ego_layer_views)};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

int host(const Args& a, uint32_t* what) {
  const Window& g = a.g;
  const size_t per = (size_t)g.VH * g.VW * g.L;
  for (int i = 0; i < a.count; ++i) {
    const int r = a.rows ? a.rows[i] : i;
    if (r < 0 || r >= a.src_rows) { *what = kFaultEgoRow; return i; }
    const int p = a.players ? a.players[i] : 0;
    if (p < 0 || p >= g.P) { *what = kFaultEgoPlayer; return i; }
    const uint8_t* rec = a.src + (size_t)r * (size_t)a.stride;
    const int np = a.players ? 1 : g.P;
    int32_t* blk = a.dst + (size_t)i * np * per;
    for (int q = 0; q < np; ++q)
      for (int vy = 0; vy < g.VH; ++vy)
        for (int vx = 0; vx < g.VW; ++vx)
          for (int l = 0; l < g.L; ++l)
            *blk++ = value(g, rec, rec + a.grid_pad, a.lut, (uint32_t)(p + q), (uint32_t)vx, (uint32_t)vy, (uint32_t)l);
  }
  return -1;
}

}  // namespace ego_layer
