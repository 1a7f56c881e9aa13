// ego_layer.hip — EGO_LAYER (an MpEgoLayer request, include/mp_engine.h): the layer view in the
// avatar's own frame, drawn from records where they lie — bank rows or the engine's worlds.  No
// world is loaded, nothing of the engine's is written.  One of the three units of view_unit.h,
// which has what they share: the staged record, the report of a skipped rows[] / players[]
// index, the launch plan.
//
//   k_ego_layer_rows    every viewer of a row: one wave per row, the row's contiguous
//                       [P][VH][VW][L] block (the registered leaf; a draw without players);
//   k_ego_layer_views   one viewer of a row: one wave per (row, player), its [VH][VW][L] block.
// Both are one body.  The wave writes its block with write_layer's store scheme (step_common.h):
// up to three dwords before the block's first 16-byte boundary, 16-byte lane-contiguous chunks
// with four of a lane's values worked out before the first store, then up to three dwords.  A
// dword's (viewer, window cell, layer) is split from its index with magic_of / div_by; its value
// is ego_layer::value (ego_layer.h).  The 1 KB-a-viewer value table is read from global memory and
// stays in the caches, as write_layer reads it.
#include "view_unit.h"

namespace ego_layer {

namespace {

using stepk::div_by;
using stepk::magic_of;
using stepk::wsync;
using view_unit::kHead;
using view_unit::kMaxWaves;
using view_unit::planes_vec;

// a wave's LDS: the render planes, then the head
__host__ __device__ inline int per_wave(const Window& g) { return planes_vec(g) * 16 + kHead; }

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
    if (r < 0 || r >= a.src_rows) { view_unit::report_index(a.fault, lane, i, r, kFaultEgoRow); continue; }
    uint32_t p0 = 0u;
    if constexpr (!kAll) {
      const int p = __builtin_amdgcn_readfirstlane(a.players[i]);
      if (p < 0 || p >= g.P) { view_unit::report_index(a.fault, lane, i, p, kFaultEgoPlayer); continue; }
      p0 = (uint32_t)p;
    }
    wsync();   // (the element before this one has left the wave's LDS)
    view_unit::stage_record(a.src + (size_t)r * (size_t)a.stride, a.grid_pad, nvec, lane, planes, head);
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

Plan plan_of(const Window& g, int count, int num_cus) { return view_unit::plan_of(0, per_wave(g), count, num_cus); }

void launch(const Args& a, const Plan& p, hipStream_t stream) {
  view_unit::launch(k_ego_layer_rows, k_ego_layer_views, a, p, stream);
}

int prepare() { return view_unit::prepare(k_ego_layer_rows, k_ego_layer_views); }

int host(const Args& a, uint32_t* what) {
  const Window& g = a.g;
  const size_t per = (size_t)g.VH * g.VW * g.L;
  return view_unit::host_each(a, kFaultEgoRow, kFaultEgoPlayer, what,
                              [&](int i, const uint8_t* rec, uint32_t p, int q, int np) {
    int32_t* blk = a.dst + ((size_t)i * np + q) * per;
    for (int vy = 0; vy < g.VH; ++vy)
      for (int vx = 0; vx < g.VW; ++vx)
        for (int l = 0; l < g.L; ++l)
          *blk++ = value(g, rec, rec + a.grid_pad, a.lut, p, (uint32_t)vx, (uint32_t)vy, (uint32_t)l);
  });
}

}  // namespace ego_layer
