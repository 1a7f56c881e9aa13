// world_view.hip — WORLD.LAYER and the world planes (the MP_EGO_WORLD_* and MP_EGOPLANES_WORLD_*
// ops, include/mp_engine.h; world_view.h has the functions): the whole map of bank rows or of the
// engine's worlds as ids, int32 [H][W][L], and as class and facing planes, uint8 [C'][H][W], written
// from the records where they lie.  No world is loaded, nothing of the engine's is written.  Two
// more kernels on view_unit.h: one wave per element, the record's render planes and the head of its
// tail staged in the wave's share of the LDS.
//
//   k_world_layer_rows    the workgroup keeps the world's value table in LDS.  Output word e of an
//                         element is (cell, l) = divmod(e, L) (ego_layer::magic / divm); a lane works
//                         out four consecutive words and stores them as one 16-byte vector, with up to
//                         three dwords before the element's first 16-byte boundary and behind its
//                         last (ego_layer.hip's scheme).
//   k_world_planes_rows   the workgroup keeps the table with the classes folded in.  Per element:
//     masks   lane i owns cells i, i + 64, ...: it ORs 1 << class over the counted layers into one
//             u64 (world_view::cell_classes) and leaves it in the wave's LDS, H * W * 8 bytes
//             beside the planes — H * W * 4 in k_world_planes_rows32, the same body for
//             num_classes <= 32, which keeps the low word;
//     store   plane by plane (which plane, whether it is a class or a facing plane: wave-uniform).
//             A lane's 16-byte chunk is 16 consecutive cells of the plane.  The lanes read the masks
//             of 64 consecutive cells — no bank conflict — and __ballot of bit c IS those 64 cells
//             of plane c: lane j takes its 16 bits of ballot j / 4 and spreads them to bytes
//             (ego_planes.hip's spread4).  A facing plane's chunk starts at 0 and takes a bit from
//             each living avatar that stands in it (world_view::avatar_cell, from the staged head):
//             at most P cells of a plane are set.  Byte stores run up to the plane's first 16-byte
//             boundary and behind its last: `dst` may start on any byte, and no byte outside the
//             element is written.
// An entry of the class table outside [-1, num_classes) counts as -1 and is reported as a skipped
// index is (view_unit.h).
#include "view_unit.h"
#include "world_view.h"

namespace world_view {

namespace {

using ego_layer::divm;
using ego_layer::magic;
using ego_planes::class_of;
using stepk::wsync;
using view_unit::kHead;
using view_unit::kMaxWaves;
using view_unit::planes_vec;

// the workgroup's table in whole 16-byte vectors; a wave's share behind it: the render planes, the
// head, and (the planes kernel) one u64 a cell
constexpr int kTableBytes = ((kLayerLutRow * 4 + 15) >> 4) * 16;
__host__ __device__ inline int layer_wave(const Window& g) { return planes_vec(g) * 16 + kHead; }
__host__ __device__ inline int planes_wave(const Window& g, int mask_bytes) {
  return layer_wave(g) + ((g.HW * mask_bytes + 15) >> 4) * 16;
}
// a cell's class mask is a u32 while the classes fit one (clean_up: 16 waves a workgroup then fit, not 15)
__host__ __device__ inline int mask_bytes_of(int num_classes) { return num_classes <= 32 ? 4 : 8; }

// four bits -> four bytes of 0 / 1, bit 0 in the lowest byte
__device__ inline uint32_t spread4(uint32_t x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

}  // namespace

__global__ __launch_bounds__(kMaxWaves * 64) void k_world_layer_rows(LayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const Window& g = a.g;
  int32_t* const wt = reinterpret_cast<int32_t*>(smem);
  for (int s = tid; s < kLayerLutRow; s += (int)blockDim.x) wt[s] = a.lut[s];
  __syncthreads();   // (every thread of the workgroup meets it: before the element loop)
  const int nvec = planes_vec(g);
  uint8_t* const planes = smem + kTableBytes + wave * layer_wave(g);
  uint8_t* const head = planes + nvec * 16;
  const uint32_t L = (uint32_t)g.L, n = (uint32_t)g.HW * L, mL = magic(L);

  for (int i = (int)blockIdx.x * waves + wave; i < a.count; i += (int)gridDim.x * waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    if (r < 0 || r >= a.src_rows) { view_unit::report_index(a.fault, lane, i, r, kFaultWorldLayerRow); continue; }
    wsync();   // (the element before this one has left the wave's LDS)
    view_unit::stage_record(a.src + (size_t)r * (size_t)a.stride, a.grid_pad, nvec, lane, planes, head);
    wsync();

    auto val = [&](uint32_t e) -> int32_t {
      const uint32_t cell = divm(e, mL);
      return value(g, planes, wt, cell, e - cell * L);
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
        // four consecutive words: one division, then (cell, l) step by step
        uint32_t cell = divm(e, mL), l = e - cell * L;
        int32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          w[j] = value(g, planes, wt, cell, l);
          if (++l == L) { l = 0u; ++cell; }
        }
        v[k] = int4{w[0], w[1], w[2], w[3]};
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

// `Mask`: uint32_t (num_classes <= 32) or uint64_t, one a cell in the wave's LDS
template <class Mask>
__device__ inline void planes_body(const PlanesArgs& a, uint8_t* smem) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const Window& g = a.g;
  const uint32_t C = (uint32_t)a.num_classes, Cp = C + (a.facing ? 4u : 0u);
  int32_t* const table = reinterpret_cast<int32_t*>(smem);   // [kLayerLutRow]: a record byte's class, -1: none
  for (int s = tid; s < kLayerLutRow; s += (int)blockDim.x) {
    const int32_t id = a.lut[s];   // (in [0, num_ids): the host checked the table's length against the ids)
    table[s] = (uint32_t)id < (uint32_t)a.num_ids ? class_of(a.classes[id], a.num_classes) : -1;
  }
  if (blockIdx.x == 0)   // the caller's table may hold anything: one entry out of range is reported
    for (int j = tid; j < a.num_ids; j += (int)blockDim.x) {
      const int32_t c = a.classes[j];
      if (c < -1 || c >= a.num_classes) view_unit::report(a.fault, j, c, kFaultWorldPlanesClass);
    }
  __syncthreads();   // (every thread of the workgroup meets it: before the element loop)
  const int nvec = planes_vec(g);
  uint8_t* const planes = smem + kTableBytes + wave * planes_wave(g, (int)sizeof(Mask));
  uint8_t* const head = planes + nvec * 16;
  Mask* const masks = reinterpret_cast<Mask*>(head + kHead);   // [H * W]: a cell's classes
  const uint32_t HW = (uint32_t)g.HW;
  const size_t n = (size_t)Cp * HW;   // an element's bytes

  for (int i = (int)blockIdx.x * waves + wave; i < a.count; i += (int)gridDim.x * waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    if (r < 0 || r >= a.src_rows) { view_unit::report_index(a.fault, lane, i, r, kFaultWorldPlanesRow); continue; }
    wsync();   // (the element before this one has left the wave's LDS)
    view_unit::stage_record(a.src + (size_t)r * (size_t)a.stride, a.grid_pad, nvec, lane, planes, head);
    wsync();
    for (uint32_t cell = (uint32_t)lane; cell < HW; cell += 64u)
      masks[cell] = (Mask)cell_classes(g, planes, table, a.layer_mask, cell);
    wsync();

    for (uint32_t pl = 0; pl < Cp; ++pl) {
      const bool cls = pl < C;
      const int d = (int)(pl - C);
      // byte `cell` of the plane
      auto bit = [&](uint32_t cell) -> uint32_t {
        if (cls) return (uint32_t)(masks[cell] >> pl) & 1u;
        uint32_t b = 0u;
        for (int q = 0; q < g.P; ++q) b |= avatar_cell(g, head, q, d) == (int)cell ? 1u : 0u;
        return b;
      };
      uint8_t* base = a.dst + (size_t)i * n + (size_t)pl * HW;
      const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(base) & 15u;
      const uint32_t lead = ((16u - mis) & 15u) < HW ? ((16u - mis) & 15u) : HW;
      if ((uint32_t)lane < lead) base[lane] = (uint8_t)bit((uint32_t)lane);
      const uint32_t nq = (HW - lead) >> 4;
      uint4* out = reinterpret_cast<uint4*>(base + lead);
      for (uint32_t c0 = 0; c0 < nq; c0 += 64u) {   // 64 chunks: 1024 cells from lead + 16 * c0 on
        const uint32_t first = lead + 16u * c0;
        uint32_t x = 0u;
        if (cls) {
          for (uint32_t k = 0; k < 16u && c0 + 4u * k < nq; ++k) {
            const uint32_t cell = first + k * 64u + (uint32_t)lane;
            const uint64_t b = __ballot(cell < HW ? (int)((masks[cell] >> pl) & 1u) : 0);
            if (((uint32_t)lane >> 2) == k) x = (uint32_t)(b >> (((uint32_t)lane & 3u) * 16u)) & 0xffffu;
          }
        } else {
          for (int q = 0; q < g.P; ++q) {
            const int pos = avatar_cell(g, head, q, d);
            const uint32_t rel = (uint32_t)pos - (first + 16u * (uint32_t)lane);
            if (pos >= 0 && rel < 16u) x |= 1u << rel;
          }
        }
        const uint32_t c = c0 + (uint32_t)lane;
        if (c < nq) out[c] = uint4{spread4(x), spread4(x >> 4), spread4(x >> 8), spread4(x >> 12)};
      }
      const uint32_t rest = lead + 16u * nq + (uint32_t)lane;
      if (rest < HW) base[rest] = (uint8_t)bit(rest);
    }
  }
}

__global__ __launch_bounds__(kMaxWaves * 64) void k_world_planes_rows(PlanesArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  planes_body<uint64_t>(a, smem);
}

__global__ __launch_bounds__(kMaxWaves * 64) void k_world_planes_rows32(PlanesArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  planes_body<uint32_t>(a, smem);
}

Plan layer_plan(const Window& g, int count, int num_cus) {
  return view_unit::plan_of(kTableBytes, layer_wave(g), count, num_cus);
}
Plan planes_plan(const Window& g, int num_classes, int count, int num_cus) {
  return view_unit::plan_of(kTableBytes, planes_wave(g, mask_bytes_of(num_classes)), count, num_cus);
}

void launch(const LayerArgs& a, const Plan& p, hipStream_t stream) {
  hipLaunchKernelGGL(k_world_layer_rows, dim3((unsigned)p.groups), dim3((unsigned)p.waves * 64u), (size_t)p.lds,
                     stream, a);
}
void launch(const PlanesArgs& a, const Plan& p, hipStream_t stream) {
  hipLaunchKernelGGL(mask_bytes_of(a.num_classes) == 4 ? k_world_planes_rows32 : k_world_planes_rows, dim3((unsigned)p.groups), dim3((unsigned)p.waves * 64u), (size_t)p.lds,
                     stream, a);
}

int prepare() {
  const void* k[3] = {reinterpret_cast<const void*>(k_world_layer_rows),
                      reinterpret_cast<const void*>(k_world_planes_rows),
                      reinterpret_cast<const void*>(k_world_planes_rows32)};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, view_unit::kLdsMax);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// The host twins' loop: each(i, rec) of element i's record.  Returns -1, or the first position whose
// rows[] index is out of range; every element before it has been visited.
template <class A, class F>
static int host_rows(const A& a, F each) {
  for (int i = 0; i < a.count; ++i) {
    const int r = a.rows ? a.rows[i] : i;
    if (r < 0 || r >= a.src_rows) return i;
    each(i, a.src + (size_t)r * (size_t)a.stride);
  }
  return -1;
}

int host(const LayerArgs& a) {
  const Window& g = a.g;
  return host_rows(a, [&](int i, const uint8_t* rec) {
    int32_t* blk = a.dst + (size_t)i * (size_t)g.HW * (size_t)g.L;
    for (uint32_t cell = 0; cell < (uint32_t)g.HW; ++cell)
      for (uint32_t l = 0; l < (uint32_t)g.L; ++l) *blk++ = value(g, rec, a.lut, cell, l);
  });
}

int host(const PlanesArgs& a) {
  const Window& g = a.g;
  const int C = a.num_classes;
  const size_t HW = (size_t)g.HW, n = (size_t)planes_of(a) * HW;
  // the folded table, as the workgroup builds it
  int32_t table[kLayerLutRow];
  for (int s = 0; s < kLayerLutRow; ++s) {
    const int32_t id = a.lut[s];
    table[s] = (uint32_t)id < (uint32_t)a.num_ids ? class_of(a.classes[id], C) : -1;
  }
  return host_rows(a, [&](int i, const uint8_t* rec) {
    uint8_t* blk = a.dst + (size_t)i * n;
    for (size_t cell = 0; cell < HW; ++cell) {
      const uint64_t m = cell_classes(g, rec, table, a.layer_mask, (uint32_t)cell);
      for (int c = 0; c < C; ++c) blk[(size_t)c * HW + cell] = (uint8_t)((m >> c) & 1u);
    }
    if (!a.facing) return;
    for (size_t b = (size_t)C * HW; b < n; ++b) blk[b] = 0;
    for (int d = 0; d < 4; ++d)
      for (int q = 0; q < g.P; ++q) {
        const int pos = avatar_cell(g, rec + a.grid_pad, q, d);
        if (pos >= 0) blk[(size_t)(C + d) * HW + (size_t)pos] = 1;
      }
  });
}

}  // namespace world_view
