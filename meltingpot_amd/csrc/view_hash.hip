// view_hash.hip — the hash of a player's view (an MpViewHash request, include/mp_engine.h;
// view_hash.h has the function): V of every viewer of bank rows or of the engine's worlds, worked
// out from the records where they lie.  No view is drawn, no world is loaded, nothing of the
// engine's is written.  One of the three units of view_unit.h, which has what they share: the
// staged record, the report of a skipped rows[] / players[] index, the launch plan.
//
//   k_view_hash_rows    every viewer of a row: one wave per row, the row's u64 [P] block (the
//                       registered tensor; a draw without players);
//   k_view_hash_views   one viewer of a row: one wave per (row, player), one u64.
// Both are one body.  The workgroup copies the viewers' value tables [P][kLayerLutRow] into LDS
// once, through the class table when there is one (classes[lut[p][s]]: the word function then
// finds a word's class with the one LDS read that finds its id, and no global load waits in the
// chain of a word).  Lane i takes words i, i + 64, ... of a viewer, four of them at a
// time: ego_layer::value on the folded table, fmix64, a u64 sum in registers; the lanes' sums meet
// in state_hash::wave_sum (__shfl_xor, no LDS and no atomics).  k_view_hash_rows leaves viewer p's
// V in lane p and stores the row's block when all P are there: a u64 before the block's first
// 16-byte boundary, 16-byte stores of two neighbouring viewers, a u64 behind them.
// k_view_hash_views stores its 8 bytes from lane 0.
#include "view_unit.h"
#include "view_hash.h"

namespace view_hash {

namespace {

using state_hash::fmix64;
using state_hash::wave_sum;
using stepk::div_by;
using stepk::magic_of;
using stepk::wsync;
using view_unit::kHead;
using view_unit::kMaxWaves;
using view_unit::planes_vec;
using view_unit::tables_bytes;

static_assert(MP_MAX_PLAYERS <= 64, "lane p of a wave keeps viewer p's hash");

// a wave's LDS, behind the workgroup's value tables: the render planes, then the head
__host__ __device__ inline int per_wave(const Window& g) { return planes_vec(g) * 16 + kHead; }

// lane `from`'s u64 (`from` < 64; called by all 64 lanes)
__device__ inline uint64_t lane_u64(uint64_t v, int from) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, from);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), from);
  return ((uint64_t)hi << 32) | lo;
}

template <bool kAll>
__device__ inline void hash_body(const Args& a, uint8_t* smem) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const Window& g = a.g;
  const int nvec = planes_vec(g);
  int32_t* const table = reinterpret_cast<int32_t*>(smem);   // [P][kLayerLutRow]: a word's id, or its class
  for (int j = tid; j < g.P * kLayerLutRow; j += (int)blockDim.x) {
    const int32_t id = a.lut[j];   // (in [0, num_classes): the host checked the table's length against the ids)
    table[j] = a.classes ? a.classes[id] : id;
  }
  __syncthreads();   // (every thread of the workgroup meets it: before the element loop)
  smem += tables_bytes(g);
  uint8_t* const planes = smem + wave * per_wave(g);
  uint8_t* const head = planes + nvec * 16;
  const uint32_t L = (uint32_t)g.L, VW = (uint32_t)g.VW;
  const uint32_t n = (uint32_t)g.VH * VW * L;   // a viewer's words
  const uint32_t mL = magic_of(L), mVW = magic_of(VW);
  const uint32_t P = (uint32_t)g.P;

  for (int i = (int)blockIdx.x * waves + wave; i < a.count; i += (int)gridDim.x * waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    if (r < 0 || r >= a.src_rows) { view_unit::report_index(a.fault, lane, i, r, kFaultViewHashRow); continue; }
    uint32_t p0 = 0u;
    if constexpr (!kAll) {
      const int p = __builtin_amdgcn_readfirstlane(a.players[i]);
      if (p < 0 || p >= g.P) { view_unit::report_index(a.fault, lane, i, p, kFaultViewHashPlayer); continue; }
      p0 = (uint32_t)p;
    }
    wsync();   // (the element before this one has left the wave's LDS)
    view_unit::stage_record(a.src + (size_t)r * (size_t)a.stride, a.grid_pad, nvec, lane, planes, head);
    wsync();

    // this lane's share of viewer p's sum: words lane, lane + 64, ...
    auto share = [&](uint32_t p) -> uint64_t {
      uint64_t sum = 0;
#pragma unroll 4
      for (uint32_t e = (uint32_t)lane; e < n; e += 64u) {
        const uint32_t cell = div_by(e, mL), l = e - cell * L;
        const uint32_t vy = div_by(cell, mVW), vx = cell - vy * VW;
        sum += term(g, planes, head, table, nullptr, a.layer_mask, p, e, vx, vy, l);
      }
      return sum;
    };
    if constexpr (!kAll) {
      const uint64_t sum = wave_sum(share(p0));
      if (lane == 0) a.dst[i] = fmix64(sum);
    } else {
      uint64_t mine = 0;   // lane p: V of viewer p
      for (uint32_t p = 0; p < P; ++p) {
        const uint64_t sum = wave_sum(share(p));
        if ((uint32_t)lane == p) mine = fmix64(sum);
      }
      uint64_t* blk = a.dst + (size_t)i * P;
      const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(blk) >> 3) & 1u;   // (P >= 1)
      const uint32_t nq = (P - lead) >> 1;
      // lane c of the first nq: viewers lead + 2 c and lead + 2 c + 1 (every lane shuffles)
      const int first = (int)((lead + 2u * (uint32_t)lane) & 63u);
      const uint64_t q0 = lane_u64(mine, first), q1 = lane_u64(mine, (first + 1) & 63);
      if ((uint32_t)lane < lead) blk[0] = mine;
      if ((uint32_t)lane < nq) reinterpret_cast<ulonglong2*>(blk + lead)[lane] = ulonglong2{q0, q1};
      const uint32_t rest = lead + 2u * nq;
      if ((uint32_t)lane == rest && rest < P) blk[rest] = mine;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kMaxWaves * 64) void k_view_hash_rows(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  hash_body<true>(a, smem);
}

__global__ __launch_bounds__(kMaxWaves * 64) void k_view_hash_views(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  hash_body<false>(a, smem);
}

Plan plan_of(const Window& g, int count, int num_cus) {
  return view_unit::plan_of(tables_bytes(g), per_wave(g), count, num_cus);
}

void launch(const Args& a, const Plan& p, hipStream_t stream) {
  view_unit::launch(k_view_hash_rows, k_view_hash_views, a, p, stream);
}

int prepare() { return view_unit::prepare(k_view_hash_rows, k_view_hash_views); }

int host(const Args& a, uint32_t* what) {
  const Window& g = a.g;
  return view_unit::host_each(a, kFaultViewHashRow, kFaultViewHashPlayer, what,
                              [&](int i, const uint8_t* rec, uint32_t p, int q, int np) {
    uint64_t sum = 0;
    uint32_t e = 0;
    for (int vy = 0; vy < g.VH; ++vy)
      for (int vx = 0; vx < g.VW; ++vx)
        for (int l = 0; l < g.L; ++l, ++e)
          sum += term(g, rec, rec + a.grid_pad, a.lut, a.classes, a.layer_mask, p, e, (uint32_t)vx, (uint32_t)vy,
                      (uint32_t)l);
    a.dst[(size_t)i * np + q] = fmix64(sum);
  });
}

}  // namespace view_hash
