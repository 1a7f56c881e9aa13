// ego_planes.hip — class-indicator feature planes of a player's view (an MpEgoPlanes request,
// include/mp_engine.h; ego_planes.h has the functions): uint8 [C'][VH][VW] of every viewer of bank
// rows or of the engine's worlds, written from the records where they lie.  No int32 view is
// drawn, no world is loaded, nothing of the engine's is written.  One of the three units of
// view_unit.h, which has what they share: the staged record, the report of a skipped rows[] /
// players[] index, the launch plan.
//
//   k_ego_planes_rows    every viewer of a row: one wave per row, the row's [P][C'][VH][VW] block
//                        (the registered tensor; a draw without players);
//   k_ego_planes_views   one viewer of a row: one wave per (row, player), its [C'][VH][VW] block.
// Both are one body.  The workgroup folds the class table into the viewers' value tables in LDS
// once (class_of(classes[lut[p][s]]): a word's class then costs the one LDS read that finds its
// id).  Then, a viewer of the wave's staged record at a time:
//   cells   lane i owns window cells i, i + 64, ...: it ORs 1 << class over the counted layers
//           into one u64 (ego_planes::cell_classes) and, with `facing`, finds the cell's avatars
//           in the P head entries (cell_facing): a nibble.
//   turn    the destination is plane-major, the lanes hold cell-major masks.  __ballot turns them:
//           ballot((mask >> c) & 1) IS 64 cells of plane c, one bit a cell.  Lane c keeps plane
//           c's word and the wave leaves C' bit planes of ceil(cells / 64) u64 in its LDS.
//   store   the wave walks the viewer's block in byte order, (plane, cell) = divmod(byte, VH * VW)
//           with magic_of / div_by: byte b of the block is bit `cell` of bit plane `plane`.  A
//           lane's 16-byte chunk is 16 neighbouring bits — two dwords of one bit plane, or the end
//           of one plane and the head of the next — spread to bytes with one multiply and one AND a
//           dword ((x * 0x00204081) & 0x01010101 for four bits).  Neighbouring lanes read the same
//           or neighbouring dwords: no bank conflicts.  Byte stores run up to the block's first
//           16-byte boundary and behind its last; no byte outside the block is written.
// An entry of the class table outside [-1, num_classes) counts as -1 and is reported as a skipped
// index is (view_unit.h).
#include <vector>

#include "view_unit.h"
#include "ego_planes.h"

namespace ego_planes {

namespace {

using stepk::div_by;
using stepk::magic_of;
using stepk::wsync;
using view_unit::kHead;
using view_unit::kMaxWaves;
using view_unit::planes_vec;
using view_unit::tables_bytes;

static_assert(kMaxClasses == 64, "lane c of a wave keeps class plane c's ballot");

// a wave's LDS, behind the workgroup's folded value tables: the render planes, the head, then `np`
// bit planes of words64() u64 (in whole 16-byte vectors too)
__host__ __device__ inline int words64(const Window& g) { return (g.VH * g.VW + 63) >> 6; }
__host__ __device__ inline int per_wave(const Window& g, int np) {
  return planes_vec(g) * 16 + kHead + ((np * words64(g) * 8 + 15) >> 4) * 16;
}

// four bits -> four bytes of 0 / 1, bit 0 in the lowest byte
__device__ inline uint32_t spread4(uint32_t x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

template <bool kAll>
__device__ inline void planes_body(const Args& a, uint8_t* smem) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const Window& g = a.g;
  const int nvec = planes_vec(g);
  const uint32_t C = (uint32_t)a.num_classes, Cp = C + (a.facing ? 4u : 0u);
  int32_t* const table = reinterpret_cast<int32_t*>(smem);   // [P][kLayerLutRow]: a word's class, -1: none
  for (int j = tid; j < g.P * kLayerLutRow; j += (int)blockDim.x) {
    const int32_t id = a.lut[j];   // (in [0, num_ids): the host checked the table's length against the ids)
    table[j] = (uint32_t)id < (uint32_t)a.num_ids ? class_of(a.classes[id], a.num_classes) : -1;
  }
  if (blockIdx.x == 0)   // the caller's table may hold anything: one entry out of range is reported
    for (int j = tid; j < a.num_ids; j += (int)blockDim.x) {
      const int32_t c = a.classes[j];
      if (c < -1 || c >= a.num_classes) view_unit::report(a.fault, j, c, kFaultEgoPlanesClass);
    }
  __syncthreads();   // (every thread of the workgroup meets it: before the element loop)
  smem += tables_bytes(g);
  uint8_t* const planes = smem + wave * per_wave(g, (int)Cp);
  uint8_t* const head = planes + nvec * 16;
  const uint32_t VW = (uint32_t)g.VW, cells = (uint32_t)g.VH * VW;
  const uint32_t w64 = (uint32_t)words64(g), w32 = 2u * w64;
  uint64_t* const bp = reinterpret_cast<uint64_t*>(head + kHead);   // [Cp][w64]: bit `cell` of plane c
  const uint32_t* const bw = reinterpret_cast<const uint32_t*>(bp);
  const uint32_t n = Cp * cells;   // a viewer's bytes
  const uint32_t mVW = magic_of(VW), mCells = magic_of(cells);
  const uint32_t P = (uint32_t)g.P;

  // bits b .. b + want - 1 of a viewer's block (want <= 16, b + want <= n): bit t is byte b + t
  auto bits = [&](uint32_t b, uint32_t want) -> uint32_t {
    uint32_t plane = div_by(b, mCells), cell = b - plane * cells, out = 0u, got = 0u;
    while (got < want) {
      const uint32_t left = cells - cell, take = want - got < left ? want - got : left;
      const uint32_t i = cell >> 5, i1 = i + 1u < w32 ? i + 1u : i;
      const uint64_t two = ((uint64_t)bw[plane * w32 + i1] << 32) | bw[plane * w32 + i];
      out |= ((uint32_t)(two >> (cell & 31u)) & ((1u << take) - 1u)) << got;
      got += take;
      ++plane;
      cell = 0u;
    }
    return out;
  };

  for (int i = (int)blockIdx.x * waves + wave; i < a.count; i += (int)gridDim.x * waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    if (r < 0 || r >= a.src_rows) { view_unit::report_index(a.fault, lane, i, r, kFaultEgoPlanesRow); continue; }
    uint32_t p0 = 0u;
    if constexpr (!kAll) {
      const int p = __builtin_amdgcn_readfirstlane(a.players[i]);
      if (p < 0 || p >= g.P) { view_unit::report_index(a.fault, lane, i, p, kFaultEgoPlanesPlayer); continue; }
      p0 = (uint32_t)p;
    }
    wsync();   // (the element before this one has left the wave's LDS)
    view_unit::stage_record(a.src + (size_t)r * (size_t)a.stride, a.grid_pad, nvec, lane, planes, head);

    const uint32_t np = kAll ? P : 1u;
    for (uint32_t q = 0; q < np; ++q) {
      const uint32_t p = p0 + q;
      wsync();   // (the record is staged; the viewer before this one has left the bit planes)
      for (uint32_t k = 0; k < w64; ++k) {
        const uint32_t cell = k * 64u + (uint32_t)lane;
        uint64_t m = 0ull;
        uint32_t f = 0u;
        if (cell < cells) {
          const uint32_t vy = div_by(cell, mVW), vx = cell - vy * VW;
          m = cell_classes(g, planes, head, table, a.layer_mask, p, vx, vy);
          if (a.facing) f = cell_facing(g, head, p, vx, vy);
        }
        uint64_t mine = 0ull;   // lane c: 64 cells of plane c
        for (uint32_t c = 0; c < C; ++c) {
          const uint64_t b = __ballot((int)((m >> c) & 1ull));
          if ((uint32_t)lane == c) mine = b;
        }
        if ((uint32_t)lane < C) bp[(uint32_t)lane * w64 + k] = mine;
        if (a.facing) {
          for (uint32_t d = 0; d < 4u; ++d) {
            const uint64_t b = __ballot((int)((f >> d) & 1u));
            if ((uint32_t)lane == d) mine = b;
          }
          if (lane < 4) bp[(C + (uint32_t)lane) * w64 + k] = mine;
        }
      }
      wsync();

      uint8_t* blk = a.dst + ((size_t)i * np + q) * (size_t)n;
      const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(blk) & 15u;
      const uint32_t lead = ((16u - mis) & 15u) < n ? ((16u - mis) & 15u) : n;
      if ((uint32_t)lane < lead) blk[lane] = (uint8_t)bits((uint32_t)lane, 1u);
      const uint32_t nq = (n - lead) >> 4;
      uint4* out = reinterpret_cast<uint4*>(blk + lead);
      for (uint32_t c = (uint32_t)lane; c < nq; c += 64u) {
        const uint32_t x = bits(lead + 16u * c, 16u);
        out[c] = uint4{spread4(x), spread4(x >> 4), spread4(x >> 8), spread4(x >> 12)};
      }
      const uint32_t rest = lead + 16u * nq + (uint32_t)lane;
      if (rest < n) blk[rest] = (uint8_t)bits(rest, 1u);
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kMaxWaves * 64) void k_ego_planes_rows(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  planes_body<true>(a, smem);
}

__global__ __launch_bounds__(kMaxWaves * 64) void k_ego_planes_views(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  planes_body<false>(a, smem);
}

Plan plan_of(const Window& g, int num_planes, int count, int num_cus) {
  return view_unit::plan_of(tables_bytes(g), per_wave(g, num_planes), count, num_cus);
}

void launch(const Args& a, const Plan& p, hipStream_t stream) {
  view_unit::launch(k_ego_planes_rows, k_ego_planes_views, a, p, stream);
}

int prepare() { return view_unit::prepare(k_ego_planes_rows, k_ego_planes_views); }

int host(const Args& a, uint32_t* what) {
  const Window& g = a.g;
  const int C = a.num_classes;
  const size_t cells = (size_t)g.VH * g.VW, n = (size_t)planes_of(a) * cells;
  // the folded value tables, as the workgroup builds them
  std::vector<int32_t> table((size_t)g.P * kLayerLutRow);
  for (int j = 0; j < g.P * kLayerLutRow; ++j) {
    const int32_t id = a.lut[j];
    table[j] = (uint32_t)id < (uint32_t)a.num_ids ? class_of(a.classes[id], C) : -1;
  }
  return view_unit::host_each(a, kFaultEgoPlanesRow, kFaultEgoPlanesPlayer, what,
                              [&](int i, const uint8_t* rec, uint32_t p, int q, int np) {
    uint8_t* blk = a.dst + ((size_t)i * np + q) * n;
    for (int vy = 0; vy < g.VH; ++vy)
      for (int vx = 0; vx < g.VW; ++vx) {
        const size_t cell = (size_t)vy * g.VW + vx;
        const uint64_t m = cell_classes(g, rec, rec + a.grid_pad, table.data(), a.layer_mask, p, (uint32_t)vx,
                                        (uint32_t)vy);
        for (int c = 0; c < C; ++c) blk[(size_t)c * cells + cell] = (uint8_t)((m >> c) & 1u);
        if (a.facing) {
          const uint32_t f = cell_facing(g, rec + a.grid_pad, p, (uint32_t)vx, (uint32_t)vy);
          for (int d = 0; d < 4; ++d) blk[(size_t)(C + d) * cells + cell] = (uint8_t)((f >> d) & 1u);
        }
      }
  });
}

}  // namespace ego_planes
