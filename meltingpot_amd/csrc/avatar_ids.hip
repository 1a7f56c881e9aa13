// avatar_ids.hip — AVATAR_IDS_IN_VIEW and AVATAR_IDS_IN_RANGE_TO_ZAP (an MpAvatarIds request,
// include/mp_engine.h; avatar_ids.h has the functions): int32 0/1 vectors over the player slots,
// of every viewer of bank rows or of the engine's worlds, written from the records where they lie.
// No world is loaded, nothing of the engine's is written.  The fourth unit of view_unit.h, which
// has what they share: the staging loop, the report of a skipped rows[] / players[] index, the
// launch plan.
//
//   k_avatar_ids_rows    every viewer of a row: one wave per row, the row's [P][P] blocks (the
//                        registered leaves; a draw without players);
//   k_avatar_ids_views   one viewer of a row: one wave per (row, player), its [P] vectors.
// Both are one body, and one launch writes IN_VIEW, IN_RANGE or both.  The workgroup keeps the
// step tables' sinfo (1 KB) in LDS.  A wave stages what it reads of its record — the avatar_layer
// plane, from the 16-byte line it begins in to the one it ends in, and the head — not all L planes.
//   view    lane e of the block, e = viewer * P + q: avatar_ids::in_view, stored by the lane that
//           worked it out: a viewer's vector leaves in whole dwords, neighbouring lanes write
//           neighbouring dwords, and every dword of the block is written.
//   zap     the lane layout of stepk::fire_beams: lane = beam * nc + cell, `per` = 64 / nc beams a
//           round, ceil(P / per) rounds.  The ballot of "stops its ray" against the cell's
//           predecessor mask says reached or not for all cells of a round at once; a reached cell
//           that holds an avatar sets its dword of the wave's [P][P] block in LDS, which the wave
//           has cleared for THIS element, and the block leaves as the view block does.
#include "view_unit.h"
#include "avatar_ids.h"

namespace avatar_ids {

namespace {

using stepk::wsync;
using view_unit::kHead;
using view_unit::kMaxWaves;

constexpr int kSinfoBytes = stepk::kSinfoBytes;   // the workgroup's table

// the 16-byte lines of a record that hold the avatar_layer plane: from byte stage_lo, stage_vec of them
__host__ __device__ inline int stage_lo(int plane_at) { return plane_at & ~15; }
__host__ __device__ inline int stage_vec(const Window& g, int plane_at) {
  return (plane_at + g.HW - stage_lo(plane_at) + 15) >> 4;
}
// a wave's LDS: those lines, the head, the [P][P] block of the rays
__host__ __device__ inline int per_wave(const Window& g, int plane_at) {
  return stage_vec(g, plane_at) * 16 + kHead + ((g.P * g.P * 4 + 15) >> 4) * 16;
}

template <bool kAll>
__device__ inline void ids_body(const Args& a, uint8_t* smem) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const Window& g = a.g;
  uint32_t* const sinfo = reinterpret_cast<uint32_t*>(smem);
  if (a.dst_zap)
    for (int j = tid; j < 256; j += (int)blockDim.x) sinfo[j] = a.sinfo[j];
  __syncthreads();   // (every thread of the workgroup meets it: before the element loop)
  const int lo = stage_lo(a.plane_at), nvec = stage_vec(g, a.plane_at);
  uint8_t* const staged = smem + kSinfoBytes + wave * per_wave(g, a.plane_at);
  const uint8_t* const plane = staged + (a.plane_at - lo);
  uint8_t* const head = staged + nvec * 16;
  uint32_t* const hits = reinterpret_cast<uint32_t*>(head + kHead);   // [np][P]
  const uint32_t P = (uint32_t)g.P, mP = ego_layer::magic(P);
  const uint32_t np = kAll ? P : 1u, n = np * P;
  const stepk::BeamLane bm = stepk::beam_lane(a.shape, lane);

  for (int i = (int)blockIdx.x * waves + wave; i < a.count; i += (int)gridDim.x * waves) {
    const int r = __builtin_amdgcn_readfirstlane(a.rows ? a.rows[i] : i);
    if (r < 0 || r >= a.src_rows) { view_unit::report_index(a.fault, lane, i, r, kFaultAvatarIdsRow); continue; }
    uint32_t p0 = 0u;
    if constexpr (!kAll) {
      const int p = __builtin_amdgcn_readfirstlane(a.players[i]);
      if (p < 0 || p >= g.P) { view_unit::report_index(a.fault, lane, i, p, kFaultAvatarIdsPlayer); continue; }
      p0 = (uint32_t)p;
    }
    wsync();   // (the element before this one has left the wave's LDS)
    view_unit::stage_record(a.src + (size_t)r * (size_t)a.stride + lo, a.grid_pad - lo, nvec, lane, staged, head);
    if (a.dst_zap)   // (no hit of the element before survives)
      for (uint32_t e = (uint32_t)lane; e < n; e += 64u) hits[e] = 0u;
    wsync();

    if (a.dst) {
      int32_t* blk = a.dst + (size_t)i * n;
      for (uint32_t e = (uint32_t)lane; e < n; e += 64u) {
        const uint32_t v = ego_layer::divm(e, mP), q = e - v * P;   // (one viewer: v == 0)
        blk[e] = in_view(g, head, p0 + v, q);
      }
    }
    if (a.dst_zap) {
      const int nc = bm.nc, per = bm.per;
      for (int b0 = 0; b0 < (int)np; b0 += per) {
        const int v = b0 + bm.bl;   // this lane's beam: viewer v of the block
        const bool ok = bm.bl < per && v < (int)np;
        const uint32_t b = p0 + (uint32_t)(ok ? v : 0);
        const bool live = ok && head[3 * MP_MAX_PLAYERS + b] != 0;
        int cell;
        const bool in = beam_cell(g, head, b, bm.lat, bm.fw, &cell);
        // every ray stops at the first cell that is outside the map or holds something
        const unsigned long long stops = __ballot(live && ray_stops(plane, in, cell));
        const uint32_t mine = (uint32_t)(stops >> (bm.bl * nc)) & ((1u << nc) - 1u);
        if (live && in && (mine & bm.pred) == 0u) {
          const uint32_t who = avatar_at(plane, sinfo, cell);
          if (who - 1u < P) hits[(uint32_t)v * P + who - 1u] = 1u;
        }
      }
      wsync();
      int32_t* blk = a.dst_zap + (size_t)i * n;
      for (uint32_t e = (uint32_t)lane; e < n; e += 64u) blk[e] = (int32_t)hits[e];
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kMaxWaves * 64) void k_avatar_ids_rows(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  ids_body<true>(a, smem);
}

__global__ __launch_bounds__(kMaxWaves * 64) void k_avatar_ids_views(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  ids_body<false>(a, smem);
}

Plan plan_of(const Window& g, int plane_at, int count, int num_cus) {
  return view_unit::plan_of(kSinfoBytes, per_wave(g, plane_at), count, num_cus);
}

void launch(const Args& a, const Plan& p, hipStream_t stream) {
  view_unit::launch(k_avatar_ids_rows, k_avatar_ids_views, a, p, stream);
}

int prepare() { return view_unit::prepare(k_avatar_ids_rows, k_avatar_ids_views); }

int host(const Args& a, uint32_t* what) {
  const Window& g = a.g;
  const int P = g.P, nc = a.shape.n;
  return view_unit::host_each(a, kFaultAvatarIdsRow, kFaultAvatarIdsPlayer, what,
                              [&](int i, const uint8_t* rec, uint32_t p, int q, int np) {
    const uint8_t* head = rec + a.grid_pad;
    const uint8_t* plane = rec + a.plane_at;
    const size_t at = ((size_t)i * np + q) * (size_t)P;
    if (a.dst)
      for (int t = 0; t < P; ++t) a.dst[at + t] = in_view(g, head, p, (uint32_t)t);
    if (!a.dst_zap) return;
    int32_t* row = a.dst_zap + at;
    for (int t = 0; t < P; ++t) row[t] = 0;
    if (!head[3 * MP_MAX_PLAYERS + p]) return;
    uint32_t stops = 0u;   // the ballot of p's beam
    for (int j = 0; j < nc; ++j) {
      int cell;
      const bool in = beam_cell(g, head, p, cell_lat(a.shape.cell[j]), cell_fw(a.shape.cell[j]), &cell);
      if (ray_stops(plane, in, cell)) stops |= 1u << j;
    }
    for (int j = 0; j < nc; ++j) {
      int cell;
      const bool in = beam_cell(g, head, p, cell_lat(a.shape.cell[j]), cell_fw(a.shape.cell[j]), &cell);
      if (!in || (stops & cell_pred(a.shape.cell[j]))) continue;
      const uint32_t who = avatar_at(plane, a.sinfo, cell);
      if (who - 1u < (uint32_t)P) row[who - 1u] = 1;
    }
  });
}

}  // namespace avatar_ids
