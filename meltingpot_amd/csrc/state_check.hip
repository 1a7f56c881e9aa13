// state_check.hip — the well-formedness check of world records (state_check.h has the rules;
// an MpStatesCheck request, include/mp_engine.h).  A unit of its own that includes none of the
// step headers: k_frame, the single-step and the K-step kernels are compiled from exactly what
// they were compiled from before, and nothing is added inside load_world.
//
//   k_check_states   one wavefront per row, four rows per 256-thread workgroup (the geometry of
//                    the stand-alone step kernels and of k_save_worlds).  The row is read where
//                    it lies: the planes in 16-byte lane loads, the tail by the lanes p < P.  The
//                    256-entry state table is staged in LDS (a lane indexes it with a plane
//                    byte); every scalar of CheckTables is read from device memory with a uniform
//                    address.  A wave-wide minimum reduces the lanes' violations to the row's.
//                    Two forms: verdicts of rows[] (out[i] = (rule, offset word)), and the filter
//                    of a checked load (checked[w] = src[w], or -1 for a malformed row).
// An index outside the bank is never used as one.
#include "pack_decode.h"
#include "state_check.h"

namespace {

using namespace state_check;

// DecodedPack::step_blob starts with the step's u32 sinfo[256] (step_common.h: "LDS images"):
// bits 24-31 = 1 + the player whose avatar state the state is.
constexpr size_t kSinfoBytes = 256 * 4;

// The smallest key of the wave, in every lane.  Called by all 64 lanes (uniform control flow).
__device__ inline uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// filter = 0: out is int32 [count][2], element i the verdict of row rows[i] (NULL: row i).
// filter = 1: rows is a load's src[count], out is int32 [count]: src[i], or -1 for a refused row.
__global__ __launch_bounds__(256) void k_check_states(const CheckTables* __restrict__ ck,
                                                      const uint8_t* __restrict__ bank, int bank_rows,
                                                      const int32_t* __restrict__ rows, int count,
                                                      int32_t* __restrict__ out, int filter,
                                                      uint32_t* fault) {
  __shared__ uint16_t code[256];
  code[threadIdx.x] = ck->code[threadIdx.x];
  __syncthreads();   // (the only barrier: every wave of the workgroup is still here)
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (i >= count) return;   // wave-uniform
  const int r = rows ? __builtin_amdgcn_readfirstlane(rows[i]) : i;
  if (r < 0 || r >= bank_rows) {   // wave-uniform; never dereferenced
    if (filter) {
      if (lane == 0) out[i] = r;   // (-1, or an index the load itself reports)
    } else if (lane == 0) {
      out[2 * i] = -1; out[2 * i + 1] = r;
      fault[FAULT_STATE_INDEX + 1] = (uint32_t)r;
      fault[FAULT_STATE_INDEX + 2] = kFaultCheckRow;
      fault[FAULT_STATE_INDEX] = (uint32_t)i + 1u;
    }
    return;
  }
  const uint8_t* row = bank + (size_t)r * (size_t)ck->world_stride;
  const uint64_t key = wave_min(check_share(*ck, code, row, lane, 64));
  if (lane != 0) return;
  int32_t rule, offset;
  verdict_of(key, &rule, &offset);
  if (!filter) {
    out[2 * i] = rule; out[2 * i + 1] = offset;
  } else if (rule == 0) {
    out[i] = r;
  } else {
    out[i] = -1;
    fault[FAULT_STATE_INDEX + 1] = (uint32_t)r;
    fault[FAULT_STATE_INDEX + 2] = kFaultCheckRefused | ((uint32_t)rule << 8);
    fault[FAULT_STATE_INDEX] = (uint32_t)i + 1u;
    // (one refused world of the launch owns words 12-15; a report not yet read stays)
    if (atomicCAS(&fault[kFaultCheckWorld], 0u, (uint32_t)i + 1u) == 0u) {
      fault[kFaultCheckWorld + 1] = (uint32_t)r;
      fault[kFaultCheckWorld + 2] = (uint32_t)rule;
      fault[kFaultCheckWorld + 3] = (uint32_t)offset;
    }
  }
}

// The values byte array `level` of GraduatedSanctionsMarking can take: from 1, a hit at level 1
// adds inc[0], a hit at any other level adds inc[1] (step_territory.h:389-398), as a byte.
void sanction_levels(const int32_t inc[2], uint8_t* lo, uint8_t* hi) {
  bool seen[256] = {};
  int todo[256], n = 0;
  seen[1] = true; todo[n++] = 1;
  while (n > 0) {
    const int l = todo[--n];
    const int next = (l + inc[l == 1 ? 0 : 1]) & 255;
    if (!seen[next]) { seen[next] = true; todo[n++] = next; }
  }
  *lo = 255; *hi = 0;
  for (int l = 0; l < 256; ++l)
    if (seen[l]) { if (l < *lo) *lo = (uint8_t)l; if (l > *hi) *hi = (uint8_t)l; }
}

}  // namespace

void build_check_tables(const DecodedPack& d, CheckTables* out) {
  const DevTables& t = d.t;
  CheckTables ck = {};
  ck.H = t.H; ck.W = t.W; ck.L = t.L; ck.P = t.P; ck.nstates = t.nstates;
  ck.grid_planes = t.grid_planes; ck.grid_bytes = t.grid_bytes; ck.grid_pad = t.grid_pad;
  ck.world_stride = t.world_stride; ck.max_frames = t.max_frames; ck.avatar_layer = t.avatar_layer;
  ck.substrate = d.sub.substrate;
  // state -> layer, and the player whose avatar state it is: the step's own table (sinfo of the
  // LDS tables, step_common.h), so that "avatar p's state" means here what it means to a step —
  // coins' avatars have one alive state per colour
  const uint32_t* sinfo = reinterpret_cast<const uint32_t*>(d.step_blob.data());
  for (int s = 0; s < 256; ++s) {
    const bool is_state = s < t.nstates;
    const int layer = is_state && t.state_layer[s] >= 0 && t.state_layer[s] < 255 ? t.state_layer[s] : 255;
    const uint32_t player = is_state && d.step_blob.size() >= kSinfoBytes ?sinfo[s] >> 24 : 0u;
    ck.code[s] = (uint16_t)((uint32_t)layer | (player << 8));
  }
  ck.aux_lo = 0; ck.aux_hi = -1;
  for (int k = 0; k < 16; ++k) { ck.byte_lo[k] = 0; ck.byte_hi[k] = 255; }
  ck.marker_plane = -1; ck.follow_plane = -1;
  const uint8_t maxx = (uint8_t)(t.W - 1 < 255 ? t.W - 1 : 255), maxy = (uint8_t)(t.H - 1 < 255 ? t.H - 1 : 255);
  switch (d.sub.substrate) {
    case MPK_SUBSTRATE_CLEAN_UP:
      // aux_count indexes apple_thr[n_dirt + 1] (step_clean_up.h:137)
      ck.aux_lo = 0; ck.aux_hi = d.sub.cu.n_dirt;
      break;
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING: {
      // every avatar's cell is read and written on the overlay plane whether it lives or not
      // (step_cook.h:155, 159, 234); its inventory piece is connected to it (A14)
      const CookTables& c = d.sub.cc;
      ck.byte_hi[F_AX] = maxx; ck.byte_hi[F_AY] = maxy;
      ck.follow_plane = c.overlay_layer;
      ck.follow_lo[0] = c.s_plain0; ck.follow_n[0] = 4;
      ck.follow_lo[1] = c.s_off0; ck.follow_n[1] = 4;
      ck.follow_lo[2] = c.s_dir0; ck.follow_n[2] = 12;
      break;
    }
    case MPK_SUBSTRATE_COOP_MINING:
      // a miner set is a mask of avatars (step_coop.h:195-207)
      ck.plane_rule[0] = {d.sub.cm.plane_m, PLANE_RULE_SHIFT_MAX, t.P < 8 ? t.P : 8, 0};
      break;
    case MPK_SUBSTRATE_GIFT_REFINEMENTS: {
      // the inventory counts (step_gift.h:98, 150, 186)
      const int cap = d.sub.gr.capacity < 255 ? d.sub.gr.capacity : 255;
      ck.byte_hi[F_FLAG0] = ck.byte_hi[F_FLAG1] = ck.byte_hi[F_LEVEL] = (uint8_t)(cap > 0 ? cap : 0);
      break;
    }
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS: {
      // the marking's own position is used whether it is on the map or waits
      // (step_mushroom.h:303-320, 442-513).  (A live mushroom's type indexes the pack's tables,
      // :339-361: rules 1 and 2 bound it, the decoder refuses a pack whose mushroom layer holds any
      // state but the four types, pack_decode.hip:826-831.)
      const MushroomTables& c = d.sub.em;
      ck.byte_hi[F_CTIMER] = maxx; ck.byte_hi[F_FLAG1] = maxy;
      sanction_levels(c.lv_increment, &ck.byte_lo[F_LEVEL], &ck.byte_hi[F_LEVEL]);
      ck.byte_hi[F_FLAG0] = ck.byte_hi[F_LEVEL];
      ck.marker_plane = c.mark_layer; ck.marker_state = F_FLAG0; ck.marker_x = F_CTIMER; ck.marker_y = F_FLAG1;
      ck.marker_cell = 1;
      break;
    }
    case MPK_SUBSTRATE_TERRITORY: {
      // claimedBy + 1 indexes reward_count[16] (step_territory.h:297); the marking's state
      // indexes s_mark[2] (:572) and lies on its avatar's cell, dead or alive (:338, :572)
      const TerritoryTables& c = d.sub.tr;
      ck.plane_rule[0] = {c.plane_a, PLANE_RULE_SHIFT_MAX, 3, t.P};
      sanction_levels(c.lv_increment, &ck.byte_lo[F_LEVEL], &ck.byte_hi[F_LEVEL]);
      ck.byte_hi[F_FLAG0] = ck.byte_hi[F_LEVEL];
      ck.marker_plane = c.mark_layer; ck.marker_state = F_FLAG0; ck.marker_x = F_AX; ck.marker_y = F_AY;
      ck.marker_cell = 0;
      break;
    }
    case MPK_SUBSTRATE_THE_MATRIX: {
      // the readiness marker's own position is used whether it is on the map or not
      // (step_matrix.h:320-344, 531-595)
      const MatrixTables& c = d.sub.mx;
      ck.byte_hi[F_CTIMER] = maxx; ck.byte_hi[F_NOZAP] = maxy;
      ck.marker_plane = c.mark_layer; ck.marker_state = F_FLAG0; ck.marker_x = F_CTIMER; ck.marker_y = F_NOZAP;
      ck.marker_cell = 1;
      break;
    }
    default: break;   // commons_harvest, coins: the generic rules are all
  }
  *out = ck;
}

void check_rows_host(const CheckTables& ck, const uint8_t* bank, int bank_rows, const int32_t* rows,
                     int count, int32_t* out) {
  for (int i = 0; i < count; ++i) {
    const int r = rows ? rows[i] : i;
    if (r < 0 || r >= bank_rows) { out[2 * i] = -1; out[2 * i + 1] = r; continue; }
    const uint8_t* row = bank + (size_t)r * (size_t)ck.world_stride;
    verdict_of(check_share(ck, ck.code, row, 0, 1), &out[2 * i], &out[2 * i + 1]);
  }
}

void launch_check_states(const CheckTables* ck, const uint8_t* bank, int bank_rows, const int32_t* rows,
                         int count, int32_t* out, uint32_t* fault, hipStream_t stream) {
  hipLaunchKernelGGL(k_check_states, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, ck, bank,
                     bank_rows, rows, count, out, 0, fault);
}

void launch_filter_states(const CheckTables* ck, const uint8_t* bank, int bank_rows, const int32_t* src,
                          int num_worlds, int32_t* checked, uint32_t* fault, hipStream_t stream) {
  hipLaunchKernelGGL(k_check_states, dim3((unsigned)((num_worlds + 3) / 4)), dim3(256), 0, stream, ck,
                     bank, bank_rows, src, num_worlds, checked, 1, fault);
}
