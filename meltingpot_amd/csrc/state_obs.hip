// state_obs.hip — observations of rows of a bank of saved records (an MpStatesObserve request,
// include/mp_engine.h), read from the rows where they lie: no world is loaded, nothing of the
// engine's is written.  A unit of its own: k_frame, the single-step and the K-step kernels are
// compiled from exactly what they were compiled from before.
//
//   k_state_obs     the four scalar kinds that are functions of the record — what load_world's
//                   block of record functions and load_level_obs (step_load.h) write for a loaded
//                   world: one thread per (row, avatar), the tail and, for the matrix games, the
//                   player block read straight from the row;
//   k_gather_rows   the rows a pixel kind or LAYER draws, copied next to each other for the
//                   draw-only frame launch or k_layer_view (which take contiguous records).
// An index of rows[] outside the bank is never used as one: it is reported through the fault
// words (FAULT_STATE_INDEX) and its element of the destination stays as it was (behind a gather:
// for up to kObsStashSlots such elements of a request).  Several such indices of one launch
// write the three fault words without order among them: one is reported, and the position and
// the value in the message may belong to two different ones.
#include "../../include/mp_pack.h"
#include "step_load.h"
#include "state_obs.h"
#include "state_obs_rules.h"

namespace {

using namespace stepk;

template <class Tables>
__global__ __launch_bounds__(256) void k_state_obs(DevTables t, Tables c, int kind,
                                                   const uint8_t* __restrict__ bank, int bank_rows,
                                                   const int32_t* __restrict__ rows, int count,
                                                   void* __restrict__ dst) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)count * t.P) return;
  const int i = (int)(id / t.P), p = (int)(id - (long long)i * t.P);
  const int r = rows ? rows[i] : i;
  if (r < 0 || r >= bank_rows) {
    report_state_index(t, p, i, r, (int)kFaultObserveRow);
    return;
  }
  const uint8_t* rec = bank + (size_t)r * t.world_stride;
  const WorldTail* tail = reinterpret_cast<const WorldTail*>(rec + t.grid_pad);
  const size_t o = (size_t)id;
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

// One wave per row, as k_save_worlds copies a record (16-byte lines, eight of a lane in flight).
__global__ __launch_bounds__(256) void k_gather_rows(DevTables t, const uint8_t* __restrict__ bank, int bank_rows,
                                                     const int32_t* __restrict__ rows, int count,
                                                     uint8_t* __restrict__ scratch,
                                                     const uint8_t* __restrict__ dst, uint64_t elem_bytes,
                                                     uint8_t* __restrict__ stash) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (i >= count) return;
  const int r = __builtin_amdgcn_readfirstlane(rows[i]);
  const int nvec = t.world_stride >> 4;
  uint4* out = reinterpret_cast<uint4*>(scratch + (size_t)i * t.world_stride);
  if (r < 0 || r >= bank_rows) {
    report_state_index(t, lane, i, r, (int)kFaultObserveRow);
    for (int j = lane; j < nvec; j += 64) out[j] = uint4{0u, 0u, 0u, 0u};
    uint32_t* ctl = reinterpret_cast<uint32_t*>(stash);
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(&ctl[0], 1u);
    slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
    if (slot < (uint32_t)kObsStashSlots) {
      if (lane == 0) ctl[1 + slot] = (uint32_t)i;
      const uint8_t* from = dst + (uint64_t)i * elem_bytes;
      uint8_t* to = stash + 64 + (uint64_t)slot * elem_bytes;
      for (uint64_t j = (uint64_t)lane; j < elem_bytes; j += 64) to[j] = from[j];
    }
    return;
  }
  const uint4* src = reinterpret_cast<const uint4*>(bank + (size_t)r * t.world_stride);
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
}

// One workgroup puts back the elements the stash holds (none, for a request whose indices were all
// rows) and leaves it empty for the next request.
__global__ __launch_bounds__(256) void k_restore_stash(uint8_t* __restrict__ dst, uint64_t elem_bytes,
                                                       uint8_t* __restrict__ stash) {
  uint32_t* ctl = reinterpret_cast<uint32_t*>(stash);
  const uint32_t taken = ctl[0] < (uint32_t)kObsStashSlots ? ctl[0] : (uint32_t)kObsStashSlots;
  for (uint32_t s = 0; s < taken; ++s) {
    const uint8_t* from = stash + 64 + (uint64_t)s * elem_bytes;
    uint8_t* to = dst + (uint64_t)ctl[1 + s] * elem_bytes;
    for (uint64_t j = threadIdx.x; j < elem_bytes; j += 256) to[j] = from[j];
  }
  __syncthreads();   // every thread has read ctl[0]
  if (threadIdx.x == 0 && taken) ctl[0] = 0;
}

}  // namespace

static_assert(kObsStashWords * 4 <= 64, "the stash's control words take its first 64 bytes");

void launch_state_obs(const DevTables& t, const SubstrateTables& s, int kind, const uint8_t* bank,
                      int bank_rows, const int32_t* rows, int count, void* dst, hipStream_t stream) {
  const long long n = (long long)count * t.P;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define MP_LAUNCH(tables)                                                                        \
  hipLaunchKernelGGL(k_state_obs, grid, block, 0, stream, t, tables, kind, bank, bank_rows, rows, \
                     count, dst);                                                                 \
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

void launch_gather_rows(const DevTables& t, const uint8_t* bank, int bank_rows, const int32_t* rows,
                        int count, uint8_t* scratch, const uint8_t* dst, uint64_t elem_bytes,
                        uint8_t* stash, hipStream_t stream) {
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, t, bank,
                     bank_rows, rows, count, scratch, dst, elem_bytes, stash);
}

void launch_restore_stash(uint8_t* dst, uint64_t elem_bytes, uint8_t* stash, hipStream_t stream) {
  hipLaunchKernelGGL(k_restore_stash, dim3(1), dim3(256), 0, stream, dst, elem_bytes, stash);
}
