// state_hash.hip — the hash of world records (state_hash.h has the function and the mask; an
// MpStatesHash request, include/mp_engine.h).  A unit of its own that includes none of the step
// headers: k_frame, the single-step and the K-step kernels, k_check_states, k_save_worlds and the
// state_obs kernels are compiled from exactly what they were compiled from before.
//
//   k_hash_rows   one wavefront per row, four rows per 256-thread workgroup (the geometry of
//                 k_check_states and k_save_worlds).  The row and the mask are read where they
//                 lie, in 16-byte lane loads (the mask's lines from L2 after the first wave); a
//                 wave-wide 64-bit sum by __shfl_xor reduces the lanes' shares; lane 0 stores the
//                 8 bytes.  No LDS, no barrier.
// An index outside the bank is never used as one: element i of out keeps what it held and the
// fault words report the index.
#include "pack_decode.h"
#include "state_check.h"
#include "state_hash.h"

namespace {

using namespace state_hash;

__global__ __launch_bounds__(256) void k_hash_rows(const uint32_t* __restrict__ mask,
                                                   const uint8_t* __restrict__ bank, int bank_rows, int stride,
                                                   const int32_t* __restrict__ rows, int count,
                                                   uint64_t* __restrict__ out, uint32_t* fault) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (i >= count) return;   // wave-uniform
  const int r = rows ? __builtin_amdgcn_readfirstlane(rows[i]) : i;
  if (r < 0 || r >= bank_rows) {   // wave-uniform; never dereferenced, out[i] left as it was
    if (lane == 0) {
      fault[FAULT_STATE_INDEX + 1] = (uint32_t)r;
      fault[FAULT_STATE_INDEX + 2] = kFaultHashRow;
      fault[FAULT_STATE_INDEX] = (uint32_t)i + 1u;
    }
    return;
  }
  const uint8_t* row = bank + (size_t)r * (size_t)stride;
  const uint64_t sum = wave_sum(hash_share(mask, row, stride >> 4, lane, 64));
  if (lane == 0) out[i] = fmix64(sum);
}

}  // namespace

state_hash::Layout hash_layout_of(const DecodedPack& d) {
  state_check::CheckTables ck;
  build_check_tables(d, &ck);
  return layout_of(ck, d.sub.substrate == MPK_SUBSTRATE_THE_MATRIX ? d.sub.mx.player_block : -1);
}

int hash_rows_host(const uint32_t* mask, const uint8_t* bank, int bank_rows, int stride,
                   const int32_t* rows, int count, uint64_t* out) {
  int bad = -1;
  for (int i = 0; i < count; ++i) {
    const int r = rows ? rows[i] : i;
    if (r < 0 || r >= bank_rows) {
      if (bad < 0) bad = i;
      continue;
    }
    out[i] = fmix64(hash_share(mask, bank + (size_t)r * (size_t)stride, stride >> 4, 0, 1));
  }
  return bad;
}

void launch_hash_rows(const uint32_t* mask, const uint8_t* bank, int bank_rows, int stride,
                      const int32_t* rows, int count, uint64_t* out, uint32_t* fault, hipStream_t stream) {
  hipLaunchKernelGGL(k_hash_rows, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, mask, bank,
                     bank_rows, stride, rows, count, out, fault);
}
