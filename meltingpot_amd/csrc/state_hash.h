// state_hash.h — are two world records the same state?  (An MpStatesHash request and the
// MP_STEP_ROW_HASH row of a K-step request, include/mp_engine.h)
//
// Two records of one world state differ legitimately: ctr[] and reward_fx are the destination
// engine's bookkeeping, the cached visiting orders may be there or not, and the padding and the
// bytes of avatars >= P hold whatever an edit left.  A byte compare of rows therefore says
// "different" of equal states.  The hash here is a function of exactly the bytes a state's future
// and its observations depend on, chosen by a byte mask over the row (a "spec").
//
// With w_j the little-endian u32 at byte 4 j of the row and m_j the mask word of the same place
// (0xFF in every included byte):
//     c_j = fmix64((j + 1) << 32 | (w_j & m_j))      for every j with m_j != 0
//     H   = fmix64(sum_j c_j mod 2^64)
// fmix64 is a bijection of u64, so changing one included byte always changes H and changing an
// excluded byte never does; the sum commutes, so H does not depend on how callers share the words
// — the property the minimum gives state_check.h.  hash_share is plain `__host__ __device__` text
// over (mask, row, this caller's share): the kernel (one wavefront per row, lanes = 64), the
// K-step kernels (the record in LDS) and the host loop (lanes = 1) run the same lines.
//
// The mask has ONE source: build_byte_mask below, from the layout state_check.h's tables carry
// and its list of the tail's fields.  No offset is written down a second time.
//
// This header includes mp_common.h and state_check.h only.
#ifndef MP_STATE_HASH_H_INTERNAL_
#define MP_STATE_HASH_H_INTERNAL_

#include "mp_common.h"
#include "state_check.h"

namespace state_hash {

// ---- the tail's fields by index: bit i of a field mask is field i of MP_TAIL_FIELDS --------------
enum TailIndex {
#define MP_TAIL_INDEX(f) TF_##f,
  MP_TAIL_FIELDS(MP_TAIL_INDEX)
#undef MP_TAIL_INDEX
  TF_COUNT
};
static_assert(TF_COUNT == state_check::kNumTailFields && TF_COUNT < 32, "a field mask is a u32");
constexpr uint32_t kAllFields = (1u << TF_COUNT) - 1u;
// Not part of "the state": the destination engine's bookkeeping, and a cache that may be absent.
constexpr uint32_t kBookkeeping =
    (1u << TF_ctr) | (1u << TF_reward_fx) | (1u << TF_orders_step) | (1u << TF_next_orders);

// Which bytes count.  custom == 0: the default spec, "the state" (every plane, the level's block
// where there is one, every tail field but kBookkeeping); the other members are then ignored.
struct Spec {
  uint64_t plane_mask;   // bit l: grid plane l
  uint32_t field_mask;   // bit i: tail field i
  int32_t custom;
  int32_t player_block;  // the level's block [player_block, grid_bytes)
};
inline bool same_spec(const Spec& a, const Spec& b) {
  if (!a.custom || !b.custom) return !a.custom && !b.custom;
  return a.plane_mask == b.plane_mask && a.field_mask == b.field_mask && !a.player_block == !b.player_block;
}

// What the mask needs to know about the pack.
struct Layout { int32_t HW, P, grid_planes, grid_bytes, grid_pad, world_stride, player_block; };
inline Layout layout_of(const state_check::CheckTables& ck, int player_block) {
  return Layout{ck.H * ck.W, ck.P, ck.grid_planes, ck.grid_bytes, ck.grid_pad, ck.world_stride, player_block};
}

// NULL for a spec this layout can take, else what is wrong with it.
inline const char* spec_error(const Layout& l, const Spec& s) {
  if (!s.custom) return nullptr;
  if (l.grid_planes > 64) return "a custom spec names planes by a 64-bit mask; this pack has more than 64 planes";
  if (l.grid_planes < 64 && (s.plane_mask >> l.grid_planes) != 0) return "plane_mask has a bit that names no plane";
  if ((s.field_mask & ~kAllFields) != 0) return "field_mask has a bit that names no field of the tail";
  if (s.player_block && l.player_block < 0) return "this level keeps no player block";
  if (s.plane_mask == 0 && s.field_mask == 0 && !s.player_block) return "the spec includes no byte";
  return nullptr;
}

// The spec's byte mask, uint8 [world_stride]: 0xFF where a byte is included.  Never included:
// what lies behind the planes in front of the level's block, the padding up to grid_pad, what
// follows the tail's last field, and the elements >= P of every 16-element (per-avatar) field.
inline void build_byte_mask(const Layout& l, const Spec& s, uint8_t* bytes) {
  for (int i = 0; i < l.world_stride; ++i) bytes[i] = 0;
  for (int p = 0; p < l.grid_planes; ++p)
    if (!s.custom || (p < 64 && ((s.plane_mask >> p) & 1u)))
      for (int i = 0; i < l.HW; ++i) bytes[p * l.HW + i] = 0xFF;
  if (l.player_block >= 0 && (!s.custom || s.player_block))
    for (int i = l.player_block; i < l.grid_bytes; ++i) bytes[i] = 0xFF;
  const uint32_t fields = s.custom ? s.field_mask : kAllFields & ~kBookkeeping;
  for (int f = 0; f < TF_COUNT; ++f) {
    if (!((fields >> f) & 1u)) continue;
    const state_check::TailField& tf = state_check::kTailFields[f];
    const int count = tf.count == MP_MAX_PLAYERS ? l.P : tf.count;
    for (int i = 0; i < tf.elem * count; ++i) bytes[l.grid_pad + tf.offset + i] = 0xFF;
  }
}

// ---- the function -----------------------------------------------------------------------------
__host__ __device__ inline uint64_t fmix64(uint64_t h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// This caller's part of the sum: the 16-byte lines v = lane, lane + lanes, ... < nline of the row
// and of the mask (u32 [4 nline]; both 16-byte aligned, read where they lie).
__host__ __device__ inline uint64_t hash_share(const uint32_t* mask, const uint8_t* row, int nline,
                                               int lane, int lanes) {
  uint64_t sum = 0;
  for (int v = lane; v < nline; v += lanes) {
    const state_check::Line16 m = state_check::row_line(reinterpret_cast<const uint8_t*>(mask), v * 16);
    const state_check::Line16 l = state_check::row_line(row, v * 16);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint64_t c = fmix64(((uint64_t)(uint32_t)(v * 4 + b + 1) << 32) | (l.w[b] & m.w[b]));
      sum += m.w[b] != 0u ? c : 0ull;
    }
  }
  return sum;
}

#ifdef __HIPCC__
// The wave's sum, in every lane.  Called by all 64 lanes (uniform control flow).
__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
#endif

}  // namespace state_hash

struct DecodedPack;
// The layout of a decoded pack's rows (host pointers: host_stage's decode); no HIP call.
state_hash::Layout hash_layout_of(const DecodedPack& d);
// H of host rows by the host loop: out[i] = H(row rows[i]) (NULL: row i).  An index outside
// [0, bank_rows) leaves out[i] as it was; returns the position of the first such index, -1: none.
int hash_rows_host(const uint32_t* mask, const uint8_t* bank, int bank_rows, int stride,
                   const int32_t* rows, int count, uint64_t* out);
// H of device rows (out: device u64 [count]; `mask`: device u32 [stride / 4]).
void launch_hash_rows(const uint32_t* mask, const uint8_t* bank, int bank_rows, int stride,
                      const int32_t* rows, int count, uint64_t* out, uint32_t* fault, hipStream_t stream);

#endif  // MP_STATE_HASH_H_INTERNAL_
