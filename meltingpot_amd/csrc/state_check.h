// state_check.h — is a world record well-formed?  (An MpStatesCheck request, include/mp_engine.h;
// DESIGN.md §3.9 has the rule table and the source lines each rule protects.)
//
// A record (mp_common.h) is the one input that reaches the step kernels as bytes: load_world
// (step_load.h) copies a bank row over the LDS record and the level's rules then use its bytes as
// cell coordinates, state ids and table indices.  The rules here say which records those kernels
// can take.  They are plain `__host__ __device__` functions over
//   CheckTables   what the host stage knows about the pack (built once, build_check_tables),
//   code[256]     CheckTables::code where a lane can index it (LDS in the kernel),
//   row           the record, read where it lies,
//   (lane, lanes) this caller's share of the work: element i is looked at by the caller with
//                 i % lanes == lane,
// so that the kernel (state_check.hip: one wavefront per row, lanes = 64) and the host loop
// (lanes = 1) run the same text.  Every function returns the smallest violation it saw as a key
// (rule << 32 | offset word), kNoViolation for none; the row's verdict is the minimum over all
// callers, which does not depend on how the work was shared.
//
// This header includes mp_common.h only: the step and frame kernels are compiled from what they
// were compiled from before.
#ifndef MP_STATE_CHECK_H_INTERNAL_
#define MP_STATE_CHECK_H_INTERNAL_

#include <stddef.h>
#include <string.h>

#include "mp_common.h"

// ---- the tail's fields, once ---------------------------------------------------------------
// Every member of WorldTail in declaration order.  The layout a caller is told (MpStateLayout)
// and the offsets the rules use both come from this list and offsetof(); the asserts below fail
// the build when the struct and the list disagree (a member added, removed, reordered, padded).
#define MP_TAIL_FIELDS(X)                                                                          \
  X(ax) X(ay) X(aori) X(aalive) X(ztimer) X(ctimer) X(flag0) X(flag1) X(freeze) X(removal)        \
  X(aflags) X(nozap) X(level) X(tsince) X(achange) X(step) X(frame) X(done) X(cont) X(aux_count)  \
  X(group_change) X(episode) X(started) X(seed) X(ctr) X(reward_fx) X(orders_step) X(next_orders)

namespace state_check {

template <class T> struct ElemOf { static constexpr int size = (int)sizeof(T); };
template <class T, size_t N> struct ElemOf<T[N]> { static constexpr int size = (int)sizeof(T); };

struct TailField { const char* name; int offset, elem, count; };

#define MP_TAIL_FIELD_ROW(f)                                                                \
  {#f, (int)offsetof(WorldTail, f), ElemOf<decltype(WorldTail::f)>::size,                   \
   (int)(sizeof(WorldTail::f) / ElemOf<decltype(WorldTail::f)>::size)},
constexpr TailField kTailFields[] = {MP_TAIL_FIELDS(MP_TAIL_FIELD_ROW)};
#undef MP_TAIL_FIELD_ROW
constexpr int kNumTailFields = (int)(sizeof(kTailFields) / sizeof(kTailFields[0]));

constexpr bool tail_fields_cover_the_struct() {
  int at = 0;
  for (int i = 0; i < kNumTailFields; ++i) {
    if (kTailFields[i].offset != at) return false;
    at += kTailFields[i].elem * kTailFields[i].count;
  }
  return at == (int)sizeof(WorldTail);
}
static_assert(tail_fields_cover_the_struct(),
              "MP_TAIL_FIELDS must list every member of WorldTail, in order, without gaps");

// The per-avatar byte arrays at the head of the tail: field k < kByteFields is uint8 [16].
constexpr int kByteFields = 14;
constexpr bool byte_fields_are_bytes() {
  for (int i = 0; i < kByteFields; ++i)
    if (kTailFields[i].elem != 1 || kTailFields[i].count != MP_MAX_PLAYERS ||
        kTailFields[i].offset != i * MP_MAX_PLAYERS)
      return false;
  return kTailFields[kByteFields].elem != 1;
}
static_assert(byte_fields_are_bytes(), "the tail starts with kByteFields uint8[16] arrays");
enum { F_AX = 0, F_AY, F_AORI, F_AALIVE, F_ZTIMER, F_CTIMER, F_FLAG0, F_FLAG1, F_FREEZE,
       F_REMOVAL, F_AFLAGS, F_NOZAP, F_LEVEL, F_TSINCE };
static_assert(offsetof(WorldTail, tsince) == F_TSINCE * MP_MAX_PLAYERS &&
                  offsetof(WorldTail, flag0) == F_FLAG0 * MP_MAX_PLAYERS &&
                  offsetof(WorldTail, nozap) == F_NOZAP * MP_MAX_PLAYERS,
              "F_* number the byte arrays in the struct's order");

// ---- rules -----------------------------------------------------------------------------------
enum {
  RULE_OK = 0,
  RULE_STATE_RANGE = 1,    // a render plane's byte is no state of the pack
  RULE_STATE_LAYER = 2,    // a render plane's byte is a state of another layer
  RULE_TAIL_RANGE = 3,     // aori, aalive, done, cont, started, step
  RULE_AVATAR_CELL = 4,    // a living avatar is off the map, or not where the tail says
  RULE_AVATAR_STRAY = 5,   // an avatar's state where the tail does not put that avatar
  RULE_ORDERS = 6,         // the cached visiting orders
  RULE_LEVEL = 7           // a level's own use of the record; sub-code in the offset's top byte
};
// RULE_LEVEL sub-codes (offset word = sub << 24 | byte offset in the row)
enum {
  LEVEL_BYTE_FIELD = 1,    // + k: per-avatar byte array k (F_*) outside the level's range: 1 .. 14
  LEVEL_AUX_COUNT = 16,    // aux_count outside the level's table
  LEVEL_PLANE0 = 17,       // CheckTables::plane_rule[0], [1]
  LEVEL_PLANE1 = 18,
  LEVEL_MARKER_OFF_MAP = 19,   // a marker on the map whose position is not a cell
  LEVEL_MARKER_CELL = 20,      // a marker on the map whose cell of the marker plane is empty
  LEVEL_FOLLOWER = 21          // an avatar without its connected piece on its cell
};

constexpr uint64_t kNoViolation = ~0ull;
__host__ __device__ inline uint64_t violation(int rule, uint32_t offset_word) {
  return ((uint64_t)(uint32_t)rule << 32) | offset_word;
}
__host__ __device__ inline uint64_t worse(uint64_t a, uint64_t b) { return a < b ? a : b; }
__host__ __device__ inline uint32_t level_word(int sub, int offset) {
  return ((uint32_t)sub << 24) | ((uint32_t)offset & 0xffffffu);
}

// A rule over the bytes of one plane (render or hidden).
enum {
  PLANE_RULE_NONE = 0,
  PLANE_RULE_SHIFT_MAX = 1    // (byte >> a) <= b
};
struct PlaneRule { int32_t plane, kind, a, b; };

// What the rules know about the pack.  Built on the host from the decoded pack; the kernel reads
// it from device memory with uniform addresses (and `code` from its LDS copy).
struct CheckTables {
  int32_t H, W, L, P, nstates, grid_planes, grid_bytes, grid_pad, world_stride;
  int32_t max_frames, avatar_layer, substrate;
  // RULE_LEVEL
  int32_t aux_lo, aux_hi;               // aux_count's range; lo > hi: any value is fine
  uint8_t byte_lo[16], byte_hi[16];     // per-avatar byte array k of avatars p < P: lo <= v <= hi
  PlaneRule plane_rule[2];
  // a marker piece with a position of its own in the tail: on the map while byte array
  // `marker_state` is non-zero, at (marker_x, marker_y) (byte arrays); marker_plane < 0: none.
  // marker_cell: its cell of marker_plane then holds a piece.
  int32_t marker_plane, marker_state, marker_x, marker_y, marker_cell;
  // a piece connected to every avatar (alive or not) on follow_plane: its cell holds a state of
  // one of three spans [lo, lo + n); follow_plane < 0: none
  int32_t follow_plane, follow_lo[3], follow_n[3];
  int32_t pad_[2];
  // state -> layer (bits 0-7; 255: no such state) | (player whose avatar state it is + 1) << 8
  uint16_t code[256];
};
static_assert(sizeof(CheckTables) % 16 == 0, "CheckTables is copied in 16-byte lines");

// ---- the record's bytes ------------------------------------------------------------------------
__host__ __device__ inline uint32_t row_u32(const uint8_t* row, int off) {
#ifdef __HIP_DEVICE_COMPILE__
  return *reinterpret_cast<const uint32_t*>(row + off);   // (tail words are 4-byte aligned)
#else
  uint32_t v;
  memcpy(&v, row + off, 4);
  return v;
#endif
}
// Sixteen bytes of the row at a multiple of 16 (one lane load in the kernel).
struct Line16 { uint32_t w[4]; };
__host__ __device__ inline Line16 row_line(const uint8_t* row, int off) {
  Line16 l;
#ifdef __HIP_DEVICE_COMPILE__
  const uint4 v = *reinterpret_cast<const uint4*>(row + off);
  l.w[0] = v.x; l.w[1] = v.y; l.w[2] = v.z; l.w[3] = v.w;
#else
  memcpy(l.w, row + off, 16);
#endif
  return l;
}
__host__ __device__ inline int tail_off(const CheckTables& ck, int field, int p) {
  return ck.grid_pad + field * MP_MAX_PLAYERS + p;
}

// ---- rules 1, 2, 5 and the level's plane rules: every byte of the planes -------------------------
// The planes are walked in 16-byte lines (a line may straddle two planes); what follows the
// last plane in front of the tail — the matrix games' player block, the padding up to grid_pad —
// is not looked at.
__host__ __device__ inline uint64_t check_planes(const CheckTables& ck, const uint16_t* code,
                                                 const uint8_t* row, int lane, int lanes) {
  uint64_t bad = kNoViolation;
  const int HW = ck.H * ck.W, render = ck.L * HW, all = ck.grid_planes * HW;
  const int nline = (all + 15) >> 4;
  for (int v = lane; v < nline; v += lanes) {
    const Line16 line = row_line(row, v * 16);
    int plane = (v * 16) / HW, cell = v * 16 - plane * HW;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int off = v * 16 + b;
      const uint32_t s = (line.w[b >> 2] >> (8 * (b & 3))) & 255u;
      if (off < all) {
        if (off < render) {
          if (s != 0u) {
            const uint32_t e = code[s];
            if ((int)s >= ck.nstates) {
              bad = worse(bad, violation(RULE_STATE_RANGE, (uint32_t)off));
            } else if ((int)(e & 255u) != plane) {
              bad = worse(bad, violation(RULE_STATE_LAYER, (uint32_t)off));
            } else if ((e >> 8) != 0u && (int)(e >> 8) <= ck.P) {
              // an avatar's state: only where the tail puts that avatar, and only while it lives
              const int p = (int)(e >> 8) - 1;
              const int alive = row[tail_off(ck, F_AALIVE, p)];
              const int x = row[tail_off(ck, F_AX, p)], y = row[tail_off(ck, F_AY, p)];
              if (!alive || x >= ck.W || y >= ck.H || y * ck.W + x != cell)
                bad = worse(bad, violation(RULE_AVATAR_STRAY, (uint32_t)off));
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const PlaneRule& pr = ck.plane_rule[k];
          if (pr.kind == PLANE_RULE_NONE || pr.plane != plane) continue;
          if ((int)(s >> pr.a) > pr.b) bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_PLANE0 + k, off)));
        }
      }
      if (++cell == HW) { cell = 0; ++plane; }
    }
  }
  return bad;
}

// ---- rules 3, 4, 6 and the level's tail rules ----------------------------------------------------
// Caller `lane` judges avatar p = lane, lane + lanes, ... < P; the world's scalars and stream g of
// the orders are judged by the callers that own elements 0 and g.  Bytes of avatars >= P, ctr[],
// reward_fx, frame, episode, seed, achange, the timers and group_change are not judged: the
// kernels take any value of them.
__host__ __device__ inline uint64_t check_tail(const CheckTables& ck, const uint16_t* code,
                                               const uint8_t* row, int lane, int lanes) {
  uint64_t bad = kNoViolation;
  const int P = ck.P, W = ck.W, H = ck.H, HW = ck.H * ck.W, T = ck.grid_pad;
  // (a world that was never reset holds zeros: a range's lower end is asked of started worlds)
  const bool started = row_u32(row, T + (int)offsetof(WorldTail, started)) != 0u;
  for (int p = lane; p < P; p += lanes) {
    const int x = row[tail_off(ck, F_AX, p)], y = row[tail_off(ck, F_AY, p)];
    const int alive = row[tail_off(ck, F_AALIVE, p)];
    if (row[tail_off(ck, F_AORI, p)] >= 4)
      bad = worse(bad, violation(RULE_TAIL_RANGE, (uint32_t)tail_off(ck, F_AORI, p)));
    if (alive > 1) bad = worse(bad, violation(RULE_TAIL_RANGE, (uint32_t)tail_off(ck, F_AALIVE, p)));
    if (alive) {
      if (x >= W) bad = worse(bad, violation(RULE_AVATAR_CELL, (uint32_t)tail_off(ck, F_AX, p)));
      if (y >= H) bad = worse(bad, violation(RULE_AVATAR_CELL, (uint32_t)tail_off(ck, F_AY, p)));
      if (x < W && y < H) {
        const int off = ck.avatar_layer * HW + y * W + x;
        if ((int)(code[row[off]] >> 8) != p + 1)
          bad = worse(bad, violation(RULE_AVATAR_CELL, (uint32_t)off));
      }
    }
    // the level's ranges of the per-avatar bytes
#pragma unroll
    for (int k = 0; k < kByteFields; ++k) {
      const int v = row[tail_off(ck, k, p)];
      if ((started && v < ck.byte_lo[k]) || v > ck.byte_hi[k])
        bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_BYTE_FIELD + k, tail_off(ck, k, p))));
    }
    if (ck.marker_plane >= 0 && row[tail_off(ck, ck.marker_state, p)] != 0) {
      const int mx = row[tail_off(ck, ck.marker_x, p)], my = row[tail_off(ck, ck.marker_y, p)];
      if (mx >= W)
        bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_MARKER_OFF_MAP, tail_off(ck, ck.marker_x, p))));
      else if (my >= H)
        bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_MARKER_OFF_MAP, tail_off(ck, ck.marker_y, p))));
      else if (ck.marker_cell && row[ck.marker_plane * HW + my * W + mx] == 0)
        bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_MARKER_CELL, ck.marker_plane * HW + my * W + mx)));
    }
    if (ck.follow_plane >= 0 && started && x < W && y < H) {
      const int off = ck.follow_plane * HW + y * W + x, s = row[off];
      bool ok = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) ok = ok || (s >= ck.follow_lo[k] && s < ck.follow_lo[k] + ck.follow_n[k]);
      if (!ok) bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_FOLLOWER, off)));
    }
  }
  const int o_step = T + (int)offsetof(WorldTail, step), o_orders = T + (int)offsetof(WorldTail, orders_step);
  const int32_t step = (int32_t)row_u32(row, o_step);
  const uint32_t orders_step = row_u32(row, o_orders);
  if (lane == 0) {
    const int o_done = T + (int)offsetof(WorldTail, done), o_cont = T + (int)offsetof(WorldTail, cont);
    const int o_started = T + (int)offsetof(WorldTail, started), o_aux = T + (int)offsetof(WorldTail, aux_count);
    if (step < 0 || step > ck.max_frames) bad = worse(bad, violation(RULE_TAIL_RANGE, (uint32_t)o_step));
    if (row_u32(row, o_done) > 1u) bad = worse(bad, violation(RULE_TAIL_RANGE, (uint32_t)o_done));
    if (row_u32(row, o_cont) > 1u) bad = worse(bad, violation(RULE_TAIL_RANGE, (uint32_t)o_cont));
    if (row_u32(row, o_started) > 1u) bad = worse(bad, violation(RULE_TAIL_RANGE, (uint32_t)o_started));
    // (step + 1 in 64 bits: a step of INT_MAX is rule 3's, not an overflow here)
    if (orders_step != 0u && (int64_t)orders_step != (int64_t)step + 1)
      bad = worse(bad, violation(RULE_ORDERS, (uint32_t)o_orders));
    const int32_t aux = (int32_t)row_u32(row, o_aux);
    if (ck.aux_lo <= ck.aux_hi && (aux < ck.aux_lo || aux > ck.aux_hi))
      bad = worse(bad, violation(RULE_LEVEL, level_word(LEVEL_AUX_COUNT, o_aux)));
  }
  // the cached orders (step_common.h: step_orders, finish): position p's entry holds, in nibble
  // g, the avatar stream g visits p-th — per stream a permutation of the P avatars.  Read only
  // while orders_step names the next step, judged whenever it names any.
  if (orders_step != 0u) {
    const int o_next = T + (int)offsetof(WorldTail, next_orders);
    for (int g = lane; g < 4; g += lanes) {
      uint32_t seen = 0;
      for (int p = 0; p < P; ++p) {
        const uint32_t lo = row[o_next + 2 * p], hi = row[o_next + 2 * p + 1];
        const uint32_t a = ((lo | (hi << 8)) >> (4 * g)) & 15u;
        if ((int)a >= P || ((seen >> a) & 1u)) {
          bad = worse(bad, violation(RULE_ORDERS, (uint32_t)(o_next + 2 * p)));
          break;
        }
        seen |= 1u << a;
      }
    }
  }
  return bad;
}

// The whole verdict of one caller's share.
__host__ __device__ inline uint64_t check_share(const CheckTables& ck, const uint16_t* code,
                                                const uint8_t* row, int lane, int lanes) {
  return worse(check_planes(ck, code, row, lane, lanes), check_tail(ck, code, row, lane, lanes));
}

// (rule, offset word) of a key as the two int32 a caller gets; (0, 0) for a well-formed row.
__host__ __device__ inline void verdict_of(uint64_t key, int32_t* rule, int32_t* offset) {
  *rule = key == kNoViolation ? 0 : (int32_t)(key >> 32);
  *offset = key == kNoViolation ? 0 : (int32_t)(uint32_t)key;
}

}  // namespace state_check

// The check's own reports through DevTables::fault (mp_common.h: FAULT_STATE_INDEX, IndexFault): a row a
// checked load refused (word 9 = world + 1, word 10 = the row, word 11 = kFaultCheckRefused |
// rule << 8), and a rows[] index of a check that is no row of the bank (word 9 = position + 1,
// word 10 = the index, word 11 = kFaultCheckRow).  The load that follows a filter reports the
// indices IT skips through the same three words, so a refusal is also kept in words of its own,
// which the next synchronising call reports first: word 12 = world + 1, 13 = the row, 14 = the
// rule, 15 = the offset word.  Of several refused worlds of one launch ONE claims word 12 (a
// compare-and-swap from 0) and writes the other three: the four words name one world.  Words
// 9-11 are plain stores, as everywhere: theirs may belong to different worlds.
// kFaultCheckWorld is that word's offset in DevTables::fault, not a code of IndexFault.
constexpr int kFaultCheckWorld = 12;

struct DecodedPack;
// The rules' view of a decoded pack (host pointers: host_stage's decode); no HIP call.
void build_check_tables(const DecodedPack& d, state_check::CheckTables* out);
// Verdicts of host rows by the host loop: out[i] = (rule, offset word) of row rows[i] (NULL: i).
// An index outside [0, bank_rows) gives (-1, index).
void check_rows_host(const state_check::CheckTables& ck, const uint8_t* bank, int bank_rows,
                     const int32_t* rows, int count, int32_t* out);
// Verdicts of device rows (out: device int32 [count][2]); `ck` is the tables' device copy.
void launch_check_states(const state_check::CheckTables* ck, const uint8_t* bank, int bank_rows,
                         const int32_t* rows, int count, int32_t* out, uint32_t* fault,
                         hipStream_t stream);
// A checked load's filter: checked[w] = src[w] unless row src[w] is a row of the bank and
// malformed — then -1, reported through `fault`.
void launch_filter_states(const state_check::CheckTables* ck, const uint8_t* bank, int bank_rows,
                          const int32_t* src, int num_worlds, int32_t* checked, uint32_t* fault,
                          hipStream_t stream);

#endif  // MP_STATE_CHECK_H_INTERNAL_
