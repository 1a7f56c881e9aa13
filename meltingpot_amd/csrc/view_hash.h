// view_hash.h — do two players see the same thing?  (An MpViewHash request, include/mp_engine.h;
// DESIGN.md §3.13.)  A 64-bit hash of a viewer's EGO_LAYER — the layer view in the avatar's own
// frame (ego_layer.h) — worked out from the record without drawing the view: 8 bytes a viewer.
//
// With E the viewer's EGO_LAYER, int32 [VH][VW][L], e = (vy * VW + vx) * L + l, and
//     v_e = classes ? classes[E_e] : E_e
//     c_e = fmix64((u64)(e + 1) << 32 | (u32)v_e)     for every e whose layer l is included
//     V   = fmix64(sum_e c_e mod 2^64)
// (state_hash.h's fmix64 and its construction, over the view's words instead of the row's.)  The
// word function is written once, for the kernels (view_hash.hip) and for the host twin: it calls
// ego_layer::value, the one EGO_LAYER is drawn with.
//
// This header includes ego_layer.h and state_hash.h only.
#ifndef MP_VIEW_HASH_H_INTERNAL_
#define MP_VIEW_HASH_H_INTERNAL_

#include <stdint.h>

#include "ego_layer.h"
#include "state_hash.h"

namespace view_hash {

using ego_layer::Window;

// The largest id a viewer's value table (StepOutputs::layer_lut [P][kLayerLutRow]) holds, + 1: the
// length of a class table.  0: the table holds a negative value (no pack the decoder accepts).
inline int32_t num_ids(const int32_t* lut, int P) {
  int32_t top = 0;
  for (int i = 0; i < P * kLayerLutRow; ++i) {
    if (lut[i] < 0) return 0;
    if (lut[i] > top) top = lut[i];
  }
  return top + 1;
}

// The term of word e = (cell, l) of a viewer: c_e, or 0 when `layer_mask` (never 0 here: "every
// layer" is all ones) leaves layer l out.  `classes`: NULL, or the table of num_ids entries.
MP_EGO_HD inline uint64_t term(const Window& g, const uint8_t* planes, const uint8_t* head, const int32_t* lut,
                               const int32_t* classes, uint64_t layer_mask, uint32_t p, uint32_t e, uint32_t vx,
                               uint32_t vy, uint32_t l) {
  if (!((layer_mask >> l) & 1u)) return 0ull;
  int32_t v = ego_layer::value(g, planes, head, lut, p, vx, vy, l);
  if (classes) v = classes[v];
  return state_hash::fmix64(((uint64_t)(e + 1u) << 32) | (uint64_t)(uint32_t)v);
}

// What a launch reads and writes.  Element i of `dst` belongs to row rows[i] (NULL: row i) of
// `src` ([src_rows] records `stride` bytes apart, 16-byte aligned): u64 [P], every viewer's V
// (players == NULL), or one u64, V of viewer players[i].
struct Args {
  Window g;
  const uint8_t* src;
  const int32_t* rows;
  const int32_t* players;
  uint64_t* dst;
  const int32_t* lut;
  const int32_t* classes;   // NULL, or int32 [num_classes]
  uint32_t* fault;          // DevTables::fault
  uint64_t layer_mask;      // bit l: layer l is included (never 0)
  int32_t num_classes;
  int32_t src_rows, count;
  int32_t stride, grid_pad;
};

// Geometry of a launch: waves a workgroup (one element each at a time), workgroups, dynamic LDS
// (the workgroup's copy of the viewers' value tables with the classes folded in, [P][kLayerLutRow],
// then every wave's planes and head).  waves == 0: the tables and one wave's planes do not fit the
// LDS (`lds` = what they would take).
using ego_layer::Plan;
Plan plan_of(const Window& g, int count, int num_cus);

// k_view_hash_rows (players == NULL) or k_view_hash_views, on `stream`.
void launch(const Args& a, const Plan& p, hipStream_t stream);
// hipFuncSetAttribute(max dynamic LDS) of the kernels; 0 or the hipError_t.
int prepare();

// The same function on HOST rows, with no device: dst as a launch's.  Returns -1, or the first
// position whose rows[] / players[] index is out of range (*what = kFaultViewHashRow or
// kFaultViewHashPlayer); every element before it is written.
int host(const Args& a, uint32_t* what);

}  // namespace view_hash

#endif  // MP_VIEW_HASH_H_INTERNAL_
