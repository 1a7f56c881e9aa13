// ego_planes.h — class-indicator feature planes of a player's view (an MpEgoPlanes request,
// include/mp_engine.h): what a conv net reads of EGO_LAYER.  uint8, channels
// first, [C'][VH][VW] a viewer, every byte 0 or 1, worked out from the record without drawing the
// int32 view.
//
// With E the viewer's EGO_LAYER, int32 [VH][VW][L] (ego_layer.h), and `classes` a table that maps
// every id to a class in [-1, C):
//     out[c][i][j]     = 1 iff some counted layer l has classes[E[i][j][l]] == c        (c < C)
//     out[C + d][i][j] = 1 iff the viewer is alive, window cell (i, j) lies on the map at (x, y),
//                        and a living avatar q stands on (x, y) with ((aori[q] - aori[p]) & 3) == d
// (the four facing planes exist with `facing` only).  The per-cell functions are written once, for
// the kernels (ego_planes.hip) and for the host twin: the class mask is ego_layer::value — the one
// EGO_LAYER is drawn with — on a value table with the classes folded in, with the cell found once
// for all of its layers.
//
// This header includes ego_layer.h only.
#ifndef MP_EGO_PLANES_H_INTERNAL_
#define MP_EGO_PLANES_H_INTERNAL_

#include <stdint.h>

#include "ego_layer.h"

namespace ego_planes {

using ego_layer::Window;

constexpr int kMaxClasses = 64;   // a cell's classes are the bits of one u64

// An entry of a class table as the class it names: itself in [0, num_classes), else -1 ("nothing").
MP_EGO_HD inline int32_t class_of(int32_t entry, int32_t num_classes) {
  return (uint32_t)entry < (uint32_t)num_classes ? entry : -1;
}

using ego_layer::cell_of;

// The classes of window cell (vx, vy) of viewer p: bit c is set iff a layer of `layer_mask` (never
// 0 here: "every layer" is all ones) holds an id of class c.  `table`: the viewers' value tables
// [P][kLayerLutRow] with the classes folded in, class_of(classes[lut[p][s]]).  Layer l's term is
// ego_layer::value(g, planes, head, table, p, vx, vy, l) with the cell worked out once for all
// layers (cell_of), so that the L reads of a cell do not wait for one another.
MP_EGO_HD inline uint64_t cell_classes(const Window& g, const uint8_t* planes, const uint8_t* head,
                                       const int32_t* table, uint64_t layer_mask, uint32_t p, uint32_t vx,
                                       uint32_t vy) {
  int x, y;
  const bool in = cell_of(g, head, p, vx, vy, &x, &y);
  const uint8_t* at = planes + y * g.W + x;
  const int32_t* row = table + p * (uint32_t)kLayerLutRow;
  uint64_t m = 0ull;
#pragma unroll 4
  for (int l = 0; l < g.L; ++l) {
    const int s = in ? (int)at[l * g.HW] : 256;
    const int32_t c = row[s];
    m |= c >= 0 && ((layer_mask >> l) & 1u) ? 1ull << c : 0ull;
  }
  return m;
}

// The facings at window cell (vx, vy) of viewer p: bit d is set iff the viewer is alive, the cell
// maps to a cell (x, y) of the map and a living avatar q < P stands there with
// ((aori[q] - aori[p]) & 3) == d.  The viewer itself is bit 0 at (vl, vf).
MP_EGO_HD inline uint32_t cell_facing(const Window& g, const uint8_t* head, uint32_t p, uint32_t vx, uint32_t vy) {
  int x, y;
  if (!cell_of(g, head, p, vx, vy, &x, &y)) return 0u;
  const int vo = head[2 * MP_MAX_PLAYERS + p];
  uint32_t f = 0u;
  for (int q = 0; q < g.P; ++q)
    if (head[3 * MP_MAX_PLAYERS + q] && (int)head[q] == x && (int)head[MP_MAX_PLAYERS + q] == y)
      f |= 1u << (((int)head[2 * MP_MAX_PLAYERS + q] - vo) & 3);
  return f;
}

// What a launch reads and writes.  Element i of `dst` belongs to row rows[i] (NULL: row i) of
// `src` ([src_rows] records `stride` bytes apart, 16-byte aligned): uint8 [P][C'][VH][VW], every
// viewer's planes (players == NULL), or [C'][VH][VW] of viewer players[i]; C' = num_classes, + 4
// with `facing`.  `dst` may start on any byte.
struct Args {
  Window g;
  const uint8_t* src;
  const int32_t* rows;
  const int32_t* players;
  uint8_t* dst;
  const int32_t* lut;
  const int32_t* classes;   // int32 [num_ids]
  uint32_t* fault;          // DevTables::fault
  uint64_t layer_mask;      // bit l: layer l counts (never 0)
  int32_t num_ids, num_classes, facing;
  int32_t src_rows, count;
  int32_t stride, grid_pad;
};

inline int planes_of(const Args& a) { return a.num_classes + (a.facing ? 4 : 0); }

// Geometry of a launch: waves a workgroup (one element each at a time), workgroups, dynamic LDS
// (the workgroup's folded value tables, then every wave's render planes, head and bit planes).
// waves == 0: the tables and one wave's share do not fit the LDS (`lds` = what they would take).
using ego_layer::Plan;
Plan plan_of(const Window& g, int num_planes, int count, int num_cus);

// k_ego_planes_rows (players == NULL) or k_ego_planes_views, on `stream`.
void launch(const Args& a, const Plan& p, hipStream_t stream);
// hipFuncSetAttribute(max dynamic LDS) of the kernels; 0 or the hipError_t.
int prepare();

// The same function on HOST rows, with no device: dst as a launch's; every entry of a.classes is
// in [-1, num_classes) (the caller has checked).  Returns -1, or the first position whose rows[] /
// players[] index is out of range (*what = kFaultEgoPlanesRow or kFaultEgoPlanesPlayer); every
// element before it is written.
int host(const Args& a, uint32_t* what);

}  // namespace ego_planes

#endif  // MP_EGO_PLANES_H_INTERNAL_
