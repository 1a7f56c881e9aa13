// world_view.h — the world camera's twins of EGO_LAYER and the ego planes (the MP_EGO_WORLD_* ops of
// an MpEgoLayer request and the MP_EGOPLANES_WORLD_* ops of an MpEgoPlanes request,
// include/mp_engine.h): the whole map as ids and as 0/1 planes, what "WORLD.RGB" is
// rendered from.
//
//   WORLD.LAYER    int32 [H][W][L], north up: out[y][x][l] = Wt[planes[l][y][x]], with Wt the WORLD's
//                  value table — "LAYER"'s numbering through row P of view_sprite_map, no viewer's.
//                  No cell is off the map: OutOfBounds never occurs.
//   world planes   uint8 [C'][H][W], every byte 0 or 1: class plane c is 1 where a counted layer of
//                  the cell holds an id of class c; facing plane C + d where a living avatar stands
//                  with aori == d (absolute: there is no viewer).
// The value functions are written once, for the kernels (world_view.hip) and for the host twins.
#ifndef MP_WORLD_VIEW_H_INTERNAL_
#define MP_WORLD_VIEW_H_INTERNAL_

#include <stdint.h>

#include "ego_layer.h"
#include "ego_planes.h"

namespace world_view {

using ego_layer::Plan;
using ego_layer::Window;

// The world's value table is one row of kLayerLutRow words, as a viewer's: Wt[s] for a record byte
// s, and [256] — a viewer's OutOfBounds — is 0 and never read.
// 1 + the largest id of the table: the length of a class table of the world planes.
inline int32_t num_ids(const int32_t* wt) {
  int32_t m = 0;
  for (int s = 0; s < kLayerLutRow; ++s) m = wt[s] > m ? wt[s] : m;
  return m + 1;
}

// WORLD.LAYER's word `cell` * L + l.  `planes`: the record's render planes [L][H][W].
MP_EGO_HD inline int32_t value(const Window& g, const uint8_t* planes, const int32_t* wt, uint32_t cell, uint32_t l) {
  return wt[planes[l * (uint32_t)g.HW + cell]];
}

// The classes of map cell `cell`: bit c is set iff a layer of `layer_mask` (never 0 here) holds an
// id of class c.  `table`: the world's value table with the classes folded in,
// ego_planes::class_of(classes[Wt[s]]) — layer l's term is value() on that table.
MP_EGO_HD inline uint64_t cell_classes(const Window& g, const uint8_t* planes, const int32_t* table,
                                       uint64_t layer_mask, uint32_t cell) {
  uint64_t m = 0ull;
#pragma unroll 4
  for (int l = 0; l < g.L; ++l) {
    const int32_t c = value(g, planes, table, cell, (uint32_t)l);
    m |= c >= 0 && ((layer_mask >> l) & 1u) ? 1ull << c : 0ull;
  }
  return m;
}

// The cell avatar q sets in facing plane d, or -1: it is dead, off the map, or faces another way.
// `head`: the head of the record's tail, ax[16] ay[16] aori[16] aalive[16].
MP_EGO_HD inline int avatar_cell(const Window& g, const uint8_t* head, int q, int d) {
  const int x = head[q], y = head[MP_MAX_PLAYERS + q];
  if (!head[3 * MP_MAX_PLAYERS + q] || (int)head[2 * MP_MAX_PLAYERS + q] != d || x >= g.W || y >= g.H) return -1;
  return y * g.W + x;
}

// What a WORLD.LAYER launch reads and writes.  Element i of `dst` is int32 [H][W][L] of row rows[i]
// (NULL: row i) of `src` ([src_rows] records `stride` bytes apart, 16-byte aligned).  `players` is
// NULL always: the field is what the requests' front fills in every unit's Args.
struct LayerArgs {
  Window g;
  const uint8_t* src;
  const int32_t* rows;
  const int32_t* players;
  int32_t* dst;
  const int32_t* lut;     // the world's value table, int32 [kLayerLutRow]
  uint32_t* fault;        // DevTables::fault
  int32_t src_rows, count;
  int32_t stride, grid_pad;
};

// ... and a world-planes launch: element i of `dst` is uint8 [C'][H][W], C' = num_classes, + 4 with
// `facing`.  `dst` may start on any byte.
struct PlanesArgs {
  Window g;
  const uint8_t* src;
  const int32_t* rows;
  const int32_t* players;
  uint8_t* dst;
  const int32_t* lut;
  const int32_t* classes;   // int32 [num_ids]
  uint32_t* fault;
  uint64_t layer_mask;      // bit l: layer l counts (never 0)
  int32_t num_ids, num_classes, facing;
  int32_t src_rows, count;
  int32_t stride, grid_pad;
};

inline int planes_of(const PlanesArgs& a) { return a.num_classes + (a.facing ? 4 : 0); }

// Geometry of a launch (view_unit::plan_of): the workgroup's table, then every wave's render planes
// and head and — the planes — its H * W class masks (u32 for num_classes <= 32, else u64).  waves == 0: they do not fit the LDS.
Plan layer_plan(const Window& g, int count, int num_cus);
Plan planes_plan(const Window& g, int num_classes, int count, int num_cus);

// k_world_layer_rows / k_world_planes_rows (k_world_planes_rows32 for num_classes <= 32) on `stream`.
void launch(const LayerArgs& a, const Plan& p, hipStream_t stream);
void launch(const PlanesArgs& a, const Plan& p, hipStream_t stream);
// hipFuncSetAttribute(max dynamic LDS) of the two kernels; 0 or the hipError_t.
int prepare();

// The same functions on HOST rows, with no device.  Returns -1, or the first position whose rows[]
// index is out of range; every element before it is written.  Every entry of a.classes is in
// [-1, num_classes) (the caller has checked).
int host(const LayerArgs& a);
int host(const PlanesArgs& a);

}  // namespace world_view

#endif  // MP_WORLD_VIEW_H_INTERNAL_
