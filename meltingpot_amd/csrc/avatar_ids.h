// avatar_ids.h — whom a player sees and whom it could zap (an MpAvatarIds request,
// include/mp_engine.h): the reference's AVATAR_IDS_IN_VIEW and
// AVATAR_IDS_IN_RANGE_TO_ZAP (avatar_library.lua:1204-1315), two 0/1 int32 vectors over the player
// slots, worked out from a record: its avatar_layer plane and the head of its tail.
//
//   IN_VIEW[p][q]  = 1 iff p and q are alive and some window cell of p lies over q's cell
//                    (ego_layer::cell_of).  The window is a rectangle and the turn a bijection of
//                    it, so "some window cell" is two interval tests on q's offset from p in the
//                    map's frame (in_view; on a torus the offsets count modulo the extents).
//   IN_RANGE[p][q] = 1 iff p is alive and some REACHED cell of p's zap footprint holds q's avatar
//                    state.  Footprint cell j = (lat, fw, pred) of ZapRules::shape lies at
//                    pos + lat * right(ori) + fw * forward(ori) under the map's topology
//                    (stepk::step_cell); it STOPS its ray when it lies off the map or its byte of
//                    the avatar_layer plane is not 0, and is reached when it is on the map and no
//                    cell of pred(j) stops (Zapper:getWhoZappable, :780-824: rays on the avatar's
//                    own layer only — blockers of other layers and the cooldown play no part).
// The per-cell functions are written once, for the kernels (avatar_ids.hip) and for the host twin.
//
// This header includes ego_layer.h only.
#ifndef MP_AVATAR_IDS_H_INTERNAL_
#define MP_AVATAR_IDS_H_INTERNAL_

#include <stdint.h>

#include "ego_layer.h"

namespace avatar_ids {

using ego_layer::Window;

// IN_VIEW[p][q].  `head`: ax[16] ay[16] aori[16] aalive[16].  The window reaches vl to the left,
// VW - 1 - vl to the right, vf ahead and VH - 1 - vf behind; turned by p's orientation
// (ego_layer::turned_cell) those are the offsets [xlo, xhi] x [ylo, yhi] in the map's frame.
MP_EGO_HD inline int32_t in_view(const Window& g, const uint8_t* head, uint32_t p, uint32_t q) {
  if (!head[3 * MP_MAX_PLAYERS + p] || !head[3 * MP_MAX_PLAYERS + q]) return 0;
  const int vo = head[2 * MP_MAX_PLAYERS + p];
  const int vr = g.VW - 1 - g.vl, vb = g.VH - 1 - g.vf;
  // ax = dx, -dy, -dx, dy and ay = dy, dx, -dy, -dx with dx in [-vl, vr], dy in [-vf, vb]
  const int xlo = vo == 0 ? -g.vl : vo == 1 ? -vb : vo == 2 ? -vr : -g.vf;
  const int xhi = vo == 0 ? vr : vo == 1 ? g.vf : vo == 2 ? g.vl : vb;
  const int ylo = vo == 0 ? -g.vf : vo == 1 ? -g.vl : vo == 2 ? -vb : -vr;
  const int yhi = vo == 0 ? vb : vo == 1 ? vr : vo == 2 ? g.vf : g.vl;
  int ux = (int)head[q] - (int)head[p] - xlo;   // q's offset counted from the window's low edge
  int uy = (int)head[MP_MAX_PLAYERS + q] - (int)head[MP_MAX_PLAYERS + p] - ylo;
  if (g.torus) {
    ux = ((ux % g.W) + g.W) % g.W;
    uy = ((uy % g.H) + g.H) % g.H;
  }
  return ux >= 0 && ux <= xhi - xlo && uy >= 0 && uy <= yhi - ylo ? 1 : 0;
}

// A cell of BeamShape::cell: lat (i8) | fwd (i8) << 8 | pred << 16.
MP_EGO_HD inline int cell_lat(uint32_t v) { return (int)(int8_t)(v & 255u); }
MP_EGO_HD inline int cell_fw(uint32_t v) { return (int)(int8_t)((v >> 8) & 255u); }
MP_EGO_HD inline uint32_t cell_pred(uint32_t v) { return v >> 16; }

// The cell of the map under footprint cell (lat, fw) of avatar b: false = off the map, and *cell is
// 0, a cell that may be read before the answer is looked at.  N E S W = 0 1 2 3, N = decreasing y.
MP_EGO_HD inline bool beam_cell(const Window& g, const uint8_t* head, uint32_t b, int lat, int fw, int* cell) {
  const int o = head[2 * MP_MAX_PLAYERS + b], r = (o + 1) & 3;
  int x = (int)head[b] + lat * ((r == 1) - (r == 3)) + fw * ((o == 1) - (o == 3));
  int y = (int)head[MP_MAX_PLAYERS + b] + lat * ((r == 2) - (r == 0)) + fw * ((o == 2) - (o == 0));
  bool in = true;
  if (g.torus) {
    x = ((x % g.W) + g.W) % g.W;
    y = ((y % g.H) + g.H) % g.H;
  } else {
    in = x >= 0 && x < g.W && y >= 0 && y < g.H;
  }
  *cell = in ? y * g.W + x : 0;
  return in;
}

// Does the footprint cell stop its ray?  `plane`: the record's avatar_layer plane [H][W].
MP_EGO_HD inline bool ray_stops(const uint8_t* plane, bool in, int cell) { return !in || plane[cell] != 0; }

// 1 + the player whose avatar stands on `cell`, 0: nobody's.  `sinfo`: the step tables' u32 [256]
// (step_common.h: bits 24.. = the player whose avatar state it is + 1).
MP_EGO_HD inline uint32_t avatar_at(const uint8_t* plane, const uint32_t* sinfo, int cell) {
  return sinfo[plane[cell]] >> 24;
}

// What a launch reads and writes.  Element i belongs to row rows[i] (NULL: row i) of `src`
// ([src_rows] records `stride` bytes apart, 16-byte aligned).  `dst` (IN_VIEW) and `dst_zap`
// (IN_RANGE), either may be NULL: int32 [count][P][P], every viewer's vector (players == NULL), or
// [count][P], the vector of viewer players[i].
struct Args {
  Window g;
  const uint8_t* src;
  const int32_t* rows;
  const int32_t* players;
  int32_t* dst;
  int32_t* dst_zap;
  const int32_t* lut;       // (unused: the field the three other units' launches fill)
  const uint32_t* sinfo;    // u32 [256] (needed with dst_zap)
  uint32_t* fault;          // DevTables::fault
  BeamShape shape;          // ZapRules::shape (needed with dst_zap)
  int32_t plane_at;         // byte offset of the avatar_layer plane in a record
  int32_t src_rows, count;
  int32_t stride, grid_pad;
};

// Geometry of a launch: waves a workgroup (one element each at a time), workgroups, dynamic LDS
// (the workgroup's sinfo, then every wave's plane, head and [P][P] block).  waves == 0: they do not
// fit the LDS (`lds` = what they would take).
using ego_layer::Plan;
Plan plan_of(const Window& g, int plane_at, int count, int num_cus);

// k_avatar_ids_rows (players == NULL) or k_avatar_ids_views, on `stream`.
void launch(const Args& a, const Plan& p, hipStream_t stream);
// hipFuncSetAttribute(max dynamic LDS) of the kernels; 0 or the hipError_t.
int prepare();

// The same functions on HOST rows, with no device: dst and dst_zap as a launch's.  Returns -1, or
// the first position whose rows[] / players[] index is out of range (*what = kFaultAvatarIdsRow or
// kFaultAvatarIdsPlayer); every element before it is written.
int host(const Args& a, uint32_t* what);

}  // namespace avatar_ids

#endif  // MP_AVATAR_IDS_H_INTERNAL_
