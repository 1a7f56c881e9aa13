// ego_layer.h — EGO_LAYER, the layer view in the avatar's own frame (an MpEgoLayer request,
// include/mp_engine.h): cell (i, j) of it names the sprites under cell (i, j) of "RGB".  The value
// function is written once, for the kernels (ego_layer.hip) and for the host twin
// (ego_layer_host), and is N.LAYER's (stepk::layer_value) with the window turned by the viewer's
// orientation, as the renderer turns it (state_view.hip).
#ifndef MP_EGO_LAYER_H_INTERNAL_
#define MP_EGO_LAYER_H_INTERNAL_

#include <stdint.h>

#include "mp_common.h"

#if defined(__HIPCC__)
#define MP_EGO_HD __host__ __device__
#else
#define MP_EGO_HD
#endif

namespace ego_layer {

// The window and the map: what the value function needs of DevTables, with the reciprocals of
// the map's extents and the offsets that make a TORUS coordinate non-negative.
struct Window {
  int32_t W, H, HW, L, P;
  int32_t vl, vf, VW, VH;
  int32_t torus, ox, oy;
  uint32_t mW, mH;
};

// n / d in one multiply (stepk::magic_of / div_by, for host and device): exact while n * d < 2^32
MP_EGO_HD inline uint32_t magic(uint32_t d) { return d > 1 ? 0xffffffffu / d + 1u : 0u; }
MP_EGO_HD inline uint32_t divm(uint32_t n, uint32_t m) { return m ? (uint32_t)(((uint64_t)n * m) >> 32) : n; }

inline Window window_of(const DevTables& t) {
  Window g;
  g.W = t.W; g.H = t.H; g.HW = t.H * t.W; g.L = t.L; g.P = t.P;
  g.vl = t.vl; g.vf = t.vf; g.VW = t.vl + t.vr + 1; g.VH = t.vf + t.vb + 1;
  g.torus = t.topology == 1;
  // (a turned offset reaches as far as the window's longest arm in either axis)
  int reach = t.vl > t.vr ? t.vl : t.vr;
  if (t.vf > reach) reach = t.vf;
  if (t.vb > reach) reach = t.vb;
  g.ox = t.W * ((reach + t.W - 1) / t.W); g.oy = t.H * ((reach + t.H - 1) / t.H);
  g.mW = magic((uint32_t)t.W); g.mH = magic((uint32_t)t.H);
  return g;
}

// The cell of the map that window cell (vx, vy) of viewer p lies over.  `head`: the head of the
// record's tail, ax[16] ay[16] aori[16] aalive[16].  The world offset of a window cell follows the
// renderer's table (the turned offset, the torus wrap).  false: (*cx, *cy) is off the map.
MP_EGO_HD inline bool turned_cell(const Window& g, const uint8_t* head, uint32_t p, uint32_t vx, uint32_t vy, int* cx,
                                  int* cy) {
  const int vo = head[2 * MP_MAX_PLAYERS + p];
  const int dx = (int)vx - g.vl, dy = (int)vy - g.vf;   // right, down in the view's frame
  const int ax = vo == 0 ? dx : vo == 1 ? -dy : vo == 2 ? -dx : dy;
  const int ay = vo == 0 ? dy : vo == 1 ? dx : vo == 2 ? -dy : -dx;
  int x = (int)head[p] + ax, y = (int)head[MP_MAX_PLAYERS + p] + ay;
  bool in;
  if (g.torus) {
    const uint32_t xx = (uint32_t)(x + g.ox), yy = (uint32_t)(y + g.oy);
    x = (int)(xx - divm(xx, g.mW) * (uint32_t)g.W);
    y = (int)(yy - divm(yy, g.mH) * (uint32_t)g.H);
    in = true;
  } else {
    in = x >= 0 && x < g.W && y >= 0 && y < g.H;
  }
  *cx = x;
  *cy = y;
  return in;
}

// The cell of the map under window cell (vx, vy) of viewer p.  false: the cell is off the map or
// the viewer is dead (A6) — EGO_LAYER's OutOfBounds — and (*cx, *cy) is (0, 0), a cell that may be
// read before the answer is looked at.
MP_EGO_HD inline bool cell_of(const Window& g, const uint8_t* head, uint32_t p, uint32_t vx, uint32_t vy, int* cx,
                              int* cy) {
  int x, y;
  bool in = turned_cell(g, head, p, vx, vy, &x, &y);
  in = in && head[3 * MP_MAX_PLAYERS + p];
  *cx = in ? x : 0;
  *cy = in ? y : 0;
  return in;
}

// EGO_LAYER's value at window cell (vx, vy), layer l of viewer p.  `planes`: the record's render
// planes [L][H][W]; `head`: as turned_cell's; `lut`: StepOutputs::layer_lut [P][kLayerLutRow].
// A cell off the map, and every cell of a dead viewer, is OutOfBounds.
MP_EGO_HD inline int32_t value(const Window& g, const uint8_t* planes, const uint8_t* head, const int32_t* lut,
                               uint32_t p, uint32_t vx, uint32_t vy, uint32_t l) {
  int x, y;
  const bool in = turned_cell(g, head, p, vx, vy, &x, &y);
  const int s = in && head[3 * MP_MAX_PLAYERS + p] ? (int)planes[(int)l * g.HW + y * g.W + x] : 256;
  return lut[p * (uint32_t)kLayerLutRow + (uint32_t)s];
}

// What a launch reads and writes.  Element i of `dst` is the block of row rows[i] (NULL: row i)
// of `src` ([src_rows] records `stride` bytes apart, 16-byte aligned): every viewer's
// [P][VH][VW][L] (players == NULL), or [VH][VW][L] of viewer players[i].
struct Args {
  Window g;
  const uint8_t* src;
  const int32_t* rows;
  const int32_t* players;
  int32_t* dst;
  const int32_t* lut;
  uint32_t* fault;        // DevTables::fault
  int32_t src_rows, count;
  int32_t stride, grid_pad;
};

// Geometry of a launch: waves a workgroup (one element each at a time), workgroups, dynamic LDS.
// waves == 0: one wave's planes do not fit the LDS (`lds` = what they would take).
struct Plan {
  int32_t waves, groups, lds;
};
Plan plan_of(const Window& g, int count, int num_cus);

// k_ego_layer_rows (players == NULL) or k_ego_layer_views, on `stream`.
void launch(const Args& a, const Plan& p, hipStream_t stream);
// hipFuncSetAttribute(max dynamic LDS) of the kernels; 0 or the hipError_t.
int prepare();

// The same function on HOST rows, with no device: dst as a launch's.  Returns -1, or the first
// position whose rows[] / players[] index is out of range (*what = kFaultEgoRow or
// kFaultEgoPlayer); every element before it is written.
int host(const Args& a, uint32_t* what);

}  // namespace ego_layer

#endif  // MP_EGO_LAYER_H_INTERNAL_
