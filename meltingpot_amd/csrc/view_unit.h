// view_unit.h — what the units that read every viewer's window of a record share (ego_layer.hip,
// view_hash.hip, ego_planes.hip; DESIGN.md §3.12–3.14): a (rows kernel, views kernel) pair, one
// wave per element.  A wave stages what ego_layer::cell_of and ego_layer::value read of its record
// in its share of the LDS — the render planes and the head of the tail (positions, orientations,
// who is alive) — and the unit's own body works on that.  Here: the LDS layout, the staging loop,
// the report of a skipped rows[] / players[] index, the launch plan, launch and prepare, and the
// host twin's element loop.  Included by those three units and by avatar_ids.hip,
// which stages one plane of the record with the same loop.
#ifndef MP_VIEW_UNIT_H_INTERNAL_
#define MP_VIEW_UNIT_H_INTERNAL_

#include <stddef.h>

#include "step_common.h"
#include "ego_layer.h"

namespace view_unit {

using ego_layer::Plan;
using ego_layer::Window;
using stepk::issued;
using stepk::wsync;

constexpr int kLdsMax = 160 * 1024;
constexpr int kMaxWaves = 16;
constexpr int kHead = 4 * MP_MAX_PLAYERS;   // ax, ay, aori, aalive
static_assert(offsetof(WorldTail, ax) == 0 && offsetof(WorldTail, ay) == MP_MAX_PLAYERS &&
                  offsetof(WorldTail, aori) == 2 * MP_MAX_PLAYERS && offsetof(WorldTail, aalive) == 3 * MP_MAX_PLAYERS,
              "the staged head of the tail is ax, ay, aori, aalive");

// a wave's LDS begins with the render planes in whole 16-byte vectors, then the head; a workgroup
// that folds the viewers' value tables [P][kLayerLutRow] keeps them in front, in whole vectors too
__host__ __device__ inline int planes_vec(const Window& g) { return (g.L * g.HW + 15) >> 4; }
__host__ __device__ inline int tables_bytes(const Window& g) { return ((g.P * kLayerLutRow * 4 + 15) >> 4) * 16; }

// Element i of a launch is row rows[i] (NULL: row i) and, in a views kernel, viewer players[i].  An
// index of rows[] that is no row or of players[] outside [0, P) is never used as one: the wave
// goes on to its next element, that element of the destination stays as it was — every such
// element — and ONE of them is reported through the fault words (FAULT_STATE_INDEX; the first to
// claim them) with the unit's own code.  (The two checks stand in each body's element loop, around
// its `continue`: as a function here they compile to other code in four of the six kernels.)
__device__ inline void report(uint32_t* fault, int at, int index, uint32_t what) {
  if (atomicCAS(&fault[FAULT_STATE_INDEX], 0u, (uint32_t)at + 1u) == 0u) {
    fault[FAULT_STATE_INDEX + 1] = (uint32_t)index;
    fault[FAULT_STATE_INDEX + 2] = what;
  }
}
__device__ inline void report_index(uint32_t* fault, int lane, int at, int index, uint32_t what) {
  if (lane == 0) report(fault, at, index, what);
}

// The wave copies record `rec` into its LDS: the planes' `nvec` vectors to `planes`, the head (at
// rec + grid_pad) to `head`.  16-byte loads, eight of a lane in flight (state_view.hip,
// step_load.h).  The caller's wsync() stands before and behind it.
__device__ inline void stage_record(const uint8_t* rec, int grid_pad, int nvec, int lane, uint8_t* planes,
                                    uint8_t* head) {
  const uint4* src = reinterpret_cast<const uint4*>(rec);
  uint4* out = reinterpret_cast<uint4*>(planes);
  const uint4 hv = lane < kHead / 16 ? src[(grid_pad >> 4) + lane] : uint4{0u, 0u, 0u, 0u};
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
  if (lane < kHead / 16) reinterpret_cast<uint4*>(head)[lane] = hv;
}

// Geometry of a launch of `count` elements: `tables` bytes of LDS a workgroup, `per` a wave.
inline Plan plan_of(int tables, int per, int count, int num_cus) {
  Plan p = {};
  int fit = tables < kLdsMax ? (kLdsMax - tables) / per : 0;
  if (fit < 1) { p.lds = tables + per; return p; }
  if (fit > kMaxWaves) fit = kMaxWaves;
  // every CU a workgroup before a workgroup gets more waves
  const int cus = num_cus > 0 ? num_cus : 1;
  int waves = (count + cus - 1) / cus;
  if (waves < 4) waves = 4;
  if (waves > fit) waves = fit;
  if (waves > count) waves = count;
  p.waves = waves;
  p.groups = (count + waves - 1) / waves;
  if (p.groups > 2 * cus) p.groups = 2 * cus;   // (a wave then takes several elements in turn)
  p.lds = tables + waves * per;
  return p;
}

// `rows` (a.players == NULL) or `views`, on `stream`.
template <class A>
inline void launch(void (*rows)(A), void (*views)(A), const A& a, const Plan& p, hipStream_t stream) {
  hipLaunchKernelGGL(a.players ? views : rows, dim3((unsigned)p.groups), dim3((unsigned)p.waves * 64u), (size_t)p.lds,
                     stream, a);
}

// hipFuncSetAttribute(max dynamic LDS) of the pair; 0 or the hipError_t.
template <class A>
inline int prepare(void (*rows)(A), void (*views)(A)) {
  const void* k[2] = {reinterpret_cast<const void*>(rows), reinterpret_cast<const void*>(views)};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// The host twin's loop: each(i, rec, p, q, np) for viewer p, the q-th of element i's np, of record
// `rec`.  Returns -1, or the first position whose rows[] / players[] index is out of range (*what
// = row_code or player_code); every element before it has been visited.
template <class A, class F>
inline int host_each(const A& a, uint32_t row_code, uint32_t player_code, uint32_t* what, F each) {
  for (int i = 0; i < a.count; ++i) {
    const int r = a.rows ? a.rows[i] : i;
    if (r < 0 || r >= a.src_rows) { *what = row_code; return i; }
    const int p = a.players ? a.players[i] : 0;
    if (p < 0 || p >= a.g.P) { *what = player_code; return i; }
    const uint8_t* rec = a.src + (size_t)r * (size_t)a.stride;
    const int np = a.players ? 1 : a.g.P;
    for (int q = 0; q < np; ++q) each(i, rec, (uint32_t)(p + q), q, np);
  }
  return -1;
}

}  // namespace view_unit

#endif  // MP_VIEW_UNIT_H_INTERNAL_
