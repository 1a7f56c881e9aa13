// step_rows.h — the per-step rows of the K-step kernels, device side: where row k of a kind lies,
// what a row holds when a step does not write the kind (the carry rule), and the copy of the level
// kinds behind a step.  run_many_masked (step_masked.h) uses all of them, under a world list with
// a shift and a column that tell the wave's world from its place in the rows.  run_many
// (step_many.hip) uses row_of ONLY: it keeps the frozen carry, the level copy and the final copy
// written out, a second copy of the carry rule, because its row families ran slower with the calls
// (profiles/r23_kstep_refactor.md).  A change to carry_fin, carry_five or copy_level_rows is made
// here AND there.  The block behind a step that writes LAYER, the state row and the hash row is
// text in both loops as well: as a function it changed the code of k_many_until_* (same note).
//
// The K-step form of run_one_world: the tables, the site lists and the record are loaded once,
// the marks and the level's extras set up once (as a feeder of k_frame does for the worlds it
// steps one after the other on one scratch), and per step only the event scratch is cleared, the
// action looked up and the level's step run on the record in LDS.  Step k + 1's action ids are
// requested before step k's work.  finish() still stores the record after every step: those are
// stores nobody waits for, and the next step works on the LDS copy; the record HBM holds in the
// end is step K's.  The five per-step kinds go to row k of the caller's buffers where given; the
// wave then copies row K - 1 to the in-place buffers, every lane reading back exactly the words
// it stored itself (program order of one thread: no fence, no second launch).
//
// Rows (an MpStepTrajectory request, `r`): per-step rows of the other non-pixel kinds, row k =
// what the in-place buffer of the kind holds after step k of the loop of single steps.  That
// buffer KEEPS its value where a step does not write the kind, so the rows carry it:
//  * r.fin (READY_TO_SHOOT, AUX0, POSITION, ORIENTATION) are retargeted to row k like the five.
//    finish() writes them on every path but the frozen one (dispatch(): done without
//    auto-reset), element w * P + lane from lane `lane` (the_matrix's second store of READY
//    too).  Before a frozen step each lane copies its own element from row k - 1 (k = 0: from
//    the in-place buffer, stored by an earlier launch) to row k: it loads what it stored
//    itself, by finish() or by this copy one step earlier, so program order of one thread
//    covers it, and a step that is not frozen pays nothing.  Row K - 1 goes to the in-place
//    buffers in the end, lane by lane, as for the five.
//  * r.level: a level writes these where and when its rules say (INTERACTION_REWARDS from the
//    two lanes of an interaction, the zap matrix from the lane of the beam cell that hit), so
//    the step keeps writing the in-place buffer and the wave copies the world's slice of it to
//    row k after the step.  Here a lane does load words that OTHER lanes of its wave stored
//    during the step.  wsync() between the step and the loads orders them: a release and an
//    acquire fence at workgroup scope around a wave barrier.  Workgroup scope is enough, since
//    the stores and the loads come from one wave on one CU, and on gfx950 it costs no
//    instruction: outside threadgroup-split mode the compiler lowers these fences to a wait for
//    LDS only, because a CU's write-through vector L1 performs the vector memory instructions
//    of a wave in the order they were issued, so a load issued behind a store of the same CU
//    sees it (no L1 invalidate, no L2 write-back: nothing another CU could observe, tens of
//    cycles where the agent-scope forms cost microseconds).  The fences are still needed: they
//    are what keeps the compiler from moving the loads.  What the copy does cost is its own
//    s_waitcnt before the stores to row k: vmcnt counts loads and stores in one order, so the
//    loaded words arrive behind the record's write-back of finish().  Only a request that names
//    one of these kinds pays that.  The loop-top wsync() keeps the next step's stores to the
//    in-place buffer behind these loads.
//  * r.layer: write_layer() on row k from the record in LDS after every step of a started
//    world, a frozen one included (the same bytes again).
//  * the state rows (MP_STEP_ROW_STATE, `sp`): store_record() of the record in LDS to row k
//    after every step of a started world — the bytes finish() has just written back to the
//    world's own record, so what MP_STATES_SAVE would copy from there.  It reads the LDS record
//    behind the same wsync() as the layer row; the loop-top wsync() keeps the next step's writes
//    behind it.
//  * the hash rows (MP_STEP_ROW_HASH, `hp`): the hash of the record in LDS (state_hash.h: every
//    lane's share of the masked words, a wave-wide sum, 8 bytes from lane 0) to element w of row
//    k, behind the same wsync() and under the same `started` test as the state row — so row k is
//    the hash of what the state row's row k holds.  The mask's lines come from device memory (L2
//    after the first wave).
// Which kinds are asked for is wave-uniform: every branch on it is a scalar one.
#ifndef MP_STEP_ROWS_H_
#define MP_STEP_ROWS_H_

#include "step_load.h"
#include "step_many.h"
#include "state_hash.h"

namespace stepk {

// Row k of a kind, or the in-place buffer where no rows are asked for.  `shift` (bytes) is for a wave
// whose world w writes column i != w of the rows (a world list, step_masked.h): the level code
// (step_world, finish(), load_world) and the carry helpers below index every output by w, so the
// row's base is moved by (i - w) worlds' elements and element w of it is column i.  The in-place
// buffers stay by world.
template <class T>
__device__ inline T* row_of(uint8_t* base, long long bytes, int k, T* in_place, long long shift = 0) {
  return base ? reinterpret_cast<T*>(base + (long long)k * bytes + shift) : in_place;
}

// The outputs of step k: row k of every kind of the five and of r.fin that is asked for, the
// in-place buffer of the others.  d = i - w worlds (row_of's shift; P players a world), 0 where
// world w is column w.
__device__ inline StepOutputs outputs_of_row(const StepOutputs& in_place, const ManyArgs& m, const StepRows& r, int k,
                                             long long d = 0, int P = 0) {
  StepOutputs o = in_place;
  o.reward = row_of(m.row[0], m.row_bytes[0], k, in_place.reward, d * P * 8);
  o.collective = row_of(m.row[1], m.row_bytes[1], k, in_place.collective, d * 8);
  o.step_type = row_of(m.row[2], m.row_bytes[2], k, in_place.step_type, d * 4);
  o.discount = row_of(m.row[3], m.row_bytes[3], k, in_place.discount, d * 8);
  o.events = row_of(m.row[4], m.row_bytes[4], k, in_place.events, d * (MP_EVENT_ROWS * 16));
  o.ready = row_of(r.fin[0], r.fin_bytes[0], k, in_place.ready, d * P * 8);
  o.aux0 = row_of(r.fin[1], r.fin_bytes[1], k, in_place.aux0, d * P * 8);
  o.position = row_of(r.fin[2], r.fin_bytes[2], k, in_place.position, d * P * 8);
  o.orientation = row_of(r.fin[3], r.fin_bytes[3], k, in_place.orientation, d * P * 4);
  return o;
}

// READY_TO_SHOOT, AUX0, POSITION and ORIENTATION of world w, where asked for as rows: `from` ->
// `to`, each lane its own element (in front of a frozen step, for a skipped one, and from row
// K - 1 to the in-place buffers in the end).
__device__ inline void carry_fin(const DevTables& t, const StepRows& r, const StepOutputs& to,
                                 const StepOutputs& from, int w, int lane) {
  if (lane >= t.P) return;
  const size_t o = (size_t)w * t.P + lane;
  if (r.fin[0]) to.ready[o] = from.ready[o];
  if (r.fin[1]) to.aux0[o] = from.aux0[o];
  if (r.fin[2]) {
    to.position[o * 2 + 0] = from.position[o * 2 + 0];
    to.position[o * 2 + 1] = from.position[o * 2 + 1];
  }
  if (r.fin[3]) to.orientation[o] = from.orientation[o];
}

// REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT and EVENTS (the header row and the rows it
// counts) of world w, where asked for as rows: `from` -> `to` (for a skipped step, and from row
// K - 1 to the in-place buffers in the end).
__device__ inline void carry_five(const DevTables& t, const ManyArgs& m, const StepOutputs& to,
                                  const StepOutputs& from, int w, int lane) {
  const size_t o = (size_t)w * t.P + lane;
  if (m.row[0] && lane < t.P) to.reward[o] = from.reward[o];
  if (lane == 0) {
    if (m.row[1]) to.collective[w] = from.collective[w];
    if (m.row[2]) to.step_type[w] = from.step_type[w];
    if (m.row[3]) to.discount[w] = from.discount[w];
  }
  if (m.row[4]) {
    const int4* src = reinterpret_cast<const int4*>(from.events) + (size_t)w * MP_EVENT_ROWS;
    int4* dst = reinterpret_cast<int4*>(to.events) + (size_t)w * MP_EVENT_ROWS;
    int n = 0;
    if (lane == 0) { const int4 h = src[0]; dst[0] = h; n = h.x; }
    n = __builtin_amdgcn_readfirstlane(n);
    n = n < 0 ? 0 : n > MP_EVENT_ROWS - 1 ? MP_EVENT_ROWS - 1 : n;
    for (int i = lane; i < n; i += 64) dst[1 + i] = src[1 + i];   // (row 1 + i: lane i % 64's own store)
  }
}

// The level kinds of world w (StepRows::level): world w's slice of the in-place buffer -> column
// `col` of row k (col = w but under a world list).
__device__ inline void copy_level_rows(const StepRows& r, int k, int w, int col, int lane) {
  for (int l = 0; l < r.n_level; ++l) {
    const long long n = r.level[l].count;
    const double* src = r.level[l].src + (size_t)w * n;
    double* dst = reinterpret_cast<double*>(r.level[l].row + (long long)k * r.level[l].bytes) + (size_t)col * n;
    for (int j = lane; j < n; j += 64) dst[j] = src[j];
  }
}

}  // namespace stepk

#endif  // MP_STEP_ROWS_H_
