// state_view.h — what the host hands the kernels that draw sampled (row, player) views of a bank
// of saved records (state_view.hip; an MpStatesView request, include/mp_engine.h).
#ifndef MP_STATE_VIEW_H_INTERNAL_
#define MP_STATE_VIEW_H_INTERNAL_

#include "mp_common.h"

// Geometry of a k_state_view launch (state_view_plan): waves a workgroup (one view each at a
// time), workgroups, dynamic LDS.  waves == 0: one wave's share does not fit the LDS (`lds` = what
// it would take).
struct StateViewPlan {
  int32_t waves, groups, lds;
  uint32_t view_bytes;   // what the launch writes per element
};
// kind: MP_OBS_LAYER, MP_OBS_RGB or MP_OBS_RGB_POOL2/4/8.
StateViewPlan state_view_plan(const DevTables& t, int kind, int count, int num_cus);

// Element i of `dst` (`count` elements of the kind's per-player layout, on any byte the kind's
// element size allows) = the view of player players[i] of row rows[i] (NULL: row i) of `bank`.
// LAYER and the pixel kinds; layer_lut: StepOutputs::layer_lut.
void launch_state_view(const DevTables& t, const StateViewPlan& plan, int kind, const uint8_t* bank,
                       int bank_rows, const int32_t* rows, const int32_t* players, int count,
                       void* dst, const int32_t* layer_lut, hipStream_t stream);
// MP_OBS_READY_TO_SHOOT, MP_OBS_POSITION, MP_OBS_ORIENTATION or MP_OBS_INVENTORY.
void launch_state_view_scalar(const DevTables& t, const SubstrateTables& s, int kind,
                              const uint8_t* bank, int bank_rows, const int32_t* rows,
                              const int32_t* players, int count, void* dst, hipStream_t stream);
// hipFuncSetAttribute(max dynamic LDS) of the kernels; 0 or the hipError_t.
int prepare_state_view();

#endif  // MP_STATE_VIEW_H_INTERNAL_
