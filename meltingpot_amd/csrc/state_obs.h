// state_obs.h — what the host hands the kernels that read observations straight from rows of a
// bank of saved records (state_obs.hip; an MpStatesObserve request, include/mp_engine.h).
#ifndef MP_STATE_OBS_H_INTERNAL_
#define MP_STATE_OBS_H_INTERNAL_

#include "mp_common.h"

// Elements of a gathered view (a pixel kind, LAYER) whose rows[] index was out of range are kept
// aside while the draw runs and put back after it; a request keeps this many.
constexpr int kObsStashSlots = 8;
// The stash's control words behind its kObsStashSlots elements: [0] slots taken, [1 + s] the
// element slot s holds.
constexpr int kObsStashWords = 1 + kObsStashSlots;

// MP_OBS_READY_TO_SHOOT, MP_OBS_POSITION, MP_OBS_ORIENTATION or MP_OBS_INVENTORY of `count` rows:
// element i of `dst` (the kind's [N]... layout) from row rows[i] (NULL: row i) of `bank`.
void launch_state_obs(const DevTables& t, const SubstrateTables& s, int kind, const uint8_t* bank,
                      int bank_rows, const int32_t* rows, int count, void* dst, hipStream_t stream);

// Row i of `scratch` = row rows[i] of `bank`, for the launches that draw contiguous records
// (the draw-only frame launch, k_layer_view).  An index out of
// range: the scratch row is zeroed (an empty record, which the launch can draw), element i of
// `dst` (`elem_bytes` each) goes to a free slot of `stash`, and the index is reported.
void launch_gather_rows(const DevTables& t, const uint8_t* bank, int bank_rows, const int32_t* rows,
                        int count, uint8_t* scratch, const uint8_t* dst, uint64_t elem_bytes,
                        uint8_t* stash, hipStream_t stream);
// ... and after the draw: the stashed elements back where they were, the stash empty again.
void launch_restore_stash(uint8_t* dst, uint64_t elem_bytes, uint8_t* stash, hipStream_t stream);

#endif  // MP_STATE_OBS_H_INTERNAL_
