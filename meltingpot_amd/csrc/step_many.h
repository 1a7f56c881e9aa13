// step_many.h — what the host hands the K-step kernels (step_many.hip) besides StepArgs.
#ifndef MP_STEP_MANY_H_INTERNAL_
#define MP_STEP_MANY_H_INTERNAL_

#include "step_common.h"

// The per-step rows of an MpStepTrajectory request beyond MpStepMany's five: row 0 of the
// caller's buffer of each kind (NULL: not asked for) and the distance between two rows in bytes.
// Three groups, by who writes the kind in a step (step_many.hip: run_many):
//   fin    the kinds finish() writes for every world that is reset or stepped, element
//          w * P + lane from lane `lane`: READY_TO_SHOOT, AUX0, POSITION, ORIENTATION;
//   layer  MP_OBS_LAYER, a function of the record (`layer_lut`: StepOutputs::layer_lut);
//   level  the kinds a level's own code writes, some of them only when something happens and
//          from whichever lane it happens in (AUX1..4, ZAP_MATRIX, INVENTORY,
//          INTERACTION_INVENTORIES, MATRIX_CUMULANTS, INTERACTION_REWARDS): all f64, `count`
//          values a world, `src` the in-place (or bound) buffer the step writes.  The host
//          names the buffer by `which` (kLevel*); launch_step_many resolves `src` from the
//          StepOutputs of THIS submission (a rollout ring points them at a new slot each time).
enum { kLevelDbg0 = 0, kLevelZapMatrix = 4, kLevelInventory, kLevelInteraction, kLevelCumulants,
       kLevelInteractionRewards };
inline const double* level_source(const StepOutputs& o, int which) {
  switch (which) {
    case kLevelZapMatrix: return o.zap_matrix;
    case kLevelInventory: return o.inventory;
    case kLevelInteraction: return o.interaction;
    case kLevelCumulants: return o.cumulants;
    case kLevelInteractionRewards: return o.interaction_rewards;
    default: return o.dbg[which & 3];
  }
}

struct StepRows {
  uint8_t* fin[4];
  long long fin_bytes[4];
  uint8_t* layer;
  long long layer_bytes;
  const int32_t* layer_lut;
  int n_level;
  struct Level {
    int which;
    const double* src;
    uint8_t* row;
    long long bytes;
    long long count;
  } level[9];
};

// K steps of every world in one launch: `rows` / `row_bytes` are MpStepMany's five per-step
// buffers (NULL: not asked for), `actions_step` the distance between two steps' action blocks in
// int32.  more == NULL runs the kernels an MpStepMany request has always run.
void launch_step_many(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                      int steps, long long actions_step, void* const rows[5],
                      const uint64_t row_bytes[5], const StepRows* more, hipStream_t stream);
int prepare_step_many();

#endif  // MP_STEP_MANY_H_INTERNAL_
