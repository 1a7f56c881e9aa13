// step_many.h — what the host hands the K-step kernels (step_many.hip) besides StepArgs, and the
// one description of a per-step row that the host's check (engine_requests.hip: step_request) reads.
#ifndef MP_STEP_MANY_H_INTERNAL_
#define MP_STEP_MANY_H_INTERNAL_

#include "step_common.h"

// The geometry of the stand-alone step kernels (step_kernels.hip), which the K-step ones share.
int step_lds_bytes(const DevTables& t, const SubstrateTables& s, int wpg);
int step_worlds_per_group(const DevTables& t, const SubstrateTables& s);

// One step of every world (step_kernels.hip), the same with the engine's registered episode
// starts (step_starts.hip), and mp_observe's LAYER from the records in HBM (step_kernels.hip).
void launch_step(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                 hipStream_t stream);
int prepare_step();
void launch_step_starts(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const stepk::StartArgs& st, hipStream_t stream);
int prepare_step_starts();
void launch_layer_view(const DevTables& t, const uint8_t* state, int32_t* out, int num_worlds,
                       hipStream_t stream);

// Every kind a K-step launch can stack per step, by MpObsKind: its name in messages, its element
// size (a row distance is a multiple of it, a buffer aligned to it) and where its rows go — slot
// `slot` of ManyArgs::row (the five kinds of MpStepMany) or of StepRows::fin, StepRows::layer, or
// one of StepRows::level.  name == NULL: no per-step rows (the pixel kinds).  The last entry,
// index kStepRowStateIndex, is MP_STEP_ROW_STATE: the world's record itself (StateRows), which
// is no observation kind (step_row_index maps a request's kind to its entry); behind it, index
// kStepRowHashIndex, MP_STEP_ROW_HASH: the record's 64-bit hash (HashRows).
enum StepRowPlace { kRowFive = 1, kRowFin, kRowLayer, kRowLevel, kRowState, kRowHash };
constexpr int kStepRowStateIndex = MP_OBS_KINDS;
constexpr int kStepRowHashIndex = MP_OBS_KINDS + 1;
constexpr int kStepRowCount = MP_OBS_KINDS + 2;
constexpr int step_row_index(int kind) {
  return kind == MP_STEP_ROW_STATE  ? kStepRowStateIndex
         : kind == MP_STEP_ROW_HASH ? kStepRowHashIndex
         : kind >= 0 && kind < MP_OBS_KINDS ? kind : -1;
}
struct StepRowKind {
  const char* name;
  int elem;
  int place;
  int slot;
};
struct StepRowKinds { StepRowKind of[kStepRowCount]; };
constexpr StepRowKinds make_step_row_kinds() {
  StepRowKinds k = {};
  k.of[MP_OBS_REWARD] = {"REWARD", 8, kRowFive, 0};
  k.of[MP_OBS_COLLECTIVE_REWARD] = {"COLLECTIVE_REWARD", 8, kRowFive, 1};
  k.of[MP_OBS_STEP_TYPE] = {"STEP_TYPE", 4, kRowFive, 2};
  k.of[MP_OBS_DISCOUNT] = {"DISCOUNT", 8, kRowFive, 3};
  k.of[MP_OBS_EVENTS] = {"EVENTS", 16, kRowFive, 4};   // (rows are stored as int4)
  k.of[MP_OBS_READY_TO_SHOOT] = {"READY_TO_SHOOT", 8, kRowFin, 0};
  k.of[MP_OBS_AUX0] = {"AUX0", 8, kRowFin, 1};
  k.of[MP_OBS_POSITION] = {"POSITION", 4, kRowFin, 2};
  k.of[MP_OBS_ORIENTATION] = {"ORIENTATION", 4, kRowFin, 3};
  k.of[MP_OBS_LAYER] = {"LAYER", 4, kRowLayer, 0};
  k.of[MP_OBS_AUX1] = {"AUX1", 8, kRowLevel, 0};
  k.of[MP_OBS_AUX2] = {"AUX2", 8, kRowLevel, 0};
  k.of[MP_OBS_AUX3] = {"AUX3", 8, kRowLevel, 0};
  k.of[MP_OBS_AUX4] = {"AUX4", 8, kRowLevel, 0};
  k.of[MP_OBS_ZAP_MATRIX] = {"ZAP_MATRIX", 8, kRowLevel, 0};
  k.of[MP_OBS_INVENTORY] = {"INVENTORY", 8, kRowLevel, 0};
  k.of[MP_OBS_INTERACTION_INVENTORIES] = {"INTERACTION_INVENTORIES", 8, kRowLevel, 0};
  k.of[MP_OBS_MATRIX_CUMULANTS] = {"MATRIX_CUMULANTS", 8, kRowLevel, 0};
  k.of[MP_OBS_INTERACTION_REWARDS] = {"INTERACTION_REWARDS", 8, kRowLevel, 0};
  k.of[kStepRowStateIndex] = {"STATE", 16, kRowState, 0};   // (a record is copied in 16-byte lines)
  k.of[kStepRowHashIndex] = {"HASH", 8, kRowHash, 0};     // (one u64 a world)
  return k;
}
constexpr StepRowKinds kStepRowKinds = make_step_row_kinds();

// What a K-step launch gets besides StepArgs: args.actions is step 0's block, step k's lies
// actions_step int32 further (0: the same block every step).  row[i] (NULL: not asked for) is
// row 0 of the caller's per-step buffer of kind i, row_bytes[i] the distance between two rows.
struct ManyArgs {
  int steps;
  long long actions_step;
  uint8_t* row[5];          // REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT, EVENTS
  long long row_bytes[5];
};

// The per-step rows of a request beyond MpStepMany's five: row 0 of the caller's buffer of each
// kind (NULL: not asked for) and the distance between two rows in bytes.
// Three groups of observation kinds, by who writes the kind in a step (step_many.hip: run_many):
//   fin    the kinds finish() writes for every world that is reset or stepped, element
//          w * P + lane from lane `lane`: READY_TO_SHOOT, AUX0, POSITION, ORIENTATION;
//   layer  MP_OBS_LAYER, a function of the record (`layer_lut`: StepOutputs::layer_lut);
//   level  the kinds a level's own code writes, some of them only when something happens and
//          from whichever lane it happens in (AUX1..4, ZAP_MATRIX, INVENTORY,
//          INTERACTION_INVENTORIES, MATRIX_CUMULANTS, INTERACTION_REWARDS): all f64, `count`
//          values a world, `src` the in-place (or bound) buffer the step writes.  The host
//          names the buffer by its kind (`which`: the MP_OBS_* value); launch_step_many resolves
//          `src` from the StepOutputs of THIS submission (a rollout ring points them at a new
//          slot each time).
inline const double* level_source(const StepOutputs& o, int kind) {
  switch (kind) {
    case MP_OBS_AUX1: case MP_OBS_AUX2: case MP_OBS_AUX3: case MP_OBS_AUX4:
      return o.dbg[kind - MP_OBS_AUX1];
    case MP_OBS_ZAP_MATRIX: return o.zap_matrix;
    case MP_OBS_INVENTORY: return o.inventory;
    case MP_OBS_INTERACTION_INVENTORIES: return o.interaction;
    case MP_OBS_MATRIX_CUMULANTS: return o.cumulants;
    case MP_OBS_INTERACTION_REWARDS: return o.interaction_rewards;
    default: return nullptr;
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

// The per-step world states (MP_STEP_ROW_STATE): row k = uint8 [N][world_stride], the records
// after step k (`row`: row 0, NULL: not asked for; `bytes`: the distance between two rows).  An
// argument of its own, of a kernel family of its own (k_step_states_<level>): StepRows and the
// kernels that take only it are what they were.
struct StateRows {
  uint8_t* row;
  long long bytes;
};

// The per-step state hashes (MP_STEP_ROW_HASH): row k = u64 [N], the hash (state_hash.h, the
// default spec, whose mask `mask` is: device u32 [world_stride / 4]) of the records after step k.
// An argument of its own, of a kernel family of its own (k_step_hashes_<level>), which also
// writes the state rows when the request names both.
struct HashRows {
  uint8_t* row;
  long long bytes;
  const uint32_t* mask;
};

// The mask of an MpStepActive request (step_active.hip): world w runs step k where
// active[k * step + w] != 0 (`step`: the distance between two steps' rows in bytes, 0: the same
// row every step).  active == NULL: no mask, which is every other K-step request.
struct ActiveArgs {
  const uint8_t* active;
  long long step;
};

// One checked K-step request, as submit() hands it to launch_step_many: the five kinds' rows,
// the rows of the other kinds, whether there is one of those (any_rows == false runs the
// kernels an MpStepMany request has always run), the state rows and the hash rows — and the mask
// of an MpStepActive request, with which submit() hands it to launch_step_active instead.
struct StepManyLaunch {
  ManyArgs many;
  StepRows rows;
  bool any_rows;
  StateRows state;
  HashRows hash;
  const stepk::StartArgs* starts;   // the engine's registered episode starts (submit() sets it), or NULL
  ActiveArgs active;
};

void launch_step_many(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                      const StepManyLaunch& l, hipStream_t stream);
int prepare_step_many();
// (step_active.hip)
void launch_step_active(const DevTables& t, const SubstrateTables& s, const stepk::StepArgs& args,
                        const StepManyLaunch& l, hipStream_t stream);
int prepare_step_active();

#endif  // MP_STEP_MANY_H_INTERNAL_
