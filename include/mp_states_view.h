/* mp_states_view.h — sampled (row, player) views of saved world states (MpStatesView) as a plain C
 * function.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and this wrapper
 * builds the MpStatesView request that mp_snapshot carries (mp_engine.h documents the semantics
 * and the refusals).  Same return codes as every entry point. */
#ifndef MP_STATES_VIEW_H_
#define MP_STATES_VIEW_H_

#include <string.h>

#include "mp_engine.h"

/* Element i of dst_device (`count` elements of the kind's per-player layout) = observation `kind`
 * of player players_device[i] of row rows_device[i] of bank_device (uint8 [bank_rows][S]);
 * rows_device NULL = rows 0 .. count - 1.  `fingerprint`: the rows' (of the engine that saved
 * them).  Stream-ordered, no synchronisation, no allocation; nothing of the engine's is written. */
static inline int mp_observe_views(MpEngine* eng, MpObsKind kind, const void* bank_device,
                                   int32_t bank_rows, const int32_t* rows_device,
                                   const int32_t* players_device, int32_t count, void* dst_device,
                                   uint64_t dst_bytes, uint64_t fingerprint) {
  MpStatesView r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.kind = (int32_t)kind;
  r.fingerprint = fingerprint;
  r.bank = bank_device;
  r.bank_rows = bank_rows;
  r.rows = rows_device;
  r.players = players_device;
  r.count = count;
  r.dst = dst_device;
  r.dst_bytes = dst_bytes;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

#endif /* MP_STATES_VIEW_H_ */
