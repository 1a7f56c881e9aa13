/* mp_episode_starts.h — registered episode starts (MpEpisodeStarts) as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the request that mp_restore carries (mp_engine.h documents the semantics and the
 * refusals).  Same return codes as every entry point. */
#ifndef MP_EPISODE_STARTS_H_
#define MP_EPISODE_STARTS_H_

#include <string.h>

#include "mp_engine.h"

/* From now on a world of `eng` that auto-resets starts from row rows_device[w] of bank_device
 * (uint8 [bank_rows][S]; -1: the level's own reset).  verdicts_device: int32 [bank_rows][2] of an
 * MP_CHECK_ROWS request over the whole bank, or NULL (every row is taken).  All three are read in
 * place by every later stepping submission: keep them alive until the registration is cleared or
 * replaced.  No launch, no synchronisation. */
static inline int mp_set_episode_starts(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                        const int32_t* rows_device, const int32_t* verdicts_device,
                                        int32_t fresh, uint64_t fingerprint) {
  MpEpisodeStarts r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.fresh = fresh;
  r.fingerprint = fingerprint;
  r.bank = bank_device;
  r.rows = rows_device;
  r.verdicts = verdicts_device;
  r.bank_rows = bank_rows;
  if (!eng || !bank_device) return mp_restore(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_restore(eng, &r, sizeof r);
}

/* Episodes start from the level's own map again. */
static inline int mp_clear_episode_starts(MpEngine* eng) {
  MpEpisodeStarts r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  if (!eng) return mp_restore(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_restore(eng, &r, sizeof r);
}

#endif /* MP_EPISODE_STARTS_H_ */
