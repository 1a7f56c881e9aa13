/* mp_world_states.h — the world-state operations of libmp_engine.so as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpWorldStates request that mp_snapshot / mp_restore carry (mp_engine.h documents the
 * semantics, the refusals and what a load writes).  Same return codes as every entry point. */
#ifndef MP_WORLD_STATES_H_
#define MP_WORLD_STATES_H_

#include <string.h>

#include "mp_engine.h"

/* The engine's state fingerprint (0 for a NULL engine or on error): rows load only into an engine
 * with the same value. */
static inline uint64_t mp_state_fingerprint(MpEngine* eng) {
  MpWorldStates r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_STATES_FINGERPRINT;
  if (!eng || mp_snapshot(eng, &r, sizeof r) != MP_OK) return 0;
  return r.fingerprint;
}

/* Row i of dst_device (uint8 [count][S]) = the record of world worlds_device[i] (device int32
 * [count]; NULL = every world, count = N).  Stream-ordered, no synchronisation. */
static inline int mp_save_worlds(MpEngine* eng, const int32_t* worlds_device, int32_t count,
                                 void* dst_device, uint64_t dst_bytes) {
  MpWorldStates r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_STATES_SAVE;
  r.worlds = worlds_device;
  r.count = count;
  r.bank = dst_device;
  r.bank_bytes = dst_bytes;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* World w starts from row src_device[w] of bank_device (uint8 [bank_rows][S]), -1 leaves it
 * alone: one launch shaped like a masked mp_reset.  `fingerprint`: the rows' (of the engine that
 * saved them).  Stream-ordered, no synchronisation. */
static inline int mp_load_worlds(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                 const int32_t* src_device, uint64_t fingerprint) {
  MpWorldStates r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_STATES_LOAD;
  r.bank = (void*)bank_device;
  r.bank_rows = bank_rows;
  r.src = src_device;
  r.fingerprint = fingerprint;
  if (!eng) return mp_restore(eng, NULL, 0);
  return mp_restore(eng, &r, sizeof r);
}

#endif /* MP_WORLD_STATES_H_ */
