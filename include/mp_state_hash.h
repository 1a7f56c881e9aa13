/* mp_state_hash.h — the hash of world records (MpStatesHash) as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the requests that mp_snapshot carries (mp_engine.h documents the function, the specs and
 * the refusals).  Same return codes as every entry point.  Hashes compare only between rows of
 * one state fingerprint, hashed with one spec. */
#ifndef MP_STATE_HASH_H_
#define MP_STATE_HASH_H_

#include <string.h>

#include "mp_engine.h"

/* Which bytes of a row count.  All zero: the default spec, "the state". */
typedef struct {
  uint64_t plane_mask;   /* bit l = grid plane l */
  uint32_t field_mask;   /* bit i = tail field i of MpStateLayout */
  int32_t flags;         /* 0, or MP_HASH_CUSTOM [| MP_HASH_PLAYER_BLOCK] */
} MpHashSpec;

static inline void mp_hash_request_(MpStatesHash* r, int32_t op, const MpHashSpec* spec) {
  memset(r, 0, sizeof *r);
  r->struct_size = sizeof *r;
  r->op = op;
  if (spec) {
    r->plane_mask = spec->plane_mask;
    r->field_mask = spec->field_mask;
    r->flags = spec->flags;
  }
}

/* out_device[i] (u64 [count]) = H of row rows_device[i] of bank_device (uint8 [bank_rows][S]);
 * rows_device NULL = rows 0 .. count - 1; spec NULL = the default spec.  Stream-ordered, no
 * synchronisation; nothing of the engine's is written. */
static inline int mp_hash_states(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                 const int32_t* rows_device, int32_t count, uint64_t* out_device,
                                 uint64_t fingerprint, const MpHashSpec* spec) {
  MpStatesHash r;
  mp_hash_request_(&r, MP_HASH_ROWS, spec);
  r.fingerprint = fingerprint;
  r.bank = bank_device;
  r.bank_rows = bank_rows;
  r.rows = rows_device;
  r.count = count;
  r.out = out_device;
  r.out_bytes = (uint64_t)(count > 0 ? count : 0) * 8u;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* The same of the engine's own worlds where they lie: worlds_device NULL = every world, in order
 * (count = num_worlds). */
static inline int mp_hash_worlds(MpEngine* eng, const int32_t* worlds_device, int32_t count,
                                 uint64_t* out_device, const MpHashSpec* spec) {
  MpStatesHash r;
  mp_hash_request_(&r, MP_HASH_WORLDS, spec);
  r.rows = worlds_device;
  r.count = count;
  r.out = out_device;
  r.out_bytes = (uint64_t)(count > 0 ? count : 0) * 8u;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* H of HOST rows into a HOST out, without an engine or a device. */
static inline int mp_hash_states_host(const void* pack, uint64_t pack_len, const MpConfig* cfg,
                                      const void* bank_host, int32_t bank_rows, const int32_t* rows_host,
                                      int32_t count, uint64_t* out_host, uint64_t fingerprint,
                                      const MpHashSpec* spec) {
  MpStatesHash r;
  mp_hash_request_(&r, MP_HASH_HOST, spec);
  r.fingerprint = fingerprint;
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  r.bank = bank_host;
  r.bank_rows = bank_rows;
  r.rows = rows_host;
  r.count = count;
  r.out = out_host;
  r.out_bytes = (uint64_t)(count > 0 ? count : 0) * 8u;
  return mp_snapshot(NULL, &r, sizeof r);
}

/* mask_host (uint8 [mask_bytes], mask_bytes >= S) = the spec's byte mask: 0xFF where a byte of a
 * row counts.  eng, or eng == NULL with pack, pack_len, cfg. */
static inline int mp_state_hash_mask(MpEngine* eng, const void* pack, uint64_t pack_len, const MpConfig* cfg,
                                     uint8_t* mask_host, uint64_t mask_bytes, const MpHashSpec* spec) {
  MpStatesHash r;
  mp_hash_request_(&r, MP_HASH_MASK, spec);
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  r.out = mask_host;
  r.out_bytes = mask_bytes;
  return mp_snapshot(eng, &r, sizeof r);
}

#endif /* MP_STATE_HASH_H_ */
