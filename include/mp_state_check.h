/* mp_state_check.h — the layout of a world record (MpStateLayout) and the check of edited records
 * (MpStatesCheck) as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the requests that mp_snapshot carries (mp_engine.h documents the semantics, the rules and
 * the refusals).  Same return codes as every entry point. */
#ifndef MP_STATE_CHECK_H_
#define MP_STATE_CHECK_H_

#include <string.h>

#include "mp_engine.h"

/* The layout of the rows `eng` saves and loads — or, eng == NULL, of the rows an engine created
 * with mp_create(pack, pack_len, cfg) would, worked out on the host alone.  `fields` (NULL, or
 * fields_cap entries) takes the tail's named fields; out->num_fields says how many there are. */
static inline int mp_state_layout(MpEngine* eng, const void* pack, uint64_t pack_len,
                                  const MpConfig* cfg, MpStateField* fields, int32_t fields_cap,
                                  MpStateLayout* out) {
  memset(out, 0, sizeof *out);
  out->struct_size = sizeof *out;
  out->pack = pack;
  out->pack_len = pack_len;
  out->cfg = cfg;
  out->fields = fields;
  out->fields_cap = fields_cap;
  return mp_snapshot(eng, out, sizeof *out);
}

/* out_device[i] (int32 [count][2]) = the verdict (rule, offset word) of row rows_device[i] of
 * bank_device (uint8 [bank_rows][S]); rows_device NULL = rows 0 .. count - 1.  (0, 0) is a
 * well-formed row.  Stream-ordered, no synchronisation; nothing of the engine's is written. */
static inline int mp_check_states(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                  const int32_t* rows_device, int32_t count, int32_t* out_device,
                                  uint64_t fingerprint) {
  MpStatesCheck r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_CHECK_ROWS;
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

/* The same verdicts of HOST rows into a HOST out, without an engine or a device: the rows are
 * judged against the layout and tables mp_create(pack, pack_len, cfg) would have. */
static inline int mp_check_states_host(const void* pack, uint64_t pack_len, const MpConfig* cfg,
                                       const void* bank_host, int32_t bank_rows,
                                       const int32_t* rows_host, int32_t count, int32_t* out_host,
                                       uint64_t fingerprint) {
  MpStatesCheck r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_CHECK_HOST;
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

/* A checked load (include/mp_world_states.h: mp_load_worlds): checked_device[w] = src_device[w]
 * unless row src_device[w] is a malformed row of the bank, then -1; mp_load_worlds(eng, bank,
 * bank_rows, checked_device, fingerprint) afterwards loads the well-formed rows only.  Two
 * submissions, no synchronisation; a refused world is named by the next synchronising call. */
static inline int mp_filter_states(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                   const int32_t* src_device, int32_t num_worlds,
                                   int32_t* checked_device, uint64_t fingerprint) {
  MpStatesCheck r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_CHECK_FILTER;
  r.fingerprint = fingerprint;
  r.bank = bank_device;
  r.bank_rows = bank_rows;
  r.rows = src_device;
  r.count = num_worlds;
  r.out = checked_device;
  r.out_bytes = (uint64_t)(num_worlds > 0 ? num_worlds : 0) * 4u;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

#endif /* MP_STATE_CHECK_H_ */
