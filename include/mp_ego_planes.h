/* mp_ego_planes.h — class-indicator feature planes of each player's view (MpEgoPlanes), as plain C
 * functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpEgoPlanes request that mp_snapshot carries (mp_engine.h documents the planes, the
 * semantics and the refusals).  Same return codes as every entry point. */
#ifndef MP_EGO_PLANES_H_
#define MP_EGO_PLANES_H_

#include <string.h>

#include "mp_engine.h"

/* The length a class table must have: one entry per id a view can hold.  `eng`, or (eng == NULL)
 * `pack`, `pack_len`, `cfg` as for mp_create. */
static inline int mp_ego_planes_num_ids(MpEngine* eng, const void* pack, uint64_t pack_len, const MpConfig* cfg,
                                        int32_t* num_ids) {
  MpEgoPlanes r;
  int rc;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = eng ? MP_EGOPLANES_DRAW : MP_EGOPLANES_HOST;
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  rc = mp_snapshot(eng, &r, sizeof r);
  if (rc == MP_OK && num_ids) *num_ids = r.num_ids;
  return rc;
}

/* Element i of dst_device = the planes of row rows_device[i] (NULL: row i) of bank_device (uint8
 * [bank_rows][S]; NULL: the engine's worlds, rows_device then world indices): every viewer, uint8
 * [count][P][C'][VH][VW], with players_device NULL; else of player players_device[i], uint8
 * [count][C'][VH][VW].  C' = num_classes, + 4 with `facing`.  `layer_mask`: bit l = layer l, 0 =
 * every layer; `classes_device`: int32 [classes_len], every entry in [-1, num_classes).
 * `fingerprint`: the rows' (of the engine that saved them).  dst_device may start on any byte.
 * Stream-ordered, no synchronisation, no allocation; nothing of the engine's is written. */
static inline int mp_ego_planes_draw(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                     const int32_t* rows_device, const int32_t* players_device, int32_t count,
                                     uint64_t layer_mask, const int32_t* classes_device, int32_t classes_len,
                                     int32_t num_classes, int32_t facing, void* dst_device, uint64_t dst_bytes,
                                     uint64_t fingerprint) {
  MpEgoPlanes r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_EGOPLANES_DRAW;
  r.fingerprint = fingerprint;
  r.bank = bank_device;
  r.bank_rows = bank_rows;
  r.rows = rows_device;
  r.players = players_device;
  r.count = count;
  r.layer_mask = layer_mask;
  r.classes = classes_device;
  r.classes_len = classes_len;
  r.num_classes = num_classes;
  r.facing = facing;
  r.dst = dst_device;
  r.dst_bytes = dst_bytes;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* From now on every submission is followed by one launch that rewrites every viewer's planes into
 * dst_device, uint8 [N][P][C'][VH][VW] (slots == 0), or into slot s = the ring slot the submission
 * wrote, at dst_device + s * slot_stride bytes (slots = the engine's ring slots).  dst_device NULL
 * clears the registration. */
static inline int mp_ego_planes_register(MpEngine* eng, void* dst_device, uint64_t dst_bytes, uint64_t slot_stride,
                                         int32_t slots, uint64_t layer_mask, const int32_t* classes_device,
                                         int32_t classes_len, int32_t num_classes, int32_t facing) {
  MpEgoPlanes r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_EGOPLANES_REGISTER;
  r.dst = dst_device;
  r.dst_bytes = dst_bytes;
  r.slot_stride = slot_stride;
  r.slots = slots;
  r.layer_mask = layer_mask;
  r.classes = classes_device;
  r.classes_len = classes_len;
  r.num_classes = num_classes;
  r.facing = facing;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* The planes of HOST rows into a HOST dst, computed without a device: `pack`, `pack_len`, `cfg` as
 * for mp_create; `classes_host`: a HOST table; `fingerprint`: the rows'. */
static inline int mp_ego_planes_host(const void* pack, uint64_t pack_len, const MpConfig* cfg, const void* bank_host,
                                     int32_t bank_rows, const int32_t* rows_host, const int32_t* players_host,
                                     int32_t count, uint64_t layer_mask, const int32_t* classes_host,
                                     int32_t classes_len, int32_t num_classes, int32_t facing, void* dst_host,
                                     uint64_t dst_bytes, uint64_t fingerprint) {
  MpEgoPlanes r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_EGOPLANES_HOST;
  r.fingerprint = fingerprint;
  r.bank = bank_host;
  r.bank_rows = bank_rows;
  r.rows = rows_host;
  r.players = players_host;
  r.count = count;
  r.layer_mask = layer_mask;
  r.classes = classes_host;
  r.classes_len = classes_len;
  r.num_classes = num_classes;
  r.facing = facing;
  r.dst = dst_host;
  r.dst_bytes = dst_bytes;
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  return mp_snapshot(NULL, &r, sizeof r);
}

#endif /* MP_EGO_PLANES_H_ */
