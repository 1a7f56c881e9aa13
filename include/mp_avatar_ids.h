/* mp_avatar_ids.h — whom each player sees and whom it could zap (MpAvatarIds), as plain C
 * functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpAvatarIds request that mp_snapshot carries (mp_engine.h documents the two
 * observations, the semantics and the refusals).  Same return codes as every entry point. */
#ifndef MP_AVATAR_IDS_H_
#define MP_AVATAR_IDS_H_

#include <string.h>

#include "mp_engine.h"

/* Element i of view_device (IN_VIEW) and of zap_device (IN_RANGE), either may be NULL = the
 * vectors of row rows_device[i] (NULL: row i) of bank_device (uint8 [bank_rows][S]; NULL: the
 * engine's worlds, rows_device then world indices): every viewer, int32 [count][P][P], with
 * players_device NULL; else of player players_device[i], int32 [count][P].  `fingerprint`: the
 * rows' (of the engine that saved them).  Stream-ordered, no synchronisation, no allocation;
 * nothing of the engine's is written. */
static inline int mp_avatar_ids_draw(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                     const int32_t* rows_device, const int32_t* players_device, int32_t count,
                                     void* view_device, uint64_t view_bytes, void* zap_device, uint64_t zap_bytes,
                                     uint64_t fingerprint) {
  MpAvatarIds r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_AVATARIDS_DRAW;
  r.fingerprint = fingerprint;
  r.bank = bank_device;
  r.bank_rows = bank_rows;
  r.rows = rows_device;
  r.players = players_device;
  r.count = count;
  r.dst = view_device;
  r.dst_bytes = view_bytes;
  r.dst_zap = zap_device;
  r.dst_zap_bytes = zap_bytes;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* From now on every submission is followed by one launch that rewrites every viewer's vectors into
 * view_device and zap_device, int32 [N][P][P] each (slots == 0; either may be NULL), or into slot
 * s = the ring slot the submission wrote, at + s * slot_stride bytes of each (slots = the engine's
 * ring slots).  Both NULL clears the registration. */
static inline int mp_avatar_ids_register(MpEngine* eng, void* view_device, uint64_t view_bytes, void* zap_device,
                                         uint64_t zap_bytes, uint64_t slot_stride, int32_t slots) {
  MpAvatarIds r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_AVATARIDS_REGISTER;
  r.dst = view_device;
  r.dst_bytes = view_bytes;
  r.dst_zap = zap_device;
  r.dst_zap_bytes = zap_bytes;
  r.slot_stride = slot_stride;
  r.slots = slots;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* The vectors of HOST rows into HOST destinations, computed without a device: `pack`, `pack_len`,
 * `cfg` as for mp_create; `fingerprint`: the rows'. */
static inline int mp_avatar_ids_host(const void* pack, uint64_t pack_len, const MpConfig* cfg, const void* bank_host,
                                     int32_t bank_rows, const int32_t* rows_host, const int32_t* players_host,
                                     int32_t count, void* view_host, uint64_t view_bytes, void* zap_host,
                                     uint64_t zap_bytes, uint64_t fingerprint) {
  MpAvatarIds r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_AVATARIDS_HOST;
  r.fingerprint = fingerprint;
  r.bank = bank_host;
  r.bank_rows = bank_rows;
  r.rows = rows_host;
  r.players = players_host;
  r.count = count;
  r.dst = view_host;
  r.dst_bytes = view_bytes;
  r.dst_zap = zap_host;
  r.dst_zap_bytes = zap_bytes;
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  return mp_snapshot(NULL, &r, sizeof r);
}

#endif /* MP_AVATAR_IDS_H_ */
