/* mp_ego_layer.h — EGO_LAYER, the layer view in the avatar's own frame (MpEgoLayer), as plain C
 * functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpEgoLayer request that mp_snapshot carries (mp_engine.h documents the definition, the
 * semantics and the refusals).  Same return codes as every entry point. */
#ifndef MP_EGO_LAYER_H_
#define MP_EGO_LAYER_H_

#include <string.h>

#include "mp_engine.h"

/* Element i of dst_device = EGO_LAYER of row rows_device[i] (NULL: row i) of bank_device (uint8
 * [bank_rows][S]; NULL: the engine's worlds, rows_device then world indices): every viewer,
 * int32 [count][P][VH][VW][L], with players_device NULL; else the view of player
 * players_device[i], int32 [count][VH][VW][L].  `fingerprint`: the rows' (of the engine that
 * saved them).  Stream-ordered, no synchronisation, no allocation; nothing of the engine's is
 * written. */
static inline int mp_ego_layer_draw(MpEngine* eng, const void* bank_device, int32_t bank_rows,
                                    const int32_t* rows_device, const int32_t* players_device,
                                    int32_t count, void* dst_device, uint64_t dst_bytes,
                                    uint64_t fingerprint) {
  MpEgoLayer r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_EGO_DRAW;
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

/* From now on every submission is followed by one launch that redraws every world's EGO_LAYER
 * into dst_device, int32 [N][P][VH][VW][L] (slots == 0), or into slot s = the ring slot the
 * submission wrote, at dst_device + s * slot_stride bytes (slots = the engine's ring slots).
 * dst_device NULL clears the registration. */
static inline int mp_ego_layer_register(MpEngine* eng, void* dst_device, uint64_t dst_bytes,
                                        uint64_t slot_stride, int32_t slots) {
  MpEgoLayer r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_EGO_REGISTER;
  r.dst = dst_device;
  r.dst_bytes = dst_bytes;
  r.slot_stride = slot_stride;
  r.slots = slots;
  if (!eng) return mp_snapshot(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_snapshot(eng, &r, sizeof r);
}

/* The draw of HOST rows into a HOST dst, computed without a device: `pack`, `pack_len`, `cfg` as
 * for mp_create; `fingerprint`: the rows'. */
static inline int mp_ego_layer_host(const void* pack, uint64_t pack_len, const MpConfig* cfg,
                                    const void* bank_host, int32_t bank_rows, const int32_t* rows_host,
                                    const int32_t* players_host, int32_t count, void* dst_host,
                                    uint64_t dst_bytes, uint64_t fingerprint) {
  MpEgoLayer r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_EGO_HOST;
  r.fingerprint = fingerprint;
  r.bank = bank_host;
  r.bank_rows = bank_rows;
  r.rows = rows_host;
  r.players = players_host;
  r.count = count;
  r.dst = dst_host;
  r.dst_bytes = dst_bytes;
  r.pack = pack;
  r.pack_len = pack_len;
  r.cfg = cfg;
  return mp_snapshot(NULL, &r, sizeof r);
}

#endif /* MP_EGO_LAYER_H_ */
