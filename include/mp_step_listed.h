/* mp_step_listed.h — stepping the worlds a device index list names: one wave per entry of the
 * list, [K][M][..] actions and rows for its M entries, whatever the engine's N is, as plain C
 * functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the MpStepListed request that mp_restore carries (mp_engine.h documents the semantics, the
 * defining identity with the masked request over all worlds, the bad entries and the refusals).
 * Same return codes as every entry point. */
#ifndef MP_STEP_LISTED_H_
#define MP_STEP_LISTED_H_

#include <string.h>

#include "mp_engine.h"

/* worlds_device: int32 [count], the world of entry i.  actions_device, rows, active_device,
 * ran_device, returns_device: as mp_step_many_until takes them (mp_step_until.h), with `count`
 * columns where that has N.  stopped_device: uint8 [N], by WORLD, or NULL.  Stream-ordered, no
 * synchronisation. */
static inline int mp_step_many_listed(MpEngine* eng, const int32_t* worlds_device, int32_t count,
                                      const int32_t* actions_device, int32_t steps, int32_t fields,
                                      uint64_t actions_step_bytes, const MpStepRow* rows,
                                      int32_t num_rows, const uint8_t* active_device,
                                      uint64_t active_step_bytes, uint32_t stop,
                                      uint8_t* stopped_device, int32_t* ran_device,
                                      double* returns_device, double gamma) {
  MpStepListed r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.steps = steps;
  r.fields = fields;
  r.num_rows = num_rows;
  r.actions = actions_device;
  r.actions_step_bytes = actions_step_bytes;
  r.rows = rows;
  r.active = active_device;
  r.active_step_bytes = active_step_bytes;
  r.stop = stop;
  r.stopped = stopped_device;
  r.ran = ran_device;
  r.returns = returns_device;
  r.gamma = gamma;
  r.worlds = worlds_device;
  r.count = count;
  return mp_restore(eng, &r, sizeof r);
}

/* One step of the listed worlds: actions_device int32 [count][P] (fields = 1: [count][P][A]),
 * entry i the actions of world worlds_device[i].  Every other world is not touched. */
static inline int mp_step_listed(MpEngine* eng, const int32_t* worlds_device, int32_t count,
                                 const int32_t* actions_device, int32_t fields) {
  return mp_step_many_listed(eng, worlds_device, count, actions_device, 1, fields, 0, NULL, 0, NULL, 0,
                             0, NULL, NULL, NULL, 1.0);
}

#endif /* MP_STEP_LISTED_H_ */
