/* mp_episode_stats.h — episode statistics on the device (MpEpisodeStats) as plain C functions.
 *
 * Header only: the library's exported entry points are those of mp_engine.h, and these wrappers
 * build the request that mp_restore carries (mp_engine.h documents the rule, the tensors and the
 * refusals).  Same return codes as every entry point. */
#ifndef MP_EPISODE_STATS_H_
#define MP_EPISODE_STATS_H_

#include <string.h>

#include "mp_engine.h"

/* An unfiltered column: events of `type`, credited to the player in payload a (payload = 0) or b
 * (1), ((value >> shift) & mask). */
static inline MpEventColumn mp_event_column(int32_t type, int payload, int shift, uint32_t mask) {
  MpEventColumn c;
  memset(&c, 0, sizeof c);
  c.type = type;
  c.player_payload = (uint8_t)payload;
  c.player_shift = (uint8_t)shift;
  c.player_mask = mask;
  return c;
}

/* `stats` names the columns and the device tensors (op and struct_size are set here).  From now on
 * every submission of `eng` is followed by the launch that folds it into them.  No launch, no
 * synchronisation. */
static inline int mp_set_episode_stats(MpEngine* eng, const MpEpisodeStats* stats) {
  MpEpisodeStats r;
  if (!eng || !stats) return mp_restore(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  r = *stats;
  r.struct_size = sizeof r;
  r.op = MP_STATS_REGISTER;
  return mp_restore(eng, &r, sizeof r);
}

/* The engine issues the launches it issued before the registration. */
static inline int mp_clear_episode_stats(MpEngine* eng) {
  MpEpisodeStats r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_STATS_CLEAR;
  if (!eng) return mp_restore(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_restore(eng, &r, sizeof r);
}

/* counts_device (int32 [count][C][P]) and pairs_device (int32 [count][C2][P][P], NULL with no pair
 * column) := the tally of events_device (int32 [steps][count][MP_EVENT_ROWS][4]) over the steps
 * that ran (active_device u8 [steps][count] or NULL, ran_device i32 [count] or NULL). */
static inline int mp_tally_events(MpEngine* eng, const MpEventColumn* columns, int32_t num_columns,
                                  const MpEventColumn* pairs, int32_t num_pairs,
                                  const int32_t* events_device, int32_t steps, int32_t count,
                                  const uint8_t* active_device, const int32_t* ran_device,
                                  int32_t* counts_device, int32_t* pairs_device) {
  MpEpisodeStats r;
  memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.op = MP_STATS_TALLY;
  r.columns = columns; r.num_columns = num_columns;
  r.pairs = pairs; r.num_pairs = num_pairs;
  r.events = events_device; r.steps = steps; r.count = count;
  r.active = active_device; r.ran = ran_device;
  r.running.counts = counts_device; r.running.pairs = pairs_device;
  if (!eng) return mp_restore(eng, NULL, 0);   /* (MP_ERR_INVALID, with its message) */
  return mp_restore(eng, &r, sizeof r);
}

/* The rule on HOST rows and HOST statistics, without an engine or a device: `stats` names the
 * columns, the statistics of `count` worlds and the rows (steps, count, num_players, step_type,
 * reward, events, active, ran). */
static inline int mp_episode_stats_host(const MpEpisodeStats* stats) {
  MpEpisodeStats r;
  if (!stats) return mp_restore(NULL, NULL, 0);
  r = *stats;
  r.struct_size = sizeof r;
  r.op = MP_STATS_HOST;
  return mp_restore(NULL, &r, sizeof r);
}

#endif /* MP_EPISODE_STATS_H_ */
