// episode_stats.h — what the host hands k_episode_stats (episode_stats.hip), and the rule of an
// MpEpisodeStats request (include/mp_engine.h) written once for the device and the host: which
// player an event row credits in a column (stats_credit) and what one step that ran does to a
// world's statistics (stats_rule).  A header of its own: no step unit includes it.
#ifndef MP_EPISODE_STATS_H_INTERNAL_
#define MP_EPISODE_STATS_H_INTERNAL_

#include "mp_common.h"

namespace episode_stats {

// The columns of a registration, a by-value kernel argument (wave-uniform reads).
struct Columns {
  int C, C2;
  MpEventColumn col[MP_STATS_MAX_COLUMNS];
  MpEventColumn pair[MP_STATS_MAX_PAIRS];
};

// The statistics tensors (MpEpisodeStats documents shapes and types).
struct Banks {
  uint8_t* open;
  int32_t* episodes;
  int32_t* dropped;
  MpStatsBank running, last, total;
};

// The rows one launch folds: `columns` waves, wave i reads column i of every row and writes the
// statistics of world w (= i, or worlds[i] under a list).  Distances between two steps' rows are in
// bytes; K = 1 with the engine's in-place buffers serves the single steps.
struct Rows {
  int columns, K, P;
  const int32_t* step_type; long long step_type_bytes;
  const double* reward; long long reward_bytes;
  const int32_t* events; long long events_bytes;   // NULL: no event rows (no column registered)
  const uint8_t* active; long long active_bytes;   // NULL: every step; 0: one row for every step
  const int32_t* ran;                              // NULL: no limit; else the first ran[i] active steps
  const uint8_t* sel8;                             // masked reset: u8 [N], by world
  const int32_t* sel32; int sel_rows;              // load: src [N], a world ran where it names a row
  const int32_t* worlds;                           // MpStepListed: the list, its claim table and tag
  const unsigned long long* claim;
  uint32_t generation;
  int num_worlds;
  const uint8_t* started; long long started_stride;   // &WorldTail::started of world 0, or NULL
};

// Does event row {type, a, b} count in column c, and for whom?  *player and *other are 0-based;
// *other is -1 when the other payload names no player (a pair column then skips the event).
__host__ __device__ inline bool stats_credit(const MpEventColumn& c, int type, uint32_t a, uint32_t b, int P,
                                             int* player, int* other) {
  if (type != c.type) return false;
  if (c.filter_payload) {
    const uint32_t v = c.filter_payload == 1 ? a : b;
    if (((v >> c.filter_shift) & c.filter_mask) != c.filter_value) return false;
  }
  const uint32_t pv = c.player_payload ? b : a, ov = c.player_payload ? a : b;
  const uint32_t p = (pv >> c.player_shift) & c.player_mask;
  if (p < 1u || p > (uint32_t)P) return false;
  const uint32_t q = (ov >> c.other_shift) & c.other_mask;
  *player = (int)p - 1;
  *other = q >= 1u && q <= (uint32_t)P ? (int)q - 1 : -1;
  return true;
}

// What a step that ran and left step type `st` does to a world whose episode is `open`.
enum { kZero = 1, kAccumulate = 2, kTally = 4, kClose = 8 };
__host__ __device__ inline int stats_rule(int st, int open) {
  if (st == 0) return kZero | kTally;
  if (!open) return 0;
  return kAccumulate | kTally | (st == 2 ? kClose : 0);
}

// Rows the header counts (it never counts more than the buffer holds, but a row a caller built may).
__host__ __device__ inline int stats_event_count(int header_count) {
  return header_count < 0 ? 0 : header_count > MP_EVENT_ROWS - 1 ? MP_EVENT_ROWS - 1 : header_count;
}

}  // namespace episode_stats

// One launch on `stream`: ceil(columns / 4) workgroups of four waves.  tally_only: the pure tally
// of MP_STATS_TALLY into b.running.counts / pairs, indexed by column.
void launch_episode_stats(const episode_stats::Columns& c, const episode_stats::Banks& b,
                          const episode_stats::Rows& r, bool tally_only, hipStream_t stream);
// The same rule over host rows and host statistics (MP_STATS_HOST); sequential.
void episode_stats_host(const episode_stats::Columns& c, const episode_stats::Banks& b,
                        const episode_stats::Rows& r);

#endif  // MP_EPISODE_STATS_H_INTERNAL_
