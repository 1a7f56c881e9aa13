// episode_stats.hip — k_episode_stats: the launch behind every submission of an engine with
// registered episode statistics (MpEpisodeStats, include/mp_engine.h), the pure tally of
// MP_STATS_TALLY, and the same rule over host rows (MP_STATS_HOST).  One wave per column (a world,
// or an entry of a world list), four waves per workgroup; a world's statistics have one writer
// and its steps are walked in order, so there is no global atomic and every value is reproducible
// bit for bit.  The unit includes no step header and no kernel of another unit changes with it.
#include "episode_stats.h"

#include <limits.h>
#include <string.h>

namespace {

using namespace episode_stats;

constexpr int kWaves = 4;
// a wave's slice of LDS: counts [C][P], then pairs [C2][P][P]
constexpr int kSlice = MP_STATS_MAX_COLUMNS * MP_MAX_PLAYERS + MP_STATS_MAX_PAIRS * MP_MAX_PLAYERS * MP_MAX_PLAYERS;

// LDS operations of one wave execute in order; this keeps the compiler from moving a lane's
// accesses over the point where it reads what other lanes of its wave added.
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <class T>
__device__ inline const T* row_at(const T* base, long long bytes, int k) {
  return reinterpret_cast<const T*>(reinterpret_cast<const uint8_t*>(base) + (long long)k * bytes);
}

// The event rows of one step against every column, into the wave's slice: the header row, then
// rows 1 + lane and 65 + lane as 16-byte loads.
__device__ inline void tally_step(const Columns& sc, const int4* __restrict__ ev, int count, int P, int* s,
                                  int lane) {
  const int CP = sc.C * P;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = 1 + lane + 64 * half;
    if (row > count) continue;
    const int4 e = ev[row];
    for (int c = 0; c < sc.C; ++c) {
      int p, q;
      if (stats_credit(sc.col[c], e.x, (uint32_t)e.y, (uint32_t)e.z, P, &p, &q)) atomicAdd(&s[c * P + p], 1);
    }
    for (int c = 0; c < sc.C2; ++c) {
      int p, q;
      if (stats_credit(sc.pair[c], e.x, (uint32_t)e.y, (uint32_t)e.z, P, &p, &q) && q >= 0)
        atomicAdd(&s[CP + (c * P + p) * P + q], 1);
    }
  }
}

__global__ __launch_bounds__(kWaves * 64) void k_episode_stats(const Columns sc, const Banks b, const Rows r,
                                                               const int tally_only) {
  __shared__ int lds[kWaves][kSlice];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int i = blockIdx.x * kWaves + wave;
  if (i >= r.columns) return;   // (no workgroup barrier anywhere below)
  const int P = r.P, CP = sc.C * P, n = CP + sc.C2 * P * P;
  int* s = lds[wave];

  // which world, and did it run anything at all?
  int w = i;
  bool live = true;
  if (r.worlds) {   // (a listed step's liveness test, step_masked.h: a world, and this entry's tag in its claim word)
    w = __builtin_amdgcn_readfirstlane(r.worlds[i]);
    if (w < 0 || w >= r.num_worlds) { live = false; w = 0; }
    else {
      const unsigned long long tag = listed_tag(r.generation, i);
      live = r.claim[w] == tag;
    }
  }
  if (live && r.started) live = *reinterpret_cast<const int32_t*>(r.started + (long long)w * r.started_stride) != 0;
  if (live && r.sel8) live = r.sel8[w] != 0;
  if (live && r.sel32) { const int src = r.sel32[w]; live = src >= 0 && src < r.sel_rows; }
  int limit = INT_MAX;
  if (live && r.ran) limit = r.ran[i];
  live = __builtin_amdgcn_readfirstlane((int)(live && limit > 0)) != 0;
  if (!live && !tally_only) return;   // nothing ran: the statistics are what they were

  // the running bank: counts and pairs in LDS, lane p holds player p's return
  int open = 0, length = 0, episodes = 0, dropped = 0;
  double ret = 0.0;
  const int32_t* run_counts = (const int32_t*)b.running.counts;
  const int32_t* run_pairs = (const int32_t*)b.running.pairs;
  if (tally_only) {
    for (int j = lane; j < n; j += 64) s[j] = 0;
  } else {
    open = b.open[w] != 0;
    length = ((const int32_t*)b.running.length)[w];
    episodes = b.episodes[w];
    dropped = b.dropped[w];
    if (lane < P) ret = b.running.returns[(size_t)w * P + lane];
    for (int j = lane; j < CP; j += 64) s[j] = run_counts[(size_t)w * CP + j];
    for (int j = lane; j < n - CP; j += 64) s[CP + j] = run_pairs[(size_t)w * (n - CP) + j];
  }
  wave_sync();

  int done = 0;
  const bool per_step = r.active && r.active_bytes != 0;
  const bool one_byte = r.active && !per_step ? r.active[i] != 0 : true;
  for (int base = 0; live && base < r.K && done < limit; base += 64) {
    // the mask and step type of 64 steps across the lanes
    const int k = base + lane;
    bool act = k < r.K && one_byte;
    if (act && per_step) act = r.active[(long long)k * r.active_bytes + i] != 0;
    int st = 0;
    if (act && r.step_type) st = row_at(r.step_type, r.step_type_bytes, k)[i];
    unsigned long long m = __ballot(act);
    while (m != 0ull && done < limit) {
      const int j = __builtin_ctzll(m);
      m &= m - 1ull;
      ++done;
      const int kk = base + j;
      const int st_j = __shfl(st, j);
      int count = 0;
      const int4* ev = nullptr;
      if (r.events) {
        ev = reinterpret_cast<const int4*>(row_at(r.events, r.events_bytes, kk)) + (size_t)i * MP_EVENT_ROWS;
        const int4 header = ev[0];
        count = stats_event_count(__builtin_amdgcn_readfirstlane(header.x));
        dropped += __builtin_amdgcn_readfirstlane(header.y);
      }
      const int what = tally_only ? kTally : stats_rule(st_j, open);
      if (what & kZero) {
        for (int q = lane; q < n; q += 64) s[q] = 0;
        ret = 0.0;
        length = 0;
        open = 1;
        wave_sync();
      }
      if (what & kAccumulate) {
        if (lane < P) ret = __dadd_rn(ret, row_at(r.reward, r.reward_bytes, kk)[(size_t)i * P + lane]);
        ++length;
      }
      if ((what & kTally) && ev && count > 0) {
        tally_step(sc, ev, count, P, s, lane);
        wave_sync();
      }
      if (what & kClose) {
        // last := running, total += running (this wave is the world's only writer)
        if (lane < P) {
          b.last.returns[(size_t)w * P + lane] = ret;
          double* tr = b.total.returns + (size_t)w * P + lane;
          *tr = __dadd_rn(*tr, ret);
        }
        if (lane == 0) {
          ((int32_t*)b.last.length)[w] = length;
          ((long long*)b.total.length)[w] += length;
        }
        for (int q = lane; q < CP; q += 64) {
          ((int32_t*)b.last.counts)[(size_t)w * CP + q] = s[q];
          ((long long*)b.total.counts)[(size_t)w * CP + q] += s[q];
        }
        for (int q = lane; q < n - CP; q += 64) {
          ((int32_t*)b.last.pairs)[(size_t)w * (n - CP) + q] = s[CP + q];
          ((long long*)b.total.pairs)[(size_t)w * (n - CP) + q] += s[CP + q];
        }
        ++episodes;
        open = 0;
      }
    }
  }

  // flush
  if (tally_only) {
    int32_t* out_counts = (int32_t*)b.running.counts;
    int32_t* out_pairs = (int32_t*)b.running.pairs;
    for (int j = lane; j < CP; j += 64) out_counts[(size_t)i * CP + j] = s[j];
    for (int j = lane; j < n - CP; j += 64) out_pairs[(size_t)i * (n - CP) + j] = s[CP + j];
    return;
  }
  if (lane < P) b.running.returns[(size_t)w * P + lane] = ret;
  for (int j = lane; j < CP; j += 64) ((int32_t*)b.running.counts)[(size_t)w * CP + j] = s[j];
  for (int j = lane; j < n - CP; j += 64) ((int32_t*)b.running.pairs)[(size_t)w * (n - CP) + j] = s[CP + j];
  if (lane == 0) {
    ((int32_t*)b.running.length)[w] = length;
    b.open[w] = (uint8_t)open;
    b.episodes[w] = episodes;
    b.dropped[w] = dropped;
  }
}

}  // namespace

void launch_episode_stats(const Columns& c, const Banks& b, const Rows& r, bool tally_only, hipStream_t stream) {
  if (r.columns < 1) return;
  hipLaunchKernelGGL(k_episode_stats, dim3((unsigned)((r.columns + kWaves - 1) / kWaves)), dim3(kWaves * 64), 0,
                     stream, c, b, r, tally_only ? 1 : 0);
}

// MP_STATS_HOST: column i is world i; the same stats_credit / stats_rule, one world after another.
void episode_stats_host(const Columns& sc, const Banks& b, const Rows& r) {
  const int P = r.P, CP = sc.C * P, PP = sc.C2 * P * P;
  for (int w = 0; w < r.columns; ++w) {
    const int limit = r.ran ? r.ran[w] : INT_MAX;
    int done = 0;
    int32_t* counts = (int32_t*)b.running.counts + (size_t)w * CP;
    int32_t* pairs = (int32_t*)b.running.pairs + (size_t)w * PP;
    double* ret = b.running.returns + (size_t)w * P;
    int32_t* length = (int32_t*)b.running.length + w;
    for (int k = 0; k < r.K && done < limit; ++k) {
      if (r.active && r.active[(long long)k * r.active_bytes + w] == 0) continue;
      ++done;
      const int st = reinterpret_cast<const int32_t*>((const uint8_t*)r.step_type + k * r.step_type_bytes)[w];
      const int32_t* ev = nullptr;
      int count = 0;
      if (r.events) {
        ev = reinterpret_cast<const int32_t*>((const uint8_t*)r.events + k * r.events_bytes) +
             (size_t)w * MP_EVENT_ROWS * 4;
        count = stats_event_count(ev[0]);
        b.dropped[w] += ev[1];
      }
      const int what = stats_rule(st, b.open[w] != 0);
      if (what & kZero) {
        for (int q = 0; q < CP; ++q) counts[q] = 0;
        for (int q = 0; q < PP; ++q) pairs[q] = 0;
        for (int p = 0; p < P; ++p) ret[p] = 0.0;
        *length = 0;
        b.open[w] = 1;
      }
      if (what & kAccumulate) {
        const double* rw = reinterpret_cast<const double*>((const uint8_t*)r.reward + k * r.reward_bytes) + (size_t)w * P;
        for (int p = 0; p < P; ++p) ret[p] = ret[p] + rw[p];
        *length += 1;
      }
      if (what & kTally)
        for (int row = 1; row <= count; ++row) {
          const int32_t* e = ev + 4 * row;
          int p, q;
          for (int c = 0; c < sc.C; ++c)
            if (stats_credit(sc.col[c], e[0], (uint32_t)e[1], (uint32_t)e[2], P, &p, &q)) counts[c * P + p] += 1;
          for (int c = 0; c < sc.C2; ++c)
            if (stats_credit(sc.pair[c], e[0], (uint32_t)e[1], (uint32_t)e[2], P, &p, &q) && q >= 0)
              pairs[(c * P + p) * P + q] += 1;
        }
      if (what & kClose) {
        for (int p = 0; p < P; ++p) {
          b.last.returns[(size_t)w * P + p] = ret[p];
          b.total.returns[(size_t)w * P + p] = b.total.returns[(size_t)w * P + p] + ret[p];
        }
        ((int32_t*)b.last.length)[w] = *length;
        ((long long*)b.total.length)[w] += *length;
        for (int q = 0; q < CP; ++q) {
          ((int32_t*)b.last.counts)[(size_t)w * CP + q] = counts[q];
          ((long long*)b.total.counts)[(size_t)w * CP + q] += counts[q];
        }
        for (int q = 0; q < PP; ++q) {
          ((int32_t*)b.last.pairs)[(size_t)w * PP + q] = pairs[q];
          ((long long*)b.total.pairs)[(size_t)w * PP + q] += pairs[q];
        }
        b.episodes[w] += 1;
        b.open[w] = 0;
      }
    }
  }
}
