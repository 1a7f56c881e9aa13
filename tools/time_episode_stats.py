"""Times the episode statistics (profiles/r27_episode_stats.md) on one GPU: what the launch of
k_episode_stats behind every submission costs, every figure against the same engine without a
registration in the same run.

    python tools/time_episode_stats.py [--packs clean_up,commons_harvest__open] [--worlds 4096]
                                       [--calls 128] [--rounds 7]

Per pack one JSON line with median [min, max] µs a CALL over the rounds, measured as
tools/time_step_active.py measures (its Blocker and timed(): events on the engine's stream, one
warm-up window per variant, every timed window enqueued behind a blocker, the variants alternated
over the rounds, each on an engine of its own; `device_bound` says whether the host kept ahead of the
device, per variant).  Variants:
  step, step_stats            step(A) with no view bound, unregistered / registered (default columns);
  rgb, rgb_stats              the same with WORLD.RGB bound (the fused frame launch);
  many, many_returns,         step_many(A) at K = 64: unregistered / registered with columns=()
  many_stats                  (returns and lengths: no EVENTS row) / registered with the default
                              columns (the call then carries the K x N x 2 KB EVENTS row);
  torch_update                the same update of one step written with torch (scatter_add_ per
                              column on the in-place REWARD, STEP_TYPE and EVENTS): what a user
                              has today, without the K-step case, which has no torch form.
`ratio` is each registered variant's median over its unregistered twin's."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from meltingpot_amd import engine  # noqa: E402
from time_step_active import Blocker, timed  # noqa: E402

E = engine
K_MANY = 64


class TorchStats:
  """The rule of MpEpisodeStats for one step, in torch statements over the engine's in-place
  buffers (unfiltered single-player columns only)."""

  def __init__(self, eng, columns):
    self.e = eng
    t, N, P = torch, eng.N, eng.P
    self.cols = [E.parse_event_column(c)[0] for c in columns]
    C = len(self.cols)
    dev = eng.device
    self.open = t.zeros(N, dtype=t.bool, device=dev)
    self.episodes = t.zeros(N, dtype=t.int32, device=dev)
    bank = lambda ints: {"returns": t.zeros((N, P), dtype=t.float64, device=dev), "length": t.zeros(N, dtype=ints, device=dev),
                         "counts": t.zeros((N, C, P), dtype=ints, device=dev)}
    self.running, self.last, self.total = bank(t.int32), bank(t.int32), bank(t.int64)
    self.reward, self.step_type, self.events = (eng.bind(k) for k in (E.OBS_REWARD, E.OBS_STEP_TYPE, E.OBS_EVENTS))
    self.row = t.arange(E.EVENT_ROWS - 1, device=dev)[None]

  def update(self):
    t, P = torch, self.e.P
    st, ev = self.step_type, self.events
    first, last = st == 0, st == 2
    run = self.running
    shaped = lambda m, x: m.view((-1,) + (1,) * (x.dim() - 1))   # (no boolean indexing: it would wait for the device)
    for key in run:
      run[key].masked_fill_(shaped(first, run[key]), 0)
    self.open |= first
    live = self.open & ~first
    run["returns"] += self.reward * live[:, None]
    run["length"] += live.int()
    valid = (self.row < ev[:, 0, 0:1]) & self.open[:, None]
    types = ev[:, 1:, 0]
    for c, col in enumerate(self.cols):
      who = ev[:, 1:, 2 if col.player_payload else 1]
      hit = valid & (types == col.type) & (who >= 1) & (who <= P)
      run["counts"][:, c].scatter_add_(1, (who - 1).clamp(0, P - 1).long(), hit.int())
    close = live & last
    for key in run:
      self.last[key].copy_(t.where(shaped(close, run[key]), run[key], self.last[key]))
      self.total[key] += run[key] * shaped(close, run[key])
    self.episodes += close.int()
    self.open &= ~close


def one_case(name, n, args, blocker):
  pack = engine.load_pack(name)
  rng = np.random.default_rng(0)
  probe = engine.Engine(pack, 1, device=0)
  nact, P = probe.num_actions, probe.P
  columns = probe.event_columns()
  probe.close()
  A = torch.from_numpy(rng.integers(0, nact, (K_MANY, n, P), dtype=np.int32)).cuda()
  variants = {"step": (None, False, 1), "step_stats": ("default", False, 1), "rgb": (None, True, 1),
              "rgb_stats": ("default", True, 1), "many": (None, False, K_MANY), "many_returns": ((), False, K_MANY),
              "many_stats": ("default", False, K_MANY), "torch_update": (None, False, 0)}
  engines, calls_of, fns, stats = {}, {}, {}, {}
  for how, (cols, rgb, K) in variants.items():
    e = engine.Engine(pack, n, device=0)
    if rgb:
      e.bind(E.OBS_WORLD_RGB)
    if cols is not None:
      stats[how] = e.set_episode_stats(cols)
    e.reset()
    engines[how] = e
    calls_of[how] = max(8, args.calls // max(1, K // 4))
    if K > 1:
      out = e.step_many(A)
      fns[how] = (lambda e=e, out=out: e.step_many(A, out=out))
    elif K == 1:
      fns[how] = (lambda e=e: e.step(A[0]))
    else:
      ts = TorchStats(e, columns)
      e.step(A[0])
      fns[how] = ts.update
  times = {how: [] for how in variants}
  enqueue_ms = {how: 0.0 for how in variants}
  for _ in range(args.rounds):   # alternated over the rounds
    for how in variants:
      us, host_ms = timed(fns[how], calls_of[how], blocker)
      times[how].append(us)
      enqueue_ms[how] = max(enqueue_ms[how], host_ms)
  episodes = {}
  for how, e in engines.items():
    e.sync()
    assert not e.fault_words()[:40].any()
    if how in stats:
      episodes[how] = int(stats[how].episodes.sum())
    e.close()
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  twin = {"step_stats": "step", "rgb_stats": "rgb", "many_returns": "many", "many_stats": "many"}
  return {"pack": name, "worlds": n, "K": K_MANY, "columns": len(columns), "device": torch.cuda.get_device_name(0),
          "blocker_ms": round(blocker.ms, 1), "enqueue_ms": {k: round(v, 1) for k, v in enqueue_ms.items()},
          "device_bound": {k: bool(v < blocker.ms) for k, v in enqueue_ms.items()}, "us_per_call": res,
          "ratio": {k: round(res[k][0] / res[v][0], 3) for k, v in twin.items()},
          "added_us": {k: round(res[k][0] - res[v][0], 2) for k, v in twin.items()},
          "events_row_mb": round(K_MANY * n * E.EVENT_ROWS * 16 / 1e6, 1), "episodes_counted": episodes}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--packs", default="clean_up,commons_harvest__open")
  ap.add_argument("--worlds", type=int, default=4096)
  ap.add_argument("--calls", type=int, default=128)
  ap.add_argument("--fills", type=int, default=60, help="2 GiB fills of the blocker in front of a window")
  ap.add_argument("--rounds", type=int, default=7)
  args = ap.parse_args()
  blocker = Blocker(args.fills)
  for name in args.packs.split(","):
    print(json.dumps(one_case(name, args.worlds, args, blocker)), flush=True)


if __name__ == "__main__":
  main()
