"""Times registered episode starts (profiles/r19_episode_starts.md) on one GPU, every figure
against the unregistered engine's launch for the same work in the same run.

    python tools/time_episode_starts.py [--packs clean_up,collaborative_cooking__cramped]
                                        [--worlds 4096] [--steps 64] [--calls 4] [--rounds 5]

The packs are patched to episodes of `--steps` frames, so that every world ends, and starts again,
once in every window of `--steps` steps.  Per pack, one JSON line with median [min, max] µs a step
over the rounds (events on the engine's stream, after a warm-up window):
  scalars   step() and step_many(K = steps) with no view bound, three ways: `plain` (no
            registration: the level's own reset), `minus_one` (a registration whose rows are all
            -1: the same work through the new families) and `starts` (every world starts from the
            bank once a window);
  world_rgb step() with WORLD.RGB bound: `fused` (no registration, one launch), `registered` (two
            launches, every world starting from the bank once a window) and `external` (the loop
            the registration replaces: step(), then load_worlds() with src made on the device from
            the step types before the step)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from meltingpot_amd import engine, lower, pack as pack_lib  # noqa: E402

E = engine


def short_episodes(name, frames):
  t = pack_lib.loads(engine.load_pack(name))
  t["hdr"][lower.HDR_MAXFRAMES] = frames
  return pack_lib.dumps(t)


def timed(fn, steps):
  """µs a step of fn(), which enqueues `steps` steps; one warm-up call first."""
  fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) * 1000.0 / steps


def make(pack, n, how, view):
  e = engine.Engine(pack, n, device=0)
  wrgb = e.bind(E.OBS_WORLD_RGB) if view else None
  st = e.bind(E.OBS_STEP_TYPE)
  e.reset()
  bank = e.save_worlds().clone()   # rows at the start of an episode: a started world plays a whole one
  rows = torch.arange(n, dtype=torch.int32, device=e.device)
  if how == "minus_one":
    rows.fill_(-1)
  if how in ("minus_one", "starts"):
    e.set_episode_starts(bank, rows)
  return e, bank, rows, st, wrgb


def one_pack(name, args):
  n, K = args.worlds, args.steps
  pack = short_episodes(name, K)
  rng = np.random.default_rng(0)
  probe = engine.Engine(pack, 1, device=0)
  nact, P = probe.num_actions, probe.P
  probe.close()
  A = torch.from_numpy(rng.integers(0, nact, (K, n, P), dtype=np.int32)).cuda()
  minus = torch.full((n,), -1, dtype=torch.int32, device=A.device)
  times = {}

  def record(key, value):
    times.setdefault(key, []).append(value)

  ways = {how: make(pack, n, how, False) for how in ("plain", "minus_one", "starts")}
  views = {how: make(pack, n, how, True) for how in ("plain", "starts", "external")}
  outs = {how: e.step_many(A) for how, (e, *_) in ways.items()}

  def loop(e):
    for k in range(K):
      e.step(A[k])

  def external(e, bank, rows, st):
    for k in range(K):
      src = torch.where(st == 2, rows, minus)
      e.step(A[k])
      e.load_worlds(bank, src)

  for _ in range(args.rounds):   # alternated over the rounds
    for how, (e, bank, rows, st, _) in ways.items():
      record(f"scalars.step.{how}", timed(lambda: [loop(e) for _ in range(args.calls)], K * args.calls))
      record(f"scalars.step_many.{how}",
             timed(lambda: [e.step_many(A, out=outs[how]) for _ in range(args.calls)], K * args.calls))
    for how, (e, bank, rows, st, _) in views.items():
      fn = (lambda: external(e, bank, rows, st)) if how == "external" else (lambda: loop(e))
      label = {"plain": "fused", "starts": "registered", "external": "external"}[how]
      record(f"world_rgb.step.{label}", timed(fn, K))
  fused = {how: bool(e.fused) for how, (e, *_) in views.items()}
  episodes = {}
  for group in (ways, views):
    for how, (e, *_) in group.items():
      e.sync()
      assert not e.fault_words()[:40].any()
      episodes.setdefault(how, e.counters()["episodes"])
      e.close()
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  return {"pack": name, "worlds": n, "steps": K, "device": torch.cuda.get_device_name(0),
          "fused": fused, "episodes": episodes, "us_per_step": res}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--packs", default="clean_up,collaborative_cooking__cramped")
  ap.add_argument("--worlds", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=64)
  ap.add_argument("--calls", type=int, default=4)
  ap.add_argument("--rounds", type=int, default=5)
  args = ap.parse_args()
  for name in args.packs.split(","):
    print(json.dumps(one_pack(name, args)), flush=True)


if __name__ == "__main__":
  main()
