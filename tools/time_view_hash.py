"""Times the view hash (MpViewHash) on one box: the draw forms against the EGO_LAYER draw they
replace and against the torch route (draw EGO_LAYER, hash it with torch ops), and what the
registration adds to a step; the method of tools/time_ego_layer.py (child processes under a time
limit, a warm-up, events on the engine's stream around calls that only enqueue, configurations
alternated round by round, medians and ranges).

  python tools/time_view_hash.py [--rounds 4] [--out FILE.json]

Levels clean_up (P = 7) and commons_harvest__open (P = 16), 4096 worlds.
  (a) step   us per `step` of three engines in one process, alternated: `plain` (nothing
             registered), `hash` (bind_view_hash: the step's launch and the hash launch behind it)
             and `ego` (bind_ego_layer: the launch whose stores the hash replaces with 8 bytes a
             viewer) — with no view bound and with WORLD.RGB bound.
  (b) draw   us per call at R = 256, 4096 and 32768 rows sampled, with repeats, from a bank of 4096
             worlds that have played 40 steps, alternated:
               hash_rows    hash_views(bank, rows): every viewer, int64 [R, P];
               ego_rows     observe_ego_layer(bank, rows): the draw of the same views (ego_layer.hip
                            is the parent commit's, byte for byte);
               torch_rows   ego_rows followed by the hash written with torch ops (R <= 4096: at
                            32768 rows its int64 temporaries are several GB each);
               hash_views, ego_views, torch_views: one player of each row, int64 [R];
             and at R = 4096 also hash_all / ego_all: every viewer of the bank's 4096 rows in order.
             The torch route's result is compared with the kernel's before anything is timed.
Every child runs under a time limit; the first that does not end normally, or that reports fault
words, ends the run."""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import time_step_many as base  # noqa: E402
from time_ego_layer import _rounds  # noqa: E402

LEVELS = ("clean_up", "commons_harvest__open")
COUNTS = (256, 4096, 32768)
WORLDS = 4096
CHILD_SECONDS = 240
TORCH_ROWS_MAX = 4096


def child_step(level, view, rounds, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  engines = {n: E.Engine(E.load_pack(level), WORLDS, device=0) for n in ("plain", "hash", "ego")}
  calls = {}
  for n, e in engines.items():
    e.use_current_stream()
    if view == "world":
      e.bind(E.OBS_WORLD_RGB)
    if n == "hash":
      e.bind_view_hash(torch.zeros((e.N, e.P), dtype=torch.int64, device=e.device))
    if n == "ego":
      e.bind_ego_layer(torch.zeros(e.ego_layer_shape, dtype=torch.int32, device=e.device))
    e.reset()
    acts = base._actions(e, torch, 64, 0.0)
    state = {"k": 0}
    def step(e=e, acts=acts, state=state):
      e.step(acts[state["k"] % 64])
      state["k"] += 1
    calls[n] = step
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "fused": bool(engines["plain"].fused),
         "hash_bytes": engines["hash"].N * engines["hash"].P * 8,
         "leaf_bytes": int(np.prod(engines["ego"].ego_layer_shape)) * 4}
  res["fault"] = False
  for e in engines.values():
    e.sync()
    res["fault"] = res["fault"] or bool(e.fault_words()[:10].any())
    e.close()
  return res


def _torch_hash(torch):
  """The hash of int32 views [..., VH, VW, L] with torch ops: int64 arithmetic wraps mod 2^64, and a
  logical shift is an arithmetic one with the sign's copies masked off."""
  c1, c2 = 0xff51afd7ed558ccd - (1 << 64), 0xc4ceb9fe1a85ec53 - (1 << 64)
  low31 = (1 << 31) - 1

  def fmix(h):
    h = h ^ ((h >> 33) & low31)
    h = h * c1
    h = h ^ ((h >> 33) & low31)
    h = h * c2
    return h ^ ((h >> 33) & low31)

  def hash_of(ego):
    n = ego.shape[-3] * ego.shape[-2] * ego.shape[-1]
    v = ego.reshape(ego.shape[:-3] + (n,)).long() & 0xffffffff
    e = (torch.arange(1, n + 1, device=ego.device, dtype=torch.int64) << 32)
    return fmix(fmix(e | v).sum(dim=-1))
  return hash_of


def child_draw(level, R, rounds, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  src = E.Engine(E.load_pack(level), WORLDS, device=0)
  src.reset()
  acts = base._actions(src, torch, 40, 0.0)
  for s in range(40):
    src.step(acts[s])
  bank = src.save_worlds().clone()
  src.sync()
  src.close()
  e = E.Engine(E.load_pack(level), 256, device=0)
  e.use_current_stream()
  gen = torch.Generator().manual_seed(3)
  rows = torch.randint(0, WORLDS, (R,), generator=gen).to(torch.int32).to(e.device)
  players = torch.randint(0, e.P, (R,), generator=gen).to(torch.int32).to(e.device)
  shape = e.ego_layer_shape
  ego_rows = torch.empty((R,) + shape[1:], dtype=torch.int32, device=e.device)
  ego_views = torch.empty((R,) + shape[2:], dtype=torch.int32, device=e.device)
  h_rows = torch.empty((R, e.P), dtype=torch.int64, device=e.device)
  h_views = torch.empty((R,), dtype=torch.int64, device=e.device)
  hash_of = _torch_hash(torch)
  check = min(R, 512)   # the torch route is the function the kernels compute
  assert torch.equal(hash_of(e.observe_ego_layer(bank, rows=rows[:check])), e.hash_views(bank, rows=rows[:check]))
  assert torch.equal(hash_of(e.observe_ego_layer(bank, rows=rows[:check], players=players[:check])),
                     e.hash_views(bank, rows=rows[:check], players=players[:check]))
  calls = {"hash_rows": lambda: e.hash_views(bank, rows=rows, out=h_rows),
           "ego_rows": lambda: e.observe_ego_layer(bank, rows=rows, out=ego_rows),
           "hash_views": lambda: e.hash_views(bank, rows=rows, players=players, out=h_views),
           "ego_views": lambda: e.observe_ego_layer(bank, rows=rows, players=players, out=ego_views),
           "torch_views": lambda: hash_of(e.observe_ego_layer(bank, rows=rows, players=players, out=ego_views))}
  if R <= TORCH_ROWS_MAX:
    calls["torch_rows"] = lambda: hash_of(e.observe_ego_layer(bank, rows=rows, out=ego_rows))
  if R == WORLDS:
    calls["hash_all"] = lambda: e.hash_views(bank, out=h_rows)
    calls["ego_all"] = lambda: e.observe_ego_layer(bank, out=ego_rows)
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "P": e.P,
         "rows_bytes": ego_rows.numel() * 4, "views_bytes": ego_views.numel() * 4}
  e.sync()
  res["fault"] = bool(e.fault_words()[:10].any())
  e.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=4)
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--levels", default=",".join(LEVELS))
  ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
  ap.add_argument("--out", default="")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    what, level, arg = a.child.split(":")
    if what == "step":
      print(json.dumps(child_step(level, arg, a.rounds, a.reps, a.warmup)))
    else:
      print(json.dumps(child_draw(level, int(arg), a.rounds, a.reps, a.warmup)))
    return
  if a.rounds < 2:
    raise SystemExit("--rounds must be at least 2: the configurations are alternated")
  import torch
  me = os.path.abspath(__file__)
  levels = a.levels.split(",")
  specs = [f"step:{level}:{view}" for level in levels for view in ("none", "world")]
  specs += [f"draw:{level}:{R}" for level in levels for R in a.counts.split(",")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
         "reps": a.reps, "worlds": WORLDS, "results": {}, "summary": {}}
  for spec in specs:
    out = subprocess.run([sys.executable, me, "--child", spec, "--rounds", str(a.rounds), "--reps", str(a.reps),
                          "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=CHILD_SECONDS)
    if out.returncode != 0:   # (nothing more runs on the GPU after a child that failed)
      raise RuntimeError(f"child {spec} exited {out.returncode}: {out.stderr[-2000:]}")
    got = json.loads(out.stdout.strip().splitlines()[-1])
    res["results"][spec] = got
    if got["fault"]:
      raise RuntimeError(f"child {spec} reported fault words")
    res["summary"][spec] = {n: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
                            for n, v in got["us"].items()}
    extra = {k: v for k, v in got.items() if k not in ("us", "fault")}
    print(f"{spec:40s} " + "  ".join(f"{n} {s['median']:.1f} ({s['min']:.1f}-{s['max']:.1f})"
                                      for n, s in res["summary"][spec].items()) + f"  {extra}", flush=True)
  line = json.dumps(res)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")
  else:
    print(line)


if __name__ == "__main__":
  main()
