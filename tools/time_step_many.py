"""Times `Engine.step_many` (K steps in one launch) against the loop of single steps it replaces,
on one box, at sizes a user runs, with only the scalars produced (no view bound).

  python tools/time_step_many.py [--parent-lib PATH] [--rounds 5] [--steps 2048] [--out FILE.json]
  python tools/time_step_many.py --trace clean_up   # a few step_many calls (for rocprofv3 --kernel-trace)

Per level (clean_up 4096 x 7, territory__rooms 8192 x 9 with half the actions beams,
commons_harvest__open 4096 x 16, collaborative_cooking__cramped 4096 x 2):
  (a) us per step of the loop of `Engine.step` on another build of the engine (`--parent-lib`);
  (b) the same loop on this build;
  (c) us per step of `step_many(K)`, K in 1, 4, 16, 64, with the four per-step outputs and without;
  (d) the host's wall time per step to enqueue (a) and (c): one call instead of K.
Every configuration (level x build x loop / step_many with / step_many without outputs) runs in a
child process of its own (a process loads one engine library); a step_many child times its four K
one after the other on one engine.  The configurations are alternated round by round; medians and
ranges over the rounds are reported.  GPU times are events around work that ends in a
synchronise, after a warm-up."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LEVELS = {"clean_up": (4096, 0.0), "territory__rooms": (8192, 0.5),
          "commons_harvest__open": (4096, 0.0), "collaborative_cooking__cramped": (4096, 0.0)}
KS = (1, 4, 16, 64)


def _actions(e, torch, T, beam_skew):
  gen = torch.Generator(device=e.device)
  gen.manual_seed(1)
  na = e.num_actions
  acts = torch.randint(0, na, (T, e.N, e.P), generator=gen, device=e.device, dtype=torch.int32)
  if beam_skew > 0:   # (the last two actions of the set are the beams, as in bench.py)
    beam = torch.randint(na - 2, na, (T, e.N, e.P), generator=gen, device=e.device, dtype=torch.int32)
    pick = torch.rand((T, e.N, e.P), generator=gen, device=e.device) < beam_skew
    acts = torch.where(pick, beam, acts)
  return acts


def _timed(torch, work):
  """(GPU us, host enqueue us) of work(), which only enqueues."""
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  a.record()
  work()
  b.record()
  t1 = time.perf_counter()
  b.synchronize()
  return a.elapsed_time(b) * 1e3, (t1 - t0) * 1e6


def child(level, mode, steps, warmup):
  import torch
  from meltingpot_amd import engine
  n, skew = LEVELS[level]
  e = engine.Engine(engine.load_pack(level), n, device=0)
  e.use_current_stream()
  e.reset()
  acts = _actions(e, torch, 64, skew)
  for s in range(warmup):
    e.step(acts[s % 64])
  res = {}
  if mode == "loop":
    def work():
      for s in range(steps):
        e.step(acts[s % 64])
    gpu, host = _timed(torch, work)
    res["loop"] = {"us_per_step": gpu / steps, "host_us_per_step": host / steps}
  else:
    keep = ("reward", "collective_reward", "step_type", "discount") if mode == "many_with" else ()
    for K in KS:
      out = e.step_many(acts[:K], keep=keep)   # (warm: the per-step tensors are allocated once)
      calls = max(1, steps // K)
      def work():
        for _ in range(calls):
          e.step_many(acts[:K], keep=keep, out=out)
      gpu, host = _timed(torch, work)
      res[f"K={K}"] = {"us_per_step": gpu / (calls * K), "host_us_per_step": host / (calls * K)}
  res["fault"] = bool(e.fault_words()[:6].any())
  e.close()
  return res


def trace(level):
  import torch
  from meltingpot_amd import engine
  n, skew = LEVELS[level]
  e = engine.Engine(engine.load_pack(level), n, device=0)
  e.reset()
  acts = _actions(e, torch, 64, skew)
  for K in KS:
    for _ in range(8):
      e.step_many(acts[:K])
  e.sync()
  e.close()
  return {"level": level, "calls_per_K": 8, "K": list(KS)}


def run_child(args, lib=None):
  env = dict(os.environ)
  if lib:
    env["MP_ENGINE_LIB"] = lib
  out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env,
                       capture_output=True, text=True, timeout=300)
  if out.returncode != 0:
    raise RuntimeError(f"child {args} (lib {lib}) exited {out.returncode}: {out.stderr[-2000:]}")
  return json.loads(out.stdout.strip().splitlines()[-1])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parent-lib", default="")
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--steps", type=int, default=2048)
  ap.add_argument("--warmup", type=int, default=40)
  ap.add_argument("--levels", default=",".join(LEVELS))
  ap.add_argument("--out", default="")
  ap.add_argument("--trace", default="")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.trace:
    print(json.dumps(trace(a.trace)))
    return
  if a.child:
    level, mode = a.child.split(":")
    print(json.dumps(child(level, mode, a.steps, a.warmup)))
    return
  import torch
  configs = []
  for level in a.levels.split(","):
    if a.parent_lib:
      configs.append((f"{level} | parent | loop", ["--child", f"{level}:loop"], a.parent_lib))
    configs += [(f"{level} | branch | loop", ["--child", f"{level}:loop"], None),
                (f"{level} | branch | many_with", ["--child", f"{level}:many_with"], None),
                (f"{level} | branch | many_without", ["--child", f"{level}:many_without"], None)]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "steps": a.steps,
         "rounds": a.rounds, "levels": {k: LEVELS[k][0] for k in a.levels.split(",")}, "results": {}}
  for r in range(a.rounds):
    order = configs if r % 2 == 0 else configs[::-1]
    for label, args, lib in order:
      got = run_child(args + ["--steps", str(a.steps), "--warmup", str(a.warmup)], lib)
      res["results"].setdefault(label, []).append(got)
      print(r, label, got, flush=True)
  summary = {}
  for label, rounds in res["results"].items():
    for key in rounds[0]:
      if key == "fault":
        continue
      for what in ("us_per_step", "host_us_per_step"):
        v = [g[key][what] for g in rounds]
        summary[f"{label} | {key} | {what}"] = {"median": float(np.median(v)), "min": float(min(v)),
                                                 "max": float(max(v))}
  res["summary"] = summary
  res["any_fault"] = any(g["fault"] for v in res["results"].values() for g in v)
  for k, v in summary.items():
    print(f"{k:90s} {v['median']:8.2f}  [{v['min']:.2f}, {v['max']:.2f}]")
  line = json.dumps(res)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")
  else:
    print(line)


if __name__ == "__main__":
  main()
