"""Times `Engine.step_many(observations=...)` (per-step rows of LAYER and the scalar observations,
K steps in one launch) against what it replaces, on one box; the method of tools/time_step_many.py
(child processes, a warm-up, events around work that ends in a synchronise, configurations
alternated round by round, medians and ranges; beside the GPU time per step, the host's wall time
per call).

  python tools/time_step_trajectory.py --parent-lib PATH [--rounds 5] [--steps 2048] [--out FILE.json]

Per level of tools/time_step_many.py and K in 4, 16, 64, us per step of:
  many_with  an MpStepMany request with the four per-step outputs, on the parent build and on this
             one (nothing asked for must cost nothing: both run the same kernels);
  ring       the parent's cheapest way to the bytes of `rows`: the loop of `step` with LAYER,
             READY_TO_SHOOT and the five kinds bound as a rollout ring of T = K slots;
  rows       step_many with rows of LAYER, READY_TO_SHOOT and the five kinds;
  scalars    step_many with rows of READY_TO_SHOOT, POSITION, ORIENTATION and the five kinds
             (against many_with: what the scalar rows cost)."""
import argparse
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import time_step_many as base  # noqa: E402

KS = (4, 16, 64)
FOUR = ("reward", "collective_reward", "step_type", "discount")


def child(level, mode, steps, warmup):
  import torch
  from meltingpot_amd import engine as E
  n, skew = base.LEVELS[level]
  res = {}
  fault = False
  for K in KS:
    e = E.Engine(E.load_pack(level), n, device=0)
    e.use_current_stream()
    if mode == "ring":
      for kind in (E.OBS_LAYER, E.OBS_READY_TO_SHOOT, E.OBS_REWARD, E.OBS_COLLECTIVE_REWARD,
                   E.OBS_STEP_TYPE, E.OBS_DISCOUNT, E.OBS_EVENTS):
        e.bind_ring(kind, slots=K, tune=False)
    e.reset()
    acts = base._actions(e, torch, 64, skew)
    for s in range(warmup):
      e.step(acts[s % 64])
    if mode == "ring":
      def work():
        for s in range(steps):
          e.step(acts[s % 64])
      calls = steps // K
    else:
      kw = {"many_with": dict(keep=FOUR),
            "rows": dict(keep=FOUR, events=True, observations=(E.OBS_LAYER, E.OBS_READY_TO_SHOOT)),
            "scalars": dict(keep=FOUR, events=True,
                            observations=(E.OBS_READY_TO_SHOOT, E.OBS_POSITION, E.OBS_ORIENTATION))}[mode]
      out = e.step_many(acts[:K], **kw)   # (warm: the per-step tensors are allocated once)
      calls = max(1, steps // K)
      def work():
        for _ in range(calls):
          e.step_many(acts[:K], out=out, **kw)
    gpu, host = base._timed(torch, work)
    res[f"K={K}"] = {"us_per_step": gpu / (calls * K), "host_us_per_step": host / (calls * K)}
    fault = fault or bool(e.fault_words()[:6].any())
    e.close()
    del e
    torch.cuda.empty_cache()
  res["fault"] = fault
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parent-lib", default="")
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--steps", type=int, default=2048)
  ap.add_argument("--warmup", type=int, default=40)
  ap.add_argument("--levels", default=",".join(base.LEVELS))
  ap.add_argument("--out", default="")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    level, mode = a.child.split(":")
    print(json.dumps(child(level, mode, a.steps, a.warmup)))
    return
  import torch
  me = os.path.abspath(__file__)
  configs = []
  for level in a.levels.split(","):
    if a.parent_lib:
      configs += [(f"{level} | parent | many_with", f"{level}:many_with", a.parent_lib),
                  (f"{level} | parent | ring", f"{level}:ring", a.parent_lib)]
    configs += [(f"{level} | branch | {m}", f"{level}:{m}", None) for m in ("many_with", "rows", "scalars")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "steps": a.steps,
         "rounds": a.rounds, "levels": {k: base.LEVELS[k][0] for k in a.levels.split(",")}, "results": {}}
  for r in range(a.rounds):
    order = configs if r % 2 == 0 else configs[::-1]
    for label, spec, lib in order:
      env = dict(os.environ)
      if lib:
        env["MP_ENGINE_LIB"] = lib
      import subprocess
      out = subprocess.run([sys.executable, me, "--child", spec, "--steps", str(a.steps), "--warmup",
                            str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
      if out.returncode != 0:   # (nothing more runs on the GPU after a child that failed)
        raise RuntimeError(f"child {spec} (lib {lib}) exited {out.returncode}: {out.stderr[-2000:]}")
      got = json.loads(out.stdout.strip().splitlines()[-1])
      res["results"].setdefault(label, []).append(got)
      print(r, label, got, flush=True)
      if got["fault"]:
        raise RuntimeError(f"child {spec} reported fault words")
  summary = {}
  for label, rounds in res["results"].items():
    for key in rounds[0]:
      if key == "fault":
        continue
      v = [g[key]["us_per_step"] for g in rounds]
      # (host: wall time of one call's enqueue, where the Python and C checks of a request show)
      h = [g[key]["host_us_per_step"] * int(key.split("=")[1]) for g in rounds]
      summary[f"{label} | {key}"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                     "host_us_per_call": float(np.median(h))}
  res["summary"] = summary
  for k, v in summary.items():
    print(f"{k:70s} {v['median']:8.2f}  [{v['min']:.2f}, {v['max']:.2f}]  host {v['host_us_per_call']:8.2f} us a call")
  line = json.dumps(res)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")
  else:
    print(line)


if __name__ == "__main__":
  main()
