"""Times "N.LAYER" as a policy input on clean_up at 4096 worlds x 7 players, on one box.

  python tools/time_layer_obs.py [--parent-lib PATH] [--rounds 5] [--steps 50] [--out FILE.json]
  python tools/time_layer_obs.py --trace     # 20 steps with LAYER bound alone (for rocprofv3)

(a) a step with LAYER bound, this build (one launch writes it) against another build of the
    engine (`--parent-lib`: the step launch + k_layer_view), and a step with nothing but the
    scalars bound on both, events-timed us per step;
(b) agent-steps per second of `Substrate` loops on this build: symbolic-only (LAYER +
    READY_TO_SHOOT + COLLECTIVE_REWARD, no pixels), the pooled drop-in (rgb_pool=8,
    world_rgb_pool=8) and the full drop-in (the stock observations);
(c) the bytes a LAYER step moves (LAYER written, records read and written back) against the
    time it takes.

Every configuration runs in a child process of its own (a process loads one engine library),
and the configurations are alternated round by round (paired: the same round's numbers were
taken within seconds of each other).  Medians over the rounds are reported."""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, P = 4096, 7


def child_engine(layer, steps, warmup):
  import torch
  from meltingpot_amd import engine
  e = engine.Engine(engine.load_pack("clean_up"), N, device=0)
  if layer:
    e.bind(engine.OBS_LAYER)
  e.reset()
  rng = np.random.default_rng(0)
  acts = torch.from_numpy(rng.integers(0, e.num_actions, size=(8, N, P), dtype=np.int32)).to(e.device)
  e.use_current_stream()
  for s in range(warmup):
    e.step(acts[s % 8])
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for s in range(steps):
    e.step(acts[s % 8])
  b.record()
  b.synchronize()
  us = a.elapsed_time(b) * 1e3 / steps
  fault = bool(e.fault_words()[:6].any())
  info = engine.MpInfo()
  e._L.mp_info(e._h, ctypes.byref(info))
  e.close()
  return {"us_per_step": us, "fault": fault, "world_state_bytes": int(info.world_state_bytes)}


def child_substrate(kind, steps, warmup):
  import torch
  from meltingpot_amd import substrate
  cfg = substrate.get_config("clean_up")
  kw = {}
  if kind == "symbolic":
    cfg.individual_observation_names = ["LAYER", "READY_TO_SHOOT"]
    cfg.global_observation_names = []
  elif kind == "pooled":
    kw = {"rgb_pool": 8, "world_rgb_pool": 8}
  env = substrate.build_from_config(cfg, roles=cfg.default_player_roles, num_worlds=N, **kw)
  env.reset()
  rng = np.random.default_rng(0)
  acts = torch.from_numpy(rng.integers(0, 9, size=(8, N, P), dtype=np.int32)).to("cuda")
  for s in range(warmup):
    env.step(acts[s % 8])
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for s in range(steps):
    env.step(acts[s % 8])
  b.record()
  b.synchronize()
  s_per_step = a.elapsed_time(b) * 1e-3 / steps
  fault = bool(env.engine.fault_words()[:6].any())
  env.close()
  return {"us_per_step": s_per_step * 1e6, "agent_steps_per_s": N * P / s_per_step, "fault": fault}


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
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--out", default="")
  ap.add_argument("--trace", action="store_true")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.trace:
    print(json.dumps(child_engine(True, 20, 5)))
    return
  if a.child:
    what, arg = a.child.split(":")
    got = (child_engine(arg == "layer", a.steps, a.warmup) if what == "engine"
           else child_substrate(arg, a.steps, a.warmup))
    print(json.dumps(got))
    return
  import torch
  configs = [("branch, LAYER", ["--child", "engine:layer"], None),
             ("branch, scalars only", ["--child", "engine:none"], None)]
  if a.parent_lib:
    configs += [("parent, LAYER", ["--child", "engine:layer"], a.parent_lib),
                ("parent, scalars only", ["--child", "engine:none"], a.parent_lib)]
  configs += [(f"Substrate {k}", ["--child", f"substrate:{k}"], None)
              for k in ("symbolic", "pooled", "full")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "worlds": N,
         "players": P, "steps": a.steps, "rounds": a.rounds, "results": {}}
  for r in range(a.rounds):
    order = configs if r % 2 == 0 else configs[::-1]
    for label, args, lib in order:
      got = run_child(args + ["--steps", str(a.steps), "--warmup", str(a.warmup)], lib)
      res["results"].setdefault(label, []).append(got)
      print(r, label, got, flush=True)
  med = {label: float(np.median([g["us_per_step"] for g in v])) for label, v in res["results"].items()}
  res["median_us"] = med
  res["median_agent_steps_per_s"] = {
      label: float(np.median([g["agent_steps_per_s"] for g in v]))
      for label, v in res["results"].items() if "agent_steps_per_s" in v[0]}
  res["any_fault"] = any(g["fault"] for v in res["results"].values() for g in v)
  # (c) bytes: LAYER [N][P][11][11][9] int32 written, the records read and written back
  layer_bytes = N * P * 11 * 11 * 9 * 4
  rec_bytes = 2 * N * res["results"]["branch, LAYER"][0]["world_state_bytes"]
  res["bytes_per_step"] = {"layer": layer_bytes, "records_read_and_written": rec_bytes}
  res["gb_per_s"] = (layer_bytes + rec_bytes) / (med["branch, LAYER"] * 1e-6) / 1e9
  line = json.dumps(res)
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
