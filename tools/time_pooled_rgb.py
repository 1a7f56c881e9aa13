"""Times clean_up at 4096 worlds x 7 players on one box and one buffer per binding: the pooled
per-agent view RGB_POOL8 alone, RGB_POOL8 + WORLD.RGB, the full RGB alone and with WORLD.RGB
(what `substrate.build` binds with and without rgb_pool) — events-timed us per
step (one launch each: the step's own launch draws the bound views) and agent-steps/s — and,
as the floor the pooled launch should approach, the stand-alone step kernels (nothing bound).

  python tools/time_pooled_rgb.py [--worlds 4096] [--steps 50] [--out profiles/r07_pooled_rgb.json]

Buffers are the engine's own placement (Engine.bind -> mp_place_output for the large views,
mp_tune for the plan), as `substrate.build` gets them."""
import argparse
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from meltingpot_amd import engine  # noqa: E402


def time_binding(name, n, kinds, steps, warmup):
  pack = engine.load_pack(name)
  e = engine.Engine(pack, n, device=0)
  for k in kinds:
    e.bind(k)
  e.reset()
  rng = np.random.default_rng(0)
  acts = torch.from_numpy(rng.integers(0, e.num_actions, size=(8, n, e.P), dtype=np.int32)).to(e.device)
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
  info = e.plan
  faults = bool(e.fault_words()[:6].any())
  P = e.P
  e.close()
  return {"us_per_step": round(us, 2), "agent_steps_per_s": round(n * P / us * 1e6, 0),
          "plan": info, "fault": faults}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--name", default="clean_up")
  ap.add_argument("--worlds", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--out", default="")
  a = ap.parse_args()
  E = engine
  bindings = {"step kernels alone (nothing bound)": (),
              "RGB_POOL8": (E.OBS_RGB_POOL8,),
              "RGB_POOL8 + WORLD.RGB": (E.OBS_RGB_POOL8, E.OBS_WORLD_RGB),
              "RGB (full)": (E.OBS_RGB,),
              "RGB + WORLD.RGB (full)": (E.OBS_RGB, E.OBS_WORLD_RGB)}
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
         "substrate": a.name, "worlds": a.worlds, "steps": a.steps, "results": {}}
  for label, kinds in bindings.items():
    res["results"][label] = time_binding(a.name, a.worlds, kinds, a.steps, a.warmup)
    print(label, res["results"][label], flush=True)
  line = json.dumps(res)
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
