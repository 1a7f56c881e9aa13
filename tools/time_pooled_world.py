"""Times clean_up at 4096 worlds x 7 players on one box, every binding in one process and the
bindings alternated over several rounds: WORLD.RGB full and pooled by 8 alone, RGB_POOL8 beside
WORLD.RGB full and pooled by 8, and the full RGB beside WORLD.RGB pooled by 4 — events-timed us
per step (one launch each: the step's own launch draws the bound views), each binding as
`Engine.bind` leaves it and again with the plan `mp_tune` keeps for it.

  python tools/time_pooled_world.py [--worlds 4096] [--steps 50] [--rounds 3] [--out FILE.json]

Buffers are the engine's own placement (Engine.bind -> mp_place_output and mp_tune for views of
64 MB and more; a smaller view is a plain allocation under the stock plan), as `substrate.build`
gets them; "tuned" adds an explicit mp_tune whatever the size.  Each round builds every engine anew, so
the spread between rounds includes the buffers' placement."""
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


def time_binding(name, n, world_pool, kinds, steps, warmup, tune=False):
  pack = engine.load_pack(name)
  e = engine.Engine(pack, n, device=0, world_pool=world_pool)
  nbytes = 0
  for k in kinds:
    t = e.bind(k)
    nbytes += t.numel() * t.element_size()
  if tune:
    e.tune()
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
  plan = e.plan
  faults = bool(e.fault_words()[:6].any())
  e.close()
  return {"us_per_step": round(us, 2), "pixel_bytes_per_step": nbytes, "plan": plan, "fault": faults}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--name", default="clean_up")
  ap.add_argument("--worlds", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--out", default="")
  a = ap.parse_args()
  E = engine
  # label -> (world_pool, kinds bound)
  bindings = {"WORLD.RGB full": (1, (E.OBS_WORLD_RGB,)),
              "WORLD.RGB pooled by 8": (8, (E.OBS_WORLD_RGB,)),
              "RGB_POOL8 + WORLD.RGB full": (1, (E.OBS_RGB_POOL8, E.OBS_WORLD_RGB)),
              "RGB_POOL8 + WORLD.RGB pooled by 8": (8, (E.OBS_RGB_POOL8, E.OBS_WORLD_RGB)),
              "RGB full + WORLD.RGB pooled by 4": (4, (E.OBS_RGB, E.OBS_WORLD_RGB))}
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
         "substrate": a.name, "worlds": a.worlds, "steps": a.steps, "rounds": a.rounds,
         "results": {}}
  for r in range(a.rounds):
    for label, (kw, kinds) in bindings.items():
      for tune in (False, True):
        key = label + (", tuned" if tune else "")
        got = time_binding(a.name, a.worlds, kw, kinds, a.steps, a.warmup, tune)
        res["results"].setdefault(key, []).append(got)
        print(r, key, got, flush=True)
  res["median_us"] = {label: float(np.median([g["us_per_step"] for g in v]))
                      for label, v in res["results"].items()}
  line = json.dumps(res)
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
