"""Times a mixture of the five 2-player kitchens (`substrate.build_mixture`) on one box.

  python tools/time_mixture.py [--rounds 5] [--steps 50] [--warmup 20] [--out FILE.json]

Three loops of 4096 worlds x 2 players, events-timed us per step:
  mixture   the five kitchens as one MixtureSubstrate (each member's step launch in turn);
  single    one kitchen (collaborative_cooking__cramped) as one Substrate;
  cat       what a user writes without a mixture: five Substrates stepped one after the other
            and every leaf joined with torch.cat each step.
each with the stock observations (RGB + WORLD.RGB), pooled by 8 (`rgb_pool=8,
world_rgb_pool=8`), and with a ring of T = 32 (`rollout_length=32`; for `cat` the joined leaves
are copied into a [T, N, ...] ring of the user's own, the copy a learner's rollout makes).

Every configuration runs in a child process of its own, and the configurations are alternated
round by round.  Medians over the rounds are reported."""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, P, T = 4096, 2, 32
KITCHENS = tuple(f"collaborative_cooking__{k}" for k in ("asymmetric", "circuit", "cramped", "forced", "ring"))


def _leaves(ts):
  return [ts.step_type, ts.reward, ts.discount] + [ts.observation[n] for n in sorted(ts.observation)]


def child(loop, views, steps, warmup):
  import torch
  from meltingpot_amd import substrate
  kw = {"env_seed": 1}
  if views == "pooled":
    kw.update(rgb_pool=8, world_rgb_pool=8)
  if views == "ring":
    kw.update(rollout_length=T)
  roles = ("default",) * P
  if loop == "mixture":
    env = substrate.build_mixture(KITCHENS, num_worlds=N, **kw)
    envs = [env]
    step = env.step
  elif loop == "single":
    env = substrate.build("collaborative_cooking__cramped", roles=roles, num_worlds=N, **kw)
    envs = [env]
    step = env.step
  else:
    kw.pop("rollout_length", None)
    counts = substrate.split_worlds(N, len(KITCHENS), 1)
    offsets = np.cumsum([0] + counts[:-1])
    envs = [substrate.build(n, roles=roles, num_worlds=c, world_offset=int(o), **kw)
            for n, c, o in zip(KITCHENS, counts, offsets)]
    ring = [None]
    slot = [0]

    def step(a):
      outs = [e.step(a[o:o + c]) for e, o, c in zip(envs, offsets, counts)]
      joined = [torch.cat(parts) for parts in zip(*[_leaves(ts) for ts in outs])]
      if views == "ring":
        if ring[0] is None:
          ring[0] = [torch.empty((T,) + tuple(j.shape), dtype=j.dtype, device=j.device) for j in joined]
        for r, j in zip(ring[0], joined):
          r[slot[0] % T].copy_(j)
        slot[0] += 1
      return joined
  for e in envs:
    e.reset()
  gen = torch.Generator(device="cuda").manual_seed(0)
  acts = torch.randint(0, 8, (16, N, P), dtype=torch.int32, device="cuda", generator=gen)
  for s in range(warmup):
    step(acts[s % 16])
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for s in range(steps):
    step(acts[s % 16])
  b.record()
  b.synchronize()
  s_per_step = a.elapsed_time(b) * 1e-3 / steps
  engines = envs[0].engines if loop == "mixture" else [e.engine for e in envs]
  fault = any(bool(e.fault_words()[:6].any()) for e in engines)
  for e in envs:
    e.close()
  return {"us_per_step": s_per_step * 1e6, "agent_steps_per_s": N * P / s_per_step, "fault": fault}


def run_child(args):
  out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args,
                       capture_output=True, text=True, timeout=600)
  if out.returncode != 0:
    raise RuntimeError(f"child {args} exited {out.returncode}: {out.stderr[-2000:]}")
  return json.loads(out.stdout.strip().splitlines()[-1])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--out", default="")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    loop, views = a.child.split(":")
    print(json.dumps(child(loop, views, a.steps, a.warmup)))
    return
  import torch
  configs = [f"{loop}:{views}" for views in ("stock", "pooled", "ring")
             for loop in ("mixture", "single", "cat")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "worlds": N,
         "players": P, "steps": a.steps, "rounds": a.rounds, "results": {}}
  for r in range(a.rounds):
    for label in (configs if r % 2 == 0 else configs[::-1]):
      got = run_child(["--child", label, "--steps", str(a.steps), "--warmup", str(a.warmup)])
      res["results"].setdefault(label, []).append(got)
      print(r, label, got, flush=True)
  res["median_us"] = {k: float(np.median([g["us_per_step"] for g in v])) for k, v in res["results"].items()}
  res["range_us"] = {k: [float(min(g["us_per_step"] for g in v)), float(max(g["us_per_step"] for g in v))]
                     for k, v in res["results"].items()}
  res["any_fault"] = any(g["fault"] for v in res["results"].values() for g in v)
  line = json.dumps(res)
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
