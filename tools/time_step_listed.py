"""Times stepping a list of worlds (profiles/r26_step_listed.md) on one GPU, every figure against
the masked call of the same selection and the unmasked call of the same K in the same run.

    python tools/time_step_listed.py [--packs clean_up,collaborative_cooking__cramped]
                                     [--worlds 4096,32768] [--steps 1,4,64] [--calls 128] [--rounds 7]

Scalars only (no view bound; step_many's default four per-step kinds).  Per pack, N and K, one JSON
line with median [min, max] µs a REQUEST over the rounds, measured as tools/time_step_active.py
measures (its Blocker and timed(): events on the engine's stream, one warm-up window per variant,
every timed window enqueued behind a blocker, the variants alternated over the rounds, each on an
engine of its own; `device_bound` says whether the host kept ahead of the device).  Variants:
  unmasked      step_many(A): reference (b);
  masked_1      step_many(A, active=1): the mask that hides nothing;
  masked_2, _8  whole worlds inactive, a seeded choice of exactly N / 2 and N / 8 active worlds:
                reference (a) of the listed call of the same selection;
  listed_1      step_many(A[:, perm], worlds=perm), a seeded permutation of all N worlds: what the
                dependent load of worlds[i] and the claim launch cost;
  listed_2, _8  step_many(A[:, sel], worlds=sel) with sel the worlds masked_2 / masked_8 select, in
                a seeded order: M = N / 2 and N / 8 entries, ceil(M / 4) workgroups.
`ratio` is each listed variant's median over the masked median of the same selection;
`world_steps` (the engines' counters) shows that both ran the same number of world-steps."""
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

FRACTIONS = (1, 2, 8)


def one_case(name, n, K, args, blocker):
  calls = max(8, args.calls * 4 // max(4, K) * 4096 // max(4096, n))
  pack = engine.load_pack(name)
  rng = np.random.default_rng(0)
  probe = engine.Engine(pack, 1, device=0)
  nact, P = probe.num_actions, probe.P
  probe.close()
  A = torch.from_numpy(rng.integers(0, nact, (K, n, P), dtype=np.int32)).cuda()
  variants = {"unmasked": dict(actions=A)}
  for f in FRACTIONS:
    sel = rng.permutation(n)[:n // f]          # (a seeded choice, in a seeded order)
    mask = np.zeros(n, np.uint8)
    mask[sel] = 1
    worlds = torch.from_numpy(sel.astype(np.int32)).cuda()
    variants[f"masked_{f}"] = dict(actions=A, active=torch.from_numpy(mask).cuda())
    variants[f"listed_{f}"] = dict(actions=A[:, worlds.long()].contiguous(), worlds=worlds)
  engines, outs = {}, {}
  for how, kw in variants.items():
    e = engine.Engine(pack, n, device=0)
    e.reset()
    engines[how] = e
    outs[how] = e.step_many(kw["actions"], **{k: v for k, v in kw.items() if k != "actions"})
  times = {how: [] for how in variants}
  enqueue_ms = 0.0
  for _ in range(args.rounds):   # alternated over the rounds
    for how, kw in variants.items():
      e = engines[how]
      more = {k: v for k, v in kw.items() if k != "actions"}
      us, host_ms = timed(lambda: e.step_many(kw["actions"], out=outs[how], **more), calls, blocker)
      times[how].append(us)
      enqueue_ms = max(enqueue_ms, host_ms)
  steps = {}
  for how, e in engines.items():
    e.sync()
    assert not e.fault_words()[:40].any()
    steps[how] = e.counters()["world_steps"]
    e.close()
  for f in FRACTIONS:
    assert steps[f"masked_{f}"] == steps[f"listed_{f}"], (f, steps)
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  return {"pack": name, "worlds": n, "K": K, "calls": calls, "device": torch.cuda.get_device_name(0),
          "blocker_ms": round(blocker.ms, 1), "enqueue_ms": round(enqueue_ms, 1),
          "device_bound": bool(enqueue_ms < blocker.ms), "us_per_request": res,
          "ratio": {f"listed_{f}": round(res[f"listed_{f}"][0] / res[f"masked_{f}"][0], 3) for f in FRACTIONS},
          "world_steps": steps}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--packs", default="clean_up,collaborative_cooking__cramped")
  ap.add_argument("--worlds", default="4096,32768")
  ap.add_argument("--steps", default="1,4,64")
  ap.add_argument("--calls", type=int, default=128)
  ap.add_argument("--fills", type=int, default=60, help="2 GiB fills of the blocker in front of a window")
  ap.add_argument("--rounds", type=int, default=7)
  args = ap.parse_args()
  blocker = Blocker(args.fills)
  for name in args.packs.split(","):
    for n in (int(v) for v in args.worlds.split(",")):
      for K in (int(k) for k in args.steps.split(",")):
        print(json.dumps(one_case(name, n, K, args, blocker)), flush=True)


if __name__ == "__main__":
  main()
