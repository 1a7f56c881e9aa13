"""Times masked stepping (profiles/r21_step_active.md) on one GPU, every figure against the
unmasked step_many of the same K in the same run.

    python tools/time_step_active.py [--packs clean_up,collaborative_cooking__cramped]
                                     [--worlds 4096] [--steps 1,4,64] [--calls 128] [--rounds 7]

Scalars only (no view bound; step_many's default four per-step kinds).  Per pack and K, one JSON
line with median [min, max] µs a REQUEST over the rounds (events on the engine's stream, one warm-up
window per variant, the variants alternated over the rounds, each on an engine of its own).  A
request of K = 1 runs for less time than Python needs to enqueue it, so every timed window is
enqueued BEHIND a blocker (fills of a 2 GiB buffer, `blocker_ms` long) and the first event is
recorded after it: the requests are already queued when the device reaches them, and the events see
device time only as long as `enqueue_ms` (the host's time to enqueue the slowest window) stays below
`blocker_ms` — `device_bound` says whether it did.  Variants:
  unmasked  step_many(A): the k_step_many_* kernels, which are instruction for instruction the
            parent commit's (profiles/r21_step_active.md records the comparison);
  ones      step_many(A, active=1): what the mask costs when it hides nothing;
  half, eighth   whole worlds inactive, a seeded choice of exactly N / 2 and N / 8 active worlds:
            the waves of the others return without loading their records;
  ragged    (the largest K only) lengths drawn uniformly from 1 .. K, as the mask
            arange(K)[:, None] < lengths[None]; `share` is the share of world-steps actually run.
`ratio` is each variant's median over the unmasked median."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from meltingpot_amd import engine  # noqa: E402


class Blocker:
  """Keeps the device busy while the host enqueues a timed window."""

  def __init__(self, fills):
    self.buf = torch.empty(2 << 30, dtype=torch.uint8, device="cuda")
    self.fills = fills
    self()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    self()
    b.record()
    torch.cuda.synchronize()
    self.ms = a.elapsed_time(b)

  def __call__(self):
    for _ in range(self.fills):
      self.buf.fill_(0)


def timed(fn, calls, blocker):
  """(µs a call of fn() on the device, ms the host took to enqueue the window); one warm-up
  window first."""
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0 = time.perf_counter()
  blocker()
  a.record()
  for _ in range(calls):
    fn()
  b.record()
  host_ms = (time.perf_counter() - t0) * 1000.0
  torch.cuda.synchronize()
  return a.elapsed_time(b) * 1000.0 / calls, host_ms


def chosen(n, count, rng, device):
  m = np.zeros(n, np.uint8)
  m[rng.choice(n, size=count, replace=False)] = 1
  return torch.from_numpy(m).to(device)


def one_case(name, K, args, ragged, blocker):
  n = args.worlds
  calls = max(16, args.calls * 4 // max(4, K))
  pack = engine.load_pack(name)
  rng = np.random.default_rng(0)
  probe = engine.Engine(pack, 1, device=0)
  nact, P = probe.num_actions, probe.P
  probe.close()
  A = torch.from_numpy(rng.integers(0, nact, (K, n, P), dtype=np.int32)).cuda()
  masks = {"unmasked": None, "ones": torch.ones(n, dtype=torch.uint8, device=A.device),
           "half": chosen(n, n // 2, rng, A.device), "eighth": chosen(n, n // 8, rng, A.device)}
  share = None
  if ragged:
    lengths = torch.from_numpy(rng.integers(1, K + 1, n)).to(A.device)
    masks["ragged"] = torch.arange(K, device=A.device)[:, None] < lengths[None]
    share = float(lengths.sum()) / (K * n)
  engines, outs = {}, {}
  for how, mask in masks.items():
    e = engine.Engine(pack, n, device=0)
    e.reset()
    engines[how] = e
    outs[how] = e.step_many(A, active=mask)
  times = {how: [] for how in masks}
  enqueue_ms = 0.0
  for _ in range(args.rounds):   # alternated over the rounds
    for how, mask in masks.items():
      e = engines[how]
      us, host_ms = timed(lambda: e.step_many(A, out=outs[how], active=mask), calls, blocker)
      times[how].append(us)
      enqueue_ms = max(enqueue_ms, host_ms)
  steps = {}
  for how, e in engines.items():
    e.sync()
    assert not e.fault_words()[:40].any()
    steps[how] = e.counters()["world_steps"]
    e.close()
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  base = res["unmasked"][0]
  out = {"pack": name, "worlds": n, "K": K, "calls": calls, "device": torch.cuda.get_device_name(0),
         "blocker_ms": round(blocker.ms, 1), "enqueue_ms": round(enqueue_ms, 1),
         "device_bound": bool(enqueue_ms < blocker.ms), "us_per_request": res,
         "ratio": {k: round(v[0] / base, 3) for k, v in res.items()}, "world_steps": steps}
  if share is not None:
    out["share"] = round(share, 3)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--packs", default="clean_up,collaborative_cooking__cramped")
  ap.add_argument("--worlds", type=int, default=4096)
  ap.add_argument("--steps", default="1,4,64")
  ap.add_argument("--calls", type=int, default=128)
  ap.add_argument("--fills", type=int, default=60, help="2 GiB fills of the blocker in front of a window")
  ap.add_argument("--rounds", type=int, default=7)
  args = ap.parse_args()
  Ks = [int(k) for k in args.steps.split(",")]
  blocker = Blocker(args.fills)
  for name in args.packs.split(","):
    for K in Ks:
      print(json.dumps(one_case(name, K, args, K == max(Ks) and K > 1, blocker)), flush=True)


if __name__ == "__main__":
  main()
