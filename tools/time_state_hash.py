"""Times the state hash (profiles/r18_state_hash.md) on one GPU: a hash of R rows against the
save of the same worlds (the launch that reads the same bytes), and a K-step launch with the hash
row against the same launch with no rows and with the state row.

    python tools/time_state_hash.py [--packs clean_up,collaborative_cooking__cramped] [--rows 4096]
                                    [--steps 64] [--calls 30] [--rounds 3]

Events on the engine's stream around `--calls` calls that end in a synchronise, after a warm-up;
prints one JSON line per pack: median [min, max] microseconds per call over the rounds, and per
step for the K-step launches."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from meltingpot_amd import engine  # noqa: E402


def timed(fn, calls):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(calls):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) * 1000.0 / calls


def one_pack(name, args):
  n, K = args.rows, args.steps
  e = engine.Engine(engine.load_pack(name), n, device=0)
  rng = np.random.default_rng(0)
  e.reset()
  for _ in range(40):   # rows of worlds that have played
    e.step(torch.from_numpy(rng.integers(0, e.num_actions, (n, e.P), dtype=np.int32)).to(e.device))
  bank = e.save_worlds().clone()
  S = int(bank.shape[1])
  h = torch.empty((n,), dtype=torch.int64, device=e.device)
  host = engine.hash_states_host(engine.load_pack(name), bank[:64].cpu().numpy())
  assert np.array_equal(e.hash_states(bank).cpu().numpy()[:64], host)
  save_out = torch.empty_like(bank)
  perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(e.device)
  cell = dict(planes=(e.state_layout().avatar_layer,), fields=("ax", "ay"))
  A = torch.from_numpy(rng.integers(0, e.num_actions, (K, n, e.P), dtype=np.int32)).to(e.device)
  keep = e.step_many(A)   # (the four scalar kinds every call stacks)
  out_h = dict(keep, hashes=torch.empty((K, n), dtype=torch.int64, device=e.device))
  out_s = dict(keep, states=torch.empty((K, n, S), dtype=torch.uint8, device=e.device))
  calls = {
      "save_worlds": lambda: e.save_worlds(out=save_out),
      "hash_states": lambda: e.hash_states(bank, out=h),
      "hash_states_permuted_rows": lambda: e.hash_states(bank, rows=perm, out=h),
      "hash_worlds": lambda: e.hash_worlds(out=h),
      "hash_states_cell": lambda: e.hash_states(bank, out=h, **cell),
  }
  many = {
      "step_many": lambda: e.step_many(A, out=keep),
      "step_many_hashes": lambda: e.step_many(A, out=out_h),
      "step_many_states": lambda: e.step_many(A, out=out_s),
  }
  times = {k: [] for k in list(calls) + list(many)}
  for _ in range(args.rounds):   # alternated over the rounds
    for k, fn in calls.items():
      times[k].append(timed(fn, args.calls))
    for k, fn in many.items():
      times[k].append(timed(fn, max(2, args.calls // 10)) / K)
  e.sync()
  assert not e.fault_words()[:10].any()
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  e.close()
  return {"pack": name, "rows": n, "row_bytes": S, "steps": K, "device": torch.cuda.get_device_name(0),
          "us_per_call": {k: res[k] for k in calls}, "us_per_step": {k: res[k] for k in many}}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--packs", default="clean_up,collaborative_cooking__cramped")
  ap.add_argument("--rows", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=64)
  ap.add_argument("--calls", type=int, default=30)
  ap.add_argument("--rounds", type=int, default=3)
  args = ap.parse_args()
  for name in args.packs.split(","):
    print(json.dumps(one_pack(name, args)), flush=True)


if __name__ == "__main__":
  main()
