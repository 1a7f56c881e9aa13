"""Times the record check (profiles/r17_state_check.md): a check of R rows, and a checked load
against an unchecked one, on one GPU.

    python tools/time_state_check.py [--pack clean_up] [--rows 4096] [--calls 30] [--rounds 3]

Events on the engine's stream around `--calls` calls that end in a synchronise, after a warm-up;
prints one JSON line: median [min, max] microseconds per call over the rounds."""
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pack", default="clean_up")
  ap.add_argument("--rows", type=int, default=4096)
  ap.add_argument("--calls", type=int, default=30)
  ap.add_argument("--rounds", type=int, default=3)
  args = ap.parse_args()
  n = args.rows
  e = engine.Engine(engine.load_pack(args.pack), n, device=0)
  rng = np.random.default_rng(0)
  e.reset()
  for _ in range(40):   # rows of worlds that have played
    e.step(torch.from_numpy(rng.integers(0, e.num_actions, (n, e.P), dtype=np.int32)).to(e.device))
  bank = e.save_worlds().clone()
  assert not e.check_states(bank).cpu().numpy().any()
  out = torch.empty((n, 2), dtype=torch.int32, device=e.device)
  save_out = torch.empty_like(bank)
  perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(e.device)
  src = torch.arange(n, dtype=torch.int32, device=e.device)
  what = {
      "save_worlds": lambda: e.save_worlds(out=save_out),
      "check_states": lambda: e.check_states(bank, out=out),
      "check_states_permuted_rows": lambda: e.check_states(bank, rows=perm, out=out),
      "load_worlds": lambda: e.load_worlds(bank, src),
      "load_worlds_checked": lambda: e.load_worlds(bank, src, check=True),
  }
  times = {k: [] for k in what}
  for _ in range(args.rounds):
    for k, fn in what.items():   # alternated over the rounds
      times[k].append(timed(fn, args.calls))
  e.sync()
  assert not e.fault_words()[:6].any()
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  print(json.dumps({"pack": args.pack, "rows": n, "row_bytes": int(bank.shape[1]), "us_per_call": res}))


if __name__ == "__main__":
  main()
