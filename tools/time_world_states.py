"""dev helper: what world states cost on clean_up at 4096 worlds x 7 players with WORLD.RGB bound
(profiles/r11_world_states.md).  Times, with device events around REPS launches each:
  * mp_save_worlds of every world (a 25 MB device gather), against a plain device copy of the
    same bytes;
  * mp_load_worlds of every world from a shuffled bank, against the dry masked reset (mask all
    zero: the same launch, nothing reset) and a real step;
  * the host round trip mp_snapshot + mp_restore (wall clock: both synchronise).
Prints one JSON line.

  python tools/time_world_states.py [worlds] [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meltingpot_amd import engine as E  # noqa: E402


def timed(fn, reps):
  """Mean µs of fn() over `reps` launches, between two events on the current stream."""
  fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(reps):
    fn()
  b.record()
  b.synchronize()
  return round(a.elapsed_time(b) * 1000.0 / reps, 2)


def main():
  n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
  reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
  eng = E.Engine(E.load_pack("clean_up"), n, device=0)
  eng.bind(E.OBS_WORLD_RGB)
  assert eng.fused
  eng.reset()
  acts = torch.randint(0, eng.num_actions, (n, eng.P), dtype=torch.int32, device=eng.device)
  for _ in range(20):
    eng.step(acts)
  S = eng.info.world_state_bytes
  bank = eng.save_worlds()
  shuffled = bank[torch.randperm(n, device=eng.device)].contiguous()
  src = torch.randperm(n, device=eng.device).to(torch.int32)
  copy_dst = torch.empty_like(bank)
  out = {"substrate": "clean_up", "worlds": n, "players": eng.P, "record_bytes": S,
         "bank_mb": round(n * S / 1e6, 2), "reps": reps}
  out["save_all_us"] = timed(lambda: eng.save_worlds(out=bank), reps)
  out["device_copy_us"] = timed(lambda: copy_dst.copy_(bank), reps)
  out["load_all_shuffled_us"] = timed(lambda: eng.load_worlds(shuffled, src), reps)
  none = np.zeros(n, np.uint8)
  t0 = time.perf_counter()
  for _ in range(5):
    eng.reset(mask=none)   # (mp_reset copies the mask from the host and synchronises)
  torch.cuda.synchronize()
  out["dry_masked_reset_wall_us"] = round((time.perf_counter() - t0) * 1e6 / 5, 1)
  out["dry_masked_reset_us"] = timed(lambda: eng.reset(mask=none), 10)
  # the dry masked reset's own launch, without the host copy of the mask: a load whose src is
  # all -1 is that launch (every world outside the mask)
  keep = torch.full((n,), -1, dtype=torch.int32, device=eng.device)
  out["dry_load_us"] = timed(lambda: eng.load_worlds(bank, keep), reps)
  out["step_us"] = timed(lambda: eng.step(acts), reps)
  eng.sync()
  t0 = time.perf_counter()
  for _ in range(3):
    snap = eng.snapshot()
    eng.restore(snap)
  eng.sync()
  out["host_snapshot_restore_us"] = round((time.perf_counter() - t0) * 1e6 / 3, 1)
  out["save_gb_s"] = round(2 * n * S / (out["save_all_us"] * 1e3), 1)
  assert not eng.fault_words()[:6].any()
  eng.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
