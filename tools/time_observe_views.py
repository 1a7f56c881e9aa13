"""Times `Engine.observe_views` (sampled (row, player) views of saved world states) against the only
way to get the same tensor without it, on one box; the method of tools/time_observe_states.py (child
processes, a warm-up, events on the engine's stream around calls that only enqueue, configurations
alternated round by round, medians and ranges).

  python tools/time_observe_views.py [--rounds 2] [--out FILE.json]

Levels clean_up (P = 7) and commons_harvest__open (P = 16); R = 256, 4096 and 32768 sampled views;
kinds RGB, RGB_POOL8 and LAYER.  The rows are a random sample, with repeats, of a bank of 4096 worlds
that have played 40 steps; the players are random.  us per call of:
  views    observe_views(bank, kind, players, rows, out=out): R views written;
  rows     observe_states(bank, kind, rows=rows, out=whole)[arange(R), players]: every player of
           every sampled row drawn into an [R, P, ...] intermediate, then indexed — the index is part
           of what is timed.  A configuration whose intermediate does not fit the free device memory
           is skipped, and the summary says so.
Every configuration (level, R, kind, path) runs in a child process of its own under a time limit; the
first child that does not end normally, or that reports fault words, ends the run."""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import time_step_many as base  # noqa: E402

LEVELS = ("clean_up", "commons_harvest__open")
COUNTS = (256, 4096, 32768)
KINDS = ("RGB", "RGB_POOL8", "LAYER")
BANK_ROWS = 4096
CHILD_SECONDS = 240


def _bank(E, torch, level):
  """BANK_ROWS saved records of worlds that have played 40 steps."""
  e = E.Engine(E.load_pack(level), BANK_ROWS, device=0)
  e.reset()
  acts = base._actions(e, torch, 40, 0.0)
  for s in range(40):
    e.step(acts[s])
  bank = e.save_worlds().clone()
  e.sync()
  e.close()
  return bank


def child(level, R, name, path, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  bank = _bank(E, torch, level)
  e = E.Engine(E.load_pack(level), 256, device=0)
  e.use_current_stream()
  gen = torch.Generator().manual_seed(3)
  rows = torch.randint(0, BANK_ROWS, (R,), generator=gen).to(torch.int32).to(e.device)
  players = torch.randint(0, e.P, (R,), generator=gen).to(torch.int32).to(e.device)
  kind = getattr(E, "OBS_" + name)
  shape, dtype = e.shapes[kind]
  elem = torch.empty((), dtype=dtype).element_size()
  view_bytes = int(np.prod(shape[2:])) * elem
  res = {"view_bytes": view_bytes, "bytes": R * view_bytes, "P": e.P, "skipped": ""}
  if path == "views":
    out = torch.empty((R,) + tuple(shape[2:]), dtype=dtype, device=e.device)
    call = lambda: e.observe_views(bank, kind, players, rows, out=out)
  else:
    # the intermediate, the gathered rows (the engine's scratch) and the indexed result
    need = R * e.P * view_bytes + R * int(e.info.world_state_bytes) + 2 * R * view_bytes
    free = torch.cuda.mem_get_info()[0]
    res["intermediate_bytes"] = R * e.P * view_bytes
    if need > 0.8 * free:
      res["skipped"] = f"the [R, P, ...] intermediate and its copies need {need / 1e9:.1f} GB, {free / 1e9:.1f} GB are free"
      res["fault"] = False
      e.close()
      return res
    whole = torch.empty((R,) + tuple(shape[1:]), dtype=dtype, device=e.device)
    at, who = torch.arange(R, device=e.device), players.long()
    call = lambda: e.observe_states(bank, kind, rows=rows, out=whole)[at, who]
  for _ in range(warmup):
    call()
  def work():
    for _ in range(reps):
      call()
  gpu, host = base._timed(torch, work)
  res.update({"us_per_call": gpu / reps, "host_us_per_call": host / reps})
  e.sync()
  res["fault"] = bool(e.fault_words()[:10].any())
  e.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=2)
  ap.add_argument("--reps", type=int, default=30)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--levels", default=",".join(LEVELS))
  ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
  ap.add_argument("--out", default="")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    level, R, name, path = a.child.split(":")
    print(json.dumps(child(level, int(R), name, path, a.reps, a.warmup)))
    return
  if a.rounds < 2:
    raise SystemExit("--rounds must be at least 2: the configurations are alternated")
  import torch
  me = os.path.abspath(__file__)
  configs = [(f"{level} | R={R} | {name} | {path}", f"{level}:{R}:{name}:{path}")
             for level in a.levels.split(",") for R in (int(c) for c in a.counts.split(","))
             for name in KINDS for path in ("views", "rows")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
         "reps": a.reps, "bank_rows": BANK_ROWS, "results": {}}
  for r in range(a.rounds):
    order = configs if r % 2 == 0 else configs[::-1]
    for label, spec in order:
      out = subprocess.run([sys.executable, me, "--child", spec, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=CHILD_SECONDS)
      if out.returncode != 0:   # (nothing more runs on the GPU after a child that failed)
        raise RuntimeError(f"child {spec} exited {out.returncode}: {out.stderr[-2000:]}")
      got = json.loads(out.stdout.strip().splitlines()[-1])
      res["results"].setdefault(label, []).append(got)
      print(r, label, got, flush=True)
      if got["fault"]:
        raise RuntimeError(f"child {spec} reported fault words")
  summary = {}
  for label, rounds in res["results"].items():
    if rounds[0]["skipped"]:
      summary[label] = {"skipped": rounds[0]["skipped"]}
      continue
    v = [g["us_per_call"] for g in rounds]
    summary[label] = {"median_us_per_call": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                      "MB": rounds[0]["bytes"] / 1e6}
    if "intermediate_bytes" in rounds[0]:
      summary[label]["intermediate_MB"] = rounds[0]["intermediate_bytes"] / 1e6
  res["summary"] = summary
  for k, v in summary.items():
    print(f"{k:55s} " + "  ".join(f"{n} {x:.2f}" if isinstance(x, float) else f"{n} {x}" for n, x in v.items()))
  line = json.dumps(res)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")
  else:
    print(line)


if __name__ == "__main__":
  main()
