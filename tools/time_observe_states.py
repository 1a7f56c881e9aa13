"""Times `Engine.observe_states` (observations of saved world states, drawn from bank rows) and the
per-step state rows of `Engine.step_many(states=True)` against what they stand beside, on one box;
the method of tools/time_step_many.py (child processes, a warm-up, events on the engine's stream
around work that ends in a synchronise, configurations alternated round by round, medians and
ranges).

  python tools/time_observe_states.py --parent-lib PATH [--rounds 3] [--out FILE.json]

observe_states, clean_up, R = 256 and 4096 rows, kinds RGB, WORLD.RGB, RGB_POOL8 and LAYER, us per
call of:
  observe     mp_observe(kind) of an engine of N = R worlds on the PARENT build: the same draw
              from the engine's own records, without a bank;
  rows=None   observe_states(bank, kind) on an engine of N = R: the rows as they lie;
  rows        observe_states(bank, kind, rows=a permutation): gathered (the pixel kinds copy the
              rows into the engine's scratch first);
  small       (R = 4096 only) observe_states(bank, kind) on an engine of N = 256 worlds: a plan made
              for the count, or chunks of N.
State rows, clean_up and territory__rooms, step_many(K = 64) of N = 4096 worlds, us per step of:
  none        no rows beyond the four per-step outputs (parent and this build);
  layer       + rows of LAYER (parent and this build);
  states      + the state rows (this build);
  both        + LAYER and the state rows (this build).
--variant-lib PATH adds layer, states and both on a third library: a build of this source with the
state row as one more runtime branch of the k_step_rows_* kernels instead of a kernel family of
its own (what profiles/r16_observe_states.md compares)."""
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

KINDS = ("RGB", "WORLD_RGB", "RGB_POOL8", "LAYER")
FOUR = ("reward", "collective_reward", "step_type", "discount")
K = 64


def _bank(E, torch, level, rows):
  """`rows` saved records of worlds that have played 40 steps."""
  e = E.Engine(E.load_pack(level), rows, device=0)
  e.reset()
  acts = base._actions(e, torch, 40, 0.0)
  for s in range(40):
    e.step(acts[s])
  bank = e.save_worlds().clone()
  e.sync()
  e.close()
  return bank


def child_observe(mode, R, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  n = 256 if mode == "small" else R
  e = E.Engine(E.load_pack("clean_up"), n, device=0)
  e.use_current_stream()
  res = {}
  if mode == "observe":
    e.reset()
    acts = base._actions(e, torch, 40, 0.0)
    for s in range(40):
      e.step(acts[s])
  else:
    bank = _bank(E, torch, "clean_up", R)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(e.device)
  for name in KINDS:
    kind = getattr(E, "OBS_" + name)
    shape, dtype = e.shapes[kind]
    out = torch.empty((R,) + tuple(shape[1:]), dtype=dtype, device=e.device)
    if mode == "observe":
      call = lambda: e.observe(kind, out=out)
    elif mode == "rows":
      call = lambda: e.observe_states(bank, kind, rows=perm, out=out)
    else:
      call = lambda: e.observe_states(bank, kind, out=out)
    for _ in range(warmup):
      call()
    def work():
      for _ in range(reps):
        call()
    gpu, host = base._timed(torch, work)
    res[name] = {"us_per_call": gpu / reps, "host_us_per_call": host / reps, "bytes": out.numel() * out.element_size()}
    del out
  e.sync()
  res["fault"] = bool(e.fault_words()[:10].any())
  e.close()
  return res


def child_states(level, mode, calls, warmup):
  import torch
  from meltingpot_amd import engine as E
  n, skew = base.LEVELS[level]
  n = 4096
  e = E.Engine(E.load_pack(level), n, device=0)
  e.use_current_stream()
  e.reset()
  acts = base._actions(e, torch, K, skew)
  kw = dict(keep=FOUR)
  if mode in ("layer", "both"):
    kw["observations"] = (E.OBS_LAYER,)
  if mode in ("states", "both"):
    kw["states"] = True
  out = e.step_many(acts, **kw)
  kw.pop("states", None)   # (out= carries the tensor from here on)
  for _ in range(warmup):
    e.step_many(acts, out=out, **kw)
  def work():
    for _ in range(calls):
      e.step_many(acts, out=out, **kw)
  gpu, host = base._timed(torch, work)
  row_bytes = sum(v[0].numel() * v.element_size() for v in out.values())
  res = {"us_per_step": gpu / (calls * K), "host_us_per_call": host / calls, "row_bytes_per_step": row_bytes}
  e.sync()
  res["fault"] = bool(e.fault_words()[:10].any())
  e.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parent-lib", default="")
  ap.add_argument("--variant-lib", default="")
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--reps", type=int, default=30)
  ap.add_argument("--calls", type=int, default=6)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--only", default="", help="observe or states: half of the measurement")
  ap.add_argument("--out", default="")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    what, x, mode = a.child.split(":")
    if what == "observe":
      print(json.dumps(child_observe(mode, int(x), a.reps, a.warmup)))
    else:
      print(json.dumps(child_states(x, mode, a.calls, a.warmup)))
    return
  import torch
  me = os.path.abspath(__file__)
  configs = []
  if a.only in ("", "observe"):
    for R in (256, 4096):
      if a.parent_lib:
        configs.append((f"observe | R={R} | parent | observe", f"observe:{R}:observe", a.parent_lib))
      configs += [(f"observe | R={R} | branch | {m}", f"observe:{R}:{m}", None)
                  for m in ("rows=None", "rows") + (("small",) if R == 4096 else ())]
  if a.only in ("", "states"):
    for level in ("clean_up", "territory__rooms"):
      if a.parent_lib:
        configs += [(f"states | {level} | parent | {m}", f"states:{level}:{m}", a.parent_lib) for m in ("none", "layer")]
      configs += [(f"states | {level} | branch | {m}", f"states:{level}:{m}", None)
                  for m in ("none", "layer", "states", "both")]
      if a.variant_lib:
        configs += [(f"states | {level} | variant | {m}", f"states:{level}:{m}", a.variant_lib)
                    for m in ("layer", "states", "both")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
         "reps": a.reps, "calls": a.calls, "K": K, "results": {}}
  for r in range(a.rounds):
    order = configs if r % 2 == 0 else configs[::-1]
    for label, spec, lib in order:
      env = dict(os.environ)
      if lib:
        env["MP_ENGINE_LIB"] = lib
      out = subprocess.run([sys.executable, me, "--child", spec, "--reps", str(a.reps), "--calls", str(a.calls),
                            "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
      if out.returncode != 0:   # (nothing more runs on the GPU after a child that failed)
        raise RuntimeError(f"child {spec} (lib {lib}) exited {out.returncode}: {out.stderr[-2000:]}")
      got = json.loads(out.stdout.strip().splitlines()[-1])
      res["results"].setdefault(label, []).append(got)
      print(r, label, got, flush=True)
      if got["fault"]:
        raise RuntimeError(f"child {spec} reported fault words")
  summary = {}
  for label, rounds in res["results"].items():
    if label.startswith("observe"):
      for name in KINDS:
        v = [g[name]["us_per_call"] for g in rounds]
        summary[f"{label} | {name}"] = {"median_us_per_call": float(np.median(v)), "min": float(min(v)),
                                        "max": float(max(v)), "MB": rounds[0][name]["bytes"] / 1e6}
    else:
      v = [g["us_per_step"] for g in rounds]
      summary[label] = {"median_us_per_step": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                        "row_MB_per_step": rounds[0]["row_bytes_per_step"] / 1e6}
  res["summary"] = summary
  for k, v in summary.items():
    print(f"{k:60s} " + "  ".join(f"{n} {x:.2f}" for n, x in v.items()))
  line = json.dumps(res)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")
  else:
    print(line)


if __name__ == "__main__":
  main()
