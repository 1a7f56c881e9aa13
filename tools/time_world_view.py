"""Times WORLD.LAYER and the world planes (the world ops of MpEgoLayer and MpEgoPlanes) on one box:
the draws against the torch routes that give the same bytes, k_world_layer_rows against the
EGO_LAYER draw in bytes per microsecond, and what the registrations add to a step; the method of
tools/time_ego_planes.py (child processes under a time limit, a warm-up, events on the engine's
stream around calls that only enqueue, configurations alternated round by round, medians and
ranges).

  python tools/time_world_view.py [--rounds 4] [--out FILE.json]

Levels clean_up and commons_harvest__open, 4096 worlds, 16 classes (id mod 16) with facing: C' = 20
planes.
  (a) step   us per `step` of four engines in one process, alternated: `plain` (nothing
             registered), `layer` (bind_world_layer), `planes` (bind_world_planes) and `ego`
             (bind_ego_layer, the yardstick) — with no view bound and with WORLD.RGB bound.
  (b) draw   us per call at R = 256, 4096 and 32768 rows sampled, with repeats, from a bank of 4096
             worlds that have played 40 steps, alternated:
               layer_rows    observe_world_layer(bank, rows): int32 [R, H, W, L];
               torch_layer   Wt[state_fields(bank[rows]).grid[:, :L]].permute(0, 2, 3, 1);
               planes_rows   observe_world_planes(classes, bank, rows, facing=True): uint8 [R, 20, H, W];
               torch_planes  torch_layer, the class table, one_hot, any over the layers, permute,
                             and the facing scatter (R <= 4096: its one-hot intermediate is C
                             times the map);
               ego_rows      observe_ego_layer(bank, rows): int32 [R, P, VH, VW, L], for the rate.
             The torch routes' results are compared with the kernels' before anything is timed.
             `--draw-worlds N`: the worlds of the engine the draws go to (256; the launch plan
             follows R, not N); `--no-torch`: the torch routes are checked but not timed, so that
             nothing runs between the kernels' rounds.
Every child runs under a time limit; the first that does not end normally, or that reports fault
words, ends the run."""
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
from time_ego_layer import _rounds  # noqa: E402

LEVELS = ("clean_up", "commons_harvest__open")
COUNTS = (256, 4096, 32768)
WORLDS = 4096
CLASSES = 16
CHILD_SECONDS = 240
TORCH_ROWS_MAX = 4096


def _table(torch, e):
  return (torch.arange(e.num_world_layer_ids, dtype=torch.int32) % CLASSES).to(e.device)


def child_step(level, view, rounds, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  engines = {n: E.Engine(E.load_pack(level), WORLDS, device=0) for n in ("plain", "layer", "planes", "ego")}
  calls = {}
  for n, e in engines.items():
    e.use_current_stream()
    if view == "world":
      e.bind(E.OBS_WORLD_RGB)
    if n == "layer":
      e.bind_world_layer(torch.zeros(e.world_layer_shape, dtype=torch.int32, device=e.device))
    if n == "planes":
      e.bind_world_planes(torch.zeros(e.world_planes_shape(CLASSES, True), dtype=torch.uint8, device=e.device),
                          _table(torch, e), facing=True, num_classes=CLASSES)
    if n == "ego":
      e.bind_ego_layer(torch.zeros(e.ego_layer_shape, dtype=torch.int32, device=e.device))
    e.reset()
    acts = base._actions(e, torch, 64, 0.0)
    state = {"k": 0}
    def step(e=e, acts=acts, state=state):
      e.step(acts[state["k"] % 64])
      state["k"] += 1
    calls[n] = step
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "fused": bool(engines["plain"].fused),
         "layer_bytes": int(np.prod(engines["layer"].world_layer_shape)) * 4,
         "planes_bytes": int(np.prod(engines["planes"].world_planes_shape(CLASSES, True))),
         "ego_bytes": int(np.prod(engines["ego"].ego_layer_shape)) * 4}
  res["fault"] = False
  for e in engines.values():
    e.sync()
    res["fault"] = res["fault"] or bool(e.fault_words()[:10].any())
    e.close()
  return res


def _torch_routes(torch, e, bank, classes):
  """(layer(rows), planes(rows)): WORLD.LAYER and the planes of rows of `bank` with torch ops on
  the rows' fields, through the value table rebuilt from the pack."""
  from meltingpot_amd import lower, pack as pack_lib, substrate
  t = pack_lib.loads(e.pack_bytes)
  layout = substrate.SubstrateStateLayout(e.state_layout(), t)
  hdr = t["hdr"]
  P, L = e.P, int(hdr[lower.HDR_L])
  H, W = int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W])
  nstates, nsprites = int(hdr[lower.HDR_NSTATES]), int(hdr[lower.HDR_NSPRITES])
  ssprite = np.asarray(t["state_sprite"]).reshape(-1)
  world = np.asarray(t["view_sprite_map"]).reshape(-1, nsprites)[P]
  wt = np.zeros(256, np.int32)
  for s in range(1, min(nstates, 256)):
    wt[s] = 1 + world[ssprite[s]] if ssprite[s] >= 0 else 0
  dev = e.device
  wt = torch.from_numpy(wt).to(dev)
  table = classes.long()

  def layer(rows):
    f = substrate.StateFields(bank[rows.long()], layout)
    return wt[f.grid[:, :L].long()].permute(0, 2, 3, 1).contiguous()

  def planes(rows):
    f = substrate.StateFields(bank[rows.long()], layout)
    wl = wt[f.grid[:, :L].long()].permute(0, 2, 3, 1)                     # [R, H, W, L]
    hot = torch.nn.functional.one_hot(table[wl.long()], CLASSES).any(-2)  # [R, H, W, C]
    out = torch.zeros((wl.shape[0], CLASSES + 4, H, W), dtype=torch.uint8, device=dev)
    out[:, :CLASSES] = hot.permute(0, 3, 1, 2)
    ax, ay = f.avatar_x[:, :P].long(), f.avatar_y[:, :P].long()
    vo, live = f.orientation[:, :P].long(), f.alive[:, :P] != 0
    r = torch.arange(wl.shape[0], device=dev)[:, None].expand_as(ax)
    out[r[live], CLASSES + vo[live], ay[live], ax[live]] = 1
    return out
  return layer, planes


def child_draw(level, R, rounds, reps, warmup, draw_worlds=256, torch_routes=True):
  import torch
  from meltingpot_amd import engine as E
  src = E.Engine(E.load_pack(level), WORLDS, device=0)
  src.reset()
  acts = base._actions(src, torch, 40, 0.0)
  for s in range(40):
    src.step(acts[s])
  bank = src.save_worlds().clone()
  src.sync()
  src.close()
  e = E.Engine(E.load_pack(level), draw_worlds, device=0)
  e.use_current_stream()
  gen = torch.Generator().manual_seed(3)
  rows = torch.randint(0, WORLDS, (R,), generator=gen).to(torch.int32).to(e.device)
  classes = _table(torch, e)
  l_rows = torch.empty((R,) + e.world_layer_shape[1:], dtype=torch.int32, device=e.device)
  p_rows = torch.empty((R,) + e.world_planes_shape(CLASSES, True)[1:], dtype=torch.uint8, device=e.device)
  ego_rows = torch.empty((R,) + e.ego_layer_shape[1:], dtype=torch.int32, device=e.device)
  kw = dict(facing=True, num_classes=CLASSES)
  layer, planes = _torch_routes(torch, e, bank, classes)
  check = min(R, 512)   # the torch routes give the kernels' bytes
  assert torch.equal(layer(rows[:check]), e.observe_world_layer(bank, rows=rows[:check]))
  assert torch.equal(planes(rows[:check]), e.observe_world_planes(classes, bank, rows=rows[:check], **kw))
  calls = {"layer_rows": lambda: e.observe_world_layer(bank, rows=rows, out=l_rows),
           "planes_rows": lambda: e.observe_world_planes(classes, bank, rows=rows, out=p_rows, **kw),
           "ego_rows": lambda: e.observe_ego_layer(bank, rows=rows, out=ego_rows)}
  if torch_routes:
    calls["torch_layer"] = lambda: layer(rows)
  if torch_routes and R <= TORCH_ROWS_MAX:
    calls["torch_planes"] = lambda: planes(rows)
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "P": e.P,
         "layer_rows_bytes": l_rows.numel() * 4, "planes_rows_bytes": p_rows.numel(),
         "ego_rows_bytes": ego_rows.numel() * 4}
  e.sync()
  res["fault"] = bool(e.fault_words()[:10].any())
  e.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=4)
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--levels", default=",".join(LEVELS))
  ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
  ap.add_argument("--out", default="")
  ap.add_argument("--draw-worlds", type=int, default=256)
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    what, level, arg = a.child.split(":")
    if what == "step":
      print(json.dumps(child_step(level, arg, a.rounds, a.reps, a.warmup)))
    else:
      print(json.dumps(child_draw(level, int(arg), a.rounds, a.reps, a.warmup, a.draw_worlds, not a.no_torch)))
    return
  if a.rounds < 2:
    raise SystemExit("--rounds must be at least 2: the configurations are alternated")
  import torch
  me = os.path.abspath(__file__)
  levels = a.levels.split(",")
  specs = [] if a.no_torch else [f"step:{level}:{view}" for level in levels for view in ("none", "world")]
  specs += [f"draw:{level}:{R}" for level in levels for R in a.counts.split(",")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
         "reps": a.reps, "worlds": WORLDS, "classes": CLASSES, "draw_worlds": a.draw_worlds, "torch_routes": not a.no_torch, "results": {}, "summary": {}}
  for spec in specs:
    out = subprocess.run([sys.executable, me, "--child", spec, "--rounds", str(a.rounds), "--reps", str(a.reps),
                          "--warmup", str(a.warmup), "--draw-worlds", str(a.draw_worlds)] +
                         (["--no-torch"] if a.no_torch else []), capture_output=True, text=True, timeout=CHILD_SECONDS)
    if out.returncode != 0:   # (nothing more runs on the GPU after a child that failed)
      raise RuntimeError(f"child {spec} exited {out.returncode}: {out.stderr[-2000:]}")
    got = json.loads(out.stdout.strip().splitlines()[-1])
    res["results"][spec] = got
    if got["fault"]:
      raise RuntimeError(f"child {spec} reported fault words")
    res["summary"][spec] = {n: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
                            for n, v in got["us"].items()}
    extra = {k: v for k, v in got.items() if k not in ("us", "fault")}
    print(f"{spec:40s} " + "  ".join(f"{n} {s['median']:.1f} ({s['min']:.1f}-{s['max']:.1f})"
                                      for n, s in res["summary"][spec].items()) + f"  {extra}", flush=True)
  line = json.dumps(res)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")
  else:
    print(line)


if __name__ == "__main__":
  main()
