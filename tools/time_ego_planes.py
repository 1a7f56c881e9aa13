"""Times the class and facing planes (MpEgoPlanes) on one box: the draw forms against the EGO_LAYER
draw and against the torch route that gives the same bytes (draw EGO_LAYER, gather through the
class table, one_hot, any over the layers, permute, plus the facing scatter), and what the
registration adds to a step; the method of tools/time_view_hash.py (child processes under a time
limit, a warm-up, events on the engine's stream around calls that only enqueue, configurations
alternated round by round, medians and ranges).

  python tools/time_ego_planes.py [--rounds 4] [--out FILE.json]

Levels clean_up (P = 7) and commons_harvest__open (P = 16), 4096 worlds, 16 classes (id mod 16)
with facing: C' = 20 planes.
  (a) step   us per `step` of three engines in one process, alternated: `plain` (nothing
             registered), `planes` (bind_ego_planes: the step's launch and the planes launch behind
             it) and `ego` (bind_ego_layer) — with no view bound and with WORLD.RGB bound.
  (b) draw   us per call at R = 256, 4096 and 32768 rows sampled, with repeats, from a bank of 4096
             worlds that have played 40 steps, alternated:
               planes_rows   observe_ego_planes(classes, bank, rows, facing=True): every viewer,
                             uint8 [R, P, 20, VH, VW];
               ego_rows      observe_ego_layer(bank, rows): int32 [R, P, VH, VW, L];
               torch_rows    ego_rows followed by the torch ops that turn it into the same bytes
                             (R <= 4096: its one-hot intermediate is C times the view);
               planes_views, ego_views: one player of each row;
             and at R = 4096 also planes_all / ego_all / torch_all: every viewer of the bank's 4096
             rows in order.  The torch route's result is compared with the kernel's before anything
             is timed.
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
  return (torch.arange(e.num_layer_ids, dtype=torch.int32) % CLASSES).to(e.device)


def child_step(level, view, rounds, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  engines = {n: E.Engine(E.load_pack(level), WORLDS, device=0) for n in ("plain", "planes", "ego")}
  calls = {}
  for n, e in engines.items():
    e.use_current_stream()
    if view == "world":
      e.bind(E.OBS_WORLD_RGB)
    if n == "planes":
      e.bind_ego_planes(torch.zeros(e.ego_planes_shape(CLASSES, True), dtype=torch.uint8, device=e.device),
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
         "planes_bytes": int(np.prod(engines["planes"].ego_planes_shape(CLASSES, True))),
         "leaf_bytes": int(np.prod(engines["ego"].ego_layer_shape)) * 4}
  res["fault"] = False
  for e in engines.values():
    e.sync()
    res["fault"] = res["fault"] or bool(e.fault_words()[:10].any())
    e.close()
  return res


def _torch_route(torch, e, bank, classes):
  """uint8 [R, P, C + 4, VH, VW] of rows of `bank` with torch ops on the drawn EGO_LAYER, and the
  facing planes from the rows' positions and orientations."""
  from meltingpot_amd import pack as pack_lib, substrate
  layout = substrate.SubstrateStateLayout(e.state_layout(), pack_lib.loads(e.pack_bytes))
  P = e.P
  _, _, VH, VW, _ = e.ego_layer_shape
  hdr = pack_lib.loads(e.pack_bytes)["hdr"]
  from meltingpot_amd import lower
  vl, vf = int(hdr[lower.HDR_VL]), int(hdr[lower.HDR_VF])
  H, W, torus = int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W]), int(hdr[lower.HDR_TOPOLOGY]) == 1
  dev = e.device
  dx = (torch.arange(VW, device=dev) - vl)[None, :].expand(VH, VW)
  dy = (torch.arange(VH, device=dev) - vf)[:, None].expand(VH, VW)
  turned_x, turned_y = torch.stack([dx, -dy, -dx, dy]), torch.stack([dy, dx, -dy, -dx])
  table = classes.long()

  def route(rows, ego):
    cls = table[ego.long()]                                              # [R, P, VH, VW, L]
    hot = torch.nn.functional.one_hot(cls, CLASSES).any(-2)              # [R, P, VH, VW, C]
    out = torch.empty(ego.shape[:2] + (CLASSES + 4, VH, VW), dtype=torch.uint8, device=dev)
    out[:, :, :CLASSES] = hot.permute(0, 1, 4, 2, 3)
    f = substrate.StateFields(bank[rows.long()], layout)
    ax, ay = f.avatar_x[:, :P].long(), f.avatar_y[:, :P].long()
    vo, live = f.orientation[:, :P].long(), f.alive[:, :P] != 0
    x = ax[:, :, None, None] + turned_x[vo]
    y = ay[:, :, None, None] + turned_y[vo]
    if torus:
      x, y = x % W, y % H
      inside = live[:, :, None, None].expand_as(x)
    else:
      inside = (x >= 0) & (x < W) & (y >= 0) & (y < H) & live[:, :, None, None]
    face = torch.zeros(ego.shape[:2] + (4, VH, VW), dtype=torch.bool, device=dev)
    for q in range(P):
      here = inside & live[:, q, None, None, None] & (x == ax[:, q, None, None, None]) & (y == ay[:, q, None, None, None])
      d = (vo[:, q, None] - vo) & 3
      face |= here[:, :, None] & (d[:, :, None] == torch.arange(4, device=dev))[:, :, :, None, None]
    out[:, :, CLASSES:] = face
    return out
  return route


def child_draw(level, R, rounds, reps, warmup):
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
  e = E.Engine(E.load_pack(level), 256, device=0)
  e.use_current_stream()
  gen = torch.Generator().manual_seed(3)
  rows = torch.randint(0, WORLDS, (R,), generator=gen).to(torch.int32).to(e.device)
  players = torch.randint(0, e.P, (R,), generator=gen).to(torch.int32).to(e.device)
  every = torch.arange(WORLDS, dtype=torch.int32, device=e.device)
  classes = _table(torch, e)
  shape, pshape = e.ego_layer_shape, e.ego_planes_shape(CLASSES, True)
  ego_rows = torch.empty((R,) + shape[1:], dtype=torch.int32, device=e.device)
  ego_views = torch.empty((R,) + shape[2:], dtype=torch.int32, device=e.device)
  p_rows = torch.empty((R,) + pshape[1:], dtype=torch.uint8, device=e.device)
  p_views = torch.empty((R,) + pshape[2:], dtype=torch.uint8, device=e.device)
  kw = dict(facing=True, num_classes=CLASSES)
  route = _torch_route(torch, e, bank, classes)
  check = min(R, 512)   # the torch route gives the kernel's bytes
  assert torch.equal(route(rows[:check], e.observe_ego_layer(bank, rows=rows[:check])),
                     e.observe_ego_planes(classes, bank, rows=rows[:check], **kw))
  calls = {"planes_rows": lambda: e.observe_ego_planes(classes, bank, rows=rows, out=p_rows, **kw),
           "ego_rows": lambda: e.observe_ego_layer(bank, rows=rows, out=ego_rows),
           "planes_views": lambda: e.observe_ego_planes(classes, bank, rows=rows, players=players, out=p_views, **kw),
           "ego_views": lambda: e.observe_ego_layer(bank, rows=rows, players=players, out=ego_views)}
  if R <= TORCH_ROWS_MAX:
    calls["torch_rows"] = lambda: route(rows, e.observe_ego_layer(bank, rows=rows, out=ego_rows))
  if R == WORLDS:
    calls["planes_all"] = lambda: e.observe_ego_planes(classes, bank, out=p_rows, **kw)
    calls["ego_all"] = lambda: e.observe_ego_layer(bank, out=ego_rows)
    calls["torch_all"] = lambda: route(every, e.observe_ego_layer(bank, out=ego_rows))
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "P": e.P,
         "ego_rows_bytes": ego_rows.numel() * 4, "planes_rows_bytes": p_rows.numel(),
         "ego_views_bytes": ego_views.numel() * 4, "planes_views_bytes": p_views.numel()}
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
  ap.add_argument("--child", default="")
  a = ap.parse_args()
  if a.child:
    what, level, arg = a.child.split(":")
    if what == "step":
      print(json.dumps(child_step(level, arg, a.rounds, a.reps, a.warmup)))
    else:
      print(json.dumps(child_draw(level, int(arg), a.rounds, a.reps, a.warmup)))
    return
  if a.rounds < 2:
    raise SystemExit("--rounds must be at least 2: the configurations are alternated")
  import torch
  me = os.path.abspath(__file__)
  levels = a.levels.split(",")
  specs = [f"step:{level}:{view}" for level in levels for view in ("none", "world")]
  specs += [f"draw:{level}:{R}" for level in levels for R in a.counts.split(",")]
  res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
         "reps": a.reps, "worlds": WORLDS, "classes": CLASSES, "results": {}, "summary": {}}
  for spec in specs:
    out = subprocess.run([sys.executable, me, "--child", spec, "--rounds", str(a.rounds), "--reps", str(a.reps),
                          "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=CHILD_SECONDS)
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
