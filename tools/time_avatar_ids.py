"""Times AVATAR_IDS_IN_VIEW and AVATAR_IDS_IN_RANGE_TO_ZAP (MpAvatarIds) on one box: the draw forms
against the EGO_LAYER draw of the same rows (the unit it shares staging with) and against the torch
route that gives the same values (window arithmetic over positions and orientations for the view, a
gather over the grid for the rays), and what the registration adds to a step; the method of
tools/time_ego_planes.py (child processes under a time limit, a warm-up, events on the engine's
stream around calls that only enqueue, configurations alternated round by round, medians and
ranges).

  python tools/time_avatar_ids.py [--rounds 4] [--out FILE.json]

Levels clean_up (P = 7) and commons_harvest__open (P = 16), 4096 worlds.
  (a) step   us per `step` of three engines in one process, alternated: `plain` (nothing
             registered), `ids` (bind_avatar_ids: the step's launch and the unit's launch behind it)
             and `ego` (bind_ego_layer) — with no view bound and with WORLD.RGB bound.
  (b) draw   us per call at R = 4096 and 32768 rows sampled, with repeats, from a bank of 4096
             worlds that have played 40 steps, alternated:
               ids_views / ego_views   one player of each row: observe_avatar_ids(bank, rows,
                                       players), int32 [R, P] twice / observe_ego_layer(...);
               ids_rows / ego_rows     every viewer of each row;
             and at R = 4096 also ids_all / ego_all / torch_all: every viewer of the bank's 4096
             rows in order, the torch route's result compared with the kernel's before anything is
             timed.
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
COUNTS = (4096, 32768)
WORLDS = 4096
CHILD_SECONDS = 240


def child_step(level, view, rounds, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  engines = {n: E.Engine(E.load_pack(level), WORLDS, device=0) for n in ("plain", "ids", "ego")}
  calls = {}
  for n, e in engines.items():
    e.use_current_stream()
    if view == "world":
      e.bind(E.OBS_WORLD_RGB)
    if n == "ids":
      e.bind_avatar_ids(torch.zeros(e.avatar_ids_shape, dtype=torch.int32, device=e.device),
                        torch.zeros(e.avatar_ids_shape, dtype=torch.int32, device=e.device))
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
         "ids_bytes": 2 * int(np.prod(engines["ids"].avatar_ids_shape)) * 4,
         "leaf_bytes": int(np.prod(engines["ego"].ego_layer_shape)) * 4}
  res["fault"] = False
  for e in engines.values():
    e.sync()
    res["fault"] = res["fault"] or bool(e.fault_words()[:10].any())
    e.close()
  return res


def _torch_route(torch, e, bank):
  """(in_view, in_range) int32 [R, P, P] of the rows of `bank` with torch ops: the window test on
  q's offset from p turned into p's frame, and the rays as a gather over the avatars' plane."""
  from meltingpot_amd import lower, pack as pack_lib, substrate
  tables = pack_lib.loads(e.pack_bytes)
  layout = substrate.SubstrateStateLayout(e.state_layout(), tables)
  hdr = tables["hdr"]
  P, dev = e.P, e.device
  vl, vr, vf, vb = (int(hdr[i]) for i in (lower.HDR_VL, lower.HDR_VR, lower.HDR_VF, lower.HDR_VB))
  H, W, al = int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W]), int(hdr[lower.HDR_AVATAR_LAYER])
  assert int(hdr[lower.HDR_TOPOLOGY]) != 1   # (the two levels timed here are bounded maps)
  length, radius = (int(v) for v in np.asarray(tables["zapper_i32"]).reshape(-1)[1:3])
  cells, preds = [], []   # the footprint, as tests/avatar_ids_model.py writes it
  ray = []
  for f in range(1, length + 1):
    cells.append((0, f)); preds.append(list(ray)); ray.append(len(cells) - 1)
  for side in (-1, 1):
    sideways = []
    for i in range(1, radius + 1):
      cells.append((side * i, 0)); preds.append(list(sideways)); sideways.append(len(cells) - 1)
      ray = list(sideways)
      for f in range(1, length - i + 1):
        cells.append((side * i, f)); preds.append(list(ray)); ray.append(len(cells) - 1)
  nc = len(cells)
  lat = torch.tensor([c[0] for c in cells], device=dev)
  fw = torch.tensor([c[1] for c in cells], device=dev)
  pred = torch.zeros((nc, nc), dtype=torch.bool, device=dev)
  for j, ks in enumerate(preds):
    pred[j, ks] = True
  owner = torch.zeros(256, dtype=torch.long, device=dev)   # state -> player + 1
  for p, s in enumerate(np.asarray(tables["avatar_alive_state"]).reshape(-1)[:P]):
    owner[int(s)] = p + 1
  DX = torch.tensor([0, 1, 0, -1], device=dev)
  DY = torch.tensor([-1, 0, 1, 0], device=dev)

  def route(rows):
    f = substrate.StateFields(bank[rows.long()], layout)
    ax, ay = f.avatar_x[:, :P].long(), f.avatar_y[:, :P].long()
    vo, live = f.orientation[:, :P].long(), f.alive[:, :P] != 0
    # IN_VIEW: q's offset in the map's frame, turned into p's frame
    ox, oy = ax[:, None, :] - ax[:, :, None], ay[:, None, :] - ay[:, :, None]   # [R, p, q]
    o = vo[:, :, None]
    dx = torch.where(o == 0, ox, torch.where(o == 1, oy, torch.where(o == 2, -ox, -oy)))
    dy = torch.where(o == 0, oy, torch.where(o == 1, -ox, torch.where(o == 2, -oy, ox)))
    view = (dx >= -vl) & (dx <= vr) & (dy >= -vf) & (dy <= vb) & live[:, :, None] & live[:, None, :]
    # IN_RANGE: the footprint's cells, what stops, what is reached, whose avatar stands there
    right = (vo + 1) & 3
    x = ax[:, :, None] + lat * DX[right][:, :, None] + fw * DX[vo][:, :, None]   # [R, P, nc]
    y = ay[:, :, None] + lat * DY[right][:, :, None] + fw * DY[vo][:, :, None]
    on = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    plane = f.grid[:, al].reshape(len(rows), H * W).long()
    cell = torch.where(on, y * W + x, torch.zeros_like(x))
    state = torch.gather(plane, 1, cell.reshape(len(rows), P * nc)).reshape(len(rows), P, nc)
    stops = ~on | (state != 0)
    blocked = (stops[:, :, None, :] & pred).any(-1)                              # [R, P, nc]
    who = torch.where(on & ~blocked & live[:, :, None], owner[state], torch.zeros_like(state))
    zap = torch.zeros((len(rows), P, P + 1), dtype=torch.int32, device=dev)
    zap.scatter_(2, who, torch.ones_like(who, dtype=torch.int32))
    return view.to(torch.int32), zap[:, :, 1:].contiguous()
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
  P, shape = e.P, e.ego_layer_shape
  new = lambda *s: torch.empty(s, dtype=torch.int32, device=e.device)
  ego_rows, ego_views = new(R, *shape[1:]), new(R, *shape[2:])
  ids_rows, ids_views = (new(R, P, P), new(R, P, P)), (new(R, P), new(R, P))
  route = _torch_route(torch, e, bank)
  check = rows[:512]   # the torch route gives the kernel's values
  got, want = route(check), e.observe_avatar_ids(bank, rows=check)
  assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
  calls = {"ids_rows": lambda: e.observe_avatar_ids(bank, rows=rows, out=ids_rows),
           "ego_rows": lambda: e.observe_ego_layer(bank, rows=rows, out=ego_rows),
           "ids_views": lambda: e.observe_avatar_ids(bank, rows=rows, players=players, out=ids_views),
           "ego_views": lambda: e.observe_ego_layer(bank, rows=rows, players=players, out=ego_views)}
  if R == WORLDS:
    calls["ids_all"] = lambda: e.observe_avatar_ids(bank, out=ids_rows)
    calls["view_all"] = lambda: e.observe_avatar_ids(bank, zap=False, out=(ids_rows[0], None))
    calls["ego_all"] = lambda: e.observe_ego_layer(bank, out=ego_rows)
    calls["torch_all"] = lambda: route(every)
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "P": P,
         "ego_rows_bytes": ego_rows.numel() * 4, "ids_rows_bytes": 2 * ids_rows[0].numel() * 4,
         "ego_views_bytes": ego_views.numel() * 4, "ids_views_bytes": 2 * ids_views[0].numel() * 4}
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
         "reps": a.reps, "worlds": WORLDS, "results": {}, "summary": {}}
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
