"""Times EGO_LAYER on one box: what the registered leaf adds to a step, and the draw forms against
what a caller can write without them; the method of tools/time_observe_views.py (child processes
under a time limit, a warm-up, events on the engine's stream around calls that only enqueue,
configurations alternated round by round, medians and ranges).

  python tools/time_ego_layer.py [--rounds 4] [--out FILE.json]

Levels clean_up (P = 7) and commons_harvest__open (P = 16), 4096 worlds.
  (a) step   us per `step` of three engines in one process, alternated: `plain` (nothing
             registered), `ego` (bind_ego_layer: the step's launch and the EGO_LAYER launch behind
             it) and `layer` (N.LAYER bound: written inside the stepping launch) — with no view
             bound and with WORLD.RGB bound.
  (b) draw   us per call at R = 256, 4096 and 32768 rows sampled, with repeats, from a bank of 4096
             worlds that have played 40 steps, alternated:
               ego_rows     observe_ego_layer(bank, rows): every viewer, [R, P, VH, VW, L];
               layer_rows   observe_states(bank, OBS_LAYER, rows): N.LAYER, the same bytes;
               gather_rows  the torch gather over the rows' planes with precomputed turned
                            offsets and a hand-built copy of the value table;
               ego_views, layer_views (observe_views), gather_views: one player of each row,
                            [R, VH, VW, L].
             The gather's result is compared with the kernel's before anything is timed.
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

LEVELS = ("clean_up", "commons_harvest__open")
COUNTS = (256, 4096, 32768)
WORLDS = 4096
CHILD_SECONDS = 240


def _rounds(torch, calls, rounds, reps, warmup):
  """{name: [us per call, one per round]} of `calls` (name -> a function that only enqueues),
  alternated: every round times each of them, in reverse order on odd rounds."""
  for fn in calls.values():
    for _ in range(warmup):
      fn()
  out = {n: [] for n in calls}
  for r in range(rounds):
    names = list(calls) if r % 2 == 0 else list(calls)[::-1]
    for n in names:
      def work(fn=calls[n]):
        for _ in range(reps):
          fn()
      gpu, _ = base._timed(torch, work)
      out[n].append(gpu / reps)
  return out


def child_step(level, view, rounds, reps, warmup):
  import torch
  from meltingpot_amd import engine as E
  engines = {n: E.Engine(E.load_pack(level), WORLDS, device=0) for n in ("plain", "ego", "layer")}
  calls = {}
  for n, e in engines.items():
    e.use_current_stream()
    if view == "world":
      e.bind(E.OBS_WORLD_RGB)
    if n == "ego":
      e.bind_ego_layer(torch.zeros(e.ego_layer_shape, dtype=torch.int32, device=e.device))
    if n == "layer":
      e.bind(E.OBS_LAYER)
    e.reset()
    acts = base._actions(e, torch, 64, 0.0)
    state = {"k": 0}
    def step(e=e, acts=acts, state=state):
      e.step(acts[state["k"] % 64])
      state["k"] += 1
    calls[n] = step
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "fused": bool(engines["plain"].fused),
         "leaf_bytes": int(np.prod(engines["ego"].ego_layer_shape)) * 4}
  res["fault"] = False
  for e in engines.values():
    e.sync()
    res["fault"] = res["fault"] or bool(e.fault_words()[:10].any())
    e.close()
  return res


def _gather(torch, e, bank):
  """The EGO_LAYER a caller can write today: (all viewers of rows, one viewer of each row) as
  functions of a long tensor of rows (and of players), over views of `bank`."""
  from meltingpot_amd import lower, pack as pack_lib
  t = pack_lib.loads(e.pack_bytes)
  hdr = t["hdr"]
  lay = e.state_layout()
  H, W, L, P = lay.H, lay.W, lay.L, lay.P
  vl, vr, vf, vb = (int(hdr[i]) for i in (lower.HDR_VL, lower.HDR_VR, lower.HDR_VF, lower.HDR_VB))
  torus = int(hdr[lower.HDR_TOPOLOGY]) == 1
  dev = e.device
  nsprites = int(hdr[lower.HDR_NSPRITES])
  ssprite = np.asarray(t["state_sprite"]).reshape(-1)
  vmap = np.asarray(t["view_sprite_map"]).reshape(-1, nsprites)
  lut = np.zeros((P, 257), np.int32)
  for p in range(P):
    for s in range(1, min(lay.nstates, 256)):
      lut[p, s] = 1 + vmap[p, ssprite[s]] if ssprite[s] >= 0 else 0
    lut[p, 256] = 1 + vmap[p, 0]
  lut = torch.from_numpy(lut).to(dev)
  dx = (torch.arange(vl + vr + 1) - vl)[None, :].expand(vf + vb + 1, -1)
  dy = (torch.arange(vf + vb + 1) - vf)[:, None].expand(-1, vl + vr + 1)
  TX = torch.stack([dx, -dy, -dx, dy]).to(dev)   # [4, VH, VW]
  TY = torch.stack([dy, dx, -dy, -dx]).to(dev)
  grid = bank[:, :L * H * W].view(-1, L, H * W)
  tail = lambda name: bank[:, lay.grid_pad + lay.fields[name][0]:][:, :P]
  ax, ay, aori, alive = tail("ax"), tail("ay"), tail("aori"), tail("aalive")
  viewers = torch.arange(P, device=dev)

  def views(rows, players):   # players: long [R, Q] — the viewers of each row
    R, Q = players.shape
    at = rows[:, None]
    ori = aori[at, players].long()
    x = ax[at, players].long()[:, :, None, None] + TX[ori]
    y = ay[at, players].long()[:, :, None, None] + TY[ori]
    inside = (alive[at, players] != 0)[:, :, None, None]
    if torus:
      x, y = x % W, y % H
    else:
      inside = inside & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    cell = (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)).reshape(R, 1, -1).expand(R, L, -1)
    s = torch.gather(grid[rows], 2, cell).permute(0, 2, 1).reshape(R, Q, vf + vb + 1, vl + vr + 1, L).long()
    s = torch.where(inside[..., None].expand_as(s), s, torch.full_like(s, 256))
    return lut[players[:, :, None, None, None], s]

  all_rows = lambda rows: views(rows, viewers[None, :].expand(rows.shape[0], -1))
  sampled = lambda rows, players: views(rows, players[:, None])[:, 0]
  return all_rows, sampled


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
  rows_l, players_l = rows.long(), players.long()
  shape = e.ego_layer_shape
  out_rows = torch.empty((R,) + shape[1:], dtype=torch.int32, device=e.device)
  out_views = torch.empty((R,) + shape[2:], dtype=torch.int32, device=e.device)
  lay_rows, lay_views = torch.empty_like(out_rows), torch.empty_like(out_views)
  all_rows, sampled = _gather(torch, e, bank)
  check = min(R, 512)   # the gather is the function the kernels compute
  assert torch.equal(all_rows(rows_l[:check]), e.observe_ego_layer(bank, rows=rows[:check]))
  assert torch.equal(sampled(rows_l[:check], players_l[:check]),
                     e.observe_ego_layer(bank, rows=rows[:check], players=players[:check]))
  calls = {"ego_rows": lambda: e.observe_ego_layer(bank, rows=rows, out=out_rows),
           "layer_rows": lambda: e.observe_states(bank, E.OBS_LAYER, rows=rows, out=lay_rows),
           "gather_rows": lambda: all_rows(rows_l),
           "ego_views": lambda: e.observe_ego_layer(bank, rows=rows, players=players, out=out_views),
           "layer_views": lambda: e.observe_views(bank, E.OBS_LAYER, players, rows, out=lay_views),
           "gather_views": lambda: sampled(rows_l, players_l)}
  res = {"us": _rounds(torch, calls, rounds, reps, warmup), "P": e.P,
         "rows_bytes": out_rows.numel() * 4, "views_bytes": out_views.numel() * 4}
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
