"""Hand-built situations, stated once and applied to the oracle and to the engine (test
infrastructure): tests/test_gpu_situations.py runs them on the GPU against the oracle,
tests/test_situations_cpu.py shows on the CPU that they tell a wrong rule from the right one.

A scope is a batch of situations of one level, world w of the engine and oracle w seeded
`util.world_seed(w)`.  A situation is what happens to its world after `reset()` and the scope's
scripted prefix of actions (the same in every world):
  place(p, x, y, orient, alive)    `Scope.places[w, p]`   every avatar of the scope is placed, in
                                   index order; `Scope.first[w, p]`, where a scope has it, is a
                                   round of placements before that one (it clears the cells the
                                   reset put the avatars on)
  set_cell(layer, x, y, state)     `Scope.cells[w, c]`    layer -1: no edit in this slot
then `Scope.actions[s, w]` for 1 - 42 steps (one where a move is the matter, more where a timer
has to run out or a scene has a script), with further rounds of placements behind given steps
(`Scope.later`) for the scenes of the oracle's CPU tests that place their avatars again.  On the oracle the edits are `Oracle.place_avatar` and
`Oracle.set_cell_state`.  On the engine they are writes through the named fields of saved rows
(README, "Editing states"), vectorised over all rows (`apply_edits`): the avatar's byte on the
avatar layer's plane, avatar_x, avatar_y, orientation, alive, achange where the avatar's state
changes, the pieces a level connects to its avatars (territory's marking; the kitchens' inventory,
whose state id also shows the avatar's facing; the matrix games' readiness marker, which keeps its
own position in the tail), and a cell's byte.

Hidden variables.  NO hidden plane is edited by this bridge.  A `set_cell` is only used where the
cell's byte is all there is to it: an apple site of commons_harvest between `apple` and
`appleWait`, a token of gift_refinements between `tokenWait` and `token`, and an ore of coop_mining
between `oreWait` and a raw ore, whose countdown and miner set (the level's two hidden planes) are
zero in both states; the count of live sites, `aux_count`, is kept in step.  Whatever keeps a hidden variable next to a cell — territory's claimed_by and
health, clean_up's dirt count, a partly mined ore's countdown — is left to the scripted steps: a
scope's prefix from the reset and its own actions (a gold ore becomes partial because A mines it),
which are valid on both sides by construction.  No scope here builds a claimed resource or a dirty
river cell by an edit: `blocked_beam_scope` stands its shooters where the stock map has them.

The bridge is checked before it is trusted (`run_engine`): `check_states` all zero, the checked
load reports nothing, and the engine's dump equals the oracle's in every world BEFORE any step; a
mismatch there is a `ConstructionError` carrying the situation's description, not a parity failure.
"""
import functools
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

import geometry
import util

DX = (0, 1, 0, -1)   # orientation 0 N, 1 E, 2 S, 3 W
DY = (-1, 0, 1, 0)
ORIENT = "NESW"
MOVE_NAMES = ("NOOP", "FORWARD", "STEP_RIGHT", "BACKWARD", "STEP_LEFT")   # by the `move` field, 0 - 4
VIEW_STRIDE = 16     # views are compared in every 16th world; state, rewards and events in all

# state-name prefixes of the pieces a level connects to its avatars (grid:connect): they stand on
# their avatar's cell, on a plane of their own
CONNECTED = {"territory": ("avatar_marking.",), "collaborative_cooking": ("inventory.",)}


class ConstructionError(AssertionError):
  """The two sides disagree before any step, or an edit was refused: the situation is built
  wrongly (or the edit recipe is), nothing is known about the step kernels."""


class Scope:
  """A batch of situations (see the module's docstring).  `count`: what the generator says it
  built; `describe(w)`: the situation of world w in words; `tags`: arrays [n] of the
  generator's own (which kind of case a world is)."""

  def __init__(self, name, level, pack, players, places, actions, describe, count, cells=None,
               prefix=None, tags=None, first=None, later=None):
    self.name, self.level, self.pack, self.players = name, level, pack, int(players)
    self.places = np.ascontiguousarray(places, np.int32)
    self.n = len(self.places)
    self.actions = np.ascontiguousarray(actions, np.int32)
    self.cells = (np.full((self.n, 0, 4), -1, np.int32) if cells is None
                  else np.ascontiguousarray(cells, np.int32))
    self.prefix = (np.zeros((0, self.players), np.int32) if prefix is None
                   else np.ascontiguousarray(prefix, np.int32))
    self.describe, self.count, self.tags = describe, int(count), dict(tags or {})
    self.first = None if first is None else np.ascontiguousarray(first, np.int32)
    assert self.first is None or self.first.shape == self.places.shape
    # {s: placements [n, P, 4] made after step s of `actions` (x < 0: this avatar stays)}: the
    # scenes of the oracle's CPU tests that place avatars again in the course of their script
    # several rounds behind one step are applied in their order
    self.later = {int(k): [np.ascontiguousarray(r, np.int32) for r in (v if isinstance(v, list) and np.ndim(v[0]) == 3 else [v])]
                  for k, v in (later or {}).items()}
    assert all(0 < k < self.actions.shape[0] and r.shape == self.places.shape for k, v in self.later.items() for r in v)
    assert self.places.shape == (self.n, self.players, 4), self.places.shape
    assert self.actions.ndim == 3 and self.actions.shape[1:] == (self.n, self.players), self.actions.shape
    assert self.cells.shape[0] == self.n and self.cells.shape[2] == 4
    assert self.prefix.shape[1:] == (self.players,)

  @property
  def steps(self):
    return self.actions.shape[0]

  @property
  def rounds(self):
    """The rounds of placements, in order."""
    return ([] if self.first is None else [self.first]) + [self.places]


def action_ids(level):
  """{name: id in the config's ACTION_SET}: the five moves, TURN_LEFT, TURN_RIGHT and one entry
  per beam (its field's name, "fireZap")."""
  from meltingpot_amd import substrate
  aset = substrate.get_config(level).action_set
  out = {}
  for i, a in enumerate(aset):
    on = {k: v for k, v in a.items() if v}
    if not on:
      out["NOOP"] = i
    elif list(on) == ["move"]:
      out[MOVE_NAMES[on["move"]]] = i
    elif list(on) == ["turn"]:
      out["TURN_LEFT" if on["turn"] < 0 else "TURN_RIGHT"] = i
    elif len(on) == 1:
      out[next(iter(on))] = i
  return out


def move_action(ids, orient, direction):
  """The action with which an avatar facing `orient` moves one cell in the absolute `direction`."""
  return ids[("FORWARD", "STEP_RIGHT", "BACKWARD", "STEP_LEFT")[(direction - orient) % 4]]


# ---- the oracle's side ---------------------------------------------------------------------------
def _oracle_chunk(job):
  """Worker (its own process when the batch is large): per world reset, prefix, edits, steps.
  Returns per world (accepted, dumps [steps + 1], rewards, ready, aux, events per step, views)."""
  here = os.path.dirname(os.path.abspath(__file__))
  for d in (here, os.path.dirname(here)):
    if d not in sys.path:
      sys.path.insert(0, d)
  from oracle import oracle
  pack, players, prefix, first, rounds, cells, actions, options, stride, later = job
  out = []
  for i in range(len(cells)):
    w = first + i
    o = oracle.Oracle(pack, util.world_seed(w), players)
    for k, v in options:
      o.set_option(k, v)
    o.reset()
    for a in prefix:
      o.step(a)
    ok = True
    for places in rounds:
      for p in range(players):
        x, y, ori, alive = (int(v) for v in places[i, p])
        if x >= 0:
          ok = bool(o.place_avatar(p, x, y, ori, bool(alive))) and ok
    for layer, x, y, state in cells[i]:
      if layer >= 0:
        ok = bool(o.set_cell_state(int(layer), int(x), int(y), int(state))) and ok
    look = stride > 0 and w % stride == 0

    def views():
      return (o.render_world(), np.stack([o.render_agent(p) for p in range(players)]),
              np.stack([o.layer_view(p) for p in range(players)])) if look else None
    rec = {"ok": ok, "dump": [o.dump()], "views": [views()], "rewards": [], "ready": [], "aux": [],
           "events": [], "post": {}}
    for s in range(actions.shape[0]):
      o.step(actions[s, i])
      rec["dump"].append(o.dump())
      rec["views"].append(views())
      rec["rewards"].append(o.rewards())
      rec["ready"].append(o.ready_to_shoot())
      rec["aux"].append(o.num_others_cleaned())
      rec["events"].append(o.events())
      if s + 1 in later:
        for places in later[s + 1]:
          for p in range(players):
            x, y, ori, alive = (int(v) for v in places[i, p])
            if x >= 0:
              rec["ok"] = bool(o.place_avatar(p, x, y, ori, bool(alive))) and rec["ok"]
        rec["post"][s + 1] = o.dump()
    o.close()
    out.append(rec)
  return out


def run_oracle(scope, options=(), stride=VIEW_STRIDE, workers=None):
  """The scope on the oracle.  `options`: ((name, value), ...) of `Oracle.OPTIONS`, set before the
  reset.  Returns arrays over the worlds: accepted bool [n]; grid uint8 [steps + 1, n, L, H, W],
  avat, glob (index 0: after the edits, before any step); rewards, ready, aux f64 [steps, n, P];
  events [steps][n] sorted lists; views {w: [steps + 1] of (world rgb, agent rgb [P], layer [P])}."""
  n = scope.n
  workers = workers or max(1, min(len(os.sched_getaffinity(0)), 16, (n + 255) // 256))
  chunk = (n + workers - 1) // workers
  jobs = [(scope.pack, scope.players, scope.prefix, i, [r[i:i + chunk] for r in scope.rounds], scope.cells[i:i + chunk],
           np.ascontiguousarray(scope.actions[:, i:i + chunk]), tuple(options), stride,
           {k: [r[i:i + chunk] for r in v] for k, v in scope.later.items()})
          for i in range(0, n, chunk)]
  if len(jobs) == 1:
    recs = _oracle_chunk(jobs[0])
  else:
    recs = []
    with tempfile.TemporaryDirectory(prefix="mp_situations_") as tmp:
      procs = []
      for k, job in enumerate(jobs):
        path = os.path.join(tmp, f"job{k}.pkl")
        with open(path, "wb") as f:
          pickle.dump(job, f)
        procs.append((path, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--oracle", path])))
      try:
        for path, pr in procs:
          assert pr.wait(timeout=600) == 0, "oracle worker failed"
          with open(path + ".out", "rb") as f:
            recs += pickle.load(f)
      finally:
        for _, pr in procs:
          if pr.poll() is None:
            pr.kill()
  assert len(recs) == n
  S = scope.steps
  out = {"accepted": np.array([r["ok"] for r in recs])}
  for k, name in enumerate(("grid", "avat", "glob")):
    out[name] = np.stack([np.stack([r["dump"][s][k] for r in recs]) for s in range(S + 1)])
  for name in ("rewards", "ready", "aux"):
    out[name] = np.stack([np.stack([r[name][s] for r in recs]) for s in range(S)])
  out["events"] = [[r["events"][s] for r in recs] for s in range(S)]
  out["views"] = {w: r["views"] for w, r in enumerate(recs) if r["views"][0] is not None}
  # after a later round of placements: {s: (grid, avat, glob)} as they are behind the edit
  out["post"] = {k: tuple(np.stack([r["post"][k][j] for r in recs]) for j in range(3)) for k in scope.later}
  return out


@functools.lru_cache(maxsize=2)
def reference(builder, *args):
  """(scope, its stock oracle run), computed once and shared by the tests of one scope; treat
  both as read-only.  `builder(*args)` is a generator of test_gpu_situations / this module."""
  scope = builder(*args)
  return scope, run_oracle(scope)


# ---- the engine's side -----------------------------------------------------------------------------
def apply_edits(scope, bank, layout, rounds=None, cells=None):
  """The scope's edits (or the given rounds of placements and cell edits) written into `bank`
  (uint8 [n, S] rows, torch, on any device) through the named fields, all rows at once.  `layout`:
  a substrate.SubstrateStateLayout of the rows."""
  import torch
  from meltingpot_amd import substrate
  f = substrate.StateFields(bank, layout)
  dev = bank.device
  n = scope.n
  assert bank.shape[0] == n
  rows = torch.arange(n, device=dev)
  AL = layout.avatar_layer
  matrix = "_in_the_matrix" in scope.level
  prefixes = next((v for k, v in CONNECTED.items() if scope.level.startswith(k)), ())
  connected = torch.zeros(256, dtype=torch.bool, device=dev)
  for s, name in enumerate(layout.state_names):
    if name.startswith(prefixes) and prefixes:
      connected[s] = True
  if matrix:   # the readiness markers: every state of the marker's layer
    tables = util.pack_tables(scope.pack)
    for s in tables["mx_states"][1:8]:
      connected[int(s)] = True
  planes = [l for l in range(layout.L) if l != AL] if prefixes or matrix else []
  cook = None
  if scope.level.startswith("collaborative_cooking"):
    cook = tuple(int(v) for v in util.pack_tables(scope.pack)["cc_inv_states"][2:4])
  frame = f.frame.clone()
  for places, p in ((r, p) for r in (scope.rounds if rounds is None else rounds) for p in range(scope.players)):
    places = torch.from_numpy(places).to(dev).long()
    x, y, ori, alive = (places[:, p, k] for k in range(4))
    sel = x >= 0                      # (x < 0: this avatar is not placed in this round)
    now = alive != 0
    was = f.alive[:, p] != 0
    ox, oy = f.avatar_x[:, p].long(), f.avatar_y[:, p].long()
    state = torch.full((n,), layout.avatar_states[p][0], dtype=torch.uint8, device=dev)
    # the avatar's byte leaves its old cell of the avatar layer's plane ...
    out = was & sel
    f.grid[rows[out], AL, oy[out], ox[out]] = 0
    # ... and goes to the new one; the pieces connected to a living avatar come along
    moved = was & now & sel
    for l in planes:
      b = f.grid[rows, l, oy, ox]
      take = moved & connected[b.long()]
      if cook is not None:
        # an avatar's inventory shows its facing in the state id once it holds something
        # (`inventory.tomato_offset`, `.E`, `.S`, `.W`): it turns with the avatar
        off0, dir0 = cook
        bl = b.long()
        item = torch.where(bl >= dir0, (bl - dir0) & 3, bl - off0)
        held = ((bl >= off0) & (bl < off0 + 4)) | ((bl >= dir0) & (bl < dir0 + 12))
        facing = torch.where((ori & 3) == 0, off0 + item, dir0 + ((ori & 3) - 1) * 4 + item)
        b = torch.where(held, facing, bl).to(torch.uint8)
      f.grid[rows[take], l, oy[take], ox[take]] = 0
      f.grid[rows[take], l, y[take], x[take]] = b[take]
      if matrix:   # the marker keeps its own position in the tail (ctimer: x, nozap: y)
        f.ctimer[:, p] = torch.where(take, x, f.ctimer[:, p].long()).to(torch.uint8)
        f.nozap[:, p] = torch.where(take, y, f.nozap[:, p].long()).to(torch.uint8)
    on = now & sel
    f.grid[rows[on], AL, y[on], x[on]] = state[on]
    f.avatar_x[:, p] = torch.where(on, x, ox).to(torch.uint8)
    f.avatar_y[:, p] = torch.where(on, y, oy).to(torch.uint8)
    f.orientation[:, p] = torch.where(sel, ori & 3, f.orientation[:, p].long()).to(torch.uint8)
    f.alive[:, p] = torch.where(sel, now, was).to(torch.uint8)
    # a change of state (alive <-> waiting) is dated with the current frame
    f.achange[:, p] = torch.where(sel & (now != was), frame, f.achange[:, p])
  cells = torch.from_numpy(scope.cells if cells is None else cells).to(dev).long()
  for c in range(cells.shape[1]):
    layer, x, y, state = (cells[:, c, k] for k in range(4))
    on = layer >= 0
    _set_cells(scope, f, layout, rows[on], layer[on], x[on], y[on], state[on])
  return f


def _set_cells(scope, f, layout, rows, layer, x, y, state):
  import torch
  old = f.grid[rows, layer, y, x].long()
  f.grid[rows, layer, y, x] = state.to(torch.uint8)
  if scope.level.startswith("commons_harvest"):
    # LIVE_APPLES (aux_count) counts the sites in state `apple`
    apple = layout.state_id("apple.apple")
    delta = (state == apple).int() - (old == apple).int()
    f.aux_count.index_add_(0, rows, delta)
  if scope.level == "gift_refinements":
    # aux_count counts the live tokens
    live = layout.state_id("token.token")
    delta = (state == live).int() - (old == live).int()
    f.aux_count.index_add_(0, rows, delta)
  if scope.level == "coop_mining":
    # aux_count counts the ores that are not waiting (raw or partial)
    wait = layout.state_id("ore.oreWait")
    delta = (state != wait).int() - (old != wait).int()
    f.aux_count.index_add_(0, rows, delta)


def _fail(scope, kind, w, what):
  raise kind(f"{scope.name}: world {w}: {scope.describe(w)}: {what}")


def _first_bad(a, b):
  """Index of the first world in which arrays a, b [n, ...] differ, or -1."""
  bad = (a != b).reshape(len(a), -1).any(1)
  return int(np.flatnonzero(bad)[0]) if bad.any() else -1


def compare(scope, eng, ref, s, kind=AssertionError, bound=None):
  """The engine's worlds against the oracle's after step `s` (0: before any step): what
  test_gpu_parity's _compare_state, _compare_scalars and _compare_rgb compare, the events as
  multisets, and LAYER; the views in the worlds of ref["views"], everything else in all."""
  from meltingpot_amd import engine as E
  grid, avat, glob = eng.dump()
  for name, got in (("glob", glob), ("avat", avat), ("grid", grid)):
    w = _first_bad(got, ref[name][s])
    if w >= 0:
      where = np.argwhere(got[w] != ref[name][s][w])[:6].tolist()
      _fail(scope, kind, w, f"step {s}: {name} differs at {where}: engine "
            f"{got[w][tuple(where[0])]} oracle {ref[name][s][w][tuple(where[0])]}\n"
            f"engine avatars\n{avat[w]}\noracle avatars\n{ref['avat'][s][w]}")
  if s > 0:
    rew = eng.observe(E.OBS_REWARD).cpu().numpy()
    for name, got, want in (("REWARD", rew, ref["rewards"][s - 1]),
                            ("READY_TO_SHOOT", eng.observe(E.OBS_READY_TO_SHOOT).cpu().numpy(), ref["ready"][s - 1]),
                            ("AUX0", eng.observe(E.OBS_AUX0).cpu().numpy(), ref["aux"][s - 1]),
                            ("COLLECTIVE_REWARD", eng.observe(E.OBS_COLLECTIVE_REWARD).cpu().numpy(),
                             ref["rewards"][s - 1].sum(1))):
      w = _first_bad(got, want)
      if w >= 0:
        _fail(scope, kind, w, f"step {s}: {name} engine {got[w]} oracle {want[w]}")
    rows = eng.observe(E.OBS_EVENTS).cpu().numpy()
    assert not rows[:, 0, 1].any(), "event rows dropped"
    for w in range(scope.n):
      got = sorted(tuple(int(v) for v in r[:3]) for r in rows[w, 1:1 + int(rows[w, 0, 0])])
      if got != ref["events"][s - 1][w]:
        _fail(scope, kind, w, f"step {s}: events engine {got} oracle {ref['events'][s - 1][w]}")
  bound = bound or {}   # {kind: the tensor Engine.bind returned}: drawn by the step's own launch
  sample = sorted(ref["views"])
  import torch
  index = torch.as_tensor(sample, dtype=torch.long, device=eng.device)
  pick = lambda k: (bound[k] if k in bound else eng.observe(k)).index_select(0, index).cpu().numpy()
  rgb, wrgb, layer = pick(E.OBS_RGB), pick(E.OBS_WORLD_RGB), pick(E.OBS_LAYER)
  for i, w in enumerate(sample):
    ow, oa, ol = ref["views"][w][s]
    for name, got, want in (("WORLD.RGB", wrgb[i], ow), ("RGB", rgb[i], oa), ("LAYER", layer[i], ol)):
      if not np.array_equal(got, want):
        _fail(scope, kind, w, f"step {s}: {name} differs at {np.argwhere(got != want)[:4].tolist()}")


FORMS = ("standalone", "fused", "step_many", "active")


def run_engine(scope, ref, form):
  """The scope on the engine, held to `ref` (run_oracle's result).  `form`: "standalone" (no
  view bound: the stand-alone step kernels), "fused" (the per-agent view bound: one launch steps
  and draws), "step_many" (K = 1 requests), "active" (step(active = all ones): the masked body).
  Returns the number of worlds compared."""
  import torch
  from meltingpot_amd import engine as E, substrate
  assert form in FORMS, form
  assert torch.cuda.is_available(), "gpu tests need a GPU"
  if not ref["accepted"].all():
    w = int(np.flatnonzero(~ref["accepted"])[0])
    _fail(scope, ConstructionError, w, "the oracle refused an edit")
  n = scope.n
  eng = E.Engine(scope.pack, n, num_players=scope.players)
  try:
    assert eng.P == scope.players
    bound = {}
    if form == "fused":
      bound[E.OBS_RGB] = eng.bind(E.OBS_RGB)
      assert eng.fused
    eng.reset()
    for a in scope.prefix:
      eng.step(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (n, scope.players)))).to(eng.device))
    bank = eng.save_worlds()
    layout = substrate.SubstrateStateLayout(eng.state_layout(), util.pack_tables(scope.pack))
    apply_edits(scope, bank, layout)
    verdicts = eng.check_states(bank).cpu().numpy()
    if verdicts.any():
      w = int(np.flatnonzero(verdicts.any(1))[0])
      _fail(scope, ConstructionError, w, "check_states: " + layout.describe(*verdicts[w]))
    eng.load_worlds(bank, np.arange(n), check=True)
    eng.sync()   # (a refused row would be named here)
    compare(scope, eng, ref, 0, ConstructionError, bound)
    acts = torch.from_numpy(scope.actions).to(eng.device)
    ones = torch.ones(n, dtype=torch.bool, device=eng.device)
    for s in range(scope.steps):
      if form == "step_many":
        eng.step_many(acts[s:s + 1], keep=())
      elif form == "active":
        eng.step(acts[s], active=ones)
      else:
        eng.step(acts[s])
      compare(scope, eng, ref, s + 1, bound=bound)
      if s + 1 in scope.later:   # a later round of placements: save, edit, check, load, as before
        bank = eng.save_worlds()
        apply_edits(scope, bank, layout, rounds=scope.later[s + 1], cells=np.full((n, 0, 4), -1, np.int32))
        verdicts = eng.check_states(bank).cpu().numpy()
        if verdicts.any():
          w = int(np.flatnonzero(verdicts.any(1))[0])
          _fail(scope, ConstructionError, w, f"after step {s + 1}, check_states: " + layout.describe(*verdicts[w]))
        eng.load_worlds(bank, np.arange(n), check=True)
        eng.sync()
        for name, got in zip(("grid", "avat", "glob"), eng.dump()):
          want = ref["post"][s + 1][("grid", "avat", "glob").index(name)]
          w = _first_bad(got, want)
          if w >= 0:
            _fail(scope, ConstructionError, w, f"after the placements behind step {s + 1}: {name} differs: "
                  f"engine {got[w][tuple(np.argwhere(got[w] != want[w])[0])]} at {np.argwhere(got[w] != want[w])[:4].tolist()}")
    eng.sync()
    assert not eng.fault_words()[:6].any(), eng.fault_words()[:6]
  finally:
    eng.close()
  return n


# ---- the mover scopes ------------------------------------------------------------------------------
# level -> (keyword arguments of geometry.pack, centre of a 5 x 5 patch of free floor whose ring of
# cells at distance 3 holds nothing but floor, spawn points or wall: the beam scope uses all 7 x 7).
# clean_up: three more rows of sand under the four the stock map has; territory__rooms: six columns
# of floor east of the rooms (its rooms are 5 x 5 with a resource and a spawn point inside);
# commons_harvest__open has such a patch.
PATCHES = {
    "clean_up": (dict(height=24), (10, 19)),
    "commons_harvest__open": (dict(), (12, 11)),
    "territory__rooms": (dict(width=27), (22, 10)),
}
# clean_up as a torus with open edges, the patch on corner (0, 0), at the smallest size geometry.pack
# gives: it only ever grows a map, so the smallest is the stock 30 x 21
SEAM = dict(topology="TORUS", open_edges=True)
# commons_harvest__open, A on an apple (the lowest of a diamond of sites): a blocked move re-enters
# A's own cell and eats it (A3b)
APPLE_CENTRE = (8, 5)
PAIR_OFFSETS = tuple((dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if 0 < abs(dx) + abs(dy) <= 2)
PAIR_MOVES = ("NOOP", "FORWARD", "BACKWARD", "STEP_LEFT", "STEP_RIGHT")


def level_pack(level, **kw):
  from meltingpot_amd import engine
  return geometry.pack(level, **kw) if kw else engine.load_pack(level)


def _wrap(level_shape, x, y):
  H, W = level_shape
  return x % W, y % H


def _target(shape, x, y, orient, move):
  """Where the move takes an avatar at (x, y) if nothing is in the way (torus arithmetic:
  harmless on a bounded map, whose patches touch no edge)."""
  if move == "NOOP":
    return _wrap(shape, x, y)
  d = (orient + ("FORWARD", "STEP_RIGHT", "BACKWARD", "STEP_LEFT").index(move)) % 4
  return _wrap(shape, x + DX[d], y + DY[d])


def pair_scope(level, variant="floor"):
  """Pairs of movers: A at the patch centre in 4 orientations, B on each of the 12 cells with
  |dx| + |dy| <= 2 in 4 orientations, both playing each of the 5 moves: 4 * 12 * 4 * 25 = 4800.
  `variant`: "floor" (PATCHES), "seam" (clean_up as a torus with open edges, the centre on the
  corner (0, 0): the patch lies across both edges), "apple" (commons_harvest__open, A on an
  apple).  tags: "conflict": 1 both want one free cell, 2 swap, 3 B follows into A's cell, 4 A
  follows into B's, 5 A moves into standing B, 6 B into standing A, 0 none of these."""
  if variant == "seam":
    pack, (cx, cy) = level_pack(level, **SEAM), (0, 0)
  elif variant == "apple":
    assert level == "commons_harvest__open"
    pack, (cx, cy) = level_pack(level), APPLE_CENTRE
  else:
    kw, (cx, cy) = PATCHES[level]
    pack = level_pack(level, **kw)
  shape = geometry.shape(pack)[:2]
  ids = action_ids(level)
  places, acts, text, conflict = [], [], [], []
  for oa in range(4):
    for dx, dy in PAIR_OFFSETS:
      bx, by = _wrap(shape, cx + dx, cy + dy)
      a0 = _wrap(shape, cx, cy)
      for ob in range(4):
        for ma in PAIR_MOVES:
          for mb in PAIR_MOVES:
            places.append([[a0[0], a0[1], oa, 1], [bx, by, ob, 1]])
            acts.append([ids[ma], ids[mb]])
            text.append(f"A at {a0} facing {ORIENT[oa]} plays {ma}, B at {(bx, by)} facing {ORIENT[ob]} plays {mb}")
            ta, tb = _target(shape, *a0, oa, ma), _target(shape, bx, by, ob, mb)
            b0 = (bx, by)
            conflict.append(1 if ta == tb and ta not in (a0, b0) else
                            2 if ta == b0 and tb == a0 else
                            3 if tb == a0 and ta != a0 else
                            4 if ta == b0 and tb != b0 else
                            5 if ta == b0 else
                            6 if tb == a0 else 0)
  count = 4 * len(PAIR_OFFSETS) * 4 * len(PAIR_MOVES) ** 2
  assert len(PAIR_OFFSETS) == 12 and count == 4800
  return Scope(f"pairs of movers, {level}, {variant}", level, pack, 2, places, np.array(acts)[None],
               text.__getitem__, count, tags={"conflict": np.array(conflict)})


def triple_scope(level):
  """Three movers around one free cell (the patch centre): avatars on 3 of its 4 neighbours (4
  choices), every orientation triple (64), each playing NOOP, the move that enters the cell or the
  move away from it (27): 4 * 64 * 27 = 6912.  tags: "entering": how many avatars play the
  entering move."""
  kw, (cx, cy) = PATCHES[level]
  pack = level_pack(level, **kw)
  ids = action_ids(level)
  places, acts, text, entering = [], [], [], []
  for missing in range(4):
    sides = [d for d in range(4) if d != missing]   # the avatar stands on the cell's side d
    for orients in np.ndindex(4, 4, 4):
      for kinds in np.ndindex(3, 3, 3):   # 0 NOOP, 1 enter, 2 away
        pl, ac, tx = [], [], []
        for d, o, k in zip(sides, orients, kinds):
          x, y = cx + DX[d], cy + DY[d]
          pl.append([x, y, o, 1])
          ac.append(ids["NOOP"] if k == 0 else move_action(ids, o, (d + 2) % 4 if k == 1 else d))
          tx.append(f"{(x, y)} facing {ORIENT[o]} {('stays', 'enters', 'leaves')[k]}")
        places.append(pl); acts.append(ac); text.append("around %s: " % ((cx, cy),) + ", ".join(tx))
        entering.append(sum(k == 1 for k in kinds))
  count = 4 * 64 * 27
  assert count == 6912
  return Scope(f"three movers around one cell, {level}", level, pack, 3, places, np.array(acts)[None],
               text.__getitem__, count, tags={"entering": np.array(entering)})


# ---- the beam scope --------------------------------------------------------------------------------
# level -> (beams: the fire fields of its ACTION_SET, steps, a parking cell far from the patch,
# whether the shooter goes on firing).  Step 1 plays the case; after it the target and the third
# avatar play NOOP.  commons_harvest's zapped avatar is gone at once and comes back 4 frames later
# (6 steps: out, and back in).  territory's first zap marks and freezes, the second one removes
# after a delay of one frame: there the shooter fires in every step, the cooldown of 4 frames lets
# the second shot out in step 5, and step 6 removes (7 steps).
BEAMS = {
    "clean_up": (("fireZap", "fireClean"), 2, (25, 19), False),
    "commons_harvest__open": (("fireZap",), 6, (2, 12), False),
    "territory__rooms": (("fireZap", "fireClaim"), 7, (22, 17), True),
}


def _lone_shot(pack, players, shooter, parked, action, noop):
  """Oracle: the cells whose hit layers differ between a lone shooter's shot and its NOOP."""
  from oracle import oracle
  grids = []
  for a in (action, noop):
    o = oracle.Oracle(pack, util.world_seed(0), players)
    o.reset()
    for p, (x, y, ori) in enumerate([shooter] + parked):
      assert o.place_avatar(p, x, y, ori, True)
    o.step(np.array([a] + [noop] * (players - 1), np.int32))
    grids.append(o.dump()[0])
    o.close()
  t = util.pack_tables(pack)
  layers = sorted({int(t["state_layer"][s]) for s in np.asarray(t["hit_state"]).reshape(-1)})
  diff = (grids[0][layers] != grids[1][layers]).any(0)
  return [(int(x), int(y)) for y, x in np.argwhere(diff) if (x, y) != tuple(shooter[:2])]


def _avatar_layer_cells(pack):
  """bool [H, W]: the cells of the map that hold something on the avatars' layer (init_grid)."""
  from oracle import oracle
  o = oracle.Oracle(pack, util.world_seed(0), 1)
  o.reset()
  assert o.place_avatar(0, 0, 0, 0, False)
  grid = o.dump()[0]
  from meltingpot_amd import lower
  layer = int(o.tables["hdr"][lower.HDR_AVATAR_LAYER])
  o.close()
  return grid[layer] != 0


def beam_footprint(level, beam, orient):
  """The cells a beam covers when its shooter stands at the patch centre facing `orient` with
  nothing in the way — from the ORACLE (a lone shot; test_situations_cpu checks, for the zap, that
  an avatar on each of these cells and on no other is hit), never from the kernel."""
  kw, (cx, cy) = PATCHES[level]
  pack = level_pack(level, **kw)
  ids = action_ids(level)
  px, py = BEAMS[level][2]
  cells = _lone_shot(pack, 3, (cx, cy, orient), [(px, py, 0), (px + 1, py, 0)], ids[beam], ids["NOOP"])
  assert cells and all(max(abs(x - cx), abs(y - cy)) <= 3 for x, y in cells), (level, beam, orient, cells)
  return cells


def beam_scope(level):
  """A shooter (avatar 0) at the patch centre in 4 orientations fires each beam of the level at
  every cell c of the beam's footprint F (`beam_footprint`).  Per (orientation, beam, c):
    4        a target (avatar 1) on c in each orientation
    |F| - 1  the target on c and a second avatar (2) on each other footprint cell: nearer on the
             same ray it stops the ray (A4), elsewhere it is a second victim
    4        the target on c plays each move: it leaves the cell in the same step
    <= 4     the target stands on a free neighbour of c and moves into it
    4        the target on c, in each orientation, zaps in the same step (back, where it faces
             the shooter)
  so count = sum over (orientation, beam) of |F| * (|F| + 11 + free neighbours), stated below and
  asserted.  The patches are bare floor: beams stopped by CELLS (dirt, walls, resources) are
  `blocked_beam_scope`'s."""
  kw, (cx, cy) = PATCHES[level]
  pack = level_pack(level, **kw)
  ids = action_ids(level)
  beams, steps, (px, py), refire = BEAMS[level]
  noop = ids["NOOP"]
  park2 = [px + 1, py, 0, 1]
  taken = _avatar_layer_cells(pack)   # walls and whatever else shares the avatars' layer
  places, acts, text, kinds = [], [], [], []
  count = 0

  def add(kind, shooter, target, third, a_shooter, a_target, what):
    places.append([shooter, target, third]); acts.append([a_shooter, a_target, noop])
    text.append(what); kinds.append(kind)

  for orient in range(4):
    shooter = [cx, cy, orient, 1]
    for beam in beams:
      F = beam_footprint(level, beam, orient)
      fire = ids[beam]
      head = f"shooter at {(cx, cy)} facing {ORIENT[orient]} fires {beam}"
      for c in F:
        free = [(c[0] + DX[d], c[1] + DY[d], d) for d in range(4)
                if (c[0] + DX[d], c[1] + DY[d]) != (cx, cy) and not taken[c[1] + DY[d], c[0] + DX[d]]]
        count += 4 + (len(F) - 1) + 4 + len(free) + 4
        for o in range(4):
          add(0, shooter, [c[0], c[1], o, 1], park2, fire, noop, f"{head}, target on {c} facing {ORIENT[o]}")
        for c2 in F:
          if c2 != c:
            add(1, shooter, [c[0], c[1], 0, 1], [c2[0], c2[1], 0, 1], fire, noop,
                f"{head}, target on {c}, another avatar on {c2}")
        for d in range(4):
          add(2, shooter, [c[0], c[1], 0, 1], park2, fire, move_action(ids, 0, d),
              f"{head}, target on {c} moves {ORIENT[d]}")
        for x, y, d in free:
          add(3, shooter, [x, y, 0, 1], park2, fire, move_action(ids, 0, (d + 2) % 4),
              f"{head}, target on {(x, y)} moves into {c}")
        for o in range(4):
          add(4, shooter, [c[0], c[1], o, 1], park2, fire, ids["fireZap"],
              f"{head}, target on {c} facing {ORIENT[o]} zaps")
  assert len(places) == count <= 5000, (level, len(places), count)
  actions = np.full((steps, count, 3), noop, np.int32)
  actions[0] = np.array(acts)
  if refire:
    actions[1:, :, 0] = actions[0, :, 0]
  return Scope(f"beams, {level}", level, pack, 3, places, actions, text.__getitem__, count,
               tags={"kind": np.array(kinds)})


# ---- respawn onto taken spawn points (A5) --------------------------------------------------------
RESPAWN_LEVEL = "commons_harvest__open"
RESPAWN_MAP = dict(spawn_points=("P", 4))   # the stock map with four spawn points left
RESPAWN_SEEDS = 40
RESPAWN_STEPS = 7   # the timer of 4 frames runs out, then three more attempts


def respawn_scope():
  """commons_harvest__open with 4 spawn points and 4 avatars, one of them dead since the frame of
  the edit (`place(..., alive=0)`; NOOPs let its timer of 4 frames run): the three living ones
  stand on all spawn points but one (4 choices of the free one) or on all but two, the third on
  bare floor (6 choices), for each choice of the dead avatar (4), each in RESPAWN_SEEDS worlds
  because where a respawn lands is drawn: (4 + 6) * 4 * RESPAWN_SEEDS = 1600.  The dead avatar
  lands where the oracle puts it or, on a taken point, retries in the next frame.
  NOT built: all four points taken, which needs a fifth avatar — and a reset with more avatars
  than spawn points is a situation of its own, which neither side is known to handle."""
  import itertools
  pack = level_pack(RESPAWN_LEVEL, **RESPAWN_MAP)
  t = util.pack_tables(pack)
  W = geometry.shape(pack)[1]
  points = [(int(c) % W, int(c) // W) for c in t["spawn_cells"]]
  assert len(points) == 4, points
  floor = PATCHES[RESPAWN_LEVEL][1]
  places, text, free_count = [], [], []
  first = [[floor[0] + 2 * p - 3, floor[1] + 2, 0, 1] for p in range(4)]   # off the spawn points first
  for dead in range(4):
    living = [p for p in range(4) if p != dead]
    for k in (1, 2):
      for free in itertools.combinations(range(4), k):
        taken = [points[i] for i in range(4) if i not in free] + [floor]
        pl = [None] * 4
        pl[dead] = [0, 0, 0, 0]   # (a dead avatar has no cell)
        for p, (x, y) in zip(living, taken):
          pl[p] = [x, y, p, 1]
        for _ in range(RESPAWN_SEEDS):
          places.append(pl); free_count.append(k)
          text.append(f"avatar {dead} dead, spawn points {[points[i] for i in free]} free, the others taken")
  count = (4 + 6) * 4 * RESPAWN_SEEDS
  assert len(places) == count
  actions = np.full((RESPAWN_STEPS, count, 4), action_ids(RESPAWN_LEVEL)["NOOP"], np.int32)
  return Scope("respawn onto taken spawn points", RESPAWN_LEVEL, pack, 4, places, actions,
               text.__getitem__, count, tags={"free": np.array(free_count)}, first=[first] * count)


# ---- the oracle's own scripted scenes ----------------------------------------------------------------
COOP_SEEDS = 8


def coop_scope():
  """The scenes of tests/test_oracle_coop_cpu.py (imported, not restated): A and B on either side
  of one ore, C far away.  "gold": A alone and the window of 3 frames runs out, then A and B
  inside the window; "gold, late": A, then B when the window has just run out — B starts a window
  of its own and nobody is paid; "iron": both in one frame.  Each in COOP_SEEDS worlds: 24."""
  import test_oracle_coop_cpu as C
  from meltingpot_amd import engine
  pack = C.scripted_pack(engine.load_pack("coop_mining"))
  t = util.pack_tables(pack)
  s_wait, s_iron, s_gold = (int(x) for x in t["cm_states"][:3])
  layer = int(t["state_layer"][s_wait])
  W = geometry.shape(pack)[1]
  x, y = C.ORE_CELL % W, C.ORE_CELL // W
  late = (C.GOLD_SCRIPT[0],) + (C._IDLE,) * 3 + ((C.NOOP, C.MINE, C.NOOP),)
  scenes = (("gold", s_gold, C.GOLD_SCRIPT), ("gold, late", s_gold, late), ("iron", s_iron, C.IRON_SCRIPT))
  steps = max(len(script) for _, _, script in scenes)
  places, cells, acts, text = [], [], [], []
  for name, state, script in scenes:
    for _ in range(COOP_SEEDS):
      places.append([[px, py, o, 1] for px, py, o in C.SCENE_PLACES])
      cells.append([[layer, x, y, state]])
      acts.append(list(script) + [C._IDLE] * (steps - len(script)))
      text.append(f"coop_mining, {name}: ore at {(x, y)}")
  count = 3 * COOP_SEEDS
  return Scope("coop_mining's scripted scenes", "coop_mining", pack, 3, places,
               np.array(acts).transpose(1, 0, 2), text.__getitem__, count, cells=cells,
               tags={"scene": np.repeat(np.arange(3), COOP_SEEDS)})


COOK_SEEDS = 16


def cook_scope():
  """tests/test_oracle_cook_cpu.py's two avatars at one stocked counter of `circuit`, both
  interacting in one frame, in COOK_SEEDS worlds (who is served depends on the frame's visiting
  order); a second step of NOOPs follows.  The inventories connected to the avatars move with
  them."""
  import test_oracle_cook_cpu as C
  from meltingpot_amd import engine
  pack = C.stocked(engine.load_pack(C.COUNTER_LAYOUT))
  ids = action_ids(C.COUNTER_LAYOUT)
  places = [[[x, y, o, 1] for x, y, o in C.COUNTER_PLACES]] * COOK_SEEDS
  acts = np.array([[[ids["interact"]] * 2] * COOK_SEEDS, [[ids["NOOP"]] * 2] * COOK_SEEDS])
  return Scope("two avatars at one counter", C.COUNTER_LAYOUT, pack, 2, places, acts,
               lambda w: f"both interact with the counter between {C.COUNTER_PLACES}", COOK_SEEDS)


SCENE_SEEDS = 8


def gift_scope():
  """tests/test_oracle_gift_cpu.py's scripted refinement chain in SCENE_SEEDS worlds: a live token
  set next to player 0, picked up, gifted and refined back and forth, consumed (7 steps)."""
  import test_oracle_gift_cpu as C
  from meltingpot_amd import engine
  pack = engine.load_pack("gift_refinements")
  t = util.pack_tables(pack)
  live = int(t["gr_states"][1])
  n = SCENE_SEEDS
  places = [[[x, y, o, 1] for x, y, o in C.CHAIN_PLACES]] * n
  cells = [[[int(t["state_layer"][live]), C.CHAIN_TOKEN[0], C.CHAIN_TOKEN[1], live]]] * n
  acts = np.array([list(C.CHAIN_SCRIPT)] * n).transpose(1, 0, 2)
  return Scope("gift_refinements' scripted chain", "gift_refinements", pack, 2, places, acts,
               lambda w: "the refinement chain of test_oracle_gift_cpu", n, cells=cells)


def matrix_scope():
  """tests/test_oracle_matrix_cpu.py's scenes on prisoners_dilemma_in_the_matrix__repeated, each in
  SCENE_SEEDS worlds: (0, 1) both collect a resource, are placed face to face (a second round of
  placements behind step 1) and player 0 / player 1 interacts: the freeze, the payout, both removed,
  the resources back, and on to the respawn; (2) face to face without having collected: the
  interaction is refused and the beam stops at the avatar."""
  import test_oracle_matrix_cpu as C
  from meltingpot_amd import engine
  pack = engine.load_pack(C.PD)
  mi = util.pack_tables(pack)["mx_i32"]
  freeze, respawn = int(mi[5]), int(mi[4])
  steps = 2 + freeze + 2 + respawn + 1
  n = 3 * SCENE_SEEDS
  collect = [[x, y, o, 1] for x, y, o in C.COLLECT_PLACES]
  facing = [[x, y, o, 1] for x, y, o in C.FACING_PLACES]
  places, later, acts, scene = [], [], np.zeros((steps, n, 2), np.int32), []
  for k in range(3):
    for _ in range(SCENE_SEEDS):
      w = len(places)
      places.append(facing if k == 2 else collect)
      later.append([[-1, -1, 0, 1]] * 2 if k == 2 else facing)   # (scene 2 places nobody again)
      if k < 2:
        acts[0, w] = C.FORWARD
        acts[1, w, k] = C.INTERACT
      else:
        acts[0, w, 0] = C.INTERACT
      scene.append(k)
  text = ("both collect, player 0 interacts", "both collect, player 1 interacts", "nobody has collected, player 0 interacts")
  return Scope("the matrix's scripted interaction", C.PD, pack, 2, places, acts, lambda w: text[scene[w]], n,
               tags={"scene": np.array(scene)}, later={1: later})


def soup_scope():
  """tests/test_oracle_cook_cpu.py's scripted soup on `cramped` (its `soup_ops`, played as they
  are: 12 rounds of placements in the course of 50 steps) in SCENE_SEEDS worlds: three tomatoes
  into the pot, the cooking, the dish, the soup, the delivery that pays both players 20."""
  import test_oracle_cook_cpu as C
  from meltingpot_amd import engine
  level = "collaborative_cooking__cramped"
  pack = engine.load_pack(level)
  ids = action_ids(level)
  n = SCENE_SEEDS
  rounds, acts = {}, []
  for op in C.soup_ops():   # one round per placement, in the script's order
    if op[0] == "place":
      one = [[-1, -1, 0, 1], [-1, -1, 0, 1]]
      one[op[1]] = [op[2], op[3], op[4], 1]
      rounds.setdefault(len(acts), []).append(np.array([one] * n))
    else:
      acts.append([ids["interact"] if v else ids["NOOP"] for v in op[1:]])
  first, places = rounds.pop(0)   # before the first step: player 1, then player 0
  return Scope("the scripted soup", level, pack, 2, places, np.array([acts] * n).transpose(1, 0, 2),
               lambda w: "the soup of test_oracle_cook_cpu", n, first=first, later=rounds)


# ---- beams stopped by cells of the map ---------------------------------------------------------------
# level -> (keyword arguments of geometry.pack, the band of cells (x0, y0, x1, y1) the shooter stands on,
# beams, a parking cell).  clean_up: the river, dirty at the reset, and its banks: the clean beam is
# stopped by dirt and cleans it, both beams by the wall above.  territory__rooms: a room, with its
# resource and its walls of resources: zap and claim beams are stopped, the claim beam claims.
# commons_harvest__open: along the top wall, over the apples.
BLOCKED = {
    "clean_up": (dict(), (1, 1, 28, 8), ("fireZap", "fireClean"), (25, 18)),
    "commons_harvest__open": (dict(), (1, 1, 22, 3), ("fireZap",), (2, 12)),
    "territory__rooms": (dict(), (1, 1, 5, 5), ("fireZap", "fireClaim"), (16, 16)),
}


def blocked_beam_scope(level):
  """A shooter on every free cell of BLOCKED's band, in 4 orientations, fires each beam of the level
  at whatever the stock map has there — alone (tag kind 0: whatever stops a ray is a CELL), and
  with a target avatar two cells ahead where that cell is free (kind 1: behind a dirty cell, an
  apple, or nothing).  A second step of NOOPs follows.  count = cells * 4 * beams + the worlds with
  a target, stated by the generator from the oracle's map and asserted <= 5000."""
  kw, (x0, y0, x1, y1), beams, (px, py) = BLOCKED[level]
  pack = level_pack(level, **kw)
  ids = action_ids(level)
  taken = _avatar_layer_cells(pack)
  H, W = taken.shape
  noop = ids["NOOP"]
  places, acts, text, kinds = [], [], [], []
  cells = [(x, y) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1) if not taken[y, x]]
  for x, y in cells:
    for o in range(4):
      tx, ty = x + 2 * DX[o], y + 2 * DY[o]
      ahead = 0 <= tx < W and 0 <= ty < H and not taken[ty, tx]
      for beam in beams:
        places.append([[x, y, o, 1], [px, py, 0, 1]]); acts.append([ids[beam], noop]); kinds.append(0)
        text.append(f"shooter at {(x, y)} facing {ORIENT[o]} fires {beam}, alone")
        if ahead:
          places.append([[x, y, o, 1], [tx, ty, 0, 1]]); acts.append([ids[beam], noop]); kinds.append(1)
          text.append(f"shooter at {(x, y)} facing {ORIENT[o]} fires {beam}, target at {(tx, ty)}")
  count = len(cells) * 4 * len(beams) + sum(kinds)
  assert len(places) == count <= 5000, (level, count)
  actions = np.full((2, count, 2), noop, np.int32)
  actions[0] = np.array(acts)
  # (a first round takes both avatars off the cells the reset put them on)
  return Scope(f"beams stopped by the map, {level}", level, pack, 2, places, actions, text.__getitem__, count,
               tags={"kind": np.array(kinds)}, first=[[[px, py, 0, 1], [px + 1, py, 0, 1]]] * count)


def cook_served(scope, ref):
  """The set of players served over the worlds of cook_scope's oracle run (asserts that exactly
  one is in each): the one whose inventory is no longer `inventory.empty` after step 1."""
  t = util.pack_tables(scope.pack)
  empty = bytes(t["state_names"]).split(b"\0").index(b"inventory.empty")
  layer = int(t["state_layer"][empty])
  served = set()
  for w in range(scope.n):
    held = [int(ref["grid"][1][w, layer, y, x]) != empty for x, y in ref["avat"][1][w, :, :2]]
    assert sum(held) == 1, (w, held)
    served.add(held.index(True))
  return served


def sub_scope(scope, worlds, name):
  """The situations `worlds` of `scope`, in worlds 0 .. len(worlds) - 1 (other seeds than they had
  in `scope`: a scope too large for one test is split into scopes of their own)."""
  worlds = np.asarray(worlds)
  tags = {k: v[worlds] for k, v in scope.tags.items()}
  return Scope(f"{scope.name}, {name}", scope.level, scope.pack, scope.players, scope.places[worlds],
               scope.actions[:, worlds], lambda w: scope.describe(int(worlds[w])), len(worlds),
               scope.cells[worlds], scope.prefix, tags, None if scope.first is None else scope.first[worlds],
               {k: [r[worlds] for r in v] for k, v in scope.later.items()})


def triple_half(level, half):
  """triple_scope in two tests: the neighbour sets 0, 1 and 2, 3 (3456 situations each)."""
  full = triple_scope(level)
  assert full.n == full.count == 6912
  return sub_scope(full, np.arange(3456) + 3456 * half, f"half {half}")


def pair_outcomes(scope, ref):
  """{"A": worlds in which A won a cell both wanted, "B": ..., "both": worlds in which both
  stand on it (never), "neither": worlds of a swap in which neither moved} of a pair scope's
  oracle run."""
  before, after = ref["avat"][0][:, :, :2], ref["avat"][1][:, :, :2]
  moved = (before != after).any(2)
  both = scope.tags["conflict"] == 1
  swap = scope.tags["conflict"] == 2
  return {"A": np.flatnonzero(both & moved[:, 0] & ~moved[:, 1]),
          "B": np.flatnonzero(both & ~moved[:, 0] & moved[:, 1]),
          "both": np.flatnonzero(both & moved[:, 0] & moved[:, 1]),
          "neither": np.flatnonzero(swap & ~moved[:, 0] & ~moved[:, 1])}


if __name__ == "__main__":
  if len(sys.argv) == 3 and sys.argv[1] == "--oracle":   # worker of run_oracle
    with open(sys.argv[2], "rb") as f:
      job = pickle.load(f)
    with open(sys.argv[2] + ".out", "wb") as f:
      pickle.dump(_oracle_chunk(job), f)
