"""Test infrastructure: a plain Python model of `engine.Engine` made of CPU oracles, for the
program tests (tests/api_programs.py).  It answers the calls a learner or a planner makes —
reset, masked reset, re-seed, step, step_fields, step_many with rows, save_worlds / load_worlds,
snapshot / restore, bind / bind_ring / unbind, and, composed in the same _advance / step /
step_many: masks (active=), stops (until=, stopped=, returns=, gamma=), registered episode starts
(set_episode_starts / clear_episode_starts), per-step state rows (states=) and reads of bank rows
(state_value, view_of) — and says what every output of include/mp_engine.h it models must hold
afterwards.

Per world it keeps a live `oracle.Oracle` and the world's LOG, (seed, [("reset",) | ("step", a) |
("fields", f), ...]): what the oracle was fed since it was created.  A world is copied (load,
restore) by replaying a log into a fresh oracle; nothing of an oracle is ever copied directly.

What it models, after mp_engine.h:
  * the record (`dump()`), as the oracles' dumps;
  * the scalar kinds as BUFFERS written per world by the submission that writes them — a reset, a
    step or a load writes every modelled kind of its world; a frozen world (done, auto_reset off)
    writes REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT and an empty EVENTS header only; a world
    outside a reset's mask or with src = -1 writes nothing; mp_restore is no launch and writes
    nothing.  So between launches a record-function kind (POSITION, ORIENTATION, READY_TO_SHOOT,
    INVENTORY) is the function of the record, except right after a restore, where the buffers
    still hold what the launch before wrote.  A ring-bound scalar kind is written into the slot of
    the submission, and a world that writes nothing leaves that slot's bytes as they were;
  * the views (RGB, RGB_POOL2/4/8, WORLD.RGB, LAYER) as functions of the records of ALL worlds,
    drawn into what is bound (the ring slot) by every submission;
  * mp_counters' bad_actions (kept by the destination of a load, rewound by a restore);
  * a world skipped by a mask or a stop state: nothing of it is written, its element of a bound
    LAYER included (only pixel views are redrawn for all worlds); a world paused on LAST restarts in
    its next active step; `stopped` and `rows` are the caller's arrays, read and written in place;
  * a registered start: the level's reset and on top of it what a load of the row writes.
    fresh=True is NOT modelled (the oracle takes no state): `exact` says which worlds the model
    speaks for;
  * a listed request (worlds=) as MpStepListed's identity: the masked request over all N worlds with
    the actions scattered by owning entry (the lowest that names a world), every per-call tensor
    gathered by entry on top of what it held, `stopped` by world;
  * the episode statistics (MpEpisodeStats): a tests/episode_stats_model.Model fed, per world and per
    step that ran (a reset's mask, a load's rows, the steps a mask, a stop or a list let run), the
    STEP_TYPE, REWARD and EVENTS the model says that step left;
  * the registered view units (EGO_LAYER, view hashes, planes): behind every submission the unit's
    function of ALL N records, from the oracles' dumps through tests/ego_layer_model.py,
    view_hash_model.py and ego_planes_model.py, into the tensor or the ring slot of the submission;
    a restore, being no launch, writes none.
It says nothing about the kinds under the carry rule that no record holds (AUX0 - AUX4, ZAP_MATRIX,
INTERACTION_INVENTORIES, INTERACTION_REWARDS, MATRIX_CUMULANTS): the twin engine of
api_programs.run_program covers those."""
import collections
import zlib

import numpy as np

from meltingpot_amd import engine as E
from oracle import oracle as oracle_lib
from oracle_engine import OracleBatchEngine
import ego_layer_model
import ego_planes_model
import episode_stats_model
import util
import view_hash_model

TRANSITION_KINDS = (E.OBS_REWARD, E.OBS_COLLECTIVE_REWARD, E.OBS_STEP_TYPE, E.OBS_DISCOUNT, E.OBS_EVENTS)
RECORD_SCALARS = (E.OBS_POSITION, E.OBS_ORIENTATION, E.OBS_READY_TO_SHOOT, E.OBS_INVENTORY)
VIEW_KINDS = E.PIXEL_KINDS + (E.OBS_LAYER,)


def event_rows(events, dropped=0):
  """One world's MP_OBS_EVENTS block [EVENT_ROWS, 4] holding `events` ((type, a, b) tuples)."""
  rows = np.zeros((E.EVENT_ROWS, 4), np.int32)
  rows[0, :2] = (len(events), dropped)
  for i, ev in enumerate(events):
    rows[1 + i, :3] = ev
  return rows


class ModelEngine:
  """See the module's docstring.  Arrays are numpy where `engine.Engine` has torch tensors."""

  def __init__(self, pack_bytes, n, *, auto_reset, num_players=0, world_offset=0, world_pool=1):
    self.pack_bytes = pack_bytes
    self.N = int(n)
    self._auto_reset = bool(auto_reset)
    self._num_players = int(num_players)
    self.world_pool = max(1, int(world_pool))
    self._seed = [util.world_seed(world_offset + w) for w in range(self.N)]
    self._o = [self._oracle(s) for s in self._seed]
    self._log = [[] for _ in range(self.N)]
    self._started = [False] * self.N
    o = self._o[0]
    self.P = o.P
    t = o.tables
    table = np.asarray(t["action_table"]).reshape(-1, 4)
    self.num_actions = len(table)
    # (asserted once: a bad action id steps as NOOP, and NOOP is id 0)
    assert not table[0].any(), "row 0 of the pack's action_table is not NOOP"
    self.num_action_fields = int(t["hdr"][21])
    try:
      self.num_resources = int(o.inventories()[0].shape[1])
    except AssertionError:
      self.num_resources = 0
    N, P, R = self.N, self.P, self.num_resources
    vw, vh = o.view
    k = self.world_pool
    self.shapes = {
        E.OBS_RGB: ((N, P, vh * 8, vw * 8, 3), np.uint8),
        E.OBS_WORLD_RGB: ((N, o.H * 8 // k, o.W * 8 // k, 3), np.uint8),
        E.OBS_LAYER: ((N, P, vh, vw, o.L), np.int32),
        E.OBS_REWARD: ((N, P), np.float64),
        E.OBS_COLLECTIVE_REWARD: ((N,), np.float64),
        E.OBS_STEP_TYPE: ((N,), np.int32),
        E.OBS_DISCOUNT: ((N,), np.float64),
        E.OBS_EVENTS: ((N, E.EVENT_ROWS, 4), np.int32),
        E.OBS_POSITION: ((N, P, 2), np.int32),
        E.OBS_ORIENTATION: ((N, P), np.int32),
        E.OBS_READY_TO_SHOOT: ((N, P), np.float64),
        **{kind: ((N, P, vh * 8 // p, vw * 8 // p, 3), np.uint8) for p, kind in E.OBS_RGB_POOL.items()},
    }
    if R:
      self.shapes[E.OBS_INVENTORY] = ((N, P, R), np.float64)
    self.scalar_kinds = tuple(k for k in TRANSITION_KINDS + RECORD_SCALARS if k in self.shapes)
    self.record_scalars = tuple(k for k in RECORD_SCALARS if k in self.shapes)
    self._buf = {k: np.zeros(*self.shapes[k]) for k in self.scalar_kinds}
    self._bound = {}     # kind -> array [N, ...], or [T, N, ...] for a ring kind
    self._ring_kinds = set()
    self._slots = 0
    self._cursor = 0
    self._slot = 0
    self._bad = np.zeros(self.N, np.int64)
    self._touched = None
    self.starts = None   # the registration: (bank, rows [N])
    self._fresh = False
    # exact[w]: the model speaks for world w.  A world that took a fresh=True start is one the
    # oracle cannot state (it has no state load); it stays inexact until it is re-seeded, and a row
    # saved from it, or a world loaded from such a row, is inexact too
    self.exact = np.ones(self.N, bool)
    # ... and for its output buffers, which a restore leaves as the launch before wrote them: they
    # are the model's again once an exact world has written them (a step, a reset, a load)
    self._buf_exact = np.ones(self.N, bool)
    self._paused = np.zeros(self.N, bool)   # skipped while on LAST, in front of its restart
    self.cover = collections.Counter()      # what a run contained (tests/test_api_programs_cpu.py)
    self._step_starts = []                  # (world, row index or -1) of the restarts of this step
    self._replays = {}   # row_key -> the oracle its log was replayed into
    # episode statistics (MpEpisodeStats): a tests/episode_stats_model.Model while registered, and the
    # worlds the model has spoken for ever since the registration
    self.stats = None
    self.stats_exact = np.zeros(self.N, bool)
    self._credit = None      # a listed call: {world: entry} of the owning entries
    self._stop_list = {}     # world -> the list of the listed call that set its `stopped` byte
    # world -> what its statistics must hold when the episode begun behind a cut finishes: the cut
    # one's sums nowhere (see _cut)
    self._after_cut = {}
    # registered view units: name ("ego" / "hash" / "planes") -> {"out", "ring", "exact", params}
    self.units = {}
    self._since_clear = None   # submissions since the last units_clear
    self._restored = np.zeros(self.N, bool)   # record changed by a restore, no submission ran it yet

  # -- the interface the runner drives on both sides (numpy in, numpy out here)
  def to_device(self, a):
    return np.asarray(a)

  def _oracle(self, seed):
    return oracle_lib.Oracle(self.pack_bytes, int(seed), self._num_players)

  def close(self):
    for o in list(self._o) + list(self._replays.values()):
      o.close()
    self._o, self._replays = [], {}

  # -- buffers
  def bind(self, kind, tensor=None):
    assert tensor is None
    out = np.zeros(*self.shapes[kind])
    self._drop_ring(kind)
    self._bound[kind] = out
    if kind in self._buf:
      self._buf[kind] = out
    return out

  def bind_ring(self, kind, tensor=None, slots=None, tune=True):
    assert tensor is None and slots
    shape, dtype = self.shapes[kind]
    if not self._ring_kinds - {kind}:
      self._slots, self._cursor = int(slots), 0
    assert int(slots) == self._slots, "one slot count for all ring kinds"
    self._ring_kinds.add(kind)
    self._bound[kind] = np.zeros((self._slots,) + tuple(shape), dtype)
    return self._bound[kind]

  def _drop_ring(self, kind):
    self._ring_kinds.discard(kind)
    if not self._ring_kinds:
      self._slots = self._cursor = 0

  def unbind(self, kind):
    assert kind in VIEW_KINDS, "the model unbinds views only"
    self._bound.pop(kind, None)
    self._drop_ring(kind)

  @property
  def ring(self):
    T = self._slots
    nxt = self._cursor % T if T else 0
    return {"slots": T, "next": nxt, "last": (nxt + T - 1) % T if T else 0}

  def _target(self, kind):
    """Where this submission writes scalar `kind`: [N, ...]."""
    return self._bound[kind][self._slot] if kind in self._ring_kinds else self._buf[kind]

  def _last(self, kind):
    """What mp_observe reads for scalar `kind`: a ring kind's slot written last."""
    return self._bound[kind][self.ring["last"]] if kind in self._ring_kinds else self._buf[kind]

  # -- what one world writes
  def _of_records(self, kind, oracles):
    """A kind that is a function of the record, of `oracles`: OracleBatchEngine's own values."""
    shim = OracleBatchEngine.__new__(OracleBatchEngine)
    shim._o, shim.P, shim._step_type = oracles, self.P, np.ones(len(oracles), np.int32)
    return OracleBatchEngine._value(shim, kind)

  def _write_record_kinds(self, w):
    for kind in self.record_scalars:
      self._target(kind)[w] = self._of_records(kind, [self._o[w]])[0]

  def _write_transition(self, w, step_type, rewards, events):
    self._target(E.OBS_REWARD)[w] = rewards
    self._target(E.OBS_COLLECTIVE_REWARD)[w] = float(np.sum(rewards))
    self._target(E.OBS_STEP_TYPE)[w] = step_type
    self._target(E.OBS_DISCOUNT)[w] = 1.0 if step_type == 1 else 0.0
    self._target(E.OBS_EVENTS)[w] = event_rows(events)

  def _wrote_reset(self, w):
    # (the events of a reset are the level's start-up events, the same for every world and seed:
    # AvatarStarted per avatar, externality_mushrooms' set_sanctioning_level; a load writes them too)
    self._reset_events = self._o[w].events()
    self._write_transition(w, 0, np.zeros(self.P), self._reset_events)
    self._write_record_kinds(w)

  @property
  def speaks(self):
    """bool [N]: the worlds whose record AND output buffers the model states."""
    return self.exact & self._buf_exact

  def _wrote_load(self, w, row):
    self._buf_exact[w] = row.get("exact", True)
    if row["finished"]:   # loads finished: what a frozen world reports
      self._write_transition(w, 2, np.zeros(self.P), [])
    else:                 # as a reset writes them
      self._write_transition(w, 0, np.zeros(self.P), self._reset_events)
    self._write_record_kinds(w)
    self._buf_exact[w] = self.exact[w]

  def _frozen_rewards(self, w):
    return np.zeros(self.P)

  def _wrote_frozen(self, w):
    self._write_transition(w, 2, self._frozen_rewards(w), [])

  # -- submissions
  def _begin(self, masked=False):
    """masked: a submission under a mask or a stop state (MpStepActive, MpStepUntil), which does
    not touch the worlds it skips."""
    self._touched = set() if masked else None
    if self._slots:
      self._slot = self._cursor % self._slots
      self._cursor += 1

  def view_value(self, kind):
    """A view kind as the function of the records it is, for every world."""
    return self._kind_of(kind, self._o)

  def _kind_of(self, kind, oracles):
    """A kind that is a function of the record (a view or a record scalar), of `oracles`."""
    if kind in self.record_scalars:
      return np.asarray(self._of_records(kind, oracles), self.shapes[kind][1])
    if kind == E.OBS_WORLD_RGB:
      return E.pool_rgb(self._of_records(kind, oracles), self.world_pool)
    if kind == E.OBS_LAYER:
      return np.stack([np.stack([o.layer_view(p) for p in range(self.P)]) for o in oracles])
    rgb = self._of_records(E.OBS_RGB, oracles)
    if kind == E.OBS_RGB:
      return rgb
    return E.pool_rgb(rgb, {v: k for k, v in E.OBS_RGB_POOL.items()}[kind])

  def _end(self):
    """Every bound view is drawn by the submission, from all the records — but a bound LAYER is a
    non-pixel output, which a masked submission writes for the worlds that ran only: a skipped
    world's elements keep their bytes (they differ from its record's right after a restore)."""
    for kind, out in self._bound.items():
      if kind in VIEW_KINDS:
        value = self.view_value(kind)
        target = out[self._slot] if kind in self._ring_kinds else out
        if kind == E.OBS_LAYER and self._touched is not None:
          for w in self._touched:
            target[w] = value[w]
        else:
          target[...] = value
    self._draw_units()
    if self._since_clear is not None and self.units:
      self._since_clear += 1
      if self._since_clear == max(2, self._slots):
        self.cover["units_clear followed by submissions of every slot"] += 1

  # -- registered view units: one launch behind every submission, over ALL worlds
  def _unit_worlds(self):
    """The worlds a submission's unit launch redraws: all of them, skipped and unlisted included."""
    return range(self.N)

  def _draw_units(self):
    if not self.units:
      return
    worlds = list(self._unit_worlds())
    dumps = [self._o[w].dump() for w in worlds]
    for name, u in self.units.items():
      value = self._unit_value(name, u, dumps)
      target = u["out"][self._slot] if u["ring"] else u["out"]
      exact = u["exact"][self._slot] if u["ring"] else u["exact"]
      for i, w in enumerate(worlds):
        target[w] = value[i]
        exact[w] = self.exact[w]
    avat = np.stack([d[1] for d in dumps])[:, :self.P]
    live = avat[:, :, 3] != 0
    if (~live).any():
      self.cover["a registered view of a dead viewer"] += 1
    for o in set(avat[:, :, 2][live].tolist()):
      self.cover[f"a registered view at orientation {int(o)}"] += 1
    H, W, _, (vl, vr, vf, vb), torus = ego_layer_model.geometry(self.pack_bytes)
    # the window's extent on the map's axes, by the viewer's orientation: (left, right, up, down)
    extent = np.array([(vl, vr, vf, vb), (vb, vf, vl, vr), (vr, vl, vb, vf), (vf, vb, vr, vl)])
    x, y, e = avat[:, :, 0][live], avat[:, :, 1][live], extent[avat[:, :, 2][live] & 3]
    if not torus and ((x - e[:, 0] < 0) | (x + e[:, 1] >= W) | (y - e[:, 2] < 0) | (y + e[:, 3] >= H)).any():
      self.cover["a registered window cell off the map"] += 1
    skipped = self._restored.copy()
    if self._touched is not None and self.units:
      skipped[list(self._touched)] = False
      if skipped.any():
        self.cover["restore changed a record, then a step skipped that world, a unit registered"] += 1
    self._restored[:] = False

  def _unit_value(self, name, u, dumps):
    """The function of unit `name` of the records `dumps` (oracle dumps): [len(dumps), P, ...]."""
    P = self.P
    grid = np.stack([d[0] for d in dumps])
    avat = np.stack([d[1] for d in dumps])[:, :P]
    ax, ay, ori, alive = (avat[:, :, i] for i in range(4))
    if name == "planes":
      return ego_planes_model.planes(self.pack_bytes, grid, ax, ay, ori, alive, u["classes"], u["num_classes"],
                                     u["layers"], u["facing"])
    ego = ego_layer_model.ego_layer(self.pack_bytes, grid, ax, ay, ori, alive)
    if name == "ego":
      return ego
    return view_hash_model.view_hash(ego, u["layers"], u["classes"])

  @property
  def ego_layer_shape(self):
    return tuple(self.shapes[E.OBS_LAYER][0])

  def ego_planes_shape(self, num_classes, facing=False):
    N, P, VH, VW, _ = self.ego_layer_shape
    return (N, P, int(num_classes) + (4 if facing else 0), VH, VW)

  def _register(self, name, out, base_ndim, **params):
    if out is None:
      self.units.pop(name, None)
      self._since_clear = 0
      return None
    ring = out.ndim == base_ndim + 1
    assert not ring or out.shape[0] == self._slots, "a unit's ring has the engine's slots"
    if self.units:
      self.cover["a unit registered beside a live one"] += 1
    self.units[name] = dict(params, out=out, ring=ring, exact=np.zeros(out.shape[:1 + int(ring)], bool))
    return out

  def bind_ego_layer(self, out):
    return self._register("ego", out, 5)

  def bind_ego_layer_ring(self, tensor=None, slots=None):
    return self._register("ego", tensor, 5)

  def bind_view_hash(self, out, layers=None, classes=None):
    return self._register("hash", out, 2, layers=layers, classes=classes)

  def bind_ego_planes(self, out, classes=None, layers=None, facing=False, num_classes=None):
    return self._register("planes", out, 5, classes=classes, layers=layers, facing=facing, num_classes=num_classes)

  def unit_speaks(self, name):
    """bool [N] ([T, N] of a ring): the elements of the registered tensor the model states — a world
    it spoke for when the launch that drew the element ran."""
    return self.units[name]["exact"]

  def _unit_read(self, name, params, bank, rows, players):
    if bank is None:
      idx = range(self.N) if rows is None else [int(i) for i in np.asarray(rows)]
      oracles = [self._o[i] for i in idx]
    else:
      count = len(bank) if players is None else len(np.asarray(players))
      idx = range(count) if rows is None else [int(i) for i in np.asarray(rows)]
      oracles = [self._replayed(bank[i]) for i in idx]
    value = self._unit_value(name, params, [o.dump() for o in oracles])
    return value if players is None else value[np.arange(len(value)), np.asarray(players)]

  def observe_ego_layer(self, bank=None, rows=None, players=None):
    return self._unit_read("ego", {}, bank, rows, players)

  def hash_views(self, bank=None, rows=None, players=None, layers=None, classes=None):
    return self._unit_read("hash", dict(layers=layers, classes=classes), bank, rows, players)

  def observe_ego_planes(self, classes, bank=None, rows=None, players=None, layers=None, facing=False, num_classes=None):
    return self._unit_read("planes", dict(classes=classes, layers=layers, facing=facing, num_classes=num_classes),
                           bank, rows, players)

  # -- episode statistics
  def set_episode_stats(self, columns="default", pairs=()):
    if self.stats is not None:
      self.cover["stats_set over a live registration"] += 1
    if isinstance(columns, str) and columns == "default":
      columns = E.level_event_columns(int(self._o[0].tables["hdr"][1]))
    self.stats = episode_stats_model.Model(self.N, self.P, columns, pairs)
    self.stats_exact = self.speaks.copy()
    self._after_cut = {}
    return self.stats

  def clear_episode_stats(self):
    self.stats = None

  def event_columns(self):
    return E.level_event_columns(int(self._o[0].tables["hdr"][1]))

  def _stats_world(self, w):
    """The world whose statistics a step of world w is folded into: w (a list: worlds[i], not i)."""
    return w

  def _fold(self, w, cut=None):
    """World w ran a step (a reset, a load): what it left is folded into the statistics."""
    st = self.stats
    if st is None:
      return
    v = self._stats_world(w)
    if cut and st.open[v]:
      self._cut(v, cut)
    one = np.zeros(self.N, bool)
    one[v] = True
    shift = lambda kind: np.roll(self._target(kind), v - w, axis=0) if v != w else self._target(kind)
    events = shift(E.OBS_EVENTS) if st.columns or st.pairs else None
    before = int(st.episodes[v])
    step_type = shift(E.OBS_STEP_TYPE)
    st.step(step_type, shift(E.OBS_REWARD), events, ran=one)
    own = self._after_cut.get(v)
    if own is not None and int(step_type[v]) != 0:   # (the new episode's own sums, kept apart from the model's)
      own["returns"] = own["returns"] + np.asarray(shift(E.OBS_REWARD)[v], np.float64)
      own["length"] += 1
    elif own is not None and not cut:
      # (a FIRST with no cut in front: a restore put the world on a finished record and it restarted;
      # the episode that will finish is the one that begins here)
      own["returns"], own["length"] = np.zeros(self.P), 0
    if st.episodes[v] > before:
      if self._in_many >= 1:
        self.cover["an episode finishes inside step k >= 1 of a K-step call, statistics registered"] += 1
      if own is not None:
        self._finished_after_cut(v, self._after_cut.pop(v))

  def _cut(self, v, how):
    """An open episode of world v is cut by a reset or a load (`how`: "reset", "masked reset", "load").
    Where the cut writes FIRST the episode is dropped: `running` is zeroed and nothing of it is
    counted.  A masked reset or a load that does so is remembered with the world's totals as they
    are, for `_finished_after_cut`.  (A load of a finished row writes LAST: by the rule it closes
    the open episode, which is no dropped cut.)"""
    self._after_cut.pop(v, None)
    if how != "reset" and int(self._target(E.OBS_STEP_TYPE)[v]) == 0:
      st = self.stats
      self.cover["an open episode cut by a load or a masked reset, statistics registered"] += 1
      self._after_cut[v] = {"returns": np.zeros(self.P), "length": 0, "cut": st.running["returns"][v].copy(),
                            "cut_length": int(st.running["length"][v]), "total": st.total["returns"][v].copy(),
                            "total_length": int(st.total["length"][v]), "episodes": int(st.episodes[v])}

  def _finished_after_cut(self, v, own):
    """The episode world v began behind a cut has finished: `last` holds that episode alone and
    `total` grew by it alone — the cut one's sums are in neither."""
    st = self.stats
    assert st.last["returns"][v].tobytes() == own["returns"].tobytes() and st.last["length"][v] == own["length"], \
        f"world {v}: `last` is not the episode begun behind the cut"
    assert st.total["returns"][v].tobytes() == (own["total"] + own["returns"]).tobytes(), \
        f"world {v}: `total.returns` holds more than the episodes that finished (cut sums {own['cut']})"
    assert st.total["length"][v] == own["total_length"] + own["length"] and st.episodes[v] == own["episodes"] + 1, \
        f"world {v}: `total.length` / `episodes` count the cut episode (length {own['cut_length']})"
    self.cover["an episode finishes after an open one was cut"] += 1

  def stats_arrays(self):
    return None if self.stats is None else self.stats.arrays()

  def _reset_world(self, w):
    self._o[w].reset()
    self._log[w].append(("reset",))
    self._started[w] = True
    self._wrote_reset(w)

  def _reseed(self, w, seed):
    self._o[w].close()
    self._seed[w] = int(seed)
    self._o[w] = self._oracle(seed)
    self._log[w] = []
    self.exact[w] = True

  def reset(self, seeds=None, mask=None):
    self._begin()
    for w in range(self.N):
      if mask is not None and not mask[w]:
        continue
      if seeds is not None:
        self._reseed(w, seeds[w])
      self._reset_world(w)
      self._fold(w, cut="reset" if mask is None else "masked reset")
    self._end()

  def _start_row(self, w):
    """The row world w starts its next episode from (None: the level's own reset): `rows` is read at
    this moment, the end of the world's episode."""
    if self.starts is None:
      return None
    bank, rows = self.starts
    return bank[int(rows[w])] if rows[w] >= 0 else None

  def _restart(self, w):
    """World w, done, starts its next episode: the level's reset, or its registered row."""
    row = self._start_row(w)
    self._reset_world(w)   # (what the replaced auto-reset step left)
    if self._paused[w]:
      self.cover["paused on LAST, restarts in a later active step"] += 1
    self._step_starts.append((w, -1 if row is None else int(self.starts[1][w])))
    if row is not None:    # ... and on top of it what a load of the row writes
      self._become(w, row)
      self._wrote_load(w, row)
      if self._fresh:
        self.exact[w] = self._buf_exact[w] = False
      self.cover["registered start"] += 1
      if self._in_many >= 1:
        self.cover["registered start inside step k >= 1 of a K-step call"] += 1

  def _end_step(self):
    """After every single step (each of a K-step call's): what its restarts were."""
    taken = collections.Counter(r for _, r in self._step_starts if r >= 0)
    if any(n >= 2 for n in taken.values()) and any(r < 0 for _, r in self._step_starts) and self.starts is not None:
      self.cover["two worlds take one row in one step beside a world with -1"] += 1
    self._step_starts = []

  def _advance(self, w, entry, auto_reset=None):
    """One step of world w (see `_advance_world`), folded into the statistics if it ran."""
    ran = self._advance_world(w, entry, auto_reset)
    if ran:
      self._fold(w)
    return ran

  def _advance_world(self, w, entry, auto_reset=None):
    """One step of world w; `entry`: ("step", ids [P]) or ("fields", f [P, A]).  False: a world
    never reset, which runs nothing."""
    o = self._o[w]
    if not self._started[w]:
      return False
    if o.done:
      if self._auto_reset if auto_reset is None else auto_reset:
        self._restart(w)
      else:
        self._wrote_frozen(w)
      self._paused[w] = False
      if self._touched is not None:
        self._touched.add(w)
      return True
    self._paused[w] = False
    if self._touched is not None:
      self._touched.add(w)
    if entry[0] == "step":
      a = np.array(entry[1], np.int32)
      bad = (a < 0) | (a >= self.num_actions)
      a[bad] = 0
      self._bad[w] += int(bad.sum())
      cont = o.step(a)
    else:
      a = np.array(entry[1], np.int32)
      cont = o.step_fields(a)
    self._log[w].append((entry[0], a))
    self._write_transition(w, 1 if cont else 2, o.rewards(), o.events())
    self._write_record_kinds(w)
    self._buf_exact[w] = self.exact[w]
    if not cont and np.any(o.rewards() != 0):
      self.cover["non-zero reward on the step that leaves LAST"] += 1
    return True

  # -- a listed request: the masked request over all N worlds, gathered by entry
  def _owners(self, worlds):
    """[(entry, world)] of the entries that own their world: in range, and the lowest entry that
    names it."""
    seen, out = set(), []
    for i, w in enumerate(np.asarray(worlds).tolist()):
      if 0 <= w < self.N and w not in seen:
        seen.add(w)
        out.append((i, int(w)))
    return out

  def _stopped_at(self, i, w):
    """The element of `stopped` that entry i of a list, which names world w, reads and writes."""
    return w

  def _bad_ran(self, before):
    """What a bad entry's element of `ran` holds after the call: what it held."""
    return before

  def _listed(self, a, worlds, out, kw):
    worlds = np.asarray(worlds)
    if self._slots:
      raise E.EngineError("MpStepListed: refused with a rollout ring bound")   # (MP_ERR_UNSUPPORTED)
    M = len(worlds)
    assert worlds.ndim == 1 and 1 <= M <= self.N
    repeat, fields = kw.get("repeat"), kw.get("fields", False)
    K = int(repeat) if repeat is not None else a.shape[0]
    per = (self.P, self.num_action_fields) if fields else (self.P,)
    a = np.broadcast_to(a, (K, M) + per) if repeat is not None else a.reshape((K, M) + per)
    owners = self._owners(worlds)
    full = np.zeros((K, self.N) + per, np.int32)
    mask = np.zeros((K, self.N), bool)
    active = kw.pop("active", None)
    act = None if active is None else np.broadcast_to(np.asarray(active) != 0, (K, M))
    for i, w in owners:
      full[:, w] = a[:, i]
      mask[:, w] = True if act is None else act[:, i]
    stopped = kw.pop("stopped", None)
    inner = None
    if stopped is not None:
      inner = np.zeros(self.N, np.uint8)
      for i, w in owners:
        inner[w] = stopped[self._stopped_at(i, w)]
    bad = M - len(owners)
    if bad:
      self.cover["a listed call with a repeated and an out-of-range entry"] += 1
      if self.stats is not None:
        self.cover["a listed call with bad entries, statistics registered"] += 1
    restarts = self.cover["paused on LAST, restarts in a later active step"]
    name = tuple(worlds.tolist())
    if inner is not None and any(inner[w] and self._stop_list.get(w, name) != name for _, w in owners):
      self.cover["a listed until= call meets a stopped byte set under a different list"] += 1
    was = None if inner is None else inner.copy()
    taken = self.cover["registered start inside step k >= 1 of a K-step call"]
    self._credit = {w: i for i, w in owners}
    try:
      res = self.step_many(full, **dict(kw, repeat=None, active=mask, stopped=inner))
    finally:
      self._credit = None
    if self.cover["paused on LAST, restarts in a later active step"] > restarts:
      self.cover["a listed call names a world paused on LAST"] += 1   # (which restarted in it)
    if self.cover["registered start inside step k >= 1 of a K-step call"] > taken:
      self.cover["a listed call with a registered start inside step k >= 1"] += 1
    if stopped is not None:
      for i, w in owners:
        if inner[w] and not was[w]:
          self._stop_list[w] = name
        stopped[self._stopped_at(i, w)] = inner[w]
      res["stopped"] = stopped
    out = out or {}
    gathered = {}
    for key, value in res.items():
      if key == "stopped":
        gathered[key] = value
        continue
      by_entry = key in ("ran", "returns")
      if key == "states":
        rows = [[out[key][k][i] if key in out else None for i in range(M)] for k in range(K)]
        for i, w in owners:
          for k in range(K):
            rows[k][i] = value[k][w]
        gathered[key] = rows
        continue
      shape = ((M,) if by_entry else (K, M)) + value.shape[1 if by_entry else 2:]
      g = np.array(out[key]) if key in out else np.zeros(shape, value.dtype)
      assert g.shape == shape and g.dtype == value.dtype, (key, g.shape, shape, g.dtype, value.dtype)
      if key == "ran":
        owned = {i for i, _ in owners}
        for i in range(M):
          if i not in owned:
            g[i] = self._bad_ran(g[i])
      for i, w in owners:
        if by_entry:
          g[i] = value[w]
        else:
          g[:, i] = value[:, w]
      gathered[key] = g
    return gathered

  def step(self, actions, active=None, worlds=None):
    """active: a mask [N]; a world outside it is not touched (it writes nothing).
    worlds: a list of M worlds, actions [M, P]: the K = 1 listed request of step_many."""
    if worlds is not None:
      a = np.asarray(actions, np.int32)
      self.step_many(a[None], keep=(), active=active, worlds=worlds)
      return
    a = np.asarray(actions, np.int32).reshape(self.N, self.P)
    self._begin(masked=active is not None)
    for w in range(self.N):
      if active is None or active[w]:
        self._advance(w, ("step", a[w]))
      else:
        self._skipped(w)
    self._end_step()
    self._end()

  def step_fields(self, fields, active=None):
    """active: as step()'s (the engine's form of it is the K = 1 request of step_many)."""
    f = np.asarray(fields, np.int32).reshape(self.N, self.P, self.num_action_fields)
    self._begin(masked=active is not None)
    for w in range(self.N):
      if active is None or active[w]:
        self._advance(w, ("fields", f[w]))
      else:
        self._skipped(w)
    self._end_step()
    self._end()

  def _many_auto_reset(self):
    return self._auto_reset

  _in_many = -1   # the step of the K-step call that is running (-1: none)

  def _skipped(self, w, by_mask=True):
    """World w skips a step (masked out or stopped): it is not touched."""
    if by_mask and self._started[w] and self._o[w].done:
      self._paused[w] = True

  def _stops(self, w, stop):
    """The reason bits that stop world w after a step it ran (0: it goes on)."""
    paid = bool((self._target(E.OBS_REWARD)[w] != 0).any())
    last = int(self._target(E.OBS_STEP_TYPE)[w]) == 2
    return (E.MP_STOP_LAST if (stop & E.MP_STOP_LAST) and last else 0) | \
           (E.MP_STOP_REWARD if (stop & E.MP_STOP_REWARD) and paid else 0)

  def _discount(self, g, gamma, k, w):
    """The weight of the next step world w runs, after one that ran as step k of the call."""
    return g * np.float64(gamma)

  def step_many(self, actions, *, repeat=None, fields=False, events=False, observations=(),
                keep=("reward", "collective_reward", "step_type", "discount"), active=None,
                until=None, stop=None, stopped=None, returns=False, gamma=1.0, states=False, hashes=False,
                worlds=None, out=None):
    """The loop over single steps as ONE submission; returns the per-step rows under the keys of
    `engine.Engine.step_many` (a row of LAYER is the function of the records after that step).
    active: a mask [K, N] or [N]: world w runs step k only where it is non-zero.
    until (names, as the engine takes them) or stop (MP_STOP_* bits): a world that a step leaves on
    LAST, or pays, skips the rest of the call.  stopped: the caller's array [N], read and written in
    place (None: a new one).  With any of until / stop / stopped / returns the result gains
    "stopped" and "ran" (the steps each world ran), and with returns "returns" [N, P]: g = 1; per
    step that ran ret = ret + g * r; g = g * gamma, each rounded in float64 on its own.
    states: "states", a list of K lists of the N worlds' rows (`_row`) after every step — each is a
    bank like save_worlds'.  hashes: "hashes" int64 [K, N], `hash_states` of those rows."""
    a = np.asarray(actions, np.int32)
    if worlds is not None:
      # worlds: a list of M worlds; everything per world has M columns, by entry, but `stopped` [N];
      # out: what a bad entry's elements of the rows, `ran` and `returns` held before the call
      return self._listed(a, worlds, out, dict(repeat=repeat, fields=fields, events=events, observations=observations,
                                               keep=keep, active=active, until=until, stop=stop, stopped=stopped,
                                               returns=returns, gamma=gamma, states=states, hashes=hashes))
    K = int(repeat) if repeat is not None else a.shape[0]
    if stop is None:
      names = () if until is None else (until,) if isinstance(until, str) else tuple(until)
      stop = sum(E.STOP_NAMES[n] for n in set(names))
    stopping = bool(stop) or until is not None or stopped is not None or returns is not False
    mask = None if active is None else np.broadcast_to(np.asarray(active) != 0, (K, self.N))
    names = [k for k in E.STEP_MANY_KINDS if k in tuple(keep) or (k == "events" and events)]
    keys = names + [int(k) for k in observations]
    rows = {key: [] for key in keys}
    state_rows, hash_rows = [], []
    stopped = np.zeros(self.N, np.uint8) if stopped is None else stopped
    ran = np.zeros(self.N, np.int32)
    ret = np.zeros((self.N, self.P), np.float64)
    g = np.ones(self.N, np.float64)
    self._begin(masked=mask is not None or stopping)
    for k in range(K):
      block = a if repeat is not None else a[k]
      self._in_many = k
      for w in range(self.N):
        if stopping and stopped[w]:
          self._skipped(w, by_mask=False)
          continue
        if mask is not None and not mask[k, w]:
          self._skipped(w)
          continue
        if not self._advance(w, ("fields" if fields else "step", block[w]), auto_reset=self._many_auto_reset()):
          continue
        ran[w] += 1
        ret[w] = ret[w] + g[w] * self._target(E.OBS_REWARD)[w]
        g[w] = self._discount(g[w], gamma, k, w)
        if returns is not False and float(gamma) != 1.0 and ran[w] >= 2 and np.any(self._target(E.OBS_REWARD)[w] != 0):
          self.cover["returns with gamma != 1 paid after the first step the world ran"] += 1
        reason = self._stops(w, stop)
        if reason:
          stopped[w] = reason
          if self._credit is None:
            self._stop_list.pop(w, None)   # (set by a call without a list)
          if k + 1 < K and (mask is None or mask[k + 1:, w].any()):
            for bit, name in ((E.MP_STOP_LAST, "LAST"), (E.MP_STOP_REWARD, "REWARD")):
              if reason & bit:
                self.cover[f"stopped by {name} with steps left to skip"] += 1
      for key in keys:
        kind = E.STEP_MANY_NAMES.get(key, key)
        rows[key].append(self.view_value(kind) if kind == E.OBS_LAYER else self._target(kind).copy())
      if states:
        state_rows.append([self._row(w) for w in range(self.N)])
      if hashes:
        hash_rows.append([self._hash_of(self._o[w]) for w in range(self.N)])
      self._end_step()
    self._in_many = -1
    self._end()
    out = {key: np.stack(v) for key, v in rows.items()}
    if states:
      out["states"] = state_rows
    if hashes:
      out["hashes"] = np.array(hash_rows, np.int64)
    if stopping:
      out.update(stopped=stopped, ran=ran)
      if returns is not False:
        out["returns"] = ret
    return out

  # -- episode starts
  def set_episode_starts(self, bank, rows, fresh=False):
    """From now on a world that auto-resets starts from row rows[w] of `bank` (-1: the level's
    reset); `rows` is the caller's array, read when a world's episode ends.  fresh=True is not
    modelled (the oracle takes no state): such a world is the fresh=False one here, and the
    program runner stops comparing it."""
    assert self._auto_reset, "a registration needs auto_reset"
    self.starts, self._fresh = (bank, rows), bool(fresh)

  def clear_episode_starts(self):
    self.starts = None

  # -- world states
  def _row(self, w):
    return {"seed": self._seed[w], "log": list(self._log[w]), "finished": self._o[w].done,
            "started": self._started[w], "exact": bool(self.exact[w])}

  def _replay(self, row):
    """A fresh oracle that `row`'s log was replayed into."""
    o = self._oracle(row["seed"])
    for entry in row["log"]:
      if entry[0] == "reset":
        o.reset()
      elif entry[0] == "step":
        o.step(entry[1])
      else:
        o.step_fields(entry[1])
    assert o.done == row["finished"], "a replayed log did not end where the live world did"
    return o

  def _become(self, w, row):
    """World w becomes a copy of `row`: its log replayed into a fresh oracle."""
    o = self._replay(row)
    self._o[w].close()
    self._o[w], self._seed[w], self._log[w] = o, row["seed"], list(row["log"])
    self._started[w] = row["started"]
    self.exact[w] = row.get("exact", True)
    self._paused[w] = False

  def save_worlds(self, worlds=None):
    return [self._row(int(w)) for w in (range(self.N) if worlds is None else np.asarray(worlds))]

  def _source_row(self, rows, src, w):
    """The row world w takes in a load (None: left alone)."""
    return rows[int(src[w])] if src[w] >= 0 else None

  def load_worlds(self, rows, src):
    src = np.asarray(src)
    assert src.shape == (self.N,) and src.max() < len(rows) and src.min() >= -1
    self._begin()
    for w in range(self.N):
      row = self._source_row(rows, src, w)
      if row is None:
        continue
      self._become(w, row)
      self._wrote_load(w, row)
      self._fold(w, cut="load")
    self._end()

  def snapshot(self):
    return [self._row(w) for w in range(self.N)], self._bad.copy()

  def restore(self, snap):
    """mp_restore puts the records back (counters included: they live in the records); it is no
    launch, so no output buffer, bound view or ring slot is written."""
    rows, bad = snap
    if self.stats is not None:
      self.cover["restore while statistics are registered"] += 1
    for w, row in enumerate(rows):
      if self.units and self.row_key(row) != self.row_key(self._row(w)):
        self._restored[w] = True
      self._become(w, row)
    self._bad = bad.copy()

  # -- reading saved states: nothing of the engine's is written
  @staticmethod
  def row_key(row):
    """What makes two rows the same state: the seed and the log."""
    return (int(row["seed"]), tuple((e[0],) + tuple(np.asarray(x).tobytes() for x in e[1:]) for e in row["log"]))

  def _replayed(self, row):
    """The oracle of `row`, replayed once per distinct row and kept."""
    key = self.row_key(row)
    if key not in self._replays:
      self._replays[key] = self._replay(row)
    return self._replays[key]

  def state_value(self, rows, kind):
    """Record-function `kind` of bank rows `rows` (a list): [len(rows), ...]."""
    return self._kind_of(kind, [self._replayed(r) for r in rows])

  def view_of(self, rows, players, kind):
    """Per-player `kind` of player players[i] of rows[i]: [len(rows), ...]."""
    return self.state_value(rows, kind)[np.arange(len(rows)), np.asarray(players)]

  def row_dumps(self, rows):
    return [self._replayed(r).dump() for r in rows]

  def observe_states(self, bank, kind, rows=None):
    return self.state_value(bank if rows is None else [bank[int(i)] for i in np.asarray(rows)], kind)

  def observe_views(self, bank, kind, players, rows=None):
    players = np.asarray(players)
    picked = [bank[int(i)] for i in (range(len(players)) if rows is None else np.asarray(rows))]
    return self.view_of(picked, players, kind)

  @staticmethod
  def _hash_of(o):
    """The model's stand-in for the engine's state hash (equal for equal states of one model)."""
    grid, avatars, glob = o.dump()
    h = zlib.crc32(np.ascontiguousarray(avatars).tobytes(), zlib.crc32(np.ascontiguousarray(grid).tobytes()))
    return np.int64(h | (zlib.adler32(np.ascontiguousarray(glob).tobytes()) << 32) & 0x7FFFFFFF00000000)

  def hash_worlds(self, planes=None, fields=None):
    return np.array([self._hash_of(o) for o in self._o], np.int64)

  def hash_states(self, bank, rows=None, planes=None, fields=None):
    picked = bank if rows is None else [bank[int(i)] for i in np.asarray(rows)]
    return np.array([self._hash_of(self._replayed(r)) for r in picked], np.int64)

  # -- reading
  def observe_host(self, kind):
    if kind in VIEW_KINDS:
      return self.view_value(kind)
    return np.array(self._last(kind))

  def dump(self):
    d = [o.dump() for o in self._o]
    return tuple(np.stack([x[i] for x in d]) for i in range(3))

  def counters(self):
    return {"bad_actions": int(self._bad.sum())}

  def fault_words(self):
    return np.zeros(64, np.uint32)
