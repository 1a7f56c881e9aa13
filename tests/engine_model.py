"""Test infrastructure: a plain Python model of `engine.Engine` made of CPU oracles, for the
program tests (tests/api_programs.py).  It answers the calls a learner or a planner makes —
reset, masked reset, re-seed, step, step_fields, step_many with rows, save_worlds / load_worlds,
snapshot / restore, bind / bind_ring / unbind — and says what every output of include/mp_engine.h
it models must hold afterwards.

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
  * mp_counters' bad_actions (kept by the destination of a load, rewound by a restore).
It says nothing about the kinds under the carry rule that no record holds (AUX0 - AUX4, ZAP_MATRIX,
INTERACTION_INVENTORIES, INTERACTION_REWARDS, MATRIX_CUMULANTS): the twin engine of
api_programs.run_program covers those."""
import numpy as np

from meltingpot_amd import engine as E
from oracle import oracle as oracle_lib
from oracle_engine import OracleBatchEngine
import util

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

  # -- the interface the runner drives on both sides (numpy in, numpy out here)
  def to_device(self, a):
    return np.asarray(a)

  def _oracle(self, seed):
    return oracle_lib.Oracle(self.pack_bytes, int(seed), self._num_players)

  def close(self):
    for o in self._o:
      o.close()
    self._o = []

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

  def _frozen_rewards(self, w):
    return np.zeros(self.P)

  def _wrote_frozen(self, w):
    self._write_transition(w, 2, self._frozen_rewards(w), [])

  # -- submissions
  def _begin(self):
    if self._slots:
      self._slot = self._cursor % self._slots
      self._cursor += 1

  def view_value(self, kind):
    """A view kind as the function of the records it is, for every world."""
    if kind == E.OBS_WORLD_RGB:
      return E.pool_rgb(self._of_records(kind, self._o), self.world_pool)
    if kind == E.OBS_LAYER:
      return np.stack([np.stack([o.layer_view(p) for p in range(self.P)]) for o in self._o])
    rgb = self._of_records(E.OBS_RGB, self._o)
    if kind == E.OBS_RGB:
      return rgb
    return E.pool_rgb(rgb, {v: k for k, v in E.OBS_RGB_POOL.items()}[kind])

  def _end(self):
    """Every bound view is drawn by the submission, from all the records."""
    for kind, out in self._bound.items():
      if kind in VIEW_KINDS:
        (out[self._slot] if kind in self._ring_kinds else out)[...] = self.view_value(kind)

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

  def reset(self, seeds=None, mask=None):
    self._begin()
    for w in range(self.N):
      if mask is not None and not mask[w]:
        continue
      if seeds is not None:
        self._reseed(w, seeds[w])
      self._reset_world(w)
    self._end()

  def _advance(self, w, entry, auto_reset=None):
    """One step of world w; `entry`: ("step", ids [P]) or ("fields", f [P, A])."""
    o = self._o[w]
    if not self._started[w]:
      return
    if o.done:
      if self._auto_reset if auto_reset is None else auto_reset:
        self._reset_world(w)
      else:
        self._wrote_frozen(w)
      return
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

  def step(self, actions):
    a = np.asarray(actions, np.int32).reshape(self.N, self.P)
    self._begin()
    for w in range(self.N):
      self._advance(w, ("step", a[w]))
    self._end()

  def step_fields(self, fields):
    f = np.asarray(fields, np.int32).reshape(self.N, self.P, self.num_action_fields)
    self._begin()
    for w in range(self.N):
      self._advance(w, ("fields", f[w]))
    self._end()

  def _many_auto_reset(self):
    return self._auto_reset

  def step_many(self, actions, *, repeat=None, fields=False, events=False, observations=(),
                keep=("reward", "collective_reward", "step_type", "discount")):
    """The loop over single steps as ONE submission; returns the per-step rows under the keys of
    `engine.Engine.step_many` (a row of LAYER is the function of the records after that step)."""
    a = np.asarray(actions, np.int32)
    K = int(repeat) if repeat is not None else a.shape[0]
    names = [k for k in E.STEP_MANY_KINDS if k in tuple(keep) or (k == "events" and events)]
    keys = names + [int(k) for k in observations]
    rows = {key: [] for key in keys}
    self._begin()
    for k in range(K):
      block = a if repeat is not None else a[k]
      for w in range(self.N):
        self._advance(w, ("fields" if fields else "step", block[w]), auto_reset=self._many_auto_reset())
      for key in keys:
        kind = E.STEP_MANY_NAMES.get(key, key)
        rows[key].append(self.view_value(kind) if kind == E.OBS_LAYER else self._target(kind).copy())
    self._end()
    return {key: np.stack(v) for key, v in rows.items()}

  # -- world states
  def _row(self, w):
    return {"seed": self._seed[w], "log": list(self._log[w]), "finished": self._o[w].done,
            "started": self._started[w]}

  def _become(self, w, row):
    """World w becomes a copy of `row`: its log replayed into a fresh oracle."""
    o = self._oracle(row["seed"])
    for entry in row["log"]:
      if entry[0] == "reset":
        o.reset()
      elif entry[0] == "step":
        o.step(entry[1])
      else:
        o.step_fields(entry[1])
    assert o.done == row["finished"], "a replayed log did not end where the live world did"
    self._o[w].close()
    self._o[w], self._seed[w], self._log[w] = o, row["seed"], list(row["log"])
    self._started[w] = row["started"]

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
      if row["finished"]:   # loads finished: what a frozen world reports
        self._write_transition(w, 2, np.zeros(self.P), [])
      else:                 # as a reset writes them
        self._write_transition(w, 0, np.zeros(self.P), self._reset_events)
      self._write_record_kinds(w)
    self._end()

  def snapshot(self):
    return [self._row(w) for w in range(self.N)], self._bad.copy()

  def restore(self, snap):
    """mp_restore puts the records back (counters included: they live in the records); it is no
    launch, so no output buffer, bound view or ring slot is written."""
    rows, bad = snap
    for w, row in enumerate(rows):
      self._become(w, row)
    self._bad = bad.copy()

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
