"""Host-side mirror of the reference's public substrate API for the hot path.

Same names, argument meaning and error behaviour as
  meltingpot/substrate.py:41-113           SUBSTRATES, get_config, build
  meltingpot/utils/substrates/substrate.py:50-104   Substrate.reset/step/
      observation_spec/action_spec/reward_spec/discount_spec/close
so that a training loop written against `meltingpot.substrate.build(name,
roles=...)` can switch to `meltingpot_amd.substrate.build(name, roles=...,
num_worlds=N)`.  Everything that computes lives in libmp_engine.so; this module
only validates arguments, owns the observation tensors and shapes the returned
timesteps.  (`dm_env` is not a dependency: `TimeStep` / `StepType` / the spec
classes below duck-type it — same field names, `.first()/.mid()/.last()`,
`spec.validate()`, `spec.minimum/.maximum/.num_values`.)

Two result shapes:
  * num_worlds == 1 (default), batched=False: exactly the reference's —
    `TimeStep(step_type, reward=[P x float64], discount=float,
    observation=[P x {"RGB", "READY_TO_SHOOT",
    "NUM_OTHERS_WHO_CLEANED_THIS_STEP", "COLLECTIVE_REWARD", "WORLD.RGB"}])` with
    numpy leaves (clean_up.py:813-832, collective_reward_wrapper.py:25);
  * batched: every leaf gains a leading [N] axis and is a torch tensor that
    lives on the GPU the engine runs on (no host copy, no sync).
"""

from __future__ import annotations

import dataclasses
import enum
import fnmatch
import math
import os
from typing import Any, Callable, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from meltingpot_amd import engine as engine_lib

# --------------------------------------------------------------------------
# dm_env duck types


class StepType(enum.IntEnum):
  FIRST = 0
  MID = 1
  LAST = 2

  def first(self) -> bool:
    return self is StepType.FIRST

  def mid(self) -> bool:
    return self is StepType.MID

  def last(self) -> bool:
    return self is StepType.LAST


class TimeStep(NamedTuple):
  step_type: Any
  reward: Any
  discount: Any
  observation: Any

  def first(self) -> bool:
    return self.step_type == StepType.FIRST

  def mid(self) -> bool:
    return self.step_type == StepType.MID

  def last(self) -> bool:
    return self.step_type == StepType.LAST


class RolloutTimeStep(TimeStep):
  """A TimeStep of a substrate built with `rollout_length=T`: the same four fields
  (it IS a TimeStep: unpacking, `_replace`, `.first()` all work) plus `.slot`, the
  index of this step along the leading axis of `Substrate.rollout`'s [T, N, ...]
  tensors.  Its leaves are views of that slot: they stay valid until the substrate has
  been stepped T more times."""
  slot: int = -1

  def _replace(self, **kwargs):   # (a NamedTuple's _replace builds a fresh tuple: carry the slot)
    out = super()._replace(**kwargs)
    out.slot = self.slot
    return out


class StepManyResult(NamedTuple):
  """What `Substrate.step_many` returns: the transitions of all K steps as device tensors
  stacked along a leading K, and the TimeStep of the last one."""
  step_type: Any           # int32 [K, N]
  reward: Any              # float64 [K, N, P]
  discount: Any            # float64 [K, N]
  collective_reward: Any   # float64 [K, N]
  events: Any              # int32 [K, N, EVENT_ROWS, 4] (events=True) or None
  timestep: TimeStep       # what the K-th step() would have returned


class StepManyTrajectory(StepManyResult):
  """What `Substrate.step_many` returns with `observations=`: the same six fields (it IS a
  StepManyResult) plus `.observation`, a dict from each asked leaf's name to its per-step
  device tensor [K, N, ...]: row k is the leaf after step k of the loop of `step`.  Like
  `RolloutTimeStep.slot`, `.observation` is an attribute beside the tuple's fields: `_replace`
  carries it; `_make`, slicing, `tuple()` and pickling give a plain tuple without it.
  With `states=True` it also has `.states`: the worlds' records after every step as a
  `WorldStates` of K x N rows (step k of world w is row k * N + w), a view of the engine's
  uint8 [K, N, S] tensor; carried like `.observation` (None when not asked for).
  With `hashes=True` it has `.hashes`: int64 [K, N], the state hash (`Substrate.hash_worlds`) of
  every world after every step; carried likewise."""
  observation: Any = None
  states: Any = None
  hashes: Any = None

  def _replace(self, **kwargs):   # (a NamedTuple's _replace builds a fresh tuple: carry the dict)
    out = super()._replace(**kwargs)
    out.observation = self.observation
    out.states = self.states
    out.hashes = self.hashes
    return out


class StepManyUntil(StepManyTrajectory):
  """What `Substrate.step_many` returns with `until=`, `stopped=` or `returns=`: a
  `StepManyTrajectory` (its `.observation` is empty, `.states` and `.hashes` None, where they were
  not asked for) plus `.ran`, int32 [N]: the steps each world ran in this call; `.stopped`, uint8
  [N]: 0, or the reason bits of the step that stopped the world (1: it left the world on LAST, 2:
  it paid a player), the tensor handed in where one was; and `.returns`, float64 [N, P]: the
  discounted sum of the rewards of the steps that ran (None when not asked for).  Carried like
  `.observation`."""
  ran: Any = None
  stopped: Any = None
  returns: Any = None

  def _replace(self, **kwargs):
    out = super()._replace(**kwargs)
    out.ran = self.ran
    out.stopped = self.stopped
    out.returns = self.returns
    return out


_FIVE_NAMES = {kind: name for name, kind in engine_lib.STEP_MANY_NAMES.items()}


def _many_result(r, leaves, timestep, fingerprint=None):
  """The result of a step_many call from the engine's dict `r` (`leaves`: asked name -> kind;
  `fingerprint`: the engine's, when the call asked for the per-step states)."""
  fields = (r["step_type"], r["reward"], r["discount"], r["collective_reward"], r.get("events"), timestep)
  if not leaves and fingerprint is None and r.get("hashes") is None and "ran" not in r:
    return StepManyResult(*fields)
  if "ran" in r:   # (a call with until=, stopped= or returns=)
    out = StepManyUntil(*fields)
    out.ran, out.stopped, out.returns = r["ran"], r["stopped"], r.get("returns")
  else:
    out = StepManyTrajectory(*fields)
  # (a leaf that is one of the five per-step kinds is the tensor the call stacks anyway)
  out.observation = {n: r[_FIVE_NAMES[k]] if k in _FIVE_NAMES else r[k] for n, k in leaves.items()}
  if fingerprint is not None:
    rows = r["states"]
    out.states = WorldStates(rows.view(rows.shape[0] * rows.shape[1], rows.shape[2]), fingerprint)
  out.hashes = r.get("hashes")
  return out


def _hash_fields(fields):
  """`fields` of a hash call with `StateFields`' names (avatar_x, ...) as the tail's own (ax, ...)."""
  if fields is None:
    return None
  if isinstance(fields, str):
    fields = (fields,)
  c_names = {py: c for c, py in _FIELD_NAMES.items()}
  return tuple(c_names.get(f, f) for f in fields)


def _step_mask(t, active, lengths, K: int, N: int, device, ring: bool):
  """The mask of a masked step / step_many call as a device tensor the engines read in place
  ([K, N] or [N], uint8 or bool), or None for an unmasked call.  `lengths`: int [N], world w runs
  steps 0 .. lengths[w] - 1 — arange(K)[:, None] < lengths[None], built on the device without a
  synchronisation.  `ring`: the substrate was built with rollout_length=T."""
  if active is None and lengths is None:
    return None
  if active is not None and lengths is not None:
    raise ValueError("give either active= or lengths=, not both")
  if ring:
    raise ValueError("a masked step cannot write a rollout ring (rollout_length=T): a slot row of a skipped "
                     "world has no defined content; build the substrate without rollout_length")
  if lengths is not None:
    n = lengths if isinstance(lengths, t.Tensor) else t.as_tensor(np.asarray(lengths))
    if n.dtype.is_floating_point or n.dtype == t.bool or tuple(n.shape) != (N,):
      raise ValueError(f"lengths= must be an int tensor of shape ({N},) (got {n.dtype} {tuple(n.shape)})")
    return t.arange(K, device=device)[:, None] < n.to(device)[None]
  mask, _ = engine_lib.check_step_active(active, K, N)
  if isinstance(mask, np.ndarray):
    mask = t.from_numpy(mask).to(device)
  return mask


def _step_list(t, worlds, lengths, batched: bool, N: int, P: int, ring: bool) -> Optional[int]:
  """The worlds= list of a step / step_many call: None for a call without it, else M, its number
  of entries (the engine reads or uploads the list itself).  `ring`: the substrate was built with
  rollout_length=T."""
  if worlds is None:
    return None
  if not batched:
    raise ValueError("worlds= selects worlds of a batch: build the substrate with num_worlds > 1")
  if ring:
    raise ValueError("a call with worlds= cannot write a rollout ring (rollout_length=T): a slot row of an "
                     "unlisted world has no defined content; build the substrate without rollout_length")
  return engine_lib.check_step_listed(worlds, N, P, lengths=lengths)


def _step_until(t, until, stopped, returns, gamma, N: int, P: int, device, ring: bool,
                entries: Optional[int] = None):
  """The stop arguments of a step_many call as the engines take them: None for a call without
  them, else the dict of `until`, `stopped`, `returns`, `gamma` and `ran` — the [N] / [N, P] device
  tensors allocated here where the caller gave none, so that the members of a mixture write their
  rows of ONE tensor each.  `ring`: the substrate was built with rollout_length=T.  `entries`: M of
  a call with worlds=, whose `returns` and `ran` are by entry ([M, P], [M]; `stopped` stays [N])."""
  if until is None and stopped is None and (returns is None or returns is False):
    if float(gamma) != 1.0:
      raise ValueError("gamma= goes with returns=")
    return None
  if ring:
    raise ValueError("a call that stops worlds cannot write a rollout ring (rollout_length=T): a slot row of "
                     "a stopped world has no defined content; build the substrate without rollout_length")
  if isinstance(until, str):
    until = (until,)
  elif until is not None:
    until = tuple(until)
  if entries is None:
    entries = N
    engine_lib.check_step_until(N, P, until=until, stopped=stopped, returns=returns, gamma=gamma, device=device)
  else:
    engine_lib.check_step_until(N, P, until=until, stopped=stopped, gamma=gamma, device=device)
    engine_lib.check_step_until(entries, P, returns=returns, device=device)
  if stopped is None:
    stopped = t.zeros((N,), dtype=t.uint8, device=device)
  if returns is True:
    returns = t.empty((entries, P), dtype=t.float64, device=device)
  return {"until": until, "stopped": stopped, "returns": returns, "gamma": float(gamma),
          "ran": t.empty((entries,), dtype=t.int32, device=device)}


def _until_slice(stop, out, off: int, n: int):
  """(`more`, `out`) of one member's launch: its rows [off, off + n) of the stop tensors of
  `_step_until`, in place."""
  if stop is None:
    return {}, out
  more = {"until": stop["until"], "stopped": stop["stopped"][off:off + n], "gamma": stop["gamma"],
          "returns": False if stop["returns"] is None or stop["returns"] is False else stop["returns"][off:off + n]}
  out = dict(out or {})
  out["ran"] = stop["ran"][off:off + n]
  return more, out


def _many_actions(t, actions, repeat, N: int, P: int, num_actions: Optional[int]):
  """`actions` of a step_many call as the engine takes them: an int32 device tensor (as it is:
  it may be a column slice) or a host array; shape-checked, range-checked when asked."""
  if isinstance(actions, t.Tensor) and actions.is_cuda:
    a = actions.to(t.int32)
    K = engine_lib.check_step_many(a.shape, a.dtype, N, P, repeat=repeat)
    if num_actions is not None and bool(((a < 0) | (a >= num_actions)).any()):
      raise ValueError(f"actions must be in [0, {num_actions})")
  else:
    a = np.asarray(actions)
    K = engine_lib.check_step_many(a.shape, a.dtype, N, P, repeat=repeat)
  return a, K


class WorldStates:
  """Saved worlds (`Substrate.save_state`): `data`, a uint8 [M, S] tensor on the engine's device
  whose row i is one world's whole record, and `fingerprint`, the engine's state fingerprint
  (MP_STATES_FINGERPRINT) — rows load into any substrate of the same level, player count and
  roles (`Substrate.load_state`), of any num_worlds.  `states[idx]` selects rows (an int, a
  slice, a sequence or an integer tensor) and is again a WorldStates.
  `edited` says that somebody may have written into `data` through `Substrate.state_fields`:
  `load_state` then checks the rows it loads.  The constructor and everything the engine hands
  out leave it False; `states[idx]` carries it along."""

  def __init__(self, data, fingerprint: int):
    import torch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
      raise ValueError(f"WorldStates.data must be a uint8 tensor (got {getattr(data, 'dtype', type(data))})")
    if data.dim() != 2 or data.shape[0] < 1 or data.shape[1] < 1:
      raise ValueError(f"WorldStates.data must have shape [M, S] with M, S >= 1 (got {tuple(data.shape)})")
    fingerprint = int(fingerprint)
    if not 0 <= fingerprint < (1 << 64):
      raise ValueError(f"a state fingerprint is a 64-bit unsigned value (got {fingerprint})")
    self.data = data.contiguous()
    self.fingerprint = fingerprint
    self.edited = False

  def __len__(self) -> int:
    return int(self.data.shape[0])

  @property
  def row_bytes(self) -> int:
    return int(self.data.shape[1])

  def __getitem__(self, idx) -> "WorldStates":
    import torch
    if isinstance(idx, (int, np.integer)):
      rows = self.data[int(idx)].unsqueeze(0)
    elif isinstance(idx, slice):
      rows = self.data[idx]
    else:
      index = idx if isinstance(idx, torch.Tensor) else torch.as_tensor(np.asarray(idx, np.int64))
      if index.dtype == torch.bool or index.dim() != 1:
        raise ValueError("WorldStates rows are selected by an int, a slice or a 1-D list of ints")
      rows = self.data[index.to(self.data.device, torch.int64)]
    out = WorldStates(rows, self.fingerprint)
    out.edited = self.edited
    return out

  def check(self, fingerprint: int, row_bytes: int):
    """ValueError unless these rows were saved by an engine with this fingerprint and row size."""
    if self.fingerprint != int(fingerprint):
      raise ValueError(f"world states of fingerprint {self.fingerprint:016x} do not fit this substrate "
                       f"({int(fingerprint):016x}): another level, player count, roles or library")
    if self.row_bytes != int(row_bytes):
      raise ValueError(f"world states have rows of {self.row_bytes} bytes, this substrate {row_bytes}")

  def __repr__(self):
    return f"WorldStates({len(self)} x {self.row_bytes} B, fingerprint {self.fingerprint:016x})"


# what Python calls the tail fields whose C names are abbreviations (every other field keeps its
# C name); offsets, sizes and counts are the library's (engine_lib.StateLayout.fields)
_FIELD_NAMES = {"ax": "avatar_x", "ay": "avatar_y", "aori": "orientation", "aalive": "alive"}


class SubstrateStateLayout:
  """`Engine.state_layout()` plus the pack's names: `layer_names` in plane order (the L render
  planes), `state_names` by state id with `state_id(name)`, `state_layers[state]` (the plane a
  state lives in, -1: never on the map), `avatar_states[p]` = (alive_state, wait_state) of player p, `avatar_layer`, `hidden_planes` (the level's private planes behind
  the render planes), `sprite_names` by sprite index.  Every attribute of the engine's layout (H, W, L, P, nstates, grid_planes,
  grid_pad, world_stride, fields, fingerprint, describe(), ...) is reachable here too."""

  def __init__(self, layout, tables):
    self._layout = layout
    split = lambda name: tuple(n.decode() for n in bytes(tables[name]).split(b"\0")[:-1])
    self.layer_names = split("layer_names")[:layout.L]
    self.state_names = split("state_names")[:layout.nstates]
    self.sprite_names = split("sprite_names")   # (by sprite index: id i of "LAYER" shows sprite i - 1)
    self.state_layers = tuple(int(v) for v in tables["state_layer"][:layout.nstates])   # (-1: never on the map)
    alive = [int(v) for v in tables["avatar_alive_state"]]
    wait = [int(v) for v in tables["avatar_wait_state"]]
    self.avatar_states = tuple((alive[p], wait[p]) for p in range(layout.P))
    self.hidden_planes = layout.grid_planes - layout.L

  def __getattr__(self, name):
    return getattr(self._layout, name)

  def state_id(self, name: str) -> int:
    """The state id (a plane byte) of the state called `name` ("avatar1.player1", ...)."""
    try:
      return self.state_names.index(name)
    except ValueError:
      raise KeyError(f"no state {name!r} in this pack") from None


class StateFields:
  """Named views of the rows of a `WorldStates` (`Substrate.state_fields`).  Every attribute is a
  view that shares memory with `states.data` — reading costs nothing, writing edits the rows:
    grid                 uint8 [R, grid_planes, H, W]: state ids per plane and cell, the level's
                         hidden planes behind the L render planes
    avatar_x, avatar_y, orientation, alive, and the other per-avatar byte arrays of the tail
                         (ztimer, ctimer, flag0, flag1, freeze, removal, aflags, nozap, level,
                         tsince)   uint8 [R, P]
    achange              int32 [R, P]
    step, frame, done, cont, aux_count, group_change, episode, started, reward_fx, orders_step
                         int32 [R]
    seed                 int64 [R] (the bit pattern of the u64)
    ctr                  int32 [R, 8]
    next_orders          int16 [R, P]
  `names` lists them.  What each field means is the record's own documentation (DESIGN.md §3.9;
  csrc/mp_common.h: WorldTail)."""

  def __init__(self, data, layout):
    import torch
    R = int(data.shape[0])
    if data.dim() != 2 or int(data.shape[1]) != layout.world_stride or not data.is_contiguous():
      raise ValueError(f"state rows must be a contiguous uint8 [R, {layout.world_stride}] tensor")
    dtypes = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    planes = layout.grid_planes * layout.H * layout.W
    self.grid = data[:, :planes].view(R, layout.grid_planes, layout.H, layout.W)
    names = ["grid"]
    for cname, (off, elem, count) in layout.fields.items():
      lo = layout.grid_pad + off
      # (a column slice of the rows reinterpreted: the row stride and every offset are multiples
      # of the element size)
      v = data[:, lo:lo + elem * count].view(dtypes[elem])
      if count == 1:
        v = v[:, 0]
      elif count == 16:   # a per-avatar array: the avatars that play
        v = v[:, :layout.P]
      name = _FIELD_NAMES.get(cname, cname)
      setattr(self, name, v)
      names.append(name)
    self.names = tuple(names)


def _resolve_check(states, check: Optional[bool]) -> bool:
  """load_state's `check`: None means "iff the rows may have been edited"."""
  if check is None:
    return bool(getattr(states, "edited", False))
  if not isinstance(check, (bool, np.bool_)):
    raise ValueError(f"check must be None, True or False (got {check!r})")
  return bool(check)


class Array:
  """dm_env.specs.Array look-alike."""

  def __init__(self, shape, dtype, name=None):
    self.shape = tuple(shape)
    self.dtype = np.dtype(dtype)
    self.name = name

  def validate(self, value):
    value = np.asarray(value)
    if value.shape != self.shape:
      raise ValueError(f"{self.name}: shape {value.shape} != {self.shape}")
    if value.dtype != self.dtype:
      raise ValueError(f"{self.name}: dtype {value.dtype} != {self.dtype}")
    return value

  def replace(self, **kw):
    out = self.__class__.__new__(self.__class__)
    out.__dict__.update(self.__dict__)
    out.__dict__.update(kw)
    return out

  def __repr__(self):
    return f"{type(self).__name__}(shape={self.shape}, dtype={self.dtype}, name={self.name!r})"

  # dm_env specs compare by value — shape and dtype (and bounds), NOT the name
  # (dm_env/specs.py Array.__eq__, BoundedArray.__eq__): the reference's
  # discrete_action_wrapper.py:91 compares the players' action specs with `!=`, its
  # substrate_test.py:36-47 an env's specs against the factory's differently named ones
  def __eq__(self, other):
    return isinstance(other, Array) and self.shape == other.shape and self.dtype == other.dtype

  def __ne__(self, other):
    return not self == other

  def __hash__(self):
    return hash((self.shape, self.dtype))


class BoundedArray(Array):

  def __init__(self, shape, dtype, minimum, maximum, name=None):
    super().__init__(shape, dtype, name)
    self.minimum = np.asarray(minimum, self.dtype)
    self.maximum = np.asarray(maximum, self.dtype)

  def validate(self, value):
    value = super().validate(value)
    if (value < self.minimum).any() or (value > self.maximum).any():
      raise ValueError(f"{self.name}: value out of bounds")
    return value

  def __eq__(self, other):
    return (isinstance(other, BoundedArray) and Array.__eq__(self, other) and
            bool((self.minimum == other.minimum).all()) and bool((self.maximum == other.maximum).all()))

  __hash__ = Array.__hash__


class DiscreteArray(BoundedArray):
  """specs.action(n) (reference utils/substrates/specs.py:44-45): int64 scalar."""

  def __init__(self, num_values, dtype=np.int64, name="action"):
    super().__init__((), dtype, 0, num_values - 1, name)
    self.num_values = num_values


# --------------------------------------------------------------------------
# per-substrate configuration (the fields of the reference ConfigDict that the
# hot path needs; reference: configs/substrates/clean_up.py:806-838)


class SubstrateConfig:

  def __init__(self, name, action_set, individual_observation_names,
               global_observation_names, timestep_spec, valid_roles,
               default_player_roles, aux0_name, per_role_constants=False):
    self.name = name
    self.action_set = action_set
    self.individual_observation_names = list(individual_observation_names)
    self.global_observation_names = list(global_observation_names)
    self.action_spec = DiscreteArray(len(action_set))
    self.timestep_spec = dict(timestep_spec)
    self.valid_roles = frozenset(valid_roles)
    self.default_player_roles = tuple(default_player_roles)
    self.aux0_name = aux0_name
    self.per_role_constants = per_role_constants

  # the reference hands out a locked ml_collections.ConfigDict (substrate.py:41-55);
  # callers written against it say `with config.unlocked(): config.x = ...`
  def lock(self):
    return self

  def unlock(self):
    return self

  def unlocked(self):
    import contextlib
    return contextlib.nullcontext(self)


_NOOP = {"move": 0, "turn": 0, "fireZap": 0, "fireClean": 0}


def _clean_up_config() -> SubstrateConfig:
  # clean_up.py:461-483 (ACTION_SET order is what the discrete ids index)
  def a(**kw):
    d = dict(_NOOP)
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1),
                a(turn=1), a(fireZap=1), a(fireClean=1))
  return SubstrateConfig(
      name="clean_up",
      action_set=action_set,
      individual_observation_names=("RGB", "READY_TO_SHOOT",
                                    "NUM_OTHERS_WHO_CLEANED_THIS_STEP"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "NUM_OTHERS_WHO_CLEANED_THIS_STEP": Array(
              (), np.float64, "NUM_OTHERS_WHO_CLEANED_THIS_STEP"),
          "WORLD.RGB": Array((168, 240, 3), np.uint8, "WORLD.RGB"),
      },
      valid_roles={"default"},
      default_player_roles=("default",) * 7,
      aux0_name="NUM_OTHERS_WHO_CLEANED_THIS_STEP")


def _commons_harvest_config(name: str, players: int) -> SubstrateConfig:
  # commons_harvest__open.py:252-273 (ACTION_SET), :531-558 (get_config); the
  # __closed variant shares the Lua level, the action set and the specs.  The
  # __open pack is lowered for 16 players (BASELINE.json configs[2]; the
  # reference's default is 7), the __closed pack for the default 7.
  def a(**kw):
    d = {"move": 0, "turn": 0, "fireZap": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1),
                a(turn=1), a(fireZap=1))
  return SubstrateConfig(
      name=name,
      action_set=action_set,
      individual_observation_names=("RGB", "READY_TO_SHOOT"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "WORLD.RGB": Array((144, 192, 3), np.uint8, "WORLD.RGB"),
      },
      valid_roles={"default"},
      default_player_roles=("default",) * players,
      aux0_name=None)


def _territory_config(name: str, world_hw, players: int = 9) -> SubstrateConfig:
  # territory.py:578-602 (ACTION_SET), territory__rooms.py:84-104 /
  # territory__open.py:111-131 (get_config)
  def a(**kw):
    d = {"move": 0, "turn": 0, "fireZap": 0, "fireClaim": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1),
                a(turn=1), a(fireZap=1), a(fireClaim=1))
  return SubstrateConfig(
      name=name,
      action_set=action_set,
      individual_observation_names=("RGB", "READY_TO_SHOOT"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "WORLD.RGB": Array(tuple(world_hw) + (3,), np.uint8, "WORLD.RGB"),
      },
      valid_roles={"default"},
      default_player_roles=("default",) * players,
      aux0_name=None)


def _coins_config() -> SubstrateConfig:
  # coins.py:431-491 (ACTION_SET: move / turn only, get_config)
  def a(move=0, turn=0):
    return {"move": move, "turn": turn}
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1), a(turn=1))
  return SubstrateConfig(
      name="coins",
      action_set=action_set,
      individual_observation_names=("RGB", "MISMATCHED_COIN_COLLECTED_BY_PARTNER"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "MISMATCHED_COIN_COLLECTED_BY_PARTNER": Array(
              (), np.float64, "MISMATCHED_COIN_COLLECTED_BY_PARTNER"),
          "WORLD.RGB": Array((136, 136, 3), np.uint8, "WORLD.RGB"),
      },
      valid_roles={"default"},
      default_player_roles=("default",) * 2,
      aux0_name="MISMATCHED_COIN_COLLECTED_BY_PARTNER")


def _coop_mining_config() -> SubstrateConfig:
  # coop_mining.py:423-473 (ACTION_SET: move / turn / mine; get_config)
  def a(**kw):
    d = {"move": 0, "turn": 0, "mine": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1), a(turn=1),
                a(mine=1))
  return SubstrateConfig(
      name="coop_mining",
      action_set=action_set,
      individual_observation_names=("RGB", "READY_TO_SHOOT"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "WORLD.RGB": Array((216, 216, 3), np.uint8, "WORLD.RGB"),
      },
      # (both roles build the same avatar: MineBeam.agentRole is "none" for all)
      valid_roles={"default", "target"},
      default_player_roles=("default",) * 6,
      aux0_name=None)


def _gift_refinements_config() -> SubstrateConfig:
  # gift_refinements.py:410-477 (ACTION_SET: move / turn / refineAndGift / consumeTokens; get_config)
  def a(**kw):
    d = {"move": 0, "turn": 0, "refineAndGift": 0, "consumeTokens": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1), a(turn=1),
                a(refineAndGift=1), a(consumeTokens=1))
  return SubstrateConfig(
      name="gift_refinements",
      action_set=action_set,
      individual_observation_names=("RGB", "READY_TO_SHOOT", "INVENTORY"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "INVENTORY": Array((3,), np.float64, "INVENTORY"),
          "WORLD.RGB": Array((216, 216, 3), np.uint8, "WORLD.RGB"),
      },
      # (both roles build the same avatar: GiftBeam.agentRole is "none" for all)
      valid_roles={"default", "target"},
      default_player_roles=("default",) * 6,
      aux0_name=None)


def _externality_mushrooms_config(name: str) -> SubstrateConfig:
  # externality_mushrooms.py:633-658 (ACTION_SET), :1027-1048 (get_config);
  # externality_mushrooms__dense.py:69-86 (the map, the specs, five players)
  def a(**kw):
    d = {"move": 0, "turn": 0, "fireZap": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1), a(turn=1),
                a(fireZap=1))
  return SubstrateConfig(
      name=name,
      action_set=action_set,
      individual_observation_names=("RGB", "READY_TO_SHOOT"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((88, 88, 3), np.uint8, "RGB"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "WORLD.RGB": Array((112, 184, 3), np.uint8, "WORLD.RGB"),
      },
      valid_roles={"default"},
      default_player_roles=("default",) * 5,
      aux0_name=None)


# layout -> (WORLD.RGB height, width, default players): collaborative_cooking__<layout>.py
_COOKING_LAYOUTS = {"asymmetric": (40, 72, 2), "circuit": (40, 72, 2), "cramped": (40, 72, 2),
                    "crowded": (72, 104, 9), "figure_eight": (72, 128, 6), "forced": (40, 72, 2),
                    "ring": (40, 72, 2)}


def _cooking_config(layout: str) -> SubstrateConfig:
  # collaborative_cooking.py:696-724 (ACTION_SET), :899-921 (get_config) + the layout module
  def a(**kw):
    d = {"move": 0, "turn": 0, "interact": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1), a(turn=1),
                a(interact=1))
  h, w, players = _COOKING_LAYOUTS[layout]
  return SubstrateConfig(
      name=f"collaborative_cooking__{layout}",
      action_set=action_set,
      individual_observation_names=("RGB",),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array((40, 40, 3), np.uint8, "RGB"),
          "WORLD.RGB": Array((h, w, 3), np.uint8, "WORLD.RGB"),
      },
      valid_roles={"default"},
      default_player_roles=("default",) * players,
      aux0_name=None)


def _matrix_config(name: str, resources: int, arena: bool, roles, valid_roles) -> SubstrateConfig:
  # prisoners_dilemma_in_the_matrix__repeated.py:153-173 (ACTION_SET, shared by all
  # fifteen), :518-552 (get_config); arenas: 8 players, 11 x 11 window, 24 x 25 map
  # (prisoners_dilemma_in_the_matrix__arena.py:473-512); repeated / one_shot: 2
  # players, 5 x 5 window, 15 x 23 map
  def a(**kw):
    d = {"move": 0, "turn": 0, "interact": 0}
    d.update(kw)
    return d
  action_set = (a(), a(move=1), a(move=3), a(move=4), a(move=2), a(turn=-1),
                a(turn=1), a(interact=1))
  rgb = (88, 88, 3) if arena else (40, 40, 3)
  world = (192, 200, 3) if arena else (120, 184, 3)
  return SubstrateConfig(
      name=name,
      action_set=action_set,
      individual_observation_names=("RGB", "INVENTORY", "READY_TO_SHOOT",
                                    "INTERACTION_INVENTORIES"),
      global_observation_names=("WORLD.RGB",),
      timestep_spec={
          "RGB": Array(rgb, np.uint8, "RGB"),
          "INVENTORY": Array((resources,), np.float64, "INVENTORY"),
          "READY_TO_SHOOT": Array((), np.float64, "READY_TO_SHOOT"),
          "INTERACTION_INVENTORIES": Array((2, resources), np.float64,
                                           "INTERACTION_INVENTORIES"),
          "WORLD.RGB": Array(world, np.uint8, "WORLD.RGB"),
      },
      valid_roles=set(valid_roles),
      default_player_roles=tuple(roles),
      aux0_name=None,
      # the per-player constants of the roles (DyadicRole, avatar colour) are in
      # the pack per (role, player): engine.pack_role_names
      per_role_constants=len(valid_roles) > 1)


def _matrix_configs():
  out = {}
  three = {"pure_coordination", "rationalizable_coordination", "running_with_scissors"}
  for game in ("prisoners_dilemma", "chicken", "stag_hunt", "pure_coordination",
               "rationalizable_coordination", "bach_or_stravinsky", "running_with_scissors"):
    variants = ("repeated", "arena") + (("one_shot",) if game == "running_with_scissors" else ())
    for variant in variants:
      name = f"{game}_in_the_matrix__{variant}"
      arena = variant == "arena"
      if game == "bach_or_stravinsky":
        # bach_or_stravinsky_in_the_matrix__repeated.py:535-536, __arena.py:537-538
        roles = (("bach_fan",) * 4 + ("stravinsky_fan",) * 4) if arena else (
            "bach_fan", "stravinsky_fan")
        valid = {"default", "bach_fan", "stravinsky_fan"}
      else:
        roles = ("default",) * (8 if arena else 2)
        valid = {"default"}
      out[name] = (lambda n=name, g=game, ar=arena, r=roles, v=valid:
                   _matrix_config(n, 3 if g in three else 2, ar, r, v))
  return out


_CONFIGS = {
    **_matrix_configs(),
    "coins": _coins_config,
    "coop_mining": _coop_mining_config,
    "gift_refinements": _gift_refinements_config,
    **{f"collaborative_cooking__{_l}": (lambda _l=_l: _cooking_config(_l)) for _l in _COOKING_LAYOUTS},
    "externality_mushrooms__dense": lambda: _externality_mushrooms_config("externality_mushrooms__dense"),
    "territory__rooms": lambda: _territory_config("territory__rooms", (168, 168)),
    "territory__open": lambda: _territory_config("territory__open", (184, 312)),
    "territory__inside_out": lambda: _territory_config("territory__inside_out", (184, 184), 5),
    "clean_up": _clean_up_config,
    "commons_harvest__open": lambda: _commons_harvest_config("commons_harvest__open", 7),
    "commons_harvest__closed": lambda: _commons_harvest_config("commons_harvest__closed", 7),
    "commons_harvest__partnership": lambda: _commons_harvest_config(
        "commons_harvest__partnership", 7),
}
SUBSTRATES = frozenset(_CONFIGS)


def get_config(name: str) -> SubstrateConfig:
  """reference: meltingpot/substrate.py:41-55."""
  if name not in SUBSTRATES:
    raise ValueError(f"{name} not in {sorted(SUBSTRATES)} (substrates with a "
                     "HIP engine in this build).")
  return _CONFIGS[name]()


# --------------------------------------------------------------------------


class Subject:
  """The slice of `reactivex.subject.Subject` the reference's Substrate uses
  (utils/substrates/substrate.py:56-104): subscribe / on_next / on_completed.
  reactivex is not a dependency of this package."""

  def __init__(self):
    self._observers = []
    self._completed = False

  def subscribe(self, on_next=None, on_error=None, on_completed=None):
    if on_next is not None and not callable(on_next) and hasattr(on_next, "on_next"):
      # an observer object (reactivex accepts one in place of the three callbacks:
      # utils/evaluation/evaluation.py:88-99 subscribes a ReturnSubject this way)
      observer = on_next
      on_next = observer.on_next
      on_error = getattr(observer, "on_error", None)
      on_completed = getattr(observer, "on_completed", None)
    obs = (on_next, on_error, on_completed)
    if self._completed:
      if on_completed:
        on_completed()
    else:
      self._observers.append(obs)
    subject = self

    class _Disposable:
      def dispose(self):
        if obs in subject._observers:
          subject._observers.remove(obs)
    return _Disposable()

  def on_next(self, value):
    for on_next, _, _ in list(self._observers):
      if on_next:
        on_next(value)

  def on_error(self, error):
    for _, on_error, _ in list(self._observers):
      if on_error:
        on_error(error)

  def pipe(self, *operators):
    """reactivex's `Observable.pipe`: each operator maps an observable to an observable."""
    out = self
    for op in operators:
      out = op(out)
    return out

  def on_completed(self):
    self._completed = True
    observers, self._observers = self._observers, []
    for _, _, on_completed in observers:
      if on_completed:
        on_completed()


@dataclasses.dataclass(frozen=True)
class SubstrateObservables:
  """substrate.py:30-45: `action`, `timestep` and `events` streams (the `dmlab2d`
  member has no counterpart: there is no dmlab2d underneath)."""
  action: Subject
  timestep: Subject
  events: Subject
  # batched substrates only: (world, (name, payload)) for every world of the batch
  # (`events` stays reference-shaped: the events of world 0)
  events_batched: Optional[Subject] = None


def resolve_env_seed(env_seed: Optional[int]) -> int:
  """builder.py:174-176: `if env_seed is None: env_seed = <random seed>`.  World w
  of a batch is seeded env_seed + w (one env_seed per world, as N reference
  environments built with consecutive seeds).  Any int is a seed — 0 and negative
  ones included — taken modulo 2**64 (the engine's seeds are u64)."""
  if env_seed is None:
    env_seed = int.from_bytes(os.urandom(8), "little") >> 1
  return int(env_seed) % (1 << 64)


def action_fields(eng) -> Tuple[Tuple[str, ...], Tuple[Tuple[int, int, int], ...]]:
  """(names, (min, max, default) per name) of the avatars' raw action fields in
  actionOrder — the pack's "action_names" / "action_spec" tables
  (avatar_library.lua:205-223 Avatar:discreteActionSpec)."""
  from meltingpot_amd import pack as pack_lib
  t = eng.pack_tables() if hasattr(eng, "pack_tables") else pack_lib.loads(eng.pack_bytes)
  names = tuple(n.decode() for n in bytes(t["action_names"]).split(b"\0")[:-1])
  spec = tuple(tuple(int(v) for v in row) for row in t["action_spec"].reshape(-1, 3))
  assert len(names) == len(spec)
  return names, spec


def validate_action_table(action_table, names, ranges) -> np.ndarray:
  """discrete_action_wrapper.py:28-49: every row names exactly the action spec's
  fields with values inside their ranges.  Returns the table as int32 [K, A]."""
  if not action_table:
    raise ValueError("action_table must not be empty")
  rows = np.zeros((len(action_table), len(names)), np.int32)
  for i, action in enumerate(action_table):
    ok = set(action) == set(names)
    if ok:
      for a, (n, (lo, hi, _)) in enumerate(zip(names, ranges)):
        v = int(action[n])
        ok = ok and lo <= v <= hi
        rows[i, a] = v
    if not ok:
      raise ValueError(f"Action {i} ({dict(action)}) does not match action_spec "
                       f"({dict(zip(names, ranges))}).")
  return rows


def _check_pool_factor(arg: str, k) -> int:
  if k not in (1, 2, 4, 8) or isinstance(k, bool):
    raise ValueError(f"{arg} must be 1, 2, 4 or 8, got {k!r}")
  return int(k)


class Substrate:
  """N worlds of one substrate behind the reference's `Substrate` interface.

  In batched mode the leaves of every TimeStep are the SAME device tensors,
  refreshed in place by the next reset() / step(): clone what you keep — or build
  with `rollout_length=T` and keep them for free: every leaf is then a slot of a
  [T, N, ...] ring the engine writes in turn (mp_bind_output_ring), a TimeStep's
  leaves stay untouched for T steps, and `Substrate.rollout` is the whole ring."""

  def __init__(self, config: SubstrateConfig, roles: Sequence[str],
               pack_bytes: bytes, *, num_worlds: int = 1, batched: Optional[bool] = None,
               device: int = 0, env_seed: Optional[int] = None,
               auto_reset: bool = True, world_offset: int = 0,
               debug_observations: bool = False,
               action_table: Optional[Sequence[Mapping[str, int]]] = None,
               rollout_length: int = 0, check_device_actions: bool = False,
               rgb_pool: int = 1, world_rgb_pool: int = 1,
               _leaves: Optional[Callable[[str, tuple, Any, Any], Any]] = None):
    """`action_table`: the discrete actions, as in the reference's
    `build_substrate(..., action_table)` (utils/substrates/substrate.py:107-139,
    discrete_action_wrapper.py:77-109): row i is what discrete action i does,
    any combination of the avatar's raw fields.  Default: the config's
    ACTION_SET (looked up on the device by mp_step).

    `check_device_actions`: a debugging switch — device action tensors are range-checked
    like host arrays are (ValueError; costs a host synchronisation per step).  Off, ids
    outside the table do NOOP and are counted (mp_counters: bad_actions).

    `rollout_length` = T > 0 (batched substrates): the observations a learner keeps
    without a copy.  The reference hands back fresh arrays every step
    (wrappers/multiplayer_wrapper.py:108-118, substrate.py:74-81) and a rollout just
    stores them; here submission t (every reset() and step()) writes slot t % T of
    [T, N, ...] tensors, the returned `RolloutTimeStep` holds views of its slot
    (`.slot`), and nothing is cloned, synchronised or re-tuned between steps.

    `rgb_pool` = k in (2, 4, 8): "RGB" is the player's view cut down by k with an area filter
    (k x k box average, rounded half up: `engine.pool_rgb`), e.g. (11, 11, 3) for an 88 x 88 view
    at k = 8, in the observations and in `observation_spec()`.  The engine draws the pooled
    view itself (MP_OBS_RGB_POOL<k>): the full image is never written.  1 (default): the full
    view.

    `world_rgb_pool` = k in (2, 4, 8): the same for "WORLD.RGB", the whole map — e.g. (21, 30, 3)
    for clean_up's 168 x 240 image at k = 8 (MpConfig.world_pool: the engine draws it pooled,
    the full image is never written).  The two factors are independent.

    `_leaves` (private; `MixtureSubstrate`): called as `_leaves(name, shape, dtype, device)` with
    the engine's shape of each leaf of a batched substrate, it returns the tensor to bind instead
    of one the engine allocates — [n, ...], or [T, n, ...] with a ring — e.g. a slice of a
    tensor that several substrates share."""
    self._rgb_pool = _check_pool_factor("rgb_pool", rgb_pool)
    self._world_rgb_pool = _check_pool_factor("world_rgb_pool", world_rgb_pool)
    invalid = set(roles) - config.valid_roles  # configs/substrates/__init__.py:42-45
    if invalid:
      raise ValueError(f"Invalid roles: {invalid!r}. Must be one of "
                       f"{config.valid_roles!r}")
    if num_worlds < 1:
      raise ValueError("num_worlds must be positive")
    self._config = config
    self._roles = tuple(roles)
    self._batched = (num_worlds > 1) if batched is None else bool(batched)
    if not self._batched and num_worlds != 1:
      raise ValueError("batched=False needs num_worlds == 1")
    self._T = int(rollout_length or 0)
    if self._T < 0:
      raise ValueError("rollout_length must not be negative")
    if self._T and not self._batched:
      raise ValueError("rollout_length needs a batched substrate (device tensors); the "
                       "one-world form already returns fresh numpy arrays every step")
    if _leaves is not None and not self._batched:
      raise ValueError("caller-provided leaves need a batched substrate")
    # "EGO_LAYER": a leaf behind a registration of its own (MpEgoLayer), not an engine kind
    ego = "EGO_LAYER" in config.individual_observation_names
    if ego and not self._batched:
      raise ValueError("\"EGO_LAYER\" needs a batched substrate (device tensors): build it with "
                       "num_worlds > 1; the one-world form returns numpy arrays and refuses it as it "
                       "refuses a rollout ring")
    # "AVATAR_IDS_IN_VIEW", "AVATAR_IDS_IN_RANGE_TO_ZAP": two leaves behind one registration (MpAvatarIds)
    ids = tuple(n for n in AVATAR_IDS_NAMES if n in config.individual_observation_names)
    if ids and not self._batched:
      raise ValueError(f"{list(ids)} need a batched substrate (device tensors): build it with num_worlds > 1; "
                       "the one-world form returns numpy arrays and refuses them as it refuses \"EGO_LAYER\"")
    if AVATAR_IDS_NAMES[1] in ids and not engine_lib.has_zapper(pack_bytes):
      raise ValueError(f"\"{AVATAR_IDS_NAMES[1]}\": {config.name!r} has no Zapper, so no zap could reach anybody "
                       f"(\"{AVATAR_IDS_NAMES[0]}\" works on every level)")
    # "WORLD.LAYER": a global leaf behind a registration of its own (MpEgoLayer's world ops)
    wl = "WORLD.LAYER" in config.global_observation_names
    if wl and not self._batched:
      raise ValueError("\"WORLD.LAYER\" needs a batched substrate (device tensors): build it with "
                       "num_worlds > 1; the one-world form returns numpy arrays and refuses it as it "
                       "refuses \"EGO_LAYER\"")
    self._submissions = 0
    self._check_device_actions = bool(check_device_actions)
    if not self._roles:
      raise ValueError("roles must not be empty")
    # a config with several valid roles builds per-player constants from them
    # (bach_or_stravinsky_in_the_matrix__repeated.py:473-497): the pack carries
    # them per (role, player) and the engine is created for this assignment
    role_names = engine_lib.pack_role_names(pack_bytes) if config.per_role_constants else None
    role_ids = [role_names.index(r) for r in self._roles] if role_names else None
    env_seed = resolve_env_seed(env_seed)
    # num_players = len(roles) (configs/substrates/clean_up.py:847): the first
    # len(roles) avatars of the committed pack play
    # (world_pool only when asked for: the engine's default is the full image)
    pooled = {"world_pool": self._world_rgb_pool} if self._world_rgb_pool > 1 else {}
    self._eng = engine_lib.Engine(
        pack_bytes, num_worlds, device=device, auto_reset=auto_reset,
        world_offset=world_offset, base_seed=env_seed, literal_seed=True,
        num_players=len(self._roles),
        debug_observations=debug_observations, roles=role_ids, **pooled)
    self._env_seed = env_seed
    self._action_rows = self._action_rows_dev = None
    if action_table is not None:
      names, ranges = action_fields(self._eng)
      self._action_rows = validate_action_table(action_table, names, ranges)
    E = engine_lib
    self._kinds = {"RGB": E.OBS_RGB_POOL.get(self._rgb_pool, E.OBS_RGB), "WORLD.RGB": E.OBS_WORLD_RGB,
                   "READY_TO_SHOOT": E.OBS_READY_TO_SHOOT,
                   "COLLECTIVE_REWARD": E.OBS_COLLECTIVE_REWARD,
                   "INVENTORY": E.OBS_INVENTORY,
                   "INTERACTION_INVENTORIES": E.OBS_INTERACTION_INVENTORIES,
                   "POSITION": E.OBS_POSITION, "ORIENTATION": E.OBS_ORIENTATION,
                   # the symbolic view (avatar_library.lua:246-257): written by the step's own
                   # launch, from the records while they are in LDS
                   "LAYER": E.OBS_LAYER}
    if config.aux0_name:
      self._kinds[config.aux0_name] = E.OBS_AUX0
    if config.name.split("__")[0] == "clean_up":
      # the debug observations a config built with _ENABLE_DEBUG_OBSERVATIONS reports
      # (clean_up.py:751-784): produced while bound, i.e. when a caller asks for them
      self._kinds.update({"PLAYER_CLEANED": E.OBS_AUX1, "PLAYER_ATE_APPLE": E.OBS_AUX2,
                          "NUM_OTHERS_PLAYER_ZAPPED_THIS_STEP": E.OBS_AUX3,
                          "NUM_OTHERS_WHO_ATE_THIS_STEP": E.OBS_AUX4})
    names = (list(config.individual_observation_names) +
             list(config.global_observation_names) + ["COLLECTIVE_REWARD"])
    unknown = [n for n in names if n not in self._kinds and not (ego and n == "EGO_LAYER") and n not in ids and
               not (wl and n == "WORLD.LAYER")]
    if unknown:
      raise ValueError(f"observations {unknown} are not produced by the engine for "
                       f"{config.name!r} (it offers {sorted(self._kinds) + ['EGO_LAYER'] + list(AVATAR_IDS_NAMES)}"
                       " and the global \"WORLD.LAYER\")")
    kinds = {n: self._kinds[n] for n in names if n in self._kinds}
    kinds.update({"#reward": E.OBS_REWARD, "#discount": E.OBS_DISCOUNT,
                  "#step_type": E.OBS_STEP_TYPE})
    # (None: the engine allocates the leaf itself)
    take = ((lambda n, k: None) if _leaves is None else
            (lambda n, k: _leaves(n, *self._eng.shapes[k], self._eng.device)))
    if self._batched and self._T:
      # the rollout ring: one [T, N, ...] tensor per leaf, written slot by slot
      bound = {n: self._eng.bind_ring(k, take(n, k), slots=self._T) for n, k in kinds.items()}
      self._host = None
    elif self._batched:
      bound = {n: self._eng.bind(k, take(n, k)) for n, k in kinds.items()}
      self._host = None
    else:
      # one world, numpy leaves: every output lives in one device buffer that is
      # mirrored to pinned host memory with a single copy per step
      t = self._eng._torch
      layout, total = {}, 0
      for n, k in kinds.items():
        shape, dtype = self._eng.shapes[k]
        nbytes = int(np.prod(shape)) * t.empty((), dtype=dtype).element_size()
        layout[n] = (total, nbytes, shape, dtype)
        total += (nbytes + 255) & ~255
      self._blob = t.empty(total, dtype=t.uint8, device=self._eng.device)
      self._host = t.empty(total, dtype=t.uint8, pin_memory=self._blob.is_cuda)
      view = lambda buf, n: buf[layout[n][0]:layout[n][0] + layout[n][1]].view(
          layout[n][3]).view(layout[n][2])
      bound = {n: self._eng.bind(kinds[n], view(self._blob, n)) for n in kinds}
      self._host_views = {n: view(self._host, n).numpy() for n in kinds}
    if ego:
      # the layer view in the avatar's own frame: redrawn behind every submission by a launch of
      # its own, into this tensor or into the ring slot the submission wrote
      t = self._eng._torch
      shape = self._eng.ego_layer_shape
      given = None if _leaves is None else _leaves("EGO_LAYER", shape, t.int32, self._eng.device)
      if self._T:
        bound["EGO_LAYER"] = self._eng.bind_ego_layer_ring(given, slots=self._T)
      else:
        bound["EGO_LAYER"] = self._eng.bind_ego_layer(
            given if given is not None else t.zeros(shape, dtype=t.int32, device=self._eng.device))
    if ids:
      # whom every player sees and could zap: rewritten behind every submission by ONE launch, into
      # these tensors or into the ring slot the submission wrote
      t = self._eng._torch
      shape = self._eng.avatar_ids_shape
      for n in ids:
        given = None if _leaves is None else _leaves(n, shape, t.int32, self._eng.device)
        bound[n] = given if given is not None else t.zeros(((self._T,) if self._T else ()) + shape, dtype=t.int32,
                                                            device=self._eng.device)
      self._eng.bind_avatar_ids(bound.get(AVATAR_IDS_NAMES[0]), bound.get(AVATAR_IDS_NAMES[1]))
    if wl:
      # the layer view of the whole map: redrawn behind every submission by a launch of its own, into
      # this tensor or into the ring slot the submission wrote
      t = self._eng._torch
      shape = self._eng.world_layer_shape
      given = None if _leaves is None else _leaves("WORLD.LAYER", shape, t.int32, self._eng.device)
      bound["WORLD.LAYER"] = self._eng.bind_world_layer(
          given if given is not None else t.zeros(((self._T,) if self._T else ()) + shape, dtype=t.int32,
                                                  device=self._eng.device))
    self._ego = ego
    self._ids = ids
    self._wl = wl
    self._obs = {n: bound[n] for n in names}
    self._reward = bound["#reward"]
    self._discount = bound["#discount"]
    self._step_type = bound["#step_type"]
    self._closed = False
    self._observables = SubstrateObservables(Subject(), Subject(), Subject(),
                                             Subject() if self._batched else None)

  # -- reference surface ---------------------------------------------------
  @property
  def num_worlds(self) -> int:
    return self._eng.N

  @property
  def num_players(self) -> int:
    return self._eng.P

  @property
  def engine(self) -> engine_lib.Engine:
    return self._eng

  @property
  def rollout(self) -> Optional[Dict[str, Any]]:
    """rollout_length=T: the ring itself — {"step_type": [T, N], "reward": [T, N, P],
    "discount": [T, N], "observation": {name: [T, N, ...]}} device tensors; slot s of
    every tensor is the same step (`RolloutTimeStep.slot`).  None otherwise."""
    if not self._T:
      return None
    return {"step_type": self._step_type, "reward": self._reward,
            "discount": self._discount, "observation": dict(self._obs)}

  @property
  def slot(self) -> int:
    """rollout_length=T: the slot the last reset() / step() wrote (-1 before the first) — the
    ENGINE's ring position (MpInfo.ring_next), so that submissions made through `.engine`
    (a masked reset, direct steps) are counted like this object's own."""
    if not self._T:
      return -1
    ring = self._eng.ring
    if not self._submissions and ring["next"] == 0:
      return -1
    return ring["last"]

  def reset(self) -> TimeStep:
    """Substrate.reset (substrate.py:66-72): FIRST, zero rewards, discount 0."""
    self._eng.use_current_stream()   # follow the caller's torch stream (ordered after the old one)
    self._eng.reset()
    self._submissions += 1
    return self._emit(self._timestep())

  def observation(self):
    """wrappers/base.py:60-62 `observation()`: the observation of the last reset() /
    step() again (the leaves of the last TimeStep)."""
    return self._timestep().observation

  def save_state(self, worlds=None) -> WorldStates:
    """The records of `worlds` (None: every world, in order) as device rows — a copy on the
    device, ordered on the current stream, no host synchronisation."""
    self._eng.use_current_stream()
    return WorldStates(self._eng.save_worlds(worlds), self._eng.state_fingerprint)

  def state_layout(self) -> SubstrateStateLayout:
    """What the bytes of this substrate's saved rows are: the engine's layout (planes, tail
    fields with their offsets, as the library lists them) with the pack's layer and state names."""
    if getattr(self, "_state_layout", None) is None:
      from meltingpot_amd import pack as pack_lib
      self._state_layout = SubstrateStateLayout(self._eng.state_layout(), pack_lib.loads(self._eng.pack_bytes))
    return self._state_layout

  def state_fields(self, states: WorldStates) -> StateFields:
    """The rows of `states` by named field: views that share memory with `states.data`, for
    reading (how many apples are left in each row?) and for editing (start every world with an
    empty orchard).  Marks `states` as edited, so that `load_state` checks what it loads; ask
    `check_states` yourself any time.  Edit the planes and the tail so that they agree — an
    avatar's state byte lies at (avatar_x, avatar_y) of the avatar layer's plane — and after
    changing `seed`, `episode` or `step` set `orders_step` to 0: the cached visiting orders are a
    function of those three and are drawn again when absent."""
    if not isinstance(states, WorldStates):
      raise ValueError("state_fields takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    fields = StateFields(states.data, self.state_layout())
    states.edited = True
    return fields

  def check_states(self, states: WorldStates, rows=None):
    """Is every row a record this level's kernels can take?  int32 [R, 2] device tensor of
    (rule, offset word) per row — (0, 0) for a well-formed row, else the smallest rule it breaks
    (engine.RULE_*) and where (`state_layout().describe(rule, offset)`).  The rows are judged
    where they lie; nothing of this substrate changes.  No host synchronisation."""
    if not isinstance(states, WorldStates):
      raise ValueError("check_states takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    self._eng.use_current_stream()
    return self._eng.check_states(states.data, rows=rows, fingerprint=states.fingerprint)

  def hash_states(self, states: WorldStates, rows=None, planes=None, fields=None):
    """Are two saved states the same state?  int64 [R] device tensor: a 64-bit hash of every row
    (`rows`: the rows to hash, in order, repeats allowed; default all), computed on the device
    where the rows lie.  Equal hashes mean equal states (up to a 2^-64 collision), and different
    hashes always mean different states — where comparing `states.data` byte for byte calls
    equal states different: the event counters and the reward sum (`ctr`, `reward_fx`) are the
    bookkeeping of whichever substrate a row was loaded into, the cached visiting orders
    (`orders_step`, `next_orders`) may be present or absent, and the padding and the bytes of
    avatars >= num_players hold whatever an edit left.  None of those count; every plane, the
    level's player block and every other tail field do.  `torch.unique(h, return_inverse=True)`
    is the dedup of a search frontier.
    `planes` / `fields`: hash a chosen part instead — an iterable of grid planes
    (`state_fields(...).grid`'s second axis), an iterable of field names (`StateFields.names`, or
    the tail's own; "player_block" for the matrix games' block); if one is given, None for the
    other means none of them.  An exploration "cell", e.g. the apple plane plus the avatars'
    positions.  Unknown names are a ValueError.  The first call with a NEW custom part waits for
    the stream once; repeats, and the default, only enqueue.
    Hashes compare only within one fingerprint (one level, player count, roles and library) and
    one choice of planes and fields.  Nothing of this substrate changes; no host
    synchronisation."""
    if not isinstance(states, WorldStates):
      raise ValueError("hash_states takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    self._eng.use_current_stream()
    return self._eng.hash_states(states.data, rows=rows, planes=planes, fields=_hash_fields(fields),
                                 fingerprint=states.fingerprint)

  def hash_worlds(self, worlds=None, planes=None, fields=None):
    """int64 [N] device tensor (`worlds`: a list, default every world): `hash_states` of the
    worlds as they are now, without saving them — `hash_states(save_state(worlds))`."""
    self._eng.use_current_stream()
    return self._eng.hash_worlds(worlds, planes=planes, fields=_hash_fields(fields))

  def _view_layers(self, layers):
    """`layers` of a hash_views call as layer indices: names of `state_layout().layer_names` or
    indices (None: every layer).  Unknown names are a ValueError."""
    if layers is None:
      return None
    if isinstance(layers, (str, int, np.integer)):
      layers = (layers,)
    names = list(self.state_layout().layer_names)
    picked = []
    for l in layers:
      if isinstance(l, str):
        if l not in names:
          raise ValueError(f"hash_views: {l!r} is no layer of this level (it has {names})")
        l = names.index(l)
      picked.append(l)
    return picked

  def hash_views(self, states: Optional[WorldStates] = None, rows=None, players=None, layers=None, classes=None):
    """Do two players see the same thing?  int64 [R, P] device tensor (or [R] with `players`, R
    ints: player players[i] of row rows[i]): a 64-bit hash of what each player observes — its
    "EGO_LAYER", the layer view in the avatar's own frame — in saved states, or in this
    substrate's worlds as they are now (`states` None; `rows` are then world indices).  The hash
    is worked out on the device from the records; no view is drawn.  Equal hashes mean equal views
    (up to a 2^-64 collision), different hashes always mean different views; what lies outside a
    player's window never counts, and a dead player's view is all out-of-bounds.
    `layers`: the layers that count, by name (`state_layout().layer_names`) or index (None: all);
    `classes`: `num_layer_ids` ints mapping every "LAYER" id to a class, so that ids of one class
    hash alike (e.g. every avatar colour to one "an avatar").  Per-agent novelty is
    `torch.unique(h, return_counts=True)`; an information-set key is h[w, acting_player]; "did my
    view change?" is h != h_before.  Hashes compare only within one fingerprint and one choice of
    layers and classes.  Nothing of this substrate changes; no host synchronisation."""
    if not self._batched:
      raise ValueError("hash_views needs a batched substrate (device tensors): build it with num_worlds > 1")
    self._eng.use_current_stream()
    layers = self._view_layers(layers)
    if states is None:
      return self._eng.hash_views(None, rows=rows, players=players, layers=layers, classes=classes)
    if not isinstance(states, WorldStates):
      raise ValueError("hash_views takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    return self._eng.hash_views(states.data, rows=rows, players=players, layers=layers, classes=classes,
                                fingerprint=states.fingerprint)

  @property
  def num_layer_ids(self) -> int:
    """The number of ids "LAYER" can hold: the length of `hash_views`' `classes`."""
    return self._eng.num_layer_ids

  def set_view_hashes(self, layers="all", classes=None, out=None):
    """Keeps `hash_views()` of the worlds current on the device: returns an int64 [N, P] device
    tensor — [T, N, P] on a substrate built with rollout_length=T — that one launch rewrites behind
    every reset, step, step_many and load_state, in the ring slot the submission wrote.
    `layers` ("all": every layer), `classes`: as `hash_views` takes them.  `set_view_hashes(None)`
    clears the registration, as `set_episode_stats(None)` does: the launches are then what they
    were.  There are no per-step rows in `step_many`: call step_many(states=True) and
    hash_views(result.states)."""
    if not self._batched:
      raise ValueError("set_view_hashes needs a batched substrate (device tensors): build it with num_worlds > 1")
    self._eng.use_current_stream()
    if layers is None:
      self._eng.bind_view_hash(None)
      return None
    layers = None if isinstance(layers, str) and layers == "all" else self._view_layers(layers)
    t = self._eng._torch
    shape = ((self._T,) if self._T else ()) + (self._eng.N, self._eng.P)
    if out is None:
      out = t.zeros(shape, dtype=t.int64, device=self._eng.device)
    elif not isinstance(out, t.Tensor) or tuple(out.shape) != shape:
      raise ValueError(f"set_view_hashes: out must be an int64 device tensor of shape {shape}")
    return self._eng.bind_view_hash(out, layers=layers, classes=classes)

  @property
  def layer_id_names(self) -> Tuple[str, ...]:
    """What every id of "LAYER" and "EGO_LAYER" shows: `num_layer_ids` strings, "" for id 0
    (nothing) and the name of sprite i - 1 for id i ("OutOfBounds" is id 1, then "OutOfView",
    "Avatar1", "Self", ...)."""
    return self._eng.layer_id_names

  def layer_classes(self, groups) -> np.ndarray:
    """A class table by name: int32 [num_layer_ids], class c for every id that `groups[c]` names and
    -1 for every other id — `classes` of `observe_ego_planes`, `set_ego_planes` and `hash_views`.
    A group is a name of `layer_id_names`, an `fnmatch` pattern, or an iterable of those:
      env.layer_classes(["Self", "Avatar*", "Beam*", "Wall*", "OutOfBounds"])
    ValueError for a pattern that matches no id, and for an id two groups match."""
    return _classes_by_name("layer_classes", "layer_id_names", self.layer_id_names, groups)

  # -- the world camera: "WORLD.LAYER" and the world planes ------------------------------------
  def _world_source(self, who: str, states):
    """(bank, fingerprint) of a world-view call: `states` checked, or (None, None) for the worlds."""
    if not self._batched:
      raise ValueError(f"{who} needs a batched substrate (device tensors): build it with num_worlds > 1")
    self._eng.use_current_stream()
    if states is None:
      return None, None
    if not isinstance(states, WorldStates):
      raise ValueError(f"{who} takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    return states.data, states.fingerprint

  def observe_world_layer(self, states: Optional[WorldStates] = None, rows=None):
    """"WORLD.LAYER" — the layer view of the whole map, what "WORLD.RGB" is rendered from — of saved
    states, or of this substrate's worlds as they are now (`states` None; `rows` are then world
    indices): int32 [R, H, W, L], north up.  Id i is sprite i - 1 after the WORLD's sprite map
    (`world_layer_id_names`); a dead avatar shows nowhere.  `(layer == id).sum((1, 2, 3))` counts
    things on the map.  Any batched substrate draws it, with or without the leaf.  Ordered on the
    current stream; no host synchronisation."""
    bank, fingerprint = self._world_source("observe_world_layer", states)
    return self._eng.observe_world_layer(bank, rows=rows, fingerprint=fingerprint)

  @property
  def num_world_layer_ids(self) -> int:
    """The number of ids "WORLD.LAYER" can hold: the length of `observe_world_planes`' `classes`."""
    return self._eng.num_world_layer_ids

  @property
  def world_layer_id_names(self) -> Tuple[str, ...]:
    """What every id of "WORLD.LAYER" shows: `num_world_layer_ids` strings, "" for id 0 (nothing)
    and the name of sprite i - 1 for id i, after the WORLD's sprite map."""
    return self._eng.world_layer_id_names

  def world_layer_classes(self, groups) -> np.ndarray:
    """`layer_classes` over the world's names: int32 [num_world_layer_ids], class c for every id
    that `groups[c]` names and -1 for every other — `classes` of `observe_world_planes` and
    `set_world_planes`."""
    return _classes_by_name("world_layer_classes", "world_layer_id_names", self.world_layer_id_names, groups)

  def observe_world_planes(self, classes, states: Optional[WorldStates] = None, rows=None, layers=None,
                           facing: bool = False, num_classes: Optional[int] = None, out=None):
    """The whole map as a centralised critic reads it: uint8 [R, C', H, W] device tensor of 0/1
    planes of "WORLD.LAYER", channels first, in saved states or in this substrate's worlds as they
    are now (`states` None; `rows` are then world indices), written from the records by one launch.
    `classes`: `num_world_layer_ids` ints in [-1, C) (`world_layer_classes(groups)` writes one by
    name); plane c is 1 where some counted layer of the cell holds an id of class c; -1 sets
    nothing; C = `num_classes`, by default 1 + the largest entry, at most 64.  `layers`: the layers
    that count, by name or index (None: all).  `facing`: four more planes, C' = C + 4: plane C + d
    is 1 where a living avatar stands that faces d (absolute, 0 = N).  `planes.half()` is the
    critic's input.  `out`: a uint8 tensor of the result's shape; it may start on any byte."""
    bank, fingerprint = self._world_source("observe_world_planes", states)
    return self._eng.observe_world_planes(classes, bank, rows=rows, layers=self._view_layers(layers), facing=facing,
                                          num_classes=num_classes, out=out, fingerprint=fingerprint)

  def set_world_planes(self, classes, layers="all", facing: bool = False, out=None, num_classes: Optional[int] = None):
    """Keeps `observe_world_planes(classes, ...)` of the worlds current on the device: returns a
    uint8 [N, C', H, W] device tensor — [T, N, C', H, W] on a substrate built with rollout_length=T
    — that one launch rewrites behind every reset, step, step_many and load_state, in the ring slot
    the submission wrote.  `set_world_planes(None)` clears the registration: the launches are then
    what they were.  There are no per-step rows in `step_many`: call step_many(states=True) and
    observe_world_planes(classes, result.states)."""
    if not self._batched:
      raise ValueError("set_world_planes needs a batched substrate (device tensors): build it with num_worlds > 1")
    self._eng.use_current_stream()
    if classes is None:
      self._eng.bind_world_planes(None)
      return None
    layers = None if isinstance(layers, str) and layers == "all" else self._view_layers(layers)
    t = self._eng._torch
    cls, C = self._eng._world_plane_classes(classes, num_classes)
    shape = ((self._T,) if self._T else ()) + self._eng.world_planes_shape(C, facing)
    if out is None:
      out = t.zeros(shape, dtype=t.uint8, device=self._eng.device)
    elif not isinstance(out, t.Tensor) or tuple(out.shape) != shape:
      raise ValueError(f"set_world_planes: out must be a uint8 device tensor of shape {shape}")
    return self._eng.bind_world_planes(out, cls, layers=layers, facing=facing, num_classes=C)

  def observe_ego_planes(self, classes, states: Optional[WorldStates] = None, rows=None, players=None, layers=None,
                         facing: bool = False, num_classes: Optional[int] = None):
    """What a conv net reads of each player's view: uint8 [R, P, C', VH, VW] device tensor (or
    [R, C', VH, VW] with `players`, R ints: player players[i] of row rows[i]) of 0/1 planes of its
    "EGO_LAYER", channels first, in saved states or in this substrate's worlds as they are now
    (`states` None; `rows` are then world indices), written from the records by one launch.
    `classes`: `num_layer_ids` ints in [-1, C) mapping every "LAYER" id to a class
    (`layer_classes(groups)` writes one by name); plane c is 1 where some counted layer of the cell
    holds an id of class c; -1 sets nothing; C = `num_classes`, by default 1 + the largest entry, at
    most 64.  `layers`: the layers that count, by name or index (None: all).  `facing`: four more
    planes, C' = C + 4: plane C + d is 1 where a living avatar stands whose facing in the viewer's
    frame, (ORIENTATION[q] - ORIENTATION[p]) & 3, is d — the viewer itself: d = 0 — and a dead
    viewer's are 0.  `planes.view(R * P, C', VH, VW).half()` feeds a convolution.  Nothing of this
    substrate changes; no host synchronisation with a device or numpy `classes` and `num_classes`."""
    if not self._batched:
      raise ValueError("observe_ego_planes needs a batched substrate (device tensors): build it with num_worlds > 1")
    self._eng.use_current_stream()
    layers = self._view_layers(layers)
    if states is None:
      return self._eng.observe_ego_planes(classes, None, rows=rows, players=players, layers=layers, facing=facing,
                                          num_classes=num_classes)
    if not isinstance(states, WorldStates):
      raise ValueError("observe_ego_planes takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    return self._eng.observe_ego_planes(classes, states.data, rows=rows, players=players, layers=layers,
                                        facing=facing, num_classes=num_classes, fingerprint=states.fingerprint)

  def set_ego_planes(self, classes, layers="all", facing: bool = False, out=None, num_classes: Optional[int] = None):
    """Keeps `observe_ego_planes(classes, ...)` of the worlds current on the device: returns a uint8
    [N, P, C', VH, VW] device tensor — [T, N, P, C', VH, VW] on a substrate built with
    rollout_length=T — that one launch rewrites behind every reset, step, step_many and load_state,
    in the ring slot the submission wrote.  `layers` ("all": every layer), `facing`, `num_classes`:
    as `observe_ego_planes` takes them.  `set_ego_planes(None)` clears the registration: the
    launches are then what they were.  There are no per-step rows in `step_many`: call
    step_many(states=True) and observe_ego_planes(classes, result.states)."""
    if not self._batched:
      raise ValueError("set_ego_planes needs a batched substrate (device tensors): build it with num_worlds > 1")
    self._eng.use_current_stream()
    if classes is None:
      self._eng.bind_ego_planes(None)
      return None
    layers = None if isinstance(layers, str) and layers == "all" else self._view_layers(layers)
    t = self._eng._torch
    cls, C = self._eng._plane_classes(classes, num_classes)
    shape = ((self._T,) if self._T else ()) + self._eng.ego_planes_shape(C, facing)
    if out is None:
      out = t.zeros(shape, dtype=t.uint8, device=self._eng.device)
    elif not isinstance(out, t.Tensor) or tuple(out.shape) != shape:
      raise ValueError(f"set_ego_planes: out must be a uint8 device tensor of shape {shape}")
    return self._eng.bind_ego_planes(out, cls, layers=layers, facing=facing, num_classes=C)

  def load_state(self, states: WorldStates, src, check: Optional[bool] = None) -> TimeStep:
    """World w continues from row src[w] of `states` (-1: world w is left as it is), as the
    world the row was saved from would: same seed, episode, step and future under the same
    actions.  One submission, like a masked reset: the returned TimeStep is FIRST for loaded
    worlds (LAST for a row saved from a finished episode), with the observations of their
    records; `src` has num_worlds entries (an int is enough for one world).
    check: None checks the rows iff `states.edited` (they went through `state_fields`); True /
    False force it.  A checked load leaves a world whose row is malformed as it is, and the next
    synchronising call raises ValueError naming the world, the row and the rule."""
    if not isinstance(states, WorldStates):
      raise ValueError("load_state takes the WorldStates of save_state")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    if isinstance(src, (int, np.integer)):
      src = [int(src)]
    check = _resolve_check(states, check)
    self._eng.use_current_stream()
    if check:
      self._eng.load_worlds(states.data, src, states.fingerprint, check=True)
    else:   # (exactly the call, and the launches, of a load before there was a check)
      self._eng.load_worlds(states.data, src, states.fingerprint)
    self._submissions += 1
    return self._emit(self._timestep())

  def set_episode_starts(self, states: Optional[WorldStates], rows=None, *, fresh: bool = False,
                         check: Optional[bool] = None):
    """Where auto-reset episodes begin.  From now on a world whose episode has ended starts from
    row rows[w] of `states` instead of the level's own first frame — in `step` and in every one
    of the K steps of `step_many` — as `load_state` of that row would start it: FIRST (LAST for a
    row saved from a finished episode), the row's observations, the row's seed, episode and
    future.  Returns `rows`, the int32 [num_worlds] device tensor the engine reads each time an
    episode ends (allocated and filled with -1 when None: -1 keeps the level's own reset), so

        rows = env.set_episode_starts(bank)
        rows[:] = torch.randint(len(bank), rows.shape)   # any time, no call needed

    fresh=True: a started world keeps its own seed and its own episode count (and draws its
    visiting orders anew), so worlds that start from one row diverge — what training wants; the
    default replays the saved world, what evaluation and tests want.
    check: None checks iff `states.edited` (they went through `state_fields`); True / False force
    it.  A check is one `check_states` launch over the whole bank, now; a world whose row it
    refused — or whose index is neither -1 nor a row — takes the level's own reset, and the next
    synchronising call raises ValueError naming the world, the row and the rule.  Rows edited
    after this call are not judged again: call it again.
    `states` None clears the registration.  The substrate keeps `states` and `rows` alive and
    never writes the bank.  While a registration is set a step with pixel leaves is two launches
    instead of one.  No host synchronisation."""
    self._eng.use_current_stream()
    if states is None:
      self._eng.clear_episode_starts()
      return None
    if not isinstance(states, WorldStates):
      raise ValueError("set_episode_starts takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    t = self._eng._torch
    if rows is None:
      rows = t.full((self.num_worlds,), -1, dtype=t.int32, device=self._eng.device)
    check = _resolve_check(states, check)
    verdicts = self._eng.check_states(states.data, fingerprint=states.fingerprint) if check else None
    self._eng.set_episode_starts(states.data, rows, fresh=fresh, verdicts=verdicts,
                                 fingerprint=states.fingerprint)
    return rows

  def event_columns(self):
    """The default statistics columns of this level: for every event type its rules can push, one
    unfiltered column per player-valued payload key ("zap.source", "zap.target", ...)."""
    return self._eng.event_columns()

  def set_episode_stats(self, columns="default", pairs=(), out=None):
    """Per-episode returns, lengths and event counts per player, kept on the device.  From now on
    every reset, step, step_many and load_state is followed on the same stream by one launch that
    folds what it wrote into the tensors of the returned `EpisodeStats`: `.running`, `.last` and
    `.total` (dicts of "returns" [N, P], "length" [N], "counts" [N, C, P], "pairs" [N, C2, P, P]),
    `.episodes`, `.open`, `.dropped`, `.columns`, `.index(name)`.  Episodes that end in the middle
    of a step_many launch are counted like any other; no event row goes to the host.
    columns: names like "zap.source", "player_cleaned.player_index", "mining.player[ore_type=2]"
    ("default": `event_columns()`; (): returns and lengths only); pairs: pair columns like
    "zap.source>target".  With columns a step_many call carries the EVENTS row (K x worlds x 2 KB)
    even when events=False; it stays out of the result.  None clears the registration."""
    if columns is None:
      self._eng.clear_episode_stats()
      return None
    if not self._batched:
      raise ValueError("set_episode_stats keeps statistics of a batch of worlds: build the substrate with "
                       "num_worlds > 1")
    self._eng.use_current_stream()
    return self._eng.set_episode_stats(columns, pairs, out)

  def tally_events(self, res_or_rows, columns=None, active=None, ran=None, out=None, pairs=()):
    """`Engine.tally_events` of a step_many result (its `.events`, from events=True) or of a raw
    int32 [K, M, EVENT_ROWS, 4] tensor: int32 [M, C, P] event counts per column and player, summed
    over the steps that ran, on the device."""
    rows = getattr(res_or_rows, "events", res_or_rows)
    if rows is None:
      raise ValueError("tally_events: the result holds no event rows: call step_many(events=True)")
    self._eng.use_current_stream()
    return self._eng.tally_events(rows, columns, active=active, ran=ran, out=out, pairs=pairs)

  # the leaves that are functions of a world's record (engine_lib.STATE_OBS_KINDS)
  _STATE_LEAVES =("RGB", "WORLD.RGB", "LAYER", "READY_TO_SHOOT", "POSITION", "ORIENTATION", "INVENTORY")

  def state_leaves(self) -> Dict[str, int]:
    """The leaves `observe_states` can draw from saved states, with their engine kinds: "RGB"
    (at this substrate's rgb_pool), "WORLD.RGB" (at its world_rgb_pool), "LAYER",
    "READY_TO_SHOOT", "POSITION", "ORIENTATION" and, where the level has one, "INVENTORY"."""
    leaves = {n: self._kinds[n] for n in self._STATE_LEAVES
              if n != "INVENTORY" or int(self._eng.info.num_resources) > 0}
    if getattr(self, "_ego", False):   # (a substrate built with the leaf also draws it from saved states)
      leaves["EGO_LAYER"] = engine_lib.OBS_EGO_LAYER
    if getattr(self, "_wl", False):   # (likewise: the whole map, one block a row)
      leaves["WORLD.LAYER"] = engine_lib.OBS_WORLD_LAYER
    if getattr(self, "_ids", ()):   # (likewise; drawn by a request of their own, MpAvatarIds: no engine kind)
      leaves[AVATAR_IDS_NAMES[0]] = engine_lib.OBS_AVATAR_IDS
      if self._eng.has_zapper:
        leaves[AVATAR_IDS_NAMES[1]] = engine_lib.OBS_AVATAR_IDS
    return leaves

  def _state_leaves(self, observations) -> Dict[str, int]:
    """`observations` of an observe_states call as name -> kind (None: those among this
    substrate's own leaves)."""
    offered = self.state_leaves()
    if observations is None:
      return {n: k for n, k in offered.items() if n in self._obs}
    if isinstance(observations, str):
      observations = (observations,)
    leaves = {}
    for n in observations:
      if n not in offered:
        what = ("a transition leaf: what a step or a reset reports, which no saved state holds"
                if n in self._kinds and n != "INVENTORY" else "no leaf of this substrate")
        raise ValueError(f"observe_states: observation {n!r} is {what}; it can draw {sorted(offered)}")
      leaves[n] = offered[n]
    return leaves

  def observe_states(self, states: WorldStates, observations=None, rows=None,
                     players=None) -> Dict[str, Any]:
    """The observations of saved states (`save_state`, or `step_many(states=True).states`),
    drawn from the rows as they lie: no world of this substrate is loaded or changed, no slot of
    a rollout is written.  `observations`: names among `state_leaves()` (default: those among
    this substrate's own leaves); `rows`: the rows to draw, in order, repeats allowed (default:
    all R of them).  Returns a dict from name to a device tensor [R, ...] ([R, P, ...] for a
    per-player leaf) that holds, for each row, what the leaf held right after the step (or
    reset) the row was saved behind.  `players` (R ints, one per drawn row): the sampled
    (state, player) views of a replay minibatch — every leaf holds player players[i]'s value
    of row i alone and drops its P axis ("RGB" [R, H, W, 3], "LAYER" [R, VH, VW, L], "POSITION"
    [R, 2]), equal to the [arange(R), players] elements of the call without `players`; only the
    sampled views are drawn.  "WORLD.RGB" has no player axis and is left out of the default set
    then.  Ordered on the current stream; no host synchronisation."""
    if players is not None and observations is not None:
      named = (observations,) if isinstance(observations, str) else tuple(observations)
      if "WORLD.RGB" in named:
        raise ValueError("observe_states: \"WORLD.RGB\" is one image per world, not per player: it cannot be "
                         "drawn with players=; draw it in a call of its own")
      if "WORLD.LAYER" in named:
        raise ValueError("observe_states: \"WORLD.LAYER\" is one map per world, not per player: it cannot be "
                         "drawn with players=; draw it in a call of its own")
    leaves = self._state_leaves(observations)
    if not isinstance(states, WorldStates):
      raise ValueError("observe_states takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    self._eng.use_current_stream()
    ego = leaves.pop("EGO_LAYER", None) is not None
    world_layer = leaves.pop("WORLD.LAYER", None) is not None   # (left out with players=, as "WORLD.RGB")
    ids = [leaves.pop(n, None) is not None for n in AVATAR_IDS_NAMES]

    def avatar_ids(out, r, p):   # both leaves by one launch
      if any(ids):
        got = self._eng.observe_avatar_ids(states.data, rows=r, players=p, view=ids[0], zap=ids[1],
                                           fingerprint=states.fingerprint)
        out.update({n: v for n, v in zip(AVATAR_IDS_NAMES, got) if v is not None})
      return out

    if players is None:
      out = {n: self._eng.observe_states(states.data, k, rows=rows, fingerprint=states.fingerprint)
             for n, k in leaves.items()}
      if ego:
        out["EGO_LAYER"] = self._eng.observe_ego_layer(states.data, rows=rows, fingerprint=states.fingerprint)
      if world_layer:
        out["WORLD.LAYER"] = self._eng.observe_world_layer(states.data, rows=rows, fingerprint=states.fingerprint)
      return avatar_ids(out, rows, None)
    p = self._eng._device_ints(players, "players")
    r = None if rows is None else self._eng._device_ints(rows, "rows")
    out = {n: self._eng.observe_views(states.data, k, p, rows=r, fingerprint=states.fingerprint)
           for n, k in leaves.items() if n != "WORLD.RGB"}
    if ego:
      out["EGO_LAYER"] = self._eng.observe_ego_layer(states.data, rows=r, players=p, fingerprint=states.fingerprint)
    return avatar_ids(out, r, p)

  def observe_avatar_ids(self, states: Optional[WorldStates] = None, rows=None, players=None, view: bool = True,
                         zap: Optional[bool] = None):
    """("AVATAR_IDS_IN_VIEW", "AVATAR_IDS_IN_RANGE_TO_ZAP") — the reference's per-avatar
    observations of whom a player sees and whom a zap it fired now could reach — of saved states,
    or of this substrate's worlds as they are now (`states` None; `rows` are then world indices).
    int32 [R, P, P] each, row p the 0/1 vector of player p over the player slots, or [R, P] with
    `players` (R ints: the vector of player players[i] of row rows[i]).  IN_VIEW: both alive and
    q's cell under p's window (1 at q == p).  IN_RANGE: the reference's rays on the avatars' own
    layer, whatever the cooldown — beam blockers of OTHER layers play no part, as in the reference,
    so on a level with such blockers this is the observation, not a prediction of the next beam.
    `zap` None: where the level has a Zapper; True on a level without one raises ValueError, and
    None stands in the pair for the one not worked out.  Any batched substrate draws them, with or
    without the leaves.  Ordered on the current stream; no host synchronisation."""
    if not self._batched:
      raise ValueError("observe_avatar_ids needs a batched substrate (device tensors): build it with num_worlds > 1")
    if zap is None:
      zap = self._eng.has_zapper
    if zap and not self._eng.has_zapper:
      raise ValueError(f"observe_avatar_ids: {self._config.name!r} has no Zapper, so there is no "
                       f"\"{AVATAR_IDS_NAMES[1]}\" (\"{AVATAR_IDS_NAMES[0]}\" works on every level)")
    self._eng.use_current_stream()
    if states is None:
      return self._eng.observe_avatar_ids(None, rows=rows, players=players, view=view, zap=zap)
    if not isinstance(states, WorldStates):
      raise ValueError("observe_avatar_ids takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    return self._eng.observe_avatar_ids(states.data, rows=rows, players=players, view=view, zap=zap,
                                        fingerprint=states.fingerprint)

  def observe_ego_layer(self, states: Optional[WorldStates] = None, rows=None, players=None):
    """"EGO_LAYER" — the layer view in the avatar's own frame: cell (i, j) names the sprites under
    cell (i, j) of "RGB", where "LAYER" (the reference's "N.LAYER") keeps north up whichever way
    the avatar faces — of saved states, or of this substrate's worlds as they are now (`states`
    None; `rows` are then world indices).  int32 [R, P, VH, VW, L], or [R, VH, VW, L] with
    `players` (R ints: the view of player players[i] of row rows[i]).  The ids are "LAYER"'s: no
    facing is encoded, so avatar q's facing in viewer p's frame is (ORIENTATION[q] -
    ORIENTATION[p]) & 3, and oriented beams and kitchen inventories keep their absolute ids.  Any
    batched substrate draws it, with or without the leaf.  Ordered on the current stream; no host
    synchronisation."""
    self._eng.use_current_stream()
    if states is None:
      return self._eng.observe_ego_layer(None, rows=rows, players=players)
    if not isinstance(states, WorldStates):
      raise ValueError("observe_ego_layer takes the WorldStates of save_state or step_many(states=True)")
    states.check(self._eng.state_fingerprint, self._eng.info.world_state_bytes)
    return self._eng.observe_ego_layer(states.data, rows=rows, players=players, fingerprint=states.fingerprint)

  # dmlab2d properties (wrappers/base.py:64-84): Melting Pot's levels register none —
  # the calls exist and answer like dmlab2d does for an unknown key
  def list_property(self, key: str = ""):
    if key:
      raise KeyError(key)
    return []

  def read_property(self, key: str):
    raise KeyError(key)

  def write_property(self, key: str, value):
    raise KeyError(key)

  def step(self, action, active=None, worlds=None) -> TimeStep:
    """Substrate.step (substrate.py:74-81).  `action`: P ints (unbatched), or
    an int tensor / array [N, P] (batched).
    `active` (batched substrates): a uint8 or bool mask [N]; only the worlds it selects step.
    The others are not touched, and their elements of the returned TimeStep's leaves are what
    they were.
    `worlds` (batched substrates): M world indices (a device int32 tensor is read in place);
    `action` is then [M, P] (and `active` [M]) and entry i steps world worlds[i].  The launch has
    one wave per entry, whatever N is; the other worlds are not touched.  The returned TimeStep
    is the full [N] one, with the listed worlds updated."""
    t = self._eng._torch
    if active is not None and not self._batched:
      raise ValueError("active= selects worlds of a batch: build the substrate with num_worlds > 1")
    entries = _step_list(t, worlds, None, self._batched, self._eng.N, self._eng.P, self._T > 0)
    mask = _step_mask(t, active, None, 1, self._eng.N if entries is None else entries, self._eng.device,
                      self._T > 0)
    if self._batched:
      if isinstance(action, t.Tensor) and action.is_cuda:
        a = action.to(t.int32).contiguous()
        if self._check_device_actions:
          K = (len(self._action_rows) if self._action_rows is not None
               else self._eng.num_actions)
          if bool(((a < 0) | (a >= K)).any()):
            raise ValueError(f"actions must be in [0, {K})")
      else:
        a = np.asarray(action)
    else:
      a = np.asarray(action)
      if a.shape != (self._eng.P,):
        raise ValueError(f"Expected {self._eng.P} actions, got shape {a.shape}")
      a = a.reshape(1, self._eng.P)
    self._observables.action.on_next(action)
    self._eng.use_current_stream()
    if entries is not None:
      if tuple(a.shape) != (entries, self._eng.P):
        raise ValueError(f"actions must have shape {(entries, self._eng.P)}, one row per entry of worlds=")
      self._submit_many(a[None], None, False, None, active=mask, keep=(), worlds=worlds)
    else:
      self._submit(a, mask)
    return self._emit(self._timestep())

  def _submit(self, a, active=None):
    """One step of the engine on actions `a` as `step` prepared them (an int32 device tensor
    or a host array [N, P]); `active`: the device mask [N] of a masked step."""
    t = self._eng._torch
    if active is not None:
      self._submit_many(a[None], None, False, None, active=active, keep=())
      return
    if self._action_rows is None:
      self._eng.step(a)
    else:
      # a custom table: its rows go to the engine as raw fields (mp_step_fields)
      K = len(self._action_rows)
      if isinstance(a, t.Tensor):
        if self._action_rows_dev is None:
          self._action_rows_dev = t.from_numpy(self._action_rows).to(self._eng.device)
        # (no host synchronisation on the device path: ids outside the table are the
        # caller's bug and are clamped to its ends; host arrays are validated below)
        self._eng.step_fields(self._action_rows_dev[a.long().clamp_(0, K - 1)].contiguous())
      else:
        a = a.astype(np.int64)
        if a.shape != (self._eng.N, self._eng.P):
          raise ValueError(f"actions must have shape {(self._eng.N, self._eng.P)}")
        if ((a < 0) | (a >= K)).any():
          raise ValueError(f"actions must be in [0, {K})")
        self._eng.step_fields(self._action_rows[a])
    self._submissions += 1

  def step_leaves(self) -> Dict[str, int]:
    """The leaves `step_many(observations=...)` can stack per step: this substrate's own
    observation names other than the pixel ones, with their engine kinds."""
    return {n: self._kinds[n] for n in self._obs
            if n in self._kinds and self._kinds[n] not in engine_lib.PIXEL_KINDS}

  def _many_leaves(self, observations) -> Dict[str, int]:
    """`observations` of a step_many call as name -> kind (True: every leaf of `step_leaves`)."""
    offered = self.step_leaves()
    if observations is True:
      return offered
    if observations is None or observations is False:
      return {}
    if isinstance(observations, str):
      observations = (observations,)
    leaves = {}
    for n in observations:
      if n in AVATAR_IDS_NAMES:
        raise ValueError(f"step_many: \"{n}\" has no per-step rows (it is written by a launch behind the "
                         "submission): take step_many(states=True), then "
                         f"observe_states(result.states, (\"{n}\",)) or observe_avatar_ids(result.states)")
      if n == "EGO_LAYER":
        raise ValueError("step_many: \"EGO_LAYER\" has no per-step rows (it is drawn by a launch behind the "
                         "submission, from the final records): call step_many(states=True) and draw "
                         "observe_states(result.states, (\"EGO_LAYER\",)) or observe_ego_layer(result.states)")
      if n == "WORLD.LAYER":
        raise ValueError("step_many: \"WORLD.LAYER\" has no per-step rows (it is drawn by a launch behind the "
                         "submission, from the final records): call step_many(states=True) and draw "
                         "observe_states(result.states, (\"WORLD.LAYER\",)) or observe_world_layer(result.states)")
      if n not in offered:
        what = ("a pixel leaf: step_many draws no intermediate frames (step with rollout_length=T does)"
                if n in self._obs else "no leaf of this substrate")
        raise ValueError(f"step_many: observation {n!r} is {what}; it can stack {sorted(offered)}")
      if n in leaves:
        raise ValueError(f"step_many: observation {n!r} is named twice")
      leaves[n] = offered[n]
    return leaves

  def step_many(self, actions, repeat: Optional[int] = None, events: bool = False,
                observations=(), states: bool = False, hashes: bool = False,
                active=None, lengths=None, until=None, stopped=None, returns=False,
                gamma: float = 1.0, worlds=None) -> StepManyResult:
    """K steps in ONE launch, bit-identical to K calls of `step` (batched substrates).
    `actions`: ints [K, N, P] (a device tensor is read in place; it may be a column slice
    [:, a:b] of a wider one), or one block [N, P] with `repeat=K`.  Returns the per-step
    `step_type` [K, N], `reward` [K, N, P], `discount` [K, N], `collective_reward` [K, N],
    `events` (the raw int32 [K, N, EVENT_ROWS, 4] tensor with events=True, else None) and
    `timestep`, the TimeStep the K-th `step` would have returned.  It is one submission: with
    `rollout_length=T` it writes one slot (the state after step K), and observations are
    those of the final state.  `observables()`: the action subject gets the whole sequence
    once; the timestep and events subjects get the last step's.
    `observations`: names among this substrate's non-pixel leaves (`step_leaves()`: "LAYER",
    "READY_TO_SHOOT", "INVENTORY", ...), or True for all of them: the result is then a
    `StepManyTrajectory`, whose `.observation[name]` is that leaf of every step, [K, N, ...],
    row k what `step` k would have left in the leaf (kept from the row before wherever a
    step does not write it, e.g. while a world is frozen).
    `states=True`: the result (a `StepManyTrajectory`) has `.states`, the worlds' records after
    every step as a `WorldStates` of K x N rows — step k of world w is row k * N + w, what
    `save_state` would have given after `step` k; it loads with `load_state` and draws with
    `observe_states` like any other.
    `hashes=True`: the result (a `StepManyTrajectory`) has `.hashes`, int64 [K, N]: the state
    hash (`hash_worlds`, the default part) of every world after every step — what `hash_states`
    gives of `.states`' rows, at 8 bytes a world-step instead of a record.  Stored at collection
    time it proves that a regenerated rollout is the original.  Hashes compare only within one
    fingerprint.
    `active`: a uint8 or bool mask [K, N] (or [N], the same row at every step; a device tensor is
    read in place): world w runs step k only where it is non-zero and is not touched elsewhere.
    Row k of every per-step tensor then repeats row k - 1 (row 0: the leaf as it was), so the
    rewards of skipped steps repeat: sum them under the mask.  `lengths`: an int tensor [N]
    instead — world w runs steps 0 .. lengths[w] - 1 (rollouts of different depths).  Not with
    `rollout_length=T`.
    `until`: "last", "reward" or both: a world stops inside the call on the step that leaves it on
    LAST (so a sum of its rewards ends with its episode), or that pays some player; it stands on
    that step and skips the steps behind it as `active` skips a step.  `stopped`: a device uint8
    tensor [N], read and written in place — a world whose byte is non-zero does not run and keeps
    it, a world that stops gets 1 (LAST) | 2 (reward) — which makes the condition persist over
    calls without the host; zero a byte and the world runs again.  `returns=True` (or a float64
    tensor [N, P]): the discounted sum, with `gamma`, of the rewards of the steps each world ran.
    With any of the three the result is a `StepManyUntil` with `.ran`, `.stopped`, `.returns`.
    They combine with `active` / `lengths` and everything above.  Not with `rollout_length=T`.
    `worlds`: M world indices (a device int32 tensor is read in place; a list or array is uploaded
    once): the launch has one wave per ENTRY, whatever N is, and entry i steps world worlds[i]; an
    unlisted world is not touched.  Everything per world above then has M columns, by entry:
    `actions` [K, M, P], `active` [K, M] / `lengths` [M], every per-step tensor [K, M, ...] (row k
    of entry i is what the masked call over all worlds gives for world worlds[i]), `.states` K x M
    rows (step k of entry i is row k * M + i), `.hashes` [K, M], `.ran` [M], `.returns` [M, P] —
    but `stopped` and `.stopped` stay [N], by world, since that tensor persists over calls that
    name different lists, and `.timestep` is the full [N] TimeStep.  An entry that is no world, or
    repeats an earlier entry's world, runs nothing; the next synchronising call raises ValueError
    once.  Not with `rollout_length=T`."""
    if not self._batched:
      raise ValueError("step_many steps a batch of worlds: build the substrate with num_worlds > 1")
    leaves = self._many_leaves(observations)
    t = self._eng._torch
    limit = None
    if self._check_device_actions:
      limit = len(self._action_rows) if self._action_rows is not None else self._eng.num_actions
    entries = _step_list(t, worlds, lengths, True, self._eng.N, self._eng.P, self._T > 0)
    columns = self._eng.N if entries is None else entries
    a, K = _many_actions(t, actions, repeat, columns, self._eng.P, limit)
    mask = _step_mask(t, active, lengths, K, columns, self._eng.device, self._T > 0)
    stop = _step_until(t, until, stopped, returns, gamma, self._eng.N, self._eng.P, self._eng.device,
                       self._T > 0, entries)
    more, out = _until_slice(stop, None, 0, self._eng.N)
    if entries is not None:
      more["worlds"] = worlds
    self._observables.action.on_next(actions)
    self._eng.use_current_stream()
    r = self._submit_many(a, repeat, events, out, leaves, bool(states), bool(hashes), active=mask, **more)
    return _many_result(r, leaves, self._emit(self._timestep()),
                        self._eng.state_fingerprint if states else None)

  def _submit_many(self, a, repeat, events, out, leaves=None, states=False, hashes=False, active=None,
                   **more):
    """One K-step launch of the engine on actions `a` as `_many_actions` prepared them
    (`leaves`: name -> kind of the observations to stack per step; `states`: the records too;
    `hashes`: their hashes; `active`: the device mask of a masked call)."""
    t = self._eng._torch
    if states:
      more["states"] = True
    if active is not None:
      more["active"] = active
    if hashes:
      more["hashes"] = True
    if leaves:
      more["observations"] = tuple(dict.fromkeys(
          k for k in leaves.values() if k not in _FIVE_NAMES))
    if self._action_rows is None:
      r = self._eng.step_many(a, repeat=repeat, events=events, out=out, **more)
    else:
      # a custom table: its rows go to the engine as raw fields, as in `_submit`
      K = len(self._action_rows)
      if isinstance(a, t.Tensor):
        if self._action_rows_dev is None:
          self._action_rows_dev = t.from_numpy(self._action_rows).to(self._eng.device)
        f = self._action_rows_dev[a.long().clamp_(0, K - 1)].contiguous()
      else:
        a = a.astype(np.int64)
        if ((a < 0) | (a >= K)).any():
          raise ValueError(f"actions must be in [0, {K})")
        f = self._action_rows[a]
      r = self._eng.step_many(f, repeat=repeat, fields=True, events=events, out=out, **more)
    self._submissions += 1
    return r

  def observables(self) -> SubstrateObservables:
    """substrate.py:102-104.  `events` emits (name, payload) like the reference —
    of world 0 when the substrate is batched; `events_batched` (batched substrates)
    emits (world, (name, payload)) for every world."""
    return self._observables

  def _emit(self, timestep: TimeStep) -> TimeStep:
    self._observables.timestep.on_next(timestep)
    batched = self._observables.events_batched
    if batched is not None and batched._observers:   # decoding costs a device read
      for world, events in enumerate(self._eng.events_all()):
        for event in events:
          batched.on_next((world, event))
    if self._observables.events._observers:
      for event in self.events(0):
        self._observables.events.on_next(event)
    return timestep

  def events(self, world: int = 0):
    """`Substrate.events()` (wrappers/base.py:72-74) of one world of the batch for
    the last reset()/step(): [(name, {key: int}), ...], canonical order.  The raw
    device tensor for all worlds is `engine.observe(engine.OBS_EVENTS)`."""
    return self._eng.events(world)

  def observation_spec(self) -> List[Mapping[str, Array]]:
    spec = observation_spec_of(self._config, self._eng.pack_bytes, self._rgb_pool,
                               self._world_rgb_pool, len(self._roles))
    return [dict(spec) for _ in self._roles]

  def action_spec(self) -> List[DiscreteArray]:
    spec = self._config.action_spec
    if self._action_rows is not None:
      spec = DiscreteArray(len(self._action_rows), spec.dtype, spec.name)
    # (every player's is named 'action': discrete_action_wrapper.py:103-109)
    return [spec.replace(name="action") for _ in self._roles]

  def reward_spec(self) -> List[Array]:
    return [Array((), np.float64, f"{i + 1}.REWARD") for i in range(len(self._roles))]

  def discount_spec(self) -> BoundedArray:
    return BoundedArray((), np.float64, 0.0, 1.0, "discount")

  def close(self):
    if not self._closed:
      self._closed = True
      self._eng.close()
      for subject in (self._observables.action, self._observables.timestep,
                      self._observables.events, self._observables.events_batched):
        if subject is not None:
          subject.on_completed()

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  # -- shaping -------------------------------------------------------------
  def _timestep(self) -> TimeStep:
    cfg = self._config
    if self._batched and self._T:
      s = self.slot if self._submissions else 0
      ts = RolloutTimeStep(self._step_type[s], self._reward[s], self._discount[s],
                           {n: v[s] for n, v in self._obs.items()})
      ts.slot = s
      return ts
    if self._batched:
      obs = dict(self._obs)
      return TimeStep(self._step_type, self._reward, self._discount, obs)
    # one world: the reference's per-player list of dicts, numpy leaves
    t = self._eng._torch
    self._host.copy_(self._blob, non_blocking=True)
    if self._blob.is_cuda:
      t.cuda.current_stream(self._eng.device).synchronize()
    host = {k: self._host_views[k][0].copy() for k in self._obs}
    reward = self._host_views["#reward"][0].copy()
    per_player = []
    for p in range(self._eng.P):
      d = {}
      for n in cfg.individual_observation_names:
        d[n] = host[n][p]
      for n in cfg.global_observation_names:
        d[n] = host[n]
      d["COLLECTIVE_REWARD"] = host["COLLECTIVE_REWARD"]
      per_player.append(d)
    return TimeStep(StepType(int(self._host_views["#step_type"][0])),
                    [reward[p] for p in range(self._eng.P)],
                    float(self._host_views["#discount"][0]), per_player)


# --------------------------------------------------------------------------
# The factory surface (meltingpot/substrate.py:57-113,
# utils/substrates/substrate_factory.py:24-95, utils/substrates/substrate.py:107-139)

_EXTRA_SPECS = {"POSITION": Array((2,), np.int32, "POSITION"),
                "ORIENTATION": Array((), np.int32, "ORIENTATION"),
                # clean_up's debug metrics (clean_up.py:751-784)
                "PLAYER_CLEANED": Array((), np.float64, "PLAYER_CLEANED"),
                "PLAYER_ATE_APPLE": Array((), np.float64, "PLAYER_ATE_APPLE"),
                "NUM_OTHERS_PLAYER_ZAPPED_THIS_STEP": Array(
                    (), np.float64, "NUM_OTHERS_PLAYER_ZAPPED_THIS_STEP"),
                "NUM_OTHERS_WHO_ATE_THIS_STEP": Array((), np.float64, "NUM_OTHERS_WHO_ATE_THIS_STEP")}


def _classes_by_name(who: str, listed: str, names, groups) -> np.ndarray:
  """A class table over `names` (one per id, "" for an id nothing names): class c for every id a
  name or `fnmatch` pattern of `groups[c]` matches, -1 for every other."""
  table = np.full(len(names), -1, np.int32)
  if isinstance(groups, str):
    groups = (groups,)
  for c, group in enumerate(groups):
    for pattern in ((group,) if isinstance(group, str) else tuple(group)):
      if not isinstance(pattern, str):
        raise ValueError(f"{who}: {pattern!r} is no name or pattern")
      ids = [i for i, n in enumerate(names) if n and fnmatch.fnmatchcase(n, pattern)]
      if not ids:
        raise ValueError(f"{who}: {pattern!r} matches no id of this level ({listed}: "
                         f"{[n for n in names if n]})")
      for i in ids:
        if table[i] not in (-1, c):
          raise ValueError(f"{who}: id {i} ({names[i]!r}) is matched by class {int(table[i])} and by "
                           f"class {c} ({pattern!r})")
        table[i] = c
  return table


def world_layer_spec(pack_bytes: bytes) -> Array:
  """"WORLD.LAYER" of a pack: the whole map as int32 sprite ids, one per render layer — (H, W, L);
  0 is nothing, 1 + k sprite k of the world's sprite map."""
  from meltingpot_amd import lower, pack as pack_lib
  hdr = pack_lib.loads(pack_bytes)["hdr"]
  return Array((int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W]), int(hdr[lower.HDR_L])), np.int32, "WORLD.LAYER")


def layer_spec(pack_bytes: bytes) -> Array:
  """"LAYER" of a pack (avatar_library.lua:246-257, A17): the player's window with orientation
  'N' as int32 sprite ids, one per render layer — (VH, VW, L); 0 is nothing, 1 + k sprite k."""
  from meltingpot_amd import lower, pack as pack_lib
  hdr = pack_lib.loads(pack_bytes)["hdr"]
  return Array((int(hdr[lower.HDR_VF]) + int(hdr[lower.HDR_VB]) + 1,
                int(hdr[lower.HDR_VL]) + int(hdr[lower.HDR_VR]) + 1, int(hdr[lower.HDR_L])),
               np.int32, "LAYER")


# the reference's per-avatar observations of players (avatar_library.lua:1204-1315; MpAvatarIds)
AVATAR_IDS_NAMES = ("AVATAR_IDS_IN_VIEW", "AVATAR_IDS_IN_RANGE_TO_ZAP")


def avatar_ids_specs(names: Sequence[str], num_players: int) -> Dict[str, Array]:
  """The specs of those of AVATAR_IDS_NAMES among `names`: a 0/1 int32 vector over the player slots."""
  return {n: Array((int(num_players),), np.int32, n) for n in AVATAR_IDS_NAMES if n in names}


def ego_layer_spec(pack_bytes: bytes) -> Array:
  """"EGO_LAYER" of a pack: "LAYER"'s shape and dtype, the window turned with the avatar."""
  return Array(layer_spec(pack_bytes).shape, np.int32, "EGO_LAYER")


def observation_spec_of(config: SubstrateConfig, pack_bytes: bytes, rgb_pool: int = 1,
                        world_rgb_pool: int = 1, num_players: Optional[int] = None) -> Dict[str, Array]:
  """One player's observation spec of a `Substrate` built from `config` and `pack_bytes` with
  these pooling factors (what its `observation_spec()` hands out per player).  `num_players`: the
  length of the AVATAR_IDS_* vectors (default: the config's default roles)."""
  spec = dict(config.timestep_spec)
  if "WORLD.LAYER" in config.global_observation_names:   # (beside "WORLD.RGB", among the global leaves)
    spec["WORLD.LAYER"] = world_layer_spec(pack_bytes)
  spec["COLLECTIVE_REWARD"] = Array((), np.float64, "COLLECTIVE_REWARD")
  if rgb_pool > 1 and "RGB" in spec:
    h, w, c = spec["RGB"].shape
    spec["RGB"] = Array((h // rgb_pool, w // rgb_pool, c), spec["RGB"].dtype, "RGB")
  if world_rgb_pool > 1 and "WORLD.RGB" in spec:
    k = world_rgb_pool
    h, w, c = spec["WORLD.RGB"].shape
    spec["WORLD.RGB"] = Array((h // k, w // k, c), spec["WORLD.RGB"].dtype, "WORLD.RGB")
  if "LAYER" in config.individual_observation_names:
    spec["LAYER"] = layer_spec(pack_bytes)
  if "EGO_LAYER" in config.individual_observation_names:
    spec["EGO_LAYER"] = ego_layer_spec(pack_bytes)
  spec.update(avatar_ids_specs(config.individual_observation_names,
                               len(config.default_player_roles) if num_players is None else num_players))
  return spec


def select_observations(config: SubstrateConfig, pack_bytes: bytes,
                        individual_observations: Sequence[str],
                        global_observations: Sequence[str]):
  """`build_substrate`'s choice of leaves (multiplayer_wrapper.py:108-167): the config's
  individual observations that are asked for, in the config's order, then the other names
  asked for (POSITION, LAYER, ... — unknown ones are refused when the substrate is built);
  the global ones as given.  Returns (individual, global, timestep_spec)."""
  individual = [n for n in config.individual_observation_names if n in set(individual_observations)]
  individual += [n for n in individual_observations if n not in individual]   # (unknown ones: refused below)
  spec = dict(config.timestep_spec)
  for n in list(individual) + list(global_observations):
    if n in _EXTRA_SPECS:
      spec[n] = _EXTRA_SPECS[n]
  if "LAYER" in individual:
    spec["LAYER"] = layer_spec(pack_bytes)
  if "EGO_LAYER" in individual:
    spec["EGO_LAYER"] = ego_layer_spec(pack_bytes)
  if "WORLD.LAYER" in global_observations:
    spec["WORLD.LAYER"] = world_layer_spec(pack_bytes)
  spec.update(avatar_ids_specs(individual, len(config.default_player_roles)))
  wanted = set(individual) | set(global_observations)
  return individual, list(global_observations), {n: sp for n, sp in spec.items() if n in wanted}


def timestep_spec_of(observation_spec: Mapping[str, Array]) -> TimeStep:
  """utils/substrates/specs.py:149-166 `specs.timestep`: the spec of the timestep ONE
  player sees — step_type / reward / discount specs + the observation specs, each
  named after its key."""
  return TimeStep(
      step_type=BoundedArray((), np.int64, int(min(StepType)), int(max(StepType)), "step_type"),
      reward=Array((), np.float64, "reward"),
      discount=BoundedArray((), np.float64, 0, 1, "discount"),
      observation={n: sp.replace(name=n) for n, sp in observation_spec.items()})


def build_substrate(*, lab2d_settings: Mapping[str, Any],
                    individual_observations: Sequence[str],
                    global_observations: Sequence[str],
                    action_table: Sequence[Mapping[str, int]],
                    num_worlds: int = 1, **kwargs) -> Substrate:
  """utils/substrates/substrate.py:107-139 — on the HIP engine, for N worlds at once.

  `lab2d_settings` is ANY settings dict of a level the engine implements (what a
  reference config's `build(roles, config)` returns, or one the caller has edited): it
  is lowered here, at run time (`builder.lower_settings`), and the substrate runs THAT —
  no committed pack is consulted.  `individual_observations` / `global_observations`
  choose the leaves of a player's observation as in the reference (the multiplayer
  wrapper, multiplayer_wrapper.py:108-167; COLLECTIVE_REWARD is always added,
  collective_reward_wrapper.py:25-50); `action_table[i]` is what discrete action i does
  (discrete_action_wrapper.py:77-109; it is lowered into the pack, the lookup happens
  on the device).  The number of players is the settings' `numPlayers`.  Further
  keyword arguments are `Substrate`'s (num_worlds, env_seed, device, rollout_length...)."""
  from meltingpot_amd import builder as builder_lib   # (it imports this module)
  if not action_table:
    raise ValueError("action_table must not be empty")
  table = tuple(dict(row) for row in action_table)
  level, pack_bytes, config = builder_lib.lower_settings(lab2d_settings, action_set=table)
  from meltingpot_amd import pack as pack_lib
  tables = pack_lib.loads(pack_bytes)
  names = tuple(n.decode() for n in bytes(tables["action_names"]).split(b"\0")[:-1])
  ranges = tuple(tuple(int(v) for v in row) for row in tables["action_spec"].reshape(-1, 3))
  validate_action_table(table, names, ranges)   # discrete_action_wrapper.py:28-49
  individual, global_names, spec = select_observations(config, pack_bytes, individual_observations,
                                                       global_observations)
  config = SubstrateConfig(
      name=level, action_set=table, individual_observation_names=individual,
      global_observation_names=global_names, timestep_spec=spec,
      valid_roles=config.valid_roles, default_player_roles=config.default_player_roles,
      aux0_name=config.aux0_name)
  return Substrate(config, config.default_player_roles, pack_bytes,
                   num_worlds=num_worlds, **kwargs)


class SubstrateFactory:
  """utils/substrates/substrate_factory.py:24-95, same constructor and methods;
  `build(roles, **kwargs)` also takes `Substrate`'s keyword arguments (`num_worlds`,
  `env_seed`, `rollout_length`...)."""

  def __init__(self, *, lab2d_settings_builder, individual_observations, global_observations,
               action_table, timestep_spec, action_spec, valid_roles, default_player_roles):
    self._lab2d_settings_builder = lab2d_settings_builder
    self._individual_observations = frozenset(individual_observations)
    self._global_observations = frozenset(global_observations)
    self._action_table = tuple(dict(row) for row in action_table)
    self._timestep_spec = timestep_spec
    self._action_spec = action_spec
    self._valid_roles = frozenset(valid_roles)
    self._default_player_roles = tuple(default_player_roles)
    self._packed = None   # (config, pack name): `from_packed_config`

  @classmethod
  def from_packed_config(cls, config: SubstrateConfig) -> "SubstrateFactory":
    """The factory of a substrate this package carries as a committed pack
    (`get_config(name)`, possibly edited): the config is checked against the pack —
    what it says and the pack cannot do is refused (`check_config_against_pack`), an
    edited `action_set` runs as a custom action table, edited observation lists pick
    the leaves."""
    # (like the reference configs' `timestep_spec`: without COLLECTIVE_REWARD, which the
    # built substrate's observation_spec() adds)
    obs = dict(config.timestep_spec)
    f = cls(lab2d_settings_builder=None,
            individual_observations=config.individual_observation_names,
            global_observations=config.global_observation_names,
            action_table=config.action_set, timestep_spec=timestep_spec_of(obs),
            action_spec=DiscreteArray(len(config.action_set)),
            valid_roles=config.valid_roles, default_player_roles=config.default_player_roles)
    f._packed = config
    return f

  def valid_roles(self):
    return self._valid_roles

  def default_player_roles(self):
    return self._default_player_roles

  def timestep_spec(self) -> TimeStep:
    return self._timestep_spec

  def action_spec(self) -> DiscreteArray:
    return self._action_spec

  def build(self, roles: Sequence[str], **kwargs) -> Substrate:
    if self._packed is not None:
      config = self._packed
      pack_bytes = engine_lib.load_pack(config.name)
      custom = check_config_against_pack(config, pack_bytes, len(roles))
      if custom is not None:
        kwargs.setdefault("action_table", custom)
      return Substrate(config, roles, pack_bytes, **kwargs)
    return build_substrate(
        lab2d_settings=self._lab2d_settings_builder(roles),
        individual_observations=self._individual_observations,
        global_observations=self._global_observations,
        action_table=self._action_table, **kwargs)


def check_config_against_pack(config: SubstrateConfig, pack_bytes: bytes, num_players: int):
  """What a (possibly edited) `SubstrateConfig` says, held against the committed pack
  it names.  Raises ValueError for what the pack cannot honour — observation specs of
  another geometry, more players than it was lowered for — so that an edited config
  never runs the stock substrate silently.  Returns the config's `action_set` when it
  differs from the pack's (it then runs as a custom action table), else None."""
  from meltingpot_amd import lower, pack as pack_lib
  t = pack_lib.loads(pack_bytes)
  hdr = t["hdr"]
  P = int(hdr[lower.HDR_P])
  if num_players > P:
    raise ValueError(f"{num_players} roles, but the committed pack of {config.name!r} was "
                     f"lowered for at most {P} players")
  S = int(hdr[lower.HDR_SPRITE])
  want = {"RGB": ((int(hdr[lower.HDR_VF]) + int(hdr[lower.HDR_VB]) + 1) * S,
                  (int(hdr[lower.HDR_VL]) + int(hdr[lower.HDR_VR]) + 1) * S, 3),
          "WORLD.RGB": (int(hdr[lower.HDR_H]) * S, int(hdr[lower.HDR_W]) * S, 3),
          "LAYER": layer_spec(pack_bytes).shape, "EGO_LAYER": layer_spec(pack_bytes).shape,
          "WORLD.LAYER": world_layer_spec(pack_bytes).shape}
  for n, shape in want.items():
    if n in config.timestep_spec and tuple(config.timestep_spec[n].shape) != shape:
      raise ValueError(
          f"config.timestep_spec[{n!r}] has shape {tuple(config.timestep_spec[n].shape)}, the "
          f"committed pack of {config.name!r} renders {shape}: a config that changes the map, "
          "the window or the sprite size needs its lab2d settings — build it with "
          "build_substrate(lab2d_settings=...) or from the reference's config "
          "(get_factory_from_config), which are lowered at run time")
  names = tuple(n.decode() for n in bytes(t["action_names"]).split(b"\0")[:-1])
  ranges = tuple(tuple(int(v) for v in row) for row in t["action_spec"].reshape(-1, 3))
  rows = validate_action_table(config.action_set, names, ranges)
  stock = np.asarray(t["action_table"], np.int32).reshape(-1, 4)[:, :len(names)]
  if rows.shape == stock.shape and np.array_equal(rows, stock):
    return None
  return tuple(dict(r) for r in config.action_set)


def get_factory_from_config(config) -> SubstrateFactory:
  """meltingpot/substrate.py:98-113.  `config` is either
    * a reference substrate config (an `ml_collections.ConfigDict` with
      `lab2d_settings_builder`, as `meltingpot.substrate.get_config` /
      `meltingpot.configs.substrates.get_config` return it — edited or not): the
      factory builds its lab2d settings for the roles and lowers THEM at run time,
      exactly what the config says; or
    * this package's `SubstrateConfig` (`get_config(name)`): the committed pack, with
      the config checked against it (`SubstrateFactory.from_packed_config`)."""
  if isinstance(config, SubstrateConfig):
    return SubstrateFactory.from_packed_config(config)
  if not hasattr(config, "lab2d_settings_builder"):
    raise TypeError("get_factory_from_config wants a SubstrateConfig of this package or a "
                    "reference substrate config with `lab2d_settings_builder`")

  def lab2d_settings_builder(roles):
    return config.lab2d_settings_builder(roles=roles, config=config)

  return SubstrateFactory(
      lab2d_settings_builder=lab2d_settings_builder,
      individual_observations=config.individual_observation_names,
      global_observations=config.global_observation_names,
      action_table=config.action_set,
      timestep_spec=config.timestep_spec,
      action_spec=config.action_spec,
      valid_roles=config.valid_roles,
      default_player_roles=config.default_player_roles)


def get_factory(name: str) -> SubstrateFactory:
  """meltingpot/substrate.py:92-95."""
  return get_factory_from_config(get_config(name))


def build(name: str, *, roles: Sequence[str], num_worlds: int = 1,
          **kwargs) -> Substrate:
  """reference: meltingpot/substrate.py:57-72 — plus `num_worlds` (and the other
  keyword arguments of `Substrate`)."""
  return get_factory(name).build(roles, num_worlds=num_worlds, **kwargs)


def build_from_config(config, *, roles: Sequence[str], num_worlds: int = 1,
                      **kwargs) -> Substrate:
  """reference: meltingpot/substrate.py:75-89.  The substrate that runs is the one the
  config DESCRIBES (`get_factory_from_config`): a reference config's own lab2d
  settings lowered at run time, or a `SubstrateConfig` checked against its pack."""
  return get_factory_from_config(config).build(roles, num_worlds=num_worlds, **kwargs)


# --------------------------------------------------------------------------
# Mixtures: several layouts of one level behind one batched Substrate


# Every pixel leaf of a member starts on a 16-byte boundary: the engine stages a pooled view
# (MP_OBS_RGB_POOL*, a pooled WORLD.RGB) by 16-byte lines and refuses any other buffer; a full
# view is a multiple of 192 bytes a world (3 x 8 x 8 a cell), so it never adds to the granule.
_PIXEL_ALIGN = 16
_PIXEL_LEAVES = ("RGB", "WORLD.RGB")


def leaf_bytes_per_world(config: SubstrateConfig, pack_bytes: bytes, num_players: int,
                         rgb_pool: int = 1, world_rgb_pool: int = 1) -> Dict[str, int]:
  """Bytes of one world of every leaf a batched `Substrate` of `config` binds (the
  observations, "COLLECTIVE_REWARD" and the "#reward", "#discount", "#step_type" leaves)."""
  spec = observation_spec_of(config, pack_bytes, rgb_pool, world_rgb_pool, num_players)
  out = {}
  for n, sp in spec.items():
    count = num_players if n in config.individual_observation_names else 1
    out[n] = count * int(np.prod(sp.shape, dtype=np.int64)) * sp.dtype.itemsize
  out.update({"#reward": 8 * num_players, "#discount": 8, "#step_type": 4})
  return out


def world_granule(bytes_per_world: Mapping[str, int]) -> int:
  """The smallest world count g such that a member that starts at a multiple of g worlds
  starts every leaf on the boundary the engine wants of it: 16 bytes for the pixel views,
  the element for the rest (which any offset gives).  E.g. clean_up's RGB pooled by 8 is
  11 x 11 x 3 x 7 = 2541 B a world: g = 16."""
  g = 1
  for n, b in bytes_per_world.items():
    if n in _PIXEL_LEAVES and b:
      need = _PIXEL_ALIGN // math.gcd(int(b), _PIXEL_ALIGN)
      g = g * need // math.gcd(g, need)
  return g


def split_worlds(num_worlds, members: int, granule: int) -> List[int]:
  """World counts of `members` members: `num_worlds` is one count per member, each rounded UP
  to a multiple of `granule`, or a total split as evenly as the granule allows (whole granules,
  the first members one more; at least one granule each, so the total can grow by less than
  `granule` — or to `members * granule`)."""
  if isinstance(num_worlds, (int, np.integer)) and not isinstance(num_worlds, bool):
    if num_worlds < 1:
      raise ValueError(f"num_worlds must be positive, got {num_worlds}")
    units = max(members, -(-int(num_worlds) // granule))
    base, extra = divmod(units, members)
    return [(base + (1 if i < extra else 0)) * granule for i in range(members)]
  counts = [int(n) for n in num_worlds]
  if len(counts) != members:
    raise ValueError(f"{len(counts)} world counts for {members} members")
  if any(n < 1 for n in counts):
    raise ValueError(f"every member needs at least one world, got num_worlds={counts}")
  return [-(-n // granule) * granule for n in counts]


class _SharedLeaves:
  """One tensor per leaf for all N worlds of a mixture ([T, N, ...] with a ring), allocated
  when the first member asks for it; member i binds worlds [off_i, off_i + n_i) of it.

  A ring's slot holds all N worlds; when N x bytes-per-world is not a multiple of 256 (the
  slot stride mp_bind_output_ring takes) the slot is padded and the leaf is a strided view of
  the padded allocation, so that `leaf[t]` is still [N, ...]."""

  def __init__(self, total: int, slots: int):
    self.total, self.slots = total, slots
    self.leaves: Dict[str, Any] = {}

  def _allocate(self, name, world_shape, dtype, device):
    import torch
    item = torch.empty((), dtype=dtype).element_size()
    per_world = int(np.prod(world_shape, dtype=np.int64)) * item
    # large pixel leaves from scattered 2 MB chunks, like the engine's own views (memory.py)
    mapped = name in _PIXEL_LEAVES and device.type == "cuda"
    if mapped:
      from meltingpot_amd import memory
      ctx = memory.mapped_allocations(device)
    else:
      import contextlib
      ctx = contextlib.nullcontext()
    shape = (self.total,) + tuple(world_shape)
    with ctx:
      if not self.slots:
        return torch.empty(shape, dtype=dtype, device=device)
      stride = -(-self.total * per_world // 256) * 256
      if stride == self.total * per_world:
        return torch.empty((self.slots,) + shape, dtype=dtype, device=device)
      flat = torch.empty(self.slots * stride // item, dtype=dtype, device=device)
    inner = torch.empty(shape, dtype=dtype, device="meta").stride()
    return flat.as_strided((self.slots,) + shape, (stride // item,) + tuple(inner))

  def take(self, name: str, shape, dtype, offset: int, device):
    """The slice of leaf `name` for a member whose engine wants `shape` ([n, ...]) at world
    `offset`."""
    n, world_shape = int(shape[0]), tuple(shape[1:])
    leaf = self.leaves.get(name)
    if leaf is None:
      leaf = self.leaves[name] = self._allocate(name, world_shape, dtype, device)
    have = tuple(leaf.shape[2:] if self.slots else leaf.shape[1:])
    if have != world_shape or leaf.dtype != dtype:
      raise ValueError(f"leaf {name!r}: one member's engine writes {world_shape} {dtype}, another's "
                       f"{have} {leaf.dtype}")
    return leaf[:, offset:offset + n] if self.slots else leaf[offset:offset + n]


class MixtureSubstrate:
  """Several substrates of one level — layouts, maps, payoffs — stepped as ONE batched
  `Substrate` of N = sum(n_i) worlds (`build_mixture`).

  Member i owns worlds [off_i, off_i + n_i) (`member_slice(i)`, `member_of_world`); its engine
  writes straight into that slice of every leaf, so the leaves are [N, P, ...] / [N, ...]
  tensors (and, with `rollout_length=T`, slots of [T, N, ...] rings) that nothing copies or
  concatenates.  A step is each member's own step launch on the current stream, in member order.
  Mixture world g is world g - off_i of member i, created with world_offset + off_i: it is the
  world a one-world `Substrate` of that member built with `world_offset=g` (same env_seed) runs."""

  def __init__(self, members: Sequence[Substrate], names: Sequence[str], offsets: Sequence[int],
               counts: Sequence[int], leaves: _SharedLeaves, check_device_actions: bool):
    self._members = tuple(members)
    self._names = tuple(names)
    self._offsets = tuple(int(o) for o in offsets)
    self._counts = tuple(int(n) for n in counts)
    self._shared = leaves
    self._N = sum(self._counts)
    self._T = leaves.slots
    self._check_device_actions = bool(check_device_actions)
    self._submissions = 0
    first = self._members[0]
    self._P = first.num_players
    self._obs = {n: leaves.leaves[n] for n in first._obs}
    self._reward = leaves.leaves["#reward"]
    self._discount = leaves.leaves["#discount"]
    self._step_type = leaves.leaves["#step_type"]
    t = first._eng._torch
    self._member_of_world = t.repeat_interleave(
        t.arange(len(self._members), dtype=t.int32),
        t.tensor(self._counts, dtype=t.int64)).to(first._eng.device)
    self._closed = False
    self._observables = SubstrateObservables(Subject(), Subject(), Subject(), Subject())

  # -- the mixture -----------------------------------------------------------
  @property
  def members(self) -> Tuple[str, ...]:
    """The members' substrate names, in world order."""
    return self._names

  @property
  def member_of_world(self):
    """int32 [N] device tensor: the member index of every world."""
    return self._member_of_world

  def member_slice(self, i: int) -> slice:
    """Worlds [off_i, off_i + n_i) of member i, as a slice of the leading world axis."""
    return slice(self._offsets[i], self._offsets[i] + self._counts[i])

  @property
  def engines(self) -> Tuple[engine_lib.Engine, ...]:
    return tuple(m.engine for m in self._members)

  def counters(self) -> Dict[str, int]:
    """mp_counters summed over the members."""
    out: Dict[str, int] = {}
    for m in self._members:
      for k, v in m.engine.counters().items():
        out[k] = out.get(k, 0) + v
    return out

  # -- the batched Substrate surface ----------------------------------------
  @property
  def num_worlds(self) -> int:
    return self._N

  @property
  def num_players(self) -> int:
    return self._P

  @property
  def rollout(self) -> Optional[Dict[str, Any]]:
    """As `Substrate.rollout`: the [T, N, ...] rings of all members, None without a ring."""
    if not self._T:
      return None
    return {"step_type": self._step_type, "reward": self._reward,
            "discount": self._discount, "observation": dict(self._obs)}

  @property
  def slot(self) -> int:
    """As `Substrate.slot` (every submission goes to every member: their rings move together)."""
    return self._members[0].slot if self._T else -1

  def reset(self) -> TimeStep:
    for m in self._members:
      m._eng.use_current_stream()
      m._eng.reset()
      m._submissions += 1
    self._submissions += 1
    return self._emit(self._timestep())

  def observation(self):
    return self._timestep().observation

  def step(self, action, active=None, worlds=None) -> TimeStep:
    """`action`: int [N, P], a device tensor (member i gets rows [off_i, off_i + n_i), a view)
    or a host array.  `active`: a mask [N] as `Substrate.step` takes it; member i reads its
    elements [off_i, off_i + n_i) of it in place."""
    t = self._members[0]._eng._torch
    if worlds is not None:
      raise ValueError("worlds= is not offered by a mixture: splitting a global list per member on the device "
                       "is not built; step the members' substrates on their own, or use active=")
    mask = _step_mask(t, active, None, 1, self._N, self._members[0]._eng.device,
                      any(m._T > 0 for m in self._members))
    if isinstance(action, t.Tensor) and action.is_cuda:
      a = action.to(t.int32).contiguous()
      if tuple(a.shape) != (self._N, self._P):
        raise ValueError(f"actions must have shape {(self._N, self._P)}, got {tuple(a.shape)}")
      if self._check_device_actions:
        K = self.action_spec()[0].num_values
        if bool(((a < 0) | (a >= K)).any()):
          raise ValueError(f"actions must be in [0, {K})")
    else:
      a = np.asarray(action)
      if a.shape != (self._N, self._P):
        raise ValueError(f"actions must have shape {(self._N, self._P)}, got {a.shape}")
    self._observables.action.on_next(action)
    for m, off, n in zip(self._members, self._offsets, self._counts):
      m._eng.use_current_stream()
      m._submit(a[off:off + n], None if mask is None else mask[..., off:off + n])
    self._submissions += 1
    return self._emit(self._timestep())

  def step_leaves(self) -> Dict[str, int]:
    return self._members[0].step_leaves()

  def set_episode_starts(self, states_per_member, rows=None, *, fresh: bool = False,
                         check: Optional[bool] = None):
    """`Substrate.set_episode_starts` per member: `states_per_member[i]` is member i's bank (a
    `WorldStates` of that member's fingerprint) or None (member i keeps, or returns to, the
    level's own reset).  Returns ONE int32 [N] device tensor `rows` (allocated and filled with -1
    when None): member i reads its slice `rows[member_slice(i)]` in place, nothing is copied, and
    an entry is a row of THAT member's bank."""
    states_per_member = list(states_per_member)
    if len(states_per_member) != len(self._members):
      raise ValueError(f"set_episode_starts: {len(self._members)} members, {len(states_per_member)} banks")
    t = self._members[0]._eng._torch
    device = self._members[0]._eng.device
    if rows is None:
      rows = t.full((self._N,), -1, dtype=t.int32, device=device)
    elif (not isinstance(rows, t.Tensor) or rows.dtype != t.int32 or tuple(rows.shape) != (self._N,) or
          not rows.is_contiguous()):
      raise ValueError(f"set_episode_starts: rows must be a contiguous int32 tensor [{self._N}]")
    for m, states, off, n in zip(self._members, states_per_member, self._offsets, self._counts):
      m.set_episode_starts(states, None if states is None else rows[off:off + n], fresh=fresh, check=check)
    return rows

  def observe_ego_layer(self):
    """`Substrate.observe_ego_layer()` of the worlds as they are now: ONE int32 [N, P, VH, VW, L]
    device tensor of which every member draws its slice (saved states are a member's own: draw
    them with that member's fingerprint)."""
    eng = self._members[0]._eng
    t = eng._torch
    out = t.empty((self._N,) + tuple(eng.ego_layer_shape[1:]), dtype=t.int32, device=eng.device)
    for m, off, n in zip(self._members, self._offsets, self._counts):
      if tuple(m._eng.ego_layer_shape[1:]) != tuple(out.shape[1:]):
        raise ValueError(f"observe_ego_layer: one member's view is {tuple(out.shape[1:])}, another's "
                         f"{tuple(m._eng.ego_layer_shape[1:])}")
      m._eng.use_current_stream()
      m._eng.observe_ego_layer(None, out=out[off:off + n])
    return out

  def observe_avatar_ids(self, view: bool = True, zap: Optional[bool] = None):
    """`Substrate.observe_avatar_ids()` of the worlds as they are now: ONE int32 [N, P, P] device
    tensor each, of which every member writes its slice.  `zap` None: where every member has a
    Zapper; True raises ValueError if one has none."""
    eng = self._members[0]._eng
    t = eng._torch
    have = all(m._eng.has_zapper for m in self._members)
    if zap and not have:
      lacking = [n for n, m in zip(self._names, self._members) if not m._eng.has_zapper]
      raise ValueError(f"observe_avatar_ids: {lacking} have no Zapper, so there is no \"{AVATAR_IDS_NAMES[1]}\"")
    zap = have if zap is None else bool(zap)
    if not view and not zap:
      raise ValueError("observe_avatar_ids: neither view nor zap is asked for")
    shape = (self._N, self._P, self._P)
    out = tuple(t.empty(shape, dtype=t.int32, device=eng.device) if want else None for want in (view, zap))
    for m, off, n in zip(self._members, self._offsets, self._counts):
      m._eng.use_current_stream()
      m._eng.observe_avatar_ids(None, view=view, zap=zap, out=tuple(None if o is None else o[off:off + n] for o in out))
    return out

  def hash_views(self, layers=None, classes=None):
    """`Substrate.hash_views()` of the worlds as they are now: ONE int64 [N, P] device tensor of
    which every member writes its slice.  A hash compares only with hashes of the SAME member: the
    members' fingerprints differ."""
    eng = self._members[0]._eng
    t = eng._torch
    out = t.empty((self._N, self._P), dtype=t.int64, device=eng.device)
    for m, off, n in zip(self._members, self._offsets, self._counts):
      m._eng.use_current_stream()
      m._eng.hash_views(None, layers=m._view_layers(layers), classes=classes, out=out[off:off + n])
    return out

  def set_view_hashes(self, layers="all", classes=None):
    """`Substrate.set_view_hashes` for the mixture: ONE int64 [N, P] device tensor ([T, N, P] with
    rollout_length=T) of which member i registers its slice in place.  None clears every member's
    registration."""
    if layers is None:
      for m in self._members:
        m.set_view_hashes(None)
      return None
    eng = self._members[0]._eng
    t = eng._torch
    out = t.zeros(((self._T,) if self._T else ()) + (self._N, self._P), dtype=t.int64, device=eng.device)
    for m, off, n in zip(self._members, self._offsets, self._counts):
      m.set_view_hashes(layers, classes, out=out[:, off:off + n] if self._T else out[off:off + n])
    return out

  def layer_classes(self, groups) -> List[np.ndarray]:
    """`Substrate.layer_classes(groups)` of every member, in order: the members of a mixture may
    number the same sprites differently, so a table by name is one table a member — what
    `observe_ego_planes` and `set_ego_planes` of the mixture take as `classes`."""
    return [m.layer_classes(groups) for m in self._members]

  def _planes_of_members(self, classes, num_classes, facing):
    """((VH, VW), C, a class table per member): a mixture's planes are one tensor, so the members
    must agree on (VH, VW) and C.  `classes`: one table for every member, or a list of one a member."""
    shapes = {m._eng.ego_layer_shape[2:4] for m in self._members}
    if len(shapes) != 1:
      raise ValueError(f"ego planes of a mixture: the members' views differ ({sorted(shapes)} as (VH, VW))")
    t = self._members[0]._eng._torch
    per_member = (isinstance(classes, (list, tuple)) and len(classes) > 0 and
                  all(isinstance(c, (np.ndarray, t.Tensor, list, tuple)) for c in classes))
    tables = list(classes) if per_member else [classes] * len(self._members)
    if len(tables) != len(self._members):
      raise ValueError(f"ego planes of a mixture: {len(tables)} class tables for {len(self._members)} members")
    if num_classes is None:
      num_classes = 1 + max(int(c.max()) if isinstance(c, t.Tensor) else int(np.max(np.asarray(c))) for c in tables)
    return next(iter(shapes)), int(num_classes), tables

  def observe_ego_planes(self, classes, layers=None, facing: bool = False, num_classes: Optional[int] = None):
    """`Substrate.observe_ego_planes(classes)` of the worlds as they are now: ONE uint8
    [N, P, C', VH, VW] device tensor of which every member writes its slice.  The members must agree
    on (VH, VW); `classes` is one table for all of them, or a list of one table a member
    (`layer_classes(groups)`: members may number the same sprites differently)."""
    (VH, VW), C, tables = self._planes_of_members(classes, num_classes, facing)
    eng = self._members[0]._eng
    t = eng._torch
    out = t.empty((self._N, self._P, C + (4 if facing else 0), VH, VW), dtype=t.uint8, device=eng.device)
    for m, off, n, table in zip(self._members, self._offsets, self._counts, tables):
      if not m._batched:
        raise ValueError("observe_ego_planes needs batched members (device tensors)")
      m._eng.use_current_stream()
      m._eng.observe_ego_planes(table, None, layers=m._view_layers(layers), facing=facing, num_classes=C,
                                out=out[off:off + n])
    return out

  def set_ego_planes(self, classes, layers="all", facing: bool = False, num_classes: Optional[int] = None):
    """`Substrate.set_ego_planes` for the mixture: ONE uint8 [N, P, C', VH, VW] device tensor
    ([T, N, P, C', VH, VW] with rollout_length=T) of which member i registers its slice in place.
    `classes`: as `observe_ego_planes` of the mixture takes it.  None clears every member's
    registration."""
    if classes is None:
      for m in self._members:
        m.set_ego_planes(None)
      return None
    (VH, VW), C, tables = self._planes_of_members(classes, num_classes, facing)
    eng = self._members[0]._eng
    t = eng._torch
    out = t.zeros(((self._T,) if self._T else ()) + (self._N, self._P, C + (4 if facing else 0), VH, VW),
                  dtype=t.uint8, device=eng.device)
    for m, off, n, table in zip(self._members, self._offsets, self._counts, tables):
      m.set_ego_planes(table, layers, facing, out=out[:, off:off + n] if self._T else out[off:off + n], num_classes=C)
    return out

  def event_columns(self):
    return self._members[0].event_columns()

  def set_episode_stats(self, columns="default", pairs=()):
    """`Substrate.set_episode_stats` for the mixture: ONE set of [N, ...] statistics tensors, of
    which member i registers its slice `[member_slice(i)]` in place (the world axis leads every
    tensor, so a slice is contiguous).  None clears every member's registration."""
    if columns is None:
      for m in self._members:
        m.set_episode_stats(None)
      return None
    eng = self._members[0]._eng
    t = eng._torch
    if isinstance(columns, str) and columns == "default":
      columns = self.event_columns()
    names, _ = engine_lib._column_array(columns, engine_lib.STATS_MAX_COLUMNS, False, "set_episode_stats")
    pnames, _ = engine_lib._column_array(pairs, engine_lib.STATS_MAX_PAIRS, True, "set_episode_stats")
    arrays = engine_lib.episode_stats_arrays(
        self._N, self._P, len(names), len(pnames),
        lambda shape, dtype: t.zeros(shape, dtype=getattr(t, dtype), device=eng.device))
    stats = engine_lib.EpisodeStats(names, pnames, arrays)
    for m, off, n in zip(self._members, self._offsets, self._counts):
      m._eng.use_current_stream()
      m._eng.set_episode_stats(names, pnames, out=stats.slice(off, off + n))
    return stats

  def hash_worlds(self, worlds=None, planes=None, fields=None):
    """int64 [N] device tensor: every member's `Substrate.hash_worlds` of its own worlds, in
    world order (`worlds`: a list of mixture worlds, default all).  A hash compares only with
    hashes of the SAME member: the members' fingerprints differ."""
    t = self._members[0]._eng._torch
    if worlds is None:
      out = t.empty((self._N,), dtype=t.int64, device=self._members[0]._eng.device)
      for m, off, n in zip(self._members, self._offsets, self._counts):
        m._eng.use_current_stream()
        m._eng.hash_worlds(None, out=out[off:off + n], planes=planes, fields=_hash_fields(fields))
      return out
    picked = [self._member_at(int(w)) for w in np.asarray(worlds).reshape(-1)]
    if not picked:
      raise ValueError("hash_worlds: no worlds to hash")
    # one launch per member that owns some of them, each writing its own positions of the result
    out = t.empty((len(picked),), dtype=t.int64, device=self._members[0]._eng.device)
    for m in self._members:
      at = [i for i, (owner, _) in enumerate(picked) if owner is m]
      if at:
        h = m.hash_worlds([picked[i][1] for i in at], planes=planes, fields=fields)
        out[t.as_tensor(at, device=out.device)] = h
    return out

  def step_many(self, actions, repeat: Optional[int] = None, events: bool = False,
                observations=(), states: bool = False, hashes: bool = False,
                active=None, lengths=None, until=None, stopped=None, returns=False,
                gamma: float = 1.0, worlds=None) -> StepManyResult:
    """As `Substrate.step_many`, over the members: one K-step launch per member, each reading
    its columns [:, off_i:off_i + n_i] of `actions` and writing its columns of the shared
    [K, N, ...] per-step tensors, those of `observations` included (nothing is copied or
    concatenated).  There is no `states=True` here: the members' records differ in size.
    `hashes=True` is there: a hash is 8 bytes for every member, so `.hashes` is one int64
    [K, N] tensor whose columns the members write — a per-step state identity of every world
    (comparable within one member only: the members' fingerprints differ).
    `active` / `lengths`: as `Substrate.step_many` takes them, over all N worlds; every member
    reads its columns of the one mask in place.
    `until` / `stopped` / `returns` / `gamma`: likewise; `stopped` [N], `.ran` [N] and `.returns`
    [N, P] are one tensor each, whose rows the members read and write in place."""
    if worlds is not None:
      raise ValueError("worlds= is not offered by a mixture: splitting a global list per member on the device "
                       "is not built; step the members' substrates on their own, or use active=")
    if states:
      raise ValueError("step_many: a mixture has no per-step states (states=True): its members' records "
                       "differ in size and fingerprint; step the members' substrates on their own")
    first = self._members[0]
    leaves = first._many_leaves(observations)
    t = first._eng._torch
    limit = self.action_spec()[0].num_values if self._check_device_actions else None
    a, K = _many_actions(t, actions, repeat, self._N, self._P, limit)
    dev = first._eng.device
    mask = _step_mask(t, active, lengths, K, self._N, dev, any(m._T > 0 for m in self._members))
    stop = _step_until(t, until, stopped, returns, gamma, self._N, self._P, dev,
                       any(m._T > 0 for m in self._members))
    keys = list(engine_lib.STEP_MANY_KINDS[:5 if events else 4])
    keys += [kind for kind in leaves.values() if kind not in _FIVE_NAMES]
    out = {}
    for key in keys:
      _, per_world, dtype = engine_lib.step_row(first._eng.shapes, key)
      out[key] = t.empty((K, self._N) + per_world, dtype=dtype, device=dev)
    if hashes:
      out["hashes"] = t.empty((K, self._N), dtype=t.int64, device=dev)
    self._observables.action.on_next(actions)
    for m, off, n in zip(self._members, self._offsets, self._counts):
      m._eng.use_current_stream()
      cols = a[off:off + n] if repeat is not None else a[:, off:off + n]
      if repeat is not None and isinstance(cols, t.Tensor):
        cols = cols.contiguous()
      more, rows = _until_slice(stop, {k: v[:, off:off + n] for k, v in out.items()}, off, n)
      m._submit_many(cols, repeat, events, rows, leaves,
                     active=None if mask is None else mask[..., off:off + n], **more)
    self._submissions += 1
    if stop is not None:
      out["ran"], out["stopped"] = stop["ran"], stop["stopped"]
      if stop["returns"] is not None and stop["returns"] is not False:
        out["returns"] = stop["returns"]
    return _many_result(out, leaves, self._emit(self._timestep()))

  def _member_at(self, world: int):
    if not 0 <= world < self._N:
      raise IndexError(f"world {world} outside [0, {self._N})")
    i = int(np.searchsorted(self._offsets, world, side="right")) - 1
    return self._members[i], world - self._offsets[i]

  def events(self, world: int = 0):
    """`Substrate.events` of mixture world `world`."""
    m, w = self._member_at(int(world))
    return m.events(w)

  def observables(self) -> SubstrateObservables:
    """As `Substrate.observables`; `events_batched` emits (mixture world, (name, payload))."""
    return self._observables

  def _emit(self, timestep: TimeStep) -> TimeStep:
    self._observables.timestep.on_next(timestep)
    batched = self._observables.events_batched
    if batched._observers:
      for m, off in zip(self._members, self._offsets):
        for w, events in enumerate(m.engine.events_all()):
          for event in events:
            batched.on_next((off + w, event))
    if self._observables.events._observers:
      for event in self.events(0):
        self._observables.events.on_next(event)
    return timestep

  def observation_spec(self) -> List[Mapping[str, Array]]:
    return self._members[0].observation_spec()

  def action_spec(self) -> List[DiscreteArray]:
    return self._members[0].action_spec()

  def reward_spec(self) -> List[Array]:
    return self._members[0].reward_spec()

  def discount_spec(self) -> BoundedArray:
    return self._members[0].discount_spec()

  def close(self):
    if not self._closed:
      self._closed = True
      for m in self._members:
        m.close()
      self._shared.leaves.clear()
      for subject in (self._observables.action, self._observables.timestep,
                      self._observables.events, self._observables.events_batched):
        subject.on_completed()

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def _timestep(self) -> TimeStep:
    if self._T:
      s = self.slot if self._submissions else 0
      ts = RolloutTimeStep(self._step_type[s], self._reward[s], self._discount[s],
                           {n: v[s] for n, v in self._obs.items()})
      ts.slot = s
      return ts
    return TimeStep(self._step_type, self._reward, self._discount, dict(self._obs))


_MIXTURE_KWARGS = frozenset({"env_seed", "auto_reset", "debug_observations", "action_table",
                             "rollout_length", "rgb_pool", "world_rgb_pool",
                             "check_device_actions", "device"})


def build_mixture(names: Sequence[str], *, roles: Optional[Sequence[str]] = None,
                  num_worlds, world_offset: int = 0,
                  individual_observations: Optional[Sequence[str]] = None,
                  global_observations: Optional[Sequence[str]] = None,
                  **substrate_kwargs) -> MixtureSubstrate:
  """Several registered substrates of one level as one batched substrate (`MixtureSubstrate`).

  `names`: the members, in world order.  `roles`: one role per player, valid for every member
  (default: each member's default roles — they must be as many).  `num_worlds`: one count per
  member, or a total split as evenly as possible; counts are rounded UP to the world granule
  (`world_granule`: the member offsets must keep the pooled views 16-byte aligned — 1 for full
  views, up to 16 with `rgb_pool` / `world_rgb_pool`; `split_worlds`).  `world_offset`: mixture
  world g is seeded as global world world_offset + g.  `individual_observations` /
  `global_observations` narrow the stock observation names as in `build_substrate`.  Further
  keyword arguments are a batched `Substrate`'s: env_seed, auto_reset, debug_observations,
  action_table, rollout_length, rgb_pool, world_rgb_pool, check_device_actions, device.

  The members must agree, as their configs and specs say, on the number of players, the
  number of discrete actions and the shape and dtype of every leaf: ValueError otherwise,
  naming the leaf and the members."""
  unknown = set(substrate_kwargs) - _MIXTURE_KWARGS
  if unknown:
    raise TypeError(f"build_mixture got unexpected keyword arguments {sorted(unknown)} "
                    f"(it takes {sorted(_MIXTURE_KWARGS)})")
  names = [str(n) for n in names]
  if not names:
    raise ValueError("a mixture needs at least one substrate name")
  for n in names:
    if n not in SUBSTRATES:
      raise ValueError(f"{n} not in {sorted(SUBSTRATES)} (substrates with a HIP engine in this build).")
  kw = dict(substrate_kwargs)
  rgb_pool = _check_pool_factor("rgb_pool", kw.get("rgb_pool", 1))
  world_rgb_pool = _check_pool_factor("world_rgb_pool", kw.get("world_rgb_pool", 1))
  packs = {n: engine_lib.load_pack(n) for n in set(names)}

  # the members' configs, narrowed like build_substrate's
  configs = []
  for n in names:
    c = get_config(n)
    if individual_observations is not None or global_observations is not None:
      ind, glob, spec = select_observations(
          c, packs[n],
          c.individual_observation_names if individual_observations is None else individual_observations,
          c.global_observation_names if global_observations is None else global_observations)
      c = SubstrateConfig(name=c.name, action_set=c.action_set, individual_observation_names=ind,
                          global_observation_names=glob, timestep_spec=spec,
                          valid_roles=c.valid_roles, default_player_roles=c.default_player_roles,
                          aux0_name=c.aux0_name, per_role_constants=c.per_role_constants)
    configs.append(c)

  # compatibility, from the configs and specs
  member_roles = [tuple(roles) if roles is not None else c.default_player_roles for c in configs]
  players = {n: len(r) for n, r in zip(names, member_roles)}
  if len(set(players.values())) > 1:
    raise ValueError(f"the members of a mixture must have the same number of players: {players}")
  for n, c, r in zip(names, configs, member_roles):
    invalid = set(r) - c.valid_roles
    if invalid:
      raise ValueError(f"Invalid roles for {n}: {invalid!r}. Must be one of {c.valid_roles!r}")
  if "action_table" not in kw:
    actions = {n: c.action_spec.num_values for n, c in zip(names, configs)}
    if len(set(actions.values())) > 1:
      raise ValueError(f"the members of a mixture must have the same action_spec(): {actions} "
                       "discrete actions (a common action_table=... gives them one)")
  specs = {n: observation_spec_of(c, packs[n], rgb_pool, world_rgb_pool)
           for n, c in zip(names, configs)}
  differ = {}
  for leaf in sorted(set().union(*specs.values())):
    seen = {n: (tuple(s[leaf].shape), str(s[leaf].dtype)) if leaf in s else None
            for n, s in specs.items()}
    if len(set(seen.values())) > 1:
      differ[leaf] = seen
  if differ:
    individual = sorted(l for l in differ if any(l in c.individual_observation_names for c in configs))
    drop = ([f"individual_observations=[...] without {individual}"] if individual else []) + (
        ["global_observations=()"] if set(differ) - set(individual) - {"COLLECTIVE_REWARD"} else [])
    raise ValueError(
        "the members of a mixture must have the same leaves; " + "; ".join(
            f"leaf {leaf!r} differs: " + ", ".join(
                f"{n} {'has none' if v is None else f'{v[0]} {v[1]}'}" for n, v in seen.items())
            for leaf, seen in differ.items()) +
        f". Drop it with {' and '.join(drop)} (as in build_substrate)")

  P = len(member_roles[0])
  granule = max(world_granule(leaf_bytes_per_world(c, packs[n], P, rgb_pool, world_rgb_pool))
                for n, c in zip(names, configs))
  # (every member has the same leaves and bytes per world: one granule fits all)
  counts = split_worlds(num_worlds, len(names), granule)
  total = sum(counts)
  if total < 2:
    raise ValueError("a mixture is batched (device tensors): it needs at least two worlds; "
                     "build a one-world Substrate with substrate.build(...)")
  offsets = [int(v) for v in np.cumsum([0] + counts[:-1])]
  T = int(kw.get("rollout_length", 0) or 0)
  if T < 0:
    raise ValueError("rollout_length must not be negative")
  kw["env_seed"] = resolve_env_seed(kw.get("env_seed"))   # (one seed for every member)
  check = bool(kw.pop("check_device_actions", False))
  shared = _SharedLeaves(total, T)
  members = []
  try:
    for n, c, r, off, cnt in zip(names, configs, member_roles, offsets, counts):
      m = Substrate(c, r, packs[n], num_worlds=cnt, batched=True,
                    world_offset=int(world_offset) + off,
                    _leaves=(lambda leaf, shape, dtype, device, off=off:
                             shared.take(leaf, shape, dtype, off, device)),
                    **kw)
      members.append(m)
      # the launch plan that suits the slices this engine writes (after all of them are bound)
      if hasattr(m.engine, "tune") and any(k in _PIXEL_LEAVES for k in m._obs):
        m.engine.tune()
  except BaseException:
    for m in members:
      m.close()
    raise
  return MixtureSubstrate(members, names, offsets, counts, shared, check)
