"""Registered episode starts (MpEpisodeStarts, Engine.set_episode_starts): a world that auto-resets
starts from a row of a bank of saved states, chosen by a device tensor — in step() and in every
step of step_many().  On the recipe's packs (one per level kernel, episodes of 16 frames, five
worlds): against the CPU oracle's model, against the loop it replaces (step, then load_worlds),
step_many against the loop of steps, the refusals, clearing, and a mixture.

Every run is 40 steps of seeded actions with the bank of the recipe's 25 rows (five worlds after
steps 1, 8, 16, 17 and 24): worlds 0 and 1 take ONE mid-episode row (saved after step 8, so they
end again 8 steps later and start from the bank at steps 17, 26 and 35 — the later ones in the
middle of a step_many), world 2 keeps the level's own reset (-1), world 3 takes a row with a dead
avatar where the level has one, world 4 a row saved from a finished episode.  `_coverage` asserts
that a run contained each of those."""
import numpy as np
import pytest
import torch

import states_recipe as R
import util
from engine_model import ModelEngine
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

E = engine
N, K = R.N, 40
PIXEL_PACKS = ("clean_up", R.MATRIX)
SCALARS = (E.OBS_REWARD, E.OBS_COLLECTIVE_REWARD, E.OBS_STEP_TYPE, E.OBS_DISCOUNT, E.OBS_READY_TO_SHOOT,
           E.OBS_AUX0, E.OBS_POSITION, E.OBS_ORIENTATION)
MATRIX_KINDS = (E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES, E.OBS_INTERACTION_REWARDS)


def _actions(eng):
  w = np.ones(eng.num_actions)
  w[min(7, eng.num_actions - 1)] = 4
  return util.random_actions(np.random.default_rng(7), K, N, eng.P, eng.num_actions, w)


def _tail(eng, bank, name):
  """Field `name` of the rows of `bank` (a host array [M, count])."""
  lay = eng.state_layout()
  off, elem, count = lay.fields[name]
  raw = bank[:, lay.grid_pad + off:lay.grid_pad + off + elem * count].cpu().numpy()
  return raw.view({1: np.uint8, 4: np.int32, 8: np.uint64}[elem])


def _plan(eng, name):
  """(bank, rows): the recipe's 25 rows and the row of each of the five worlds."""
  road = R.road(name)
  bank = road["all"].clone()
  alive = _tail(eng, bank, "aalive")[:, :eng.P]
  done = _tail(eng, bank, "done")[:, 0]
  dead = [i for i in range(len(bank)) if (alive[i] == 0).any() and not done[i]]
  if name in R.DEAD_AVATARS:
    assert dead, name
  mid = N * R.SAVE_AT.index(8)            # world 0 after step 8
  finished = N * R.SAVE_AT.index(16) + 4  # world 4 after step 16: LAST
  assert not done[mid] and done[finished]
  rows = np.array([mid, mid, -1, dead[0] if dead else mid + 3, finished], np.int32)
  return bank, rows, {"mid": mid, "dead": dead, "finished": finished}


def _coverage(name, types, rows, info):
  """`types`: int [K, N], the step types of the run's K steps (all worlds FIRST before it)."""
  types = np.asarray(types)
  last_before = np.vstack([np.zeros((1, N), bool), types[:-1] == 2])   # world w auto-resets in step k
  started = last_before & (rows[None, :] >= 0)
  assert (started.sum(0)[rows >= 0] >= 2).all(), (name, started.sum(0))   # every world twice
  assert started[:, 0].any() and rows[0] == info["mid"]                   # a mid-episode row
  if name in R.DEAD_AVATARS:
    assert started[:, 3].any() and rows[3] in info["dead"]                # a dead avatar
  both = started[:, 0] & started[:, 1]
  assert both.any() and rows[0] == rows[1]                                # two worlds, one row, one launch
  assert (both & last_before[:, 2]).any() and rows[2] == -1               # and a level reset beside them
  assert started[1:, :].any()                                             # not only in the first step


def _engine(name, kinds=(), **kw):
  e = engine.Engine(R.pack(name), N, device=0, **kw)
  for k in kinds:
    e.bind(k).zero_()   # (kinds that persist until an event rewrites them start equal)
  e.reset()
  return e


def _registered(name, kinds=(), fresh=False, **kw):
  e = _engine(name, kinds, **kw)
  bank, rows, info = _plan(e, name)
  drows = torch.from_numpy(rows).to(e.device)
  e.set_episode_starts(bank, drows, fresh=fresh)
  return e, bank, rows, drows, info


def _same_events(a, b, what):
  """EVENTS blocks [N, EVENT_ROWS, 4]: the header rows, and the rows they count as a set (the lanes
  of a wave queue a frame's events in no fixed order)."""
  a, b = np.asarray(a), np.asarray(b)
  assert np.array_equal(a[:, 0], b[:, 0]), (what, a[:, 0], b[:, 0])
  for w in range(a.shape[0]):
    n = int(a[w, 0, 0])
    assert sorted(map(tuple, a[w, 1:1 + n].tolist())) == sorted(map(tuple, b[w, 1:1 + n].tolist())), (what, w)


# ---- 1. against the oracle ------------------------------------------------------------------------
# (the model of registered episode starts is ModelEngine's own: tests/engine_model.py)
_MODEL_BANKS = {}


def _model_bank(name):
  """The model's own rows of the recipe's bank: the recipe's run, replayed on the oracles."""
  if name not in _MODEL_BANKS:
    m = ModelEngine(R.pack(name), N, auto_reset=True)
    A = R.actions(m.P, m.num_actions)
    m.reset()
    rows = []
    for s in range(1, R.STEPS + 1):
      m.step(A[s - 1])
      if s in R.SAVE_AT:
        rows += m.save_worlds()
    m.close()
    _MODEL_BANKS[name] = rows
  return _MODEL_BANKS[name]


def _same_as_model(e, m, what, views=()):
  for kind in m.scalar_kinds:
    got, ref = e.observe(kind).cpu().numpy(), m.observe_host(kind)
    if kind == E.OBS_EVENTS:
      _same_events(got, ref, (what, "events"))
    else:
      assert np.array_equal(got, ref), (what, kind)
  for g, r in zip(e.dump(), m.dump()):
    assert np.array_equal(g, r), what
  assert e.counters()["bad_actions"] == m.counters()["bad_actions"], what
  for kind in views:
    assert np.array_equal(e._bound[kind].cpu().numpy(), m._bound[kind]), (what, kind)


@pytest.mark.parametrize("name", R.PACKS)
def test_step_and_step_many_against_the_oracle(name):
  views = (E.OBS_RGB, E.OBS_WORLD_RGB, E.OBS_LAYER) if name in PIXEL_PACKS else ()
  mbank = _model_bank(name)
  for many in (False, True):
    e, bank, rows, drows, info = _registered(name, views)
    m = ModelEngine(R.pack(name), N, auto_reset=True)
    for kind in views:
      m.bind(kind)
    m.reset()
    m.set_episode_starts(mbank, rows)
    A = _actions(e)
    dA = torch.from_numpy(A).to(e.device)
    if many:
      got = e.step_many(dA, events=True)
      ref = m.step_many(A, events=True)
      for key in ("reward", "collective_reward", "step_type", "discount"):
        assert np.array_equal(got[key].cpu().numpy(), ref[key]), (name, key)
      for k in range(K):
        _same_events(got["events"][k].cpu().numpy(), ref["events"][k], (name, "row", k))
      types = ref["step_type"]
      _same_as_model(e, m, (name, "step_many"), views)
    else:
      types = []
      for k in range(K):
        e.step(dA[k])
        m.step(A[k])
        _same_as_model(e, m, (name, "step", k), views)
        types.append(m.observe_host(E.OBS_STEP_TYPE))
    _coverage(name, types, rows, info)
    e.sync()
    util.no_faults(e, words=40)
    e.close(); m.close()


@pytest.mark.parametrize("name", PIXEL_PACKS)
def test_a_rollout_ring_against_the_oracle(name):
  T = 4
  e, bank, rows, drows, info = _registered(name)
  m = ModelEngine(R.pack(name), N, auto_reset=True)
  m.reset()
  m.set_episode_starts(_model_bank(name), rows)
  kinds = (E.OBS_WORLD_RGB, E.OBS_REWARD, E.OBS_STEP_TYPE)
  rings = {k: e.bind_ring(k, slots=T, tune=False) for k in kinds}
  mrings = {k: m.bind_ring(k, slots=T) for k in kinds}
  A = _actions(e)
  dA = torch.from_numpy(A).to(e.device)
  for k in range(K):
    e.step(dA[k])
    m.step(A[k])
    assert e.ring["next"] == m.ring["next"], k
    slot = m.ring["last"]
    for kind in kinds:
      assert np.array_equal(rings[kind][slot].cpu().numpy(), mrings[kind][slot]), (name, k, kind)
  e.sync()
  util.no_faults(e, words=40)
  e.close(); m.close()


# ---- 2. the defining identity ---------------------------------------------------------------------
def _leaves(e):
  kinds = list(R.record_kinds(e)) + [k for k in SCALARS + (E.OBS_EVENTS,)]
  if e.info.num_resources > 0 and E.OBS_INTERACTION_REWARDS in e.shapes:
    probe = e._L.mp_obs_bytes(e._h, E.OBS_INTERACTION_REWARDS)
    if probe > 0:
      kinds += [E.OBS_INTERACTION_INVENTORIES, E.OBS_INTERACTION_REWARDS]
  return tuple(dict.fromkeys(kinds))


def _same_engines(a, b, what):
  assert torch.equal(a.save_worlds(), b.save_worlds()), what
  assert torch.equal(a.hash_worlds(), b.hash_worlds()), what
  for kind, buf in a._bound.items():
    if kind == E.OBS_EVENTS:
      _same_events(buf.cpu().numpy(), b._bound[kind].cpu().numpy(), what)
    else:
      assert torch.equal(buf, b._bound[kind]), (what, kind)
  assert a.counters() == b.counters(), what


@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("name", R.PACKS)
def test_a_step_is_step_then_load_worlds(name, fresh):
  probe = _engine(name)
  kinds = _leaves(probe)
  probe.close()
  a, bank, rows, drows, info = _registered(name, kinds, fresh=fresh)
  b = _engine(name, kinds)
  assert not a.fused and b.fused
  lay = b.state_layout()
  A = torch.from_numpy(_actions(a)).to(a.device)
  types = []
  for k in range(K):
    last = b._bound[E.OBS_STEP_TYPE].cpu().numpy() == 2
    a.step(A[k])
    b.step(A[k])
    src = np.where(last, rows, -1).astype(np.int32)
    if not fresh:
      b.load_worlds(bank, src)
    elif (src >= 0).any():
      # gather the rows, edit seed / episode / orders_step by name, load
      own = substrate.StateFields(b.save_worlds(), lay)
      take = torch.from_numpy(np.where(src >= 0, src, 0)).to(b.device).long()
      gathered = bank[take].clone()
      f = substrate.StateFields(gathered, lay)
      f.seed[:] = own.seed
      f.episode[:] = own.episode     # (the twin's own reset has just set episode + 1)
      f.orders_step[:] = 0
      b.load_worlds(gathered, np.where(src >= 0, np.arange(N), -1).astype(np.int32))
    _same_engines(a, b, (name, fresh, k))
    types.append(a._bound[E.OBS_STEP_TYPE].cpu().numpy().copy())
  # (a world that starts from a finished row reports LAST at the start: the run's own step types say
  # which worlds auto-reset in which step)
  _coverage(name, types, rows, info)
  if fresh:   # worlds 0 and 1 took one row and are different worlds from then on
    h = a.hash_worlds().cpu().numpy()
    assert h[0] != h[1], name
  for e in (a, b):
    e.sync()
    util.no_faults(e, words=40)
    e.close()


# ---- 3. step_many is the loop ---------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_step_many_is_the_loop_of_steps(name):
  probe = engine.Engine(R.pack(name), 1, device=0, debug_observations=True)
  obs = tuple(k for k in E.STEP_ROW_KINDS
              if k not in (E.OBS_REWARD, E.OBS_COLLECTIVE_REWARD, E.OBS_STEP_TYPE, E.OBS_DISCOUNT, E.OBS_EVENTS)
              and probe._L.mp_obs_bytes(probe._h, k) > 0)
  probe.close()
  a, bank, rows, drows, info = _registered(name, debug_observations=True)
  b, _, _, _, _ = _registered(name, debug_observations=True)
  A = torch.from_numpy(_actions(a)).to(a.device)
  got = a.step_many(A, events=True, observations=obs, states=True, hashes=True)
  for k in range(K):
    b.step(A[k])
    what = (name, "row", k)
    for key, kind in (("reward", E.OBS_REWARD), ("collective_reward", E.OBS_COLLECTIVE_REWARD),
                      ("step_type", E.OBS_STEP_TYPE), ("discount", E.OBS_DISCOUNT)):
      assert torch.equal(got[key][k], b.observe(kind)), (what, key)
    _same_events(got["events"][k].cpu().numpy(), b.observe(E.OBS_EVENTS).cpu().numpy(), what)
    for kind in obs:
      assert torch.equal(got[kind][k], b.observe(kind)), (what, kind)
    assert torch.equal(got["states"][k], b.save_worlds()), what
    assert torch.equal(got["hashes"][k], b.hash_worlds()), what
    assert torch.equal(got["hashes"][k], a.hash_states(got["states"][k])), what
  # row k loads: a third engine continues from it as the loop's engine does
  c = _engine(name)
  c.load_worlds(got["states"][K - 1], np.arange(N, dtype=np.int32))
  assert torch.equal(c.hash_worlds(), got["hashes"][K - 1]), name
  assert torch.equal(a.save_worlds(), b.save_worlds()) and a.counters() == b.counters(), name
  _coverage(name, got["step_type"].cpu().numpy(), rows, info)
  for e in (a, b, c):
    e.sync()
    util.no_faults(e, words=40)
    e.close()


def test_step_many_rows_one_family_at_a_time():
  """The starts family serves every combination of rows: none, the five only, LAYER only, states
  only, hashes only — each equal to the columns of the request that names them all."""
  name = "clean_up"
  full, bank, rows, drows, info = _registered(name)
  A = torch.from_numpy(_actions(full)).to(full.device)
  ref = full.step_many(A, observations=(E.OBS_LAYER,), states=True, hashes=True)
  for kw in ({}, {"keep": ()}, {"observations": (E.OBS_LAYER,)}, {"states": True}, {"hashes": True}):
    e, _, _, _, _ = _registered(name)
    got = e.step_many(A, **kw)
    for key, value in got.items():
      assert torch.equal(value, ref[key]), (kw, key)
    assert torch.equal(e.save_worlds(), full.save_worlds()), kw
    e.sync()
    util.no_faults(e, words=40)
    e.close()
  full.close()


# ---- 4. errors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["past", -2])
def test_a_bad_index_takes_the_level_reset_and_is_reported(bad):
  name = "coins"
  a, bank, rows, drows, info = _registered(name)
  b = _engine(name)
  index = len(bank) if bad == "past" else bad
  drows[1] = index
  A = torch.from_numpy(_actions(a)).to(a.device)
  for k in range(17):   # step 17 is the first start
    a.step(A[k]); b.step(A[k])
  with pytest.raises(ValueError, match=rf"MpEpisodeStarts: rows\[1\] = {index} "):
    a.sync()
  # world 1 (and world 2, which asks for it) took the level's own reset
  assert torch.equal(a.save_worlds([1, 2]), b.save_worlds([1, 2]))
  a.sync()   # reported once; the engine stays usable
  drows[1] = rows[1]
  for k in range(17, K):
    a.step(A[k])
  a.sync()
  assert int(a.observe(E.OBS_STEP_TYPE).cpu()[1]) in (0, 1, 2)
  a.close(); b.close()


def test_a_malformed_row_takes_the_level_reset_and_is_reported():
  name = "clean_up"
  a = _engine(name)
  b = _engine(name)
  bank, rows, info = _plan(a, name)
  states = substrate.WorldStates(bank, a.state_fingerprint)
  lay = a.state_layout()
  fields = substrate.StateFields(states.data, lay)
  fields.orientation[info["mid"], 0] = 7   # rule 3: aori outside 0..3
  verdicts = a.check_states(states.data)
  assert tuple(verdicts[info["mid"]].cpu().tolist())[0] == E.RULE_TAIL_RANGE
  drows = torch.from_numpy(rows).to(a.device)
  a.set_episode_starts(states.data, drows, verdicts=verdicts)
  A = torch.from_numpy(_actions(a)).to(a.device)
  a.step_many(A[:17]); b.step_many(A[:17])
  with pytest.raises(ValueError, match=rf"row {info['mid']}, which rows\[[01]\] names.*rule {E.RULE_TAIL_RANGE}"):
    a.sync()
  assert torch.equal(a.save_worlds([0, 1, 2]), b.save_worlds([0, 1, 2]))   # the level's own reset
  assert not torch.equal(a.save_worlds([3]), b.save_worlds([3]))           # world 3's row was fine
  a.step_many(A[17:30])
  with pytest.raises(ValueError, match="MpEpisodeStarts"):   # worlds 0 and 1 end again at step 33 - 17
    a.step_many(A[30:])
    a.sync()
  a.close(); b.close()


def test_refusals():
  name = "coins"
  e = _engine(name)
  bank, rows, info = _plan(e, name)
  drows = torch.from_numpy(rows).to(e.device)
  S = bank.shape[1]
  before = e.save_worlds().clone()
  with pytest.raises(ValueError, match="fingerprint"):
    e.set_episode_starts(bank, drows, fingerprint=e.state_fingerprint ^ 1)
  with pytest.raises(ValueError, match="bank"):
    e.set_episode_starts(bank[:, :S - 16], drows)
  with pytest.raises(ValueError, match="no rows"):
    e.set_episode_starts(bank[:0], drows)
  with pytest.raises(ValueError, match="rows"):
    e.set_episode_starts(bank, drows[:N - 1])
  with pytest.raises(ValueError, match="rows"):
    e.set_episode_starts(bank, drows.long())
  with pytest.raises(ValueError, match="verdicts"):
    e.set_episode_starts(bank, drows, verdicts=torch.zeros((len(bank),), dtype=torch.int32, device=e.device))
  with pytest.raises(ValueError, match="lives on"):
    e.set_episode_starts(bank.cpu(), drows)
  # the library's own checks, behind the Python ones
  import ctypes
  def raw(**kw):
    req = E.MpEpisodeStarts(ctypes.sizeof(E.MpEpisodeStarts), 0, e.state_fingerprint)
    req.bank, req.rows, req.bank_rows = bank.data_ptr(), drows.data_ptr(), len(bank)
    size = kw.pop("size", ctypes.sizeof(req))
    for k, v in kw.items():
      setattr(req, k, v)
    return e._L.mp_restore(e._h, ctypes.addressof(req), size)
  assert raw(struct_size=8) == E.MP_ERR_INVALID
  assert raw(bank_rows=0) == E.MP_ERR_INVALID
  assert raw(bank_rows=-3) == E.MP_ERR_INVALID
  assert raw(fresh=2) == E.MP_ERR_INVALID
  assert raw(rows=None) == E.MP_ERR_INVALID
  assert raw(bank_rows=len(bank) + 1000000) == E.MP_ERR_INVALID          # runs past its allocation
  assert raw(bank=bank.data_ptr() + 4) == E.MP_ERR_INVALID               # not 16-byte aligned
  host = np.zeros(N, np.int32)
  assert raw(rows=host.ctypes.data) == E.MP_ERR_INVALID                  # host memory
  assert e.episode_starts is None and e.fused
  assert torch.equal(e.save_worlds(), before)
  e.close()
  frozen = engine.Engine(R.pack(name), N, device=0, auto_reset=False)
  frozen.reset()
  with pytest.raises(ValueError, match="auto_reset"):
    frozen.set_episode_starts(bank, drows)
  frozen.close()
  one = engine.Engine(R.pack(name), N, device=0, unfused=False)
  one.reset()
  with pytest.raises(engine.EngineError, match="unfused"):
    one.set_episode_starts(bank, drows)
  one.close()


# ---- 5. clearing ----------------------------------------------------------------------------------
def test_clearing_returns_the_engine_to_what_it_was():
  name = "clean_up"
  a, bank, rows, drows, info = _registered(name, (E.OBS_WORLD_RGB,))
  b = _engine(name, (E.OBS_WORLD_RGB,))
  kept = bank.clone()
  assert not a.fused and b.fused and a.episode_starts["rows"] is drows
  A = torch.from_numpy(_actions(a)).to(a.device)
  for k in range(K):
    a.step(A[k])
  assert torch.equal(bank, kept)   # the bank is never written
  a.clear_episode_starts()
  assert a.fused and a.episode_starts is None
  # the twin joins a where it is now, and both go on without a registration
  b.load_worlds(a.save_worlds(), np.arange(N, dtype=np.int32))
  for k in range(K):
    a.step(A[k]); b.step(A[k])
    assert torch.equal(a.hash_worlds(), b.hash_worlds()), k
  assert torch.equal(a._bound[E.OBS_WORLD_RGB], b._bound[E.OBS_WORLD_RGB])
  for e in (a, b):
    e.sync()
    util.no_faults(e, words=40)
    e.close()


# ---- 6. no side effects ---------------------------------------------------------------------------
def test_reset_masked_reset_and_load_are_what_they_were():
  name = R.MATRIX
  a, bank, rows, drows, info = _registered(name, (E.OBS_WORLD_RGB, E.OBS_STEP_TYPE))
  b = _engine(name, (E.OBS_WORLD_RGB, E.OBS_STEP_TYPE))
  A = torch.from_numpy(_actions(a)).to(a.device)
  for k in range(16):   # every world is LAST now, none has started from the bank yet
    a.step(A[k]); b.step(A[k])
  assert bool((a._bound[E.OBS_STEP_TYPE] == 2).all())
  mask = np.array([1, 0, 1, 0, 0], np.uint8)
  a.reset(mask=mask); b.reset(mask=mask)
  _same_engines(a, b, "masked reset")
  src = np.array([-1, 3, -1, -1, 7], np.int32)
  a.load_worlds(bank, src); b.load_worlds(bank, src)
  _same_engines(a, b, "load")
  a.reset(); b.reset()
  _same_engines(a, b, "reset")
  snap = a.snapshot()
  a.restore(snap)
  assert a.episode_starts is not None and not a.fused   # configuration, not part of a record
  for e in (a, b):
    e.sync()
    util.no_faults(e, words=40)
    e.close()


def test_tune_leaves_the_records_and_the_registration():
  name = "clean_up"
  a, bank, rows, drows, info = _registered(name, (E.OBS_WORLD_RGB,))
  A = torch.from_numpy(_actions(a)).to(a.device)
  for k in range(16):
    a.step(A[k])      # every world is LAST: a probe that stepped with the registration would start them
  before = a.save_worlds().clone()
  a.tune()
  assert torch.equal(a.save_worlds(), before) and a.episode_starts is not None and not a.fused
  a.sync()
  util.no_faults(a, words=40)
  a.close()


# ---- the Substrate surface and a mixture ----------------------------------------------------------
def test_substrate_set_episode_starts():
  name = "collaborative_cooking__cramped"   # (its episodes end at max_frames and nowhere else)
  roles = substrate.get_config(name).default_player_roles
  env = substrate.build(name, roles=roles, num_worlds=4, env_seed=5)
  twin = substrate.build(name, roles=roles, num_worlds=4, env_seed=5)
  env.reset(); twin.reset()
  A = np.zeros((8, 4, len(roles)), np.int32)
  env.step_many(A); twin.step_many(A)
  bank = env.save_state()
  rows = env.set_episode_starts(bank)
  assert rows.dtype == torch.int32 and tuple(rows.shape) == (4,) and bool((rows == -1).all())
  assert env.engine.episode_starts["verdicts"] is None   # nothing was edited: no check
  rows[:] = torch.tensor([2, 2, -1, 0], dtype=torch.int32)
  T = int(env.engine.info.max_frames)
  assert T + 8 <= E.STEP_MANY_MAX
  noop = np.zeros((4, len(roles)), np.int32)
  env.step_many(noop, repeat=T - 8 + 1); twin.step_many(noop, repeat=T - 8 + 1)   # LAST, then the start
  assert bool((env.engine.observe(E.OBS_STEP_TYPE) == 0).all())   # every world has just started
  twin.load_state(bank, [2, 2, -1, 0])
  h, ht = env.hash_worlds().cpu().numpy(), twin.hash_worlds().cpu().numpy()
  assert (h[[0, 1, 3]] == ht[[0, 1, 3]]).all() and h[0] == h[1] and h[2] != h[0]
  # an edited bank is checked: one launch now, its verdicts handed to the engine
  fields = env.state_fields(bank)
  fields.orientation[2, 0] = 9
  rows2 = env.set_episode_starts(bank, rows)
  assert rows2 is rows and env.engine.episode_starts["verdicts"] is not None
  assert env.set_episode_starts(None) is None and env.engine.episode_starts is None
  with pytest.raises(ValueError, match="fingerprint"):
    other = substrate.WorldStates(bank.data, bank.fingerprint ^ 1)
    env.set_episode_starts(other)
  env.close(); twin.close()


def test_a_mixture_registers_per_member():
  names = ("collaborative_cooking__cramped", "collaborative_cooking__asymmetric")
  kw = dict(num_worlds=16, env_seed=3, individual_observations=("POSITION",), global_observations=())
  mix = substrate.build_mixture(names, **kw)
  plain = substrate.build_mixture(names, **kw)
  mix.reset(); plain.reset()
  n, P = mix.num_worlds, mix.num_players
  rng = np.random.default_rng(11)
  A = rng.integers(0, mix.action_spec()[0].num_values, size=(8, n, P)).astype(np.int32)
  mix.step_many(A); plain.step_many(A)
  bank0 = mix._members[0].save_state()
  rows = mix.set_episode_starts([bank0, None])
  s0, s1 = mix.member_slice(0), mix.member_slice(1)
  assert tuple(rows.shape) == (n,) and bool((rows == -1).all())
  assert mix.engines[0].episode_starts["rows"].data_ptr() == rows[s0].data_ptr()   # a view, no copy
  assert mix.engines[1].episode_starts is None
  rows[s0] = 0
  T = int(mix.engines[0].info.max_frames)
  assert T + 8 <= E.STEP_MANY_MAX
  noop = np.zeros((n, P), np.int32)
  mix.step_many(noop, repeat=T - 8 + 3); plain.step_many(noop, repeat=T - 8 + 3)
  h, hp = mix.hash_worlds(), plain.hash_worlds()
  assert torch.equal(h[s1], hp[s1])
  assert not bool((h[s0] == hp[s0]).any())
  # member 0's worlds all continue world 0's saved state, two steps on
  assert bool((h[s0] == h[s0][0]).all())
  for e in mix.engines:
    e.sync()
  mix.close(); plain.close()
