"""Action sequences with per-step rows of the observations: `step_many(observations=...)` stacks
any non-pixel kind per step.  Row k of a kind is, byte for byte, what the kind's in-place (or
bound) buffer holds after step k of the loop of `step` on a twin engine, a value a step does not
write being carried from the row before: on every pack, through auto-resets and frozen worlds,
for the kinds that change only when something happens, for worlds never reset, in every form the
call takes.  The oracle agrees without the single-step path, and every refusal happens on the
host, before any launch.  Every comparison is byte equality; EVENTS rows are compared as
tests/test_gpu_step_many.py compares them (header, then the counted rows as a sorted set)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import geometry
import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(engine.__file__), "assets")
PACKS = sorted(f[:-4] for f in os.listdir(ASSETS) if f.endswith(".mpk"))
E = engine
FIVE = {"reward": E.OBS_REWARD, "collective_reward": E.OBS_COLLECTIVE_REWARD,
        "step_type": E.OBS_STEP_TYPE, "discount": E.OBS_DISCOUNT, "events": E.OBS_EVENTS}
FIN = (E.OBS_READY_TO_SHOOT, E.OBS_AUX0, E.OBS_POSITION, E.OBS_ORIENTATION)
LEVEL = (E.OBS_AUX1, E.OBS_AUX2, E.OBS_AUX3, E.OBS_AUX4, E.OBS_ZAP_MATRIX, E.OBS_INVENTORY,
         E.OBS_INTERACTION_INVENTORIES, E.OBS_MATRIX_CUMULANTS, E.OBS_INTERACTION_REWARDS)
MP_EVENT_INTERACTION = 11
MP_ERR_UNSUPPORTED = -5


def _engine(pack, n, kinds=(), **kw):
  e = engine.Engine(pack, n, device=0, **kw)
  bufs = {k: e.bind(k) for k in kinds}
  for v in bufs.values():   # (kinds that persist until an event rewrites them start equal)
    v.zero_()
  return e, bufs


def _events(rows):
  """One world's event rows as (dropped, sorted rows the header counts)."""
  rows = np.asarray(rows)
  n = int(rows[0, 0])
  return int(rows[0, 1]), sorted(map(tuple, rows[1:1 + n].tolist()))


def _same_events(a, b, what):
  a, b = a.cpu().numpy(), b.cpu().numpy()
  for w in range(a.shape[0]):
    assert _events(a[w]) == _events(b[w]), (what, "events", w)


def _same(a, b, kind, what):
  if kind == E.OBS_EVENTS:
    _same_events(a, b, what)
  else:
    assert a.dtype == b.dtype and a.shape == b.shape, (what, kind, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), (what, kind, (a != b).nonzero()[:4].tolist())


def _supported(pack):
  """The level kinds the pack's substrate produces with debug_observations."""
  probe = engine.Engine(pack, 1, device=0, debug_observations=True)
  extra = tuple(k for k in LEVEL if probe._L.mp_obs_bytes(probe._h, k) > 0)
  probe.close()
  return extra


def _key(kind):
  for name, k in FIVE.items():
    if k == kind:
      return name
  return kind


def _loop(e, kinds, A, fields=False):
  """K calls of step on e; every kind (a key of step_many's result) cloned after every step:
  the bound buffer where the kind is bound, what observe() copies out of the in-place one (for
  LAYER: draws from the records) otherwise."""
  rows = {kind: [] for kind in kinds}
  for k in range(A.shape[0]):
    (e.step_fields if fields else e.step)(A[k])
    for kind in kinds:
      rows[kind].append(e._bound[kind].clone() if kind in e._bound else e.observe(kind))
  return {_key(kind): torch.stack(v) for kind, v in rows.items()}


def _same_rows(got, ref, what):
  assert set(got) == set(ref), (what, sorted(map(str, got)), sorted(map(str, ref)))
  for key in got:
    if key == "events":
      for k in range(ref[key].shape[0]):
        _same_events(got[key][k], ref[key][k], (what, "row", k))
    else:
      _same(got[key], ref[key], key, (what, "rows"))


def _same_engines(a, b, kinds, what):
  """Final buffers (bound or in place) of `kinds`, records, counters, fault words."""
  for kind in kinds:
    if kind == E.OBS_LAYER and kind not in a._bound:
      continue   # (an unbound LAYER has no buffer; the records below decide it)
    _same(a._bound[kind] if kind in a._bound else a.observe(kind),
          b._bound[kind] if kind in b._bound else b.observe(kind), kind, (what, "final"))
  assert torch.equal(a.save_worlds(), b.save_worlds()), what
  assert a.counters() == b.counters(), what
  util.no_faults(a); util.no_faults(b)


def _many(e, A, kinds, **kw):
  """One step_many with the five (events included) and per-step rows of `kinds`."""
  return e.step_many(A, events=True, observations=[k for k in kinds if k not in FIVE.values()], **kw)


# ---- 1. every pack ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PACKS)
def test_every_pack_equals_the_sequential_loop(name):
  pack = engine.load_pack(name)
  kinds = tuple(FIVE.values()) + FIN + _supported(pack) + (E.OBS_LAYER,)
  n = 64
  for dev in (None, {"no_next_orders": 1}):
    for bound in (True, False):
      kw = {"debug_observations": True}
      if dev:
        kw["dev"] = dev
      a, _ = _engine(pack, n, kinds if bound else (), **kw)
      b, _ = _engine(pack, n, kinds, **kw)
      P, nact = a.P, a.num_actions
      rng = np.random.default_rng(11)
      warm = torch.from_numpy(util.random_actions(rng, 20, n, P, nact)).to(a.device)
      a.reset(); b.reset()
      for s in range(20):
        a.step(warm[s]); b.step(warm[s])
      for K in (1, 7, 33):
        A = torch.from_numpy(util.random_actions(rng, K, n, P, nact)).to(a.device)
        got = _many(a, A, kinds)
        ref = _loop(b, kinds, A)
        for kind in kinds:
          if kind not in FIVE.values():
            assert tuple(got[kind].shape) == (K,) + a.shapes[kind][0] and got[kind].dtype == a.shapes[kind][1]
        _same_rows(got, ref, (name, dev, bound, K))
        _same_engines(a, b, kinds, (name, dev, bound, K))
      a.close(); b.close()


# ---- 2. episodes that end inside a sequence ----------------------------------------------------
def _episodes(pack, n, K, auto, kinds, seed):
  a, _ = _engine(pack, n, kinds, auto_reset=auto)
  b, _ = _engine(pack, n, kinds, auto_reset=auto)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(seed), K, n, a.P, a.num_actions)).to(a.device)
  a.reset(); b.reset()
  got = _many(a, A, kinds)
  ref = _loop(b, kinds, A)
  return a, b, got, ref


@pytest.mark.parametrize("auto", [True, False])
def test_episodes_end_inside_the_sequence(auto):
  """MAXFRAMES = 9 and K = 33 right after a reset: every world is LAST at row 8.  Without
  auto_reset it is frozen from row 9 on, and a frozen step writes none of READY_TO_SHOOT, AUX0,
  POSITION, ORIENTATION: rows 9.. repeat row 8 (and the record, so LAYER, stays).  With
  auto_reset rows 9, 19 and 29 are a reset's."""
  pack = util.patch_pack(engine.load_pack("clean_up"), MAXFRAMES=9)
  n, K = 16, 33
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_LAYER,)
  a, b, got, ref = _episodes(pack, n, K, auto, kinds, 13)
  st = got["step_type"].cpu().numpy()
  if auto:
    for last in (8, 18, 28):
      assert (st[last] == 2).all() and (st[last + 1] == 0).all(), (last, st[last], st[last + 1])
    # (rows 9, 19 and 29 are a reset's: FIRST above, the values by the loop's below)
    moved = (got[E.OBS_POSITION][9] != got[E.OBS_POSITION][8]).flatten(1).any(1)
    assert moved.any(), "no world's avatars respawned elsewhere at the reset"
  else:
    assert (st[:8] == 1).all() and (st[8:] == 2).all()
    for kind in FIN + (E.OBS_LAYER,):
      assert (got[kind][9:] == got[kind][8]).all(), kind      # the carry
    assert (got[E.OBS_POSITION][8] != got[E.OBS_POSITION][0]).any()   # (and row 8 is not the start)
  _same_rows(got, ref, ("episodes", auto))
  _same_engines(a, b, kinds, ("episodes", auto))
  a.close(); b.close()


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("name", ["prisoners_dilemma_in_the_matrix__arena", "gift_refinements"])
def test_episodes_end_inside_the_sequence_with_inventories(name, auto):
  pack = util.patch_pack(engine.load_pack(name), MAXFRAMES=9)
  n, K = 16, 33
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_INVENTORY, E.OBS_LAYER)
  if "matrix" in name:
    kinds += (E.OBS_INTERACTION_INVENTORIES, E.OBS_INTERACTION_REWARDS)
  a, b, got, ref = _episodes(pack, n, K, auto, kinds, 14)
  st = got["step_type"].cpu().numpy()
  if auto:
    assert (st[8] == 2).all() and (st[9] == 0).all() and (st[19] == 0).all() and (st[29] == 0).all()
  else:
    assert (st[8:] == 2).all()
    for kind in kinds[5:]:
      assert (got[kind][9:] == got[kind][8]).all(), kind
  _same_rows(got, ref, (name, auto))
  _same_engines(a, b, kinds, (name, auto))
  a.close(); b.close()


# ---- 3. kinds that are written only when something happens --------------------------------------
def test_interaction_kinds_change_at_an_interaction_and_are_carried():
  name = "prisoners_dilemma_in_the_matrix__arena"
  pack = engine.load_pack(name)
  n, warm, K = 32, 40, 60
  kinds = tuple(FIVE.values()) + (E.OBS_INTERACTION_REWARDS, E.OBS_INTERACTION_INVENTORIES,
                                  E.OBS_INVENTORY, E.OBS_MATRIX_CUMULANTS)
  a, _ = _engine(pack, n, kinds, debug_observations=True)
  b, _ = _engine(pack, n, kinds, debug_observations=True)
  P = a.P
  A = torch.from_numpy(util.random_actions(np.random.default_rng(31), warm + K, n, P, 8,
                                           [1, 6, 1, 1, 1, 2, 2, 5])).to(a.device)
  a.reset(); b.reset()
  for s in range(warm):
    a.step(A[s]); b.step(A[s])
  got = _many(a, A[warm:], kinds)
  ref = _loop(b, kinds, A[warm:])
  _same_rows(got, ref, name)
  _same_engines(a, b, kinds, name)
  # the situation: an interaction inside the sequence, whose rewards appear at its step and stay
  ev = got["events"].cpu().numpy()
  ir = got[E.OBS_INTERACTION_REWARDS].cpu().numpy()
  hits = [(k, w) for k in range(K) for w in range(n)
          if any(t == MP_EVENT_INTERACTION for t, _, _, _ in _events(ev[k, w])[1])]
  assert hits, "no interaction inside the sequence: the test shows nothing"
  shown = 0
  for k, w in hits:
    later = [k2 for k2, w2 in hits if w2 == w and k2 > k]
    end = min(later) if later else K
    before = ir[k - 1, w] if k else None
    if before is not None and not np.array_equal(ir[k, w], before):
      assert all(np.array_equal(ir[j, w], ir[k, w]) for j in range(k, end)), (k, w)
      if end == K:
        shown += 1
  assert shown, "no world's INTERACTION_REWARDS row changed at an interaction and was carried to row K - 1"
  a.close(); b.close()


# ---- 4. never-reset worlds ----------------------------------------------------------------------
def test_worlds_never_reset_write_no_rows():
  pack = engine.load_pack("prisoners_dilemma_in_the_matrix__arena")
  n, K = 12, 5
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_LAYER, E.OBS_INVENTORY, E.OBS_INTERACTION_REWARDS)
  a, _ = _engine(pack, n, kinds)
  b, _ = _engine(pack, n, kinds)
  mask = np.zeros(n, np.uint8)
  mask[::2] = 1
  a.reset(mask=mask); b.reset(mask=mask)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(32), K, n, a.P, a.num_actions)).to(a.device)
  out = {}
  for kind in kinds:
    shape, dtype = a.shapes[kind]
    out[_key(kind)] = torch.full((K,) + shape, 123, dtype=dtype, device=a.device)
  got = _many(a, A, kinds, out=out)
  ref = _loop(b, kinds, A)
  live = torch.from_numpy(mask.astype(bool)).to(a.device)
  for key, rows in got.items():
    assert rows.data_ptr() == out[key].data_ptr()
    assert (rows[:, ~live] == 123).all(), key          # the sentinel
    if key == "events":
      for k in range(K):
        _same_events(rows[k, live], ref[key][k, live], ("never reset", "row", k))
    else:
      assert torch.equal(rows[:, live], ref[key][:, live]), key
  _same_engines(a, b, kinds, "never reset")
  a.close(); b.close()


# ---- 5. against the oracle, without the single-step path ---------------------------------------
@pytest.mark.parametrize("name", ["clean_up", "commons_harvest__open", "territory__rooms",
                                  "prisoners_dilemma_in_the_matrix__arena",
                                  "collaborative_cooking__cramped"])
def test_sixty_steps_of_rows_match_the_oracle(name):
  pack = engine.load_pack(name)
  n, K = 8, 60
  e, _ = _engine(pack, n)
  matrix = "matrix" in name
  kinds = (E.OBS_LAYER, E.OBS_READY_TO_SHOOT, E.OBS_POSITION, E.OBS_ORIENTATION)
  if matrix:
    kinds += (E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES)
  A = util.random_actions(np.random.default_rng(12), K, n, e.P, e.num_actions)
  e.reset()
  got = {k: v.cpu().numpy() for k, v in
         e.step_many(torch.from_numpy(A).to(e.device), keep=("reward",), observations=kinds).items()}
  for w, o in enumerate(util.make_oracles(pack, n)):
    o.reset()
    for k in range(K):
      o.step(A[k, w])
      at = (name, w, k)
      assert np.array_equal(got["reward"][k, w], o.rewards()), at
      assert np.array_equal(got[E.OBS_LAYER][k, w], np.stack([o.layer_view(p) for p in range(e.P)])), at
      assert np.array_equal(got[E.OBS_READY_TO_SHOOT][k, w], o.ready_to_shoot()), at
      avat = o.dump()[1]
      assert np.array_equal(got[E.OBS_POSITION][k, w], avat[:, :2]), at
      assert np.array_equal(got[E.OBS_ORIENTATION][k, w], avat[:, 2]), at
      if matrix:
        inv, inter = o.inventories()
        assert np.array_equal(got[E.OBS_INVENTORY][k, w], inv), at
        assert np.array_equal(got[E.OBS_INTERACTION_INVENTORIES][k, w], inter), at
    o.close()
  util.no_faults(e)
  e.close()


# ---- 6. forms -----------------------------------------------------------------------------------
def test_repeat_and_fields():
  pack = engine.load_pack("clean_up")
  n, K = 16, 12
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_LAYER,)
  a, _ = _engine(pack, n, kinds)
  b, _ = _engine(pack, n, kinds)
  rng = np.random.default_rng(16)
  P, nact = a.P, a.num_actions
  a.reset(); b.reset()
  block = torch.from_numpy(util.random_actions(rng, 1, n, P, nact)[0]).to(a.device)
  got = _many(a, block, kinds, repeat=K)
  ref = _loop(b, kinds, block.expand(K, n, P))
  _same_rows(got, ref, "repeat")
  _same_engines(a, b, kinds, "repeat")
  table = np.asarray(util.pack_tables(pack)["action_table"], np.int32).reshape(-1, 4)
  nf = int(a.info.num_action_fields)
  F = table[util.random_actions(rng, K, n, P, nact)][..., :nf].copy()
  F[3, 2, 1, 0] = 99   # an out-of-range field: a counted NOOP
  F = torch.from_numpy(np.ascontiguousarray(F)).to(a.device)
  got = _many(a, F, kinds, fields=True)
  ref = _loop(b, kinds, F, fields=True)
  _same_rows(got, ref, "fields")
  _same_engines(a, b, kinds, "fields")
  a.close(); b.close()


def test_substrate_with_a_custom_action_table_and_a_ring():
  """Through `Substrate`: a custom action_table (its rows go to the engine as raw fields) and
  rollout_length=T (one slot is written; the rows do not depend on it)."""
  cfg = substrate.get_config("clean_up")
  n, K, T = 6, 9, 4
  custom = [dict(cfg.action_set[i]) for i in (0, 3, 1, 7, 8, 5)]
  kw = dict(roles=cfg.default_player_roles, num_worlds=n, action_table=custom, env_seed=32, rollout_length=T)
  env = substrate.build("clean_up", **kw)
  twin = substrate.build("clean_up", **kw)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(17), K, n, env.num_players,
                                           len(custom))).to(env.engine.device)
  env.reset(); twin.reset()
  env.step(A[0]); twin.step(A[0])
  before = env.slot
  ring = env.rollout
  kept = {s: {k: v[s].clone() for k, v in ring["observation"].items()} for s in range(T)}
  leaves = env.step_leaves()
  assert "READY_TO_SHOOT" in leaves and cfg.aux0_name in leaves and "RGB" not in leaves
  res = env.step_many(A, observations=True)
  assert isinstance(res, substrate.StepManyTrajectory) and set(res.observation) == set(leaves)
  assert env.slot == (before + 1) % T == res.timestep.slot
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.reward[k], ts.reward) and torch.equal(res.step_type[k], ts.step_type), k
    for name in leaves:
      assert torch.equal(res.observation[name][k], ts.observation[name]), (name, k)
  for name, leaf in ts.observation.items():
    assert torch.equal(res.timestep.observation[name], leaf), name
  for s in range(T):
    if s != env.slot:
      for name, v in kept[s].items():
        assert torch.equal(ring["observation"][name][s], v), (s, name)
  assert torch.equal(env.engine.save_worlds(), twin.engine.save_worlds())
  with pytest.raises(ValueError, match="pixel leaf"):
    env.step_many(A, observations=("RGB",))
  env.close(); twin.close()


def test_column_slices_of_wider_tensors():
  """Actions and rows as columns [:, off:off + n] of wider tensors; the slice start puts every
  world's LAYER block on an odd dword (clean_up: 7 x 11 x 11 x L int32 a world, times off = 1)."""
  pack = engine.load_pack("clean_up")
  n, K, off, total = 12, 10, 1, 15
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_LAYER,)
  a, _ = _engine(pack, n, kinds)
  b, _ = _engine(pack, n, kinds)
  P, nact = a.P, a.num_actions
  dev = a.device
  per_world = int(np.prod(a.shapes[E.OBS_LAYER][0][1:]))
  assert (off * per_world) % 2 == 1, "the slice start is meant to be an odd dword"
  wide = torch.full((K, total, P), -77, dtype=torch.int32, device=dev)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(17), K, n, P, nact)).to(dev)
  wide[:, off:off + n] = A
  outs = {}
  for kind in kinds:
    shape, dtype = a.shapes[kind]
    outs[_key(kind)] = torch.full((K, total) + shape[1:], 123, dtype=dtype, device=dev)
  a.reset(); b.reset()
  got = _many(a, wide[:, off:off + n], kinds, out={k: v[:, off:off + n] for k, v in outs.items()})
  ref = _loop(b, kinds, A)
  _same_rows(got, ref, "strides")
  _same_engines(a, b, kinds, "strides")
  for k, v in outs.items():
    assert got[k].data_ptr() == v[:, off:off + n].data_ptr()
    assert (v[:, :off] == 123).all() and (v[:, off + n:] == 123).all(), k   # the neighbours survive
  assert (wide[:, :off] == -77).all() and (wide[:, off + n:] == -77).all()
  a.close(); b.close()


def test_mixture_of_the_two_player_kitchens_stacks_layer():
  names = tuple(f"collaborative_cooking__{k}" for k in ("asymmetric", "circuit", "cramped", "forced", "ring"))
  K = 14
  kw = dict(num_worlds=40, env_seed=33, individual_observations=("LAYER", "POSITION"), global_observations=())
  mix = substrate.build_mixture(names, **kw)
  twin = substrate.build_mixture(names, **kw)
  n, P = mix.num_worlds, mix.num_players
  A = torch.from_numpy(util.random_actions(np.random.default_rng(18), K, n, P,
                                           mix.action_spec()[0].num_values)).to(mix.engines[0].device)
  mix.reset(); twin.reset()
  res = mix.step_many(A, observations=("LAYER",))
  assert isinstance(res, substrate.StepManyTrajectory) and tuple(res.observation) == ("LAYER",)
  layer = res.observation["LAYER"]
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.reward[k], ts.reward) and torch.equal(res.step_type[k], ts.step_type), k
    assert layer[k].shape == ts.observation["LAYER"].shape and layer.dtype == torch.int32
    assert torch.equal(layer[k], ts.observation["LAYER"]), k
  for name, leaf in ts.observation.items():
    assert torch.equal(res.timestep.observation[name], leaf), name
  for x, y in zip(mix.engines, twin.engines):
    assert torch.equal(x.save_worlds(), y.save_worlds())
  res = mix.step_many(A, observations=True)
  assert set(res.observation) == {"LAYER", "POSITION", "COLLECTIVE_REWARD"}
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.observation["POSITION"][k], ts.observation["POSITION"]), k
    assert torch.equal(res.observation["LAYER"][k], ts.observation["LAYER"]), k
  mix.close(); twin.close()


@pytest.mark.parametrize("n", [10, 7])
def test_the_largest_map_and_a_ragged_last_workgroup(n):
  """The 64 x 64 map steps two worlds per workgroup; n = 7 leaves its last workgroup half empty."""
  pack = geometry.pack("clean_up", width=64, height=64)
  K = 12
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_LAYER,)
  a, _ = _engine(pack, n, kinds)
  b, _ = _engine(pack, n, kinds)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(20), K, n, a.P, a.num_actions)).to(a.device)
  a.reset(); b.reset()
  got = _many(a, A, kinds)
  ref = _loop(b, kinds, A)
  _same_rows(got, ref, ("64 x 64", n))
  _same_engines(a, b, kinds, ("64 x 64", n))
  a.close(); b.close()


def test_a_world_count_that_is_no_multiple_of_the_worlds_per_workgroup():
  pack = engine.load_pack("prisoners_dilemma_in_the_matrix__arena")
  n, K = 13, 9   # (four worlds a workgroup: the last one steps one)
  kinds = tuple(FIVE.values()) + FIN + (E.OBS_LAYER, E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES)
  a, _ = _engine(pack, n)          # rows only, nothing bound
  b, _ = _engine(pack, n, kinds)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(23), K, n, a.P, a.num_actions)).to(a.device)
  a.reset(); b.reset()
  got = _many(a, A, kinds)
  ref = _loop(b, kinds, A)
  _same_rows(got, ref, "13 worlds")
  _same_engines(a, b, kinds, "13 worlds")
  a.close(); b.close()


@pytest.mark.parametrize("name", ["prisoners_dilemma_in_the_matrix__arena", "gift_refinements"])
def test_substrate_ring_and_the_inventories(name):
  """rollout_length=T ring-binds every leaf, the inventories among them: each submission writes
  another slot, and the rows of a kind the level's own code writes come from THIS call's slot."""
  cfg = substrate.get_config(name)
  n, K, T = 6, 11, 3
  kw = dict(roles=cfg.default_player_roles, num_worlds=n, env_seed=34, rollout_length=T)
  env = substrate.build(name, **kw)
  twin = substrate.build(name, **kw)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(24), 2 * K, n, env.num_players,
                                           env.action_spec()[0].num_values)).to(env.engine.device)
  env.reset(); twin.reset()
  env.step(A[0]); twin.step(A[0])
  leaves = env.step_leaves()
  assert "INVENTORY" in leaves
  for call in range(2):      # (two calls: two different slots)
    acts = A[call * K:(call + 1) * K]
    before = env.slot
    res = env.step_many(acts, observations=True)
    assert env.slot == (before + 1) % T == res.timestep.slot
    for k in range(K):
      ts = twin.step(acts[k])
      assert torch.equal(res.reward[k], ts.reward), (call, k)
      for leaf in leaves:
        assert torch.equal(res.observation[leaf][k], ts.observation[leaf]), (call, leaf, k)
    for leaf, v in ts.observation.items():
      assert torch.equal(res.timestep.observation[leaf], v), (call, leaf)
  assert torch.equal(env.engine.save_worlds(), twin.engine.save_worlds())
  env.close(); twin.close()


def test_engine_ring_of_level_kinds():
  """Engine.bind_ring of kinds the level's own code writes: the rows are read from the slot this
  submission writes, so row K - 1 is that slot, and the kinds written at every step equal the loop's."""
  pack = engine.load_pack("prisoners_dilemma_in_the_matrix__arena")
  n, K, T = 16, 20, 3
  ringed = (E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES, E.OBS_INTERACTION_REWARDS)
  a = engine.Engine(pack, n, device=0)
  b, _ = _engine(pack, n, ringed)
  rings = {k: a.bind_ring(k, slots=T, tune=False) for k in ringed}
  for v in rings.values():
    v.zero_()
  A = torch.from_numpy(util.random_actions(np.random.default_rng(25), 3 * K, n, a.P, 8,
                                           [1, 6, 1, 1, 1, 2, 2, 5])).to(a.device)
  a.reset(); b.reset()
  changed = False
  for call in range(3):
    acts = A[call * K:(call + 1) * K]
    slot = a.ring["next"]
    got = a.step_many(acts, observations=ringed)
    assert a.ring["last"] == slot
    ref = _loop(b, (E.OBS_REWARD, E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES), acts)
    assert torch.equal(got["reward"], ref["reward"]), call
    for kind in (E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES):   # written at every step
      assert torch.equal(got[kind], ref[kind]), (call, kind)
    for kind in ringed:
      assert torch.equal(got[kind][K - 1], rings[kind][slot]), (call, kind)
    changed = changed or bool((got[E.OBS_INVENTORY][0] != got[E.OBS_INVENTORY][K - 1]).any())
  assert changed, "no inventory changed in 60 steps: the slots cannot be told apart"
  assert torch.equal(a.save_worlds(), b.save_worlds())
  util.no_faults(a)
  a.close(); b.close()


# ---- 7. refusals --------------------------------------------------------------------------------
def _request(e, rows, **fields):
  """The return code of one raw MpStepTrajectory request on engine e (through mp_restore);
  rows: (kind, pointer, step_bytes) each."""
  arr = (engine.MpStepRow * max(len(rows), 1))()
  for i, (kind, ptr, dist) in enumerate(rows):
    arr[i].kind, arr[i].rows, arr[i].step_bytes = kind, ptr, dist
  req = engine.MpStepTrajectory(ctypes.sizeof(engine.MpStepTrajectory), 1)
  req.num_rows = len(rows)
  req.rows = arr
  for k, v in fields.items():
    if k == "no_rows":     # num_rows says v, the array is NULL
      req.num_rows, req.rows = v, None
    else:
      setattr(req, k, v)
  return e._L.mp_restore(e._h, ctypes.addressof(req), ctypes.sizeof(req))


def test_refusals_launch_nothing_and_leave_the_engine_as_it_was():
  pack = engine.load_pack("clean_up")
  n, K = 8, 6
  bound = tuple(FIVE.values()) + FIN
  e, bufs = _engine(pack, n, bound)
  L = e._L
  P, nact = e.P, e.num_actions
  dev = e.device
  A = torch.from_numpy(util.random_actions(np.random.default_rng(22), K, n, P, nact)).to(dev)
  ablock = n * P * 4

  def refused(word, rows=(), code=engine.MP_ERR_INVALID, **fields):
    assert _request(e, list(rows), **fields) == code, (word, fields, L.mp_last_error())
    assert b"MpStepTrajectory" in L.mp_last_error() and word.encode() in L.mp_last_error(), (word, L.mp_last_error())

  pos = torch.zeros((K, n, P, 2), dtype=torch.int32, device=dev)
  posb = n * P * 8
  refused("never been reset", [(E.OBS_POSITION, pos.data_ptr(), posb)], steps=K, actions=A.data_ptr(),
          actions_step_bytes=ablock)
  e.reset()
  e.step(A[0])
  state, ctr = e.save_worlds().clone(), e.counters()
  scal = {k: v.clone() for k, v in bufs.items()}
  ok = dict(steps=K, actions=A.data_ptr(), actions_step_bytes=ablock)
  # what MpStepMany refuses, under this request's name
  refused("NULL", steps=K, actions=None)
  null = engine.MpStepTrajectory(ctypes.sizeof(engine.MpStepTrajectory), 1)
  assert L.mp_restore(None, ctypes.addressof(null), ctypes.sizeof(null)) == engine.MP_ERR_INVALID
  refused("steps", **dict(ok, steps=0))
  refused("steps", **dict(ok, steps=engine.STEP_MANY_MAX + 1))
  refused("struct_size", **dict(ok, struct_size=8))
  refused("fields", **dict(ok, fields=2))
  refused("actions_step_bytes", **dict(ok, actions_step_bytes=ablock - 4))
  refused("actions_step_bytes", **dict(ok, actions_step_bytes=ablock + 2))
  rew = torch.zeros((K, n, P), dtype=torch.float64, device=dev)
  refused("REWARD", [(E.OBS_REWARD, rew.data_ptr(), n * P * 8 - 8)], **ok)
  refused("num_rows", **dict(ok, num_rows=-1))
  refused("num_rows", **dict(ok, no_rows=2))
  # kinds
  layer = torch.zeros((K,) + e.shapes[E.OBS_LAYER][0], dtype=torch.int32, device=dev)
  layerb = layer[0].numel() * 4
  for pixel in E.PIXEL_KINDS:
    refused("rollout ring", [(pixel, layer.data_ptr(), layerb)], **ok)
  refused("no observation kind", [(E.OBS_RGB_POOL8 + 1, layer.data_ptr(), layerb)], **ok)
  refused("no observation kind", [(-1, layer.data_ptr(), layerb)], **ok)
  refused("named twice", [(E.OBS_POSITION, pos.data_ptr(), posb), (E.OBS_POSITION, pos.data_ptr(), posb)], **ok)
  refused("named twice", [(E.OBS_REWARD, rew.data_ptr(), n * P * 8), (E.OBS_REWARD, rew.data_ptr(), n * P * 8)], **ok)
  refused("no buffer", [(E.OBS_POSITION, None, posb)], **ok)
  inv = torch.zeros((K, n, P, 3), dtype=torch.float64, device=dev)
  for kind in (E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES, E.OBS_MATRIX_CUMULANTS, E.OBS_INTERACTION_REWARDS):
    refused("no observation", [(kind, inv.data_ptr(), n * P * 24)], code=MP_ERR_UNSUPPORTED, **ok)   # clean_up has none
  aux = torch.zeros((K, n, P, P), dtype=torch.float64, device=dev)
  for kind in (E.OBS_AUX1, E.OBS_AUX2, E.OBS_AUX3, E.OBS_AUX4):   # debug kinds that are not being produced
    refused("not produced", [(kind, aux.data_ptr(), n * P * 8)], code=MP_ERR_UNSUPPORTED, **ok)
  refused("not produced", [(E.OBS_ZAP_MATRIX, aux.data_ptr(), n * P * P * 8)], code=MP_ERR_UNSUPPORTED, **ok)
  # (a debug kind the substrate HAS, on an engine that does not produce it)
  mx = engine.Engine(engine.load_pack("prisoners_dilemma_in_the_matrix__arena"), n, device=0)
  mx.reset()
  Am = torch.zeros((K, n, mx.P), dtype=torch.int32, device=dev)
  cum = torch.zeros((K,) + mx.shapes[E.OBS_MATRIX_CUMULANTS][0], dtype=torch.float64, device=dev)
  mstate = mx.save_worlds().clone()
  assert _request(mx, [(E.OBS_MATRIX_CUMULANTS, cum.data_ptr(), cum[0].numel() * 8)], steps=K,
                  actions=Am.data_ptr(), actions_step_bytes=n * mx.P * 4) == MP_ERR_UNSUPPORTED
  assert b"not produced" in L.mp_last_error() and b"MpStepTrajectory" in L.mp_last_error()
  assert torch.equal(mx.save_worlds(), mstate) and (cum == 0).all()
  mx.close()
  # distances and alignment
  refused("step_bytes", [(E.OBS_POSITION, pos.data_ptr(), posb - 4)], **ok)      # smaller than a step's rows
  refused("step_bytes", [(E.OBS_POSITION, pos.data_ptr(), posb + 2)], **ok)      # not a multiple of 4
  refused("step_bytes", [(E.OBS_READY_TO_SHOOT, rew.data_ptr(), n * P * 8 + 4)], **ok)   # f64: of 8
  refused("step_bytes", [(E.OBS_LAYER, layer.data_ptr(), layerb - 4)], **ok)
  refused("aligned", [(E.OBS_LAYER, layer.data_ptr() + 2, layerb)], **ok)
  refused("aligned", [(E.OBS_AUX0, rew.data_ptr() + 4, n * P * 8)], **ok)
  # memory the device cannot be trusted with, and extents that leave their allocation
  pinned = torch.zeros((K, n, P, 2), dtype=torch.int32).pin_memory()
  refused("host", [(E.OBS_POSITION, pinned.data_ptr(), posb)], **ok)
  hip = ctypes.CDLL("libamdhip64.so")
  def end_of_allocation(tensor):
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size),
                                     ctypes.c_void_p(tensor.data_ptr())) == 0
    return base.value + size.value
  short = dict(ok, steps=K + 1)
  refused("allocation", [(E.OBS_POSITION, end_of_allocation(pos) - K * posb, posb)], **short)
  refused("allocation", [(E.OBS_LAYER, end_of_allocation(layer) - K * layerb, layerb)], **short)
  # the Python layer
  with pytest.raises(ValueError, match="pixel kind"):
    e.step_many(A, observations=[E.OBS_RGB])
  with pytest.raises(ValueError, match="named twice"):
    e.step_many(A, observations=[E.OBS_LAYER, E.OBS_LAYER])
  with pytest.raises(ValueError, match="named twice"):
    e.step_many(A, observations=[E.OBS_REWARD])      # keep= stacks it already
  with pytest.raises(engine.EngineError, match="no observation"):
    e.step_many(A, observations=[E.OBS_INVENTORY])
  with pytest.raises(ValueError, match="out"):
    e.step_many(A, observations=[E.OBS_POSITION], out={E.OBS_POSITION: pos.to(torch.int64)})
  # nothing was launched: the engine is as it was, and goes on like a twin
  assert torch.equal(e.save_worlds(), state) and e.counters() == ctr
  for k, v in bufs.items():
    assert torch.equal(v, scal[k]), k
  twin, _ = _engine(pack, n, bound)
  twin.reset()
  twin.step(A[0])
  kinds = bound + (E.OBS_LAYER,)
  got = _many(e, A, kinds)
  ref = _loop(twin, kinds, A)
  _same_rows(got, ref, "after refusals")
  _same_engines(e, twin, kinds, "after refusals")
  # a debug kind that IS produced, because it is bound, has rows
  zm = e.bind(E.OBS_ZAP_MATRIX); tz = twin.bind(E.OBS_ZAP_MATRIX)
  zm.zero_(); tz.zero_()
  got = e.step_many(A, observations=[E.OBS_ZAP_MATRIX])
  ref = _loop(twin, (E.OBS_ZAP_MATRIX,), A)
  assert torch.equal(got[E.OBS_ZAP_MATRIX], ref[E.OBS_ZAP_MATRIX])
  e.close(); twin.close()


# ---- 8. at size ---------------------------------------------------------------------------------
def test_at_size_sampled_worlds_match_the_oracle():
  pack = engine.load_pack("clean_up")
  n, K = 4096, 16
  e, _ = _engine(pack, n)
  A = util.random_actions(np.random.default_rng(21), K, n, e.P, e.num_actions)
  e.reset()
  got = e.step_many(torch.from_numpy(A).to(e.device), keep=("reward",),
                    observations=(E.OBS_LAYER, E.OBS_READY_TO_SHOOT, E.OBS_POSITION))
  worlds = sorted(set([0, n - 1] + list(range(5, n, 256))))
  idx = torch.tensor(worlds, device=e.device)
  rows = {k: v[:, idx].cpu().numpy() for k, v in got.items()}
  for i, w in enumerate(worlds):
    o = util.make_oracles(pack, 1, offset=w)[0]
    o.reset()
    for k in range(K):
      o.step(A[k, w])
      assert np.array_equal(rows["reward"][k, i], o.rewards()), (w, k)
      assert np.array_equal(rows[E.OBS_LAYER][k, i], np.stack([o.layer_view(p) for p in range(e.P)])), (w, k)
      assert np.array_equal(rows[E.OBS_READY_TO_SHOOT][k, i], o.ready_to_shoot()), (w, k)
      assert np.array_equal(rows[E.OBS_POSITION][k, i], o.dump()[1][:, :2]), (w, k)
    o.close()
  util.no_faults(e)
  e.close()
