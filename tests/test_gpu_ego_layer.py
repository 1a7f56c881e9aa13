"""EGO_LAYER on the GPU (MpEgoLayer; Engine.observe_ego_layer / bind_ego_layer, the "EGO_LAYER"
leaf of Substrate and MixtureSubstrate): both kernels byte for byte against the numpy model of
tests/ego_layer_model.py — which the engine's own "LAYER" holds to the oracle-held leaf through
its north crop — on the stock levels and on edited geometries, the pin to "RGB" (equal stacks,
equal pixels; "LAYER" fails that check), the leaf behind every kind of submission with and
without a rollout ring, the mixture's shared leaf, and indices out of range."""
import numpy as np
import pytest
import torch

import ego_layer_model as M
import geometry
import util
from meltingpot_amd import engine, substrate
from meltingpot_amd import pack as pack_lib

pytestmark = pytest.mark.gpu

E = engine
N = 6
SEED = 5   # (chosen with the CPU oracle: all four facings and dead viewers within 25 random steps)


def _same(got, want, what):
  got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
  assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def _fields(eng, bank):
  layout = substrate.SubstrateStateLayout(eng.state_layout(), pack_lib.loads(eng.pack_bytes))
  return substrate.StateFields(bank, layout)


def _model(eng, bank, north=False):
  return M.of_fields(eng.pack_bytes, _fields(eng, bank), north)


def _all_pairs(R, P, device):
  rows = torch.arange(R, dtype=torch.int32, device=device).repeat_interleave(P)
  players = torch.arange(P, dtype=torch.int32, device=device).repeat(R)
  return rows, players


def _compare_draws(eng, bank, want, what):
  """Both kernels over every row and every (row, player) of `bank`, then a sample with repeats
  and more elements than the engine has worlds."""
  R, P = want.shape[:2]
  _same(eng.observe_ego_layer(bank), want, (what, "rows"))
  rows, players = _all_pairs(R, P, eng.device)
  _same(eng.observe_ego_layer(bank, rows=rows, players=players), want.reshape((R * P,) + want.shape[2:]),
        (what, "views"))
  rng = np.random.default_rng(11)
  count = 3 * eng.N + 1
  r = rng.integers(0, R, size=count).astype(np.int32)
  r[1] = r[0]
  p = rng.integers(0, P, size=count).astype(np.int32)
  p[1] = p[0]
  _same(eng.observe_ego_layer(bank, rows=r), want[r], (what, "repeated rows"))
  # (an odd first element: the destination of the second starts off a 16-byte line where a view is odd)
  _same(eng.observe_ego_layer(bank, rows=r, players=p), want[r, p], (what, "repeated views"))


# ---- 1. the draw form against the model ---------------------------------------------------------
@pytest.mark.parametrize("name,players", [("clean_up", 7), ("commons_harvest__open", 16)])
def test_both_kernels_equal_the_model(name, players):
  env = substrate.build(name, roles=("default",) * players, num_worlds=N, env_seed=SEED)
  eng = env.engine
  lay = eng.bind(E.OBS_LAYER)
  env.reset()
  A = util.random_actions(np.random.default_rng(SEED), 25, N, players, eng.num_actions)
  res = env.step_many(torch.from_numpy(A).to(eng.device), states=True)
  bank = res.states.data
  assert tuple(bank.shape[:1]) == (25 * N,)
  f = _fields(eng, bank)
  # the condition: every facing and a dead viewer are among the drawn views
  assert set(np.unique(f.orientation.cpu().numpy()).tolist()) == {0, 1, 2, 3}
  assert bool((f.alive.cpu().numpy() == 0).any())
  want = _model(eng, bank)
  assert want.shape == (25 * N, players) + substrate.layer_spec(eng.pack_bytes).shape
  _compare_draws(eng, bank, want, name)
  # the model's north crop is the engine's own "LAYER" of the same rows, and the bound leaf
  north = _model(eng, bank, north=True)
  _same(eng.observe_states(bank, E.OBS_LAYER), north, (name, "LAYER of the rows"))
  _same(lay, north[-N:], (name, "the bound LAYER"))
  assert (want != north).any()
  # through the Substrate, and the live worlds (states=None: rows are world indices)
  _same(env.observe_ego_layer(res.states), want, (name, "Substrate"))
  _same(env.observe_ego_layer(), want[-N:], (name, "live worlds"))
  worlds, viewers = [5, 0, 0, 3, 2, 2, 1, 4], [0, 1, 1, 2, 3, players - 1, 4, 5]
  _same(env.observe_ego_layer(rows=worlds), want[-N:][worlds], (name, "live worlds, listed"))
  _same(env.observe_ego_layer(rows=worlds, players=viewers), want[-N:][worlds, viewers], (name, "live views"))
  _same(env.observe_ego_layer(res.states, rows=worlds, players=viewers), want[worlds, viewers],
        (name, "Substrate views"))
  eng.sync()
  util.no_faults(eng)
  env.close()


# ---- 2. geometry -----------------------------------------------------------------------------------
GEOMETRIES = [dict(name="clean_up", view=(0, 0, 0, 0)),
              dict(name="clean_up", view=(0, 7, 3, 0)),
              dict(name="coins", view=(3, 18, 1, 0)),
              dict(name="clean_up", topology="TORUS", open_edges=True, view=(5, 5, 21, 1)),
              dict(name="commons_harvest__open", topology="TORUS", open_edges=True)]


@pytest.mark.parametrize("variant", GEOMETRIES, ids=geometry.variant_id)
def test_edited_windows_and_tori(variant):
  assert variant in geometry.ACCEPTED
  eng = E.Engine(geometry.variant_pack(variant), N, device=0)
  lay = eng.bind(E.OBS_LAYER)
  eng.reset()
  A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 25, N, eng.P, eng.num_actions)).to(eng.device)
  banks = []
  for k in range(25):
    eng.step(A[k])
    if k % 6 == 0 or k == 24:
      banks.append(eng.save_worlds().clone())
  bank = torch.cat(banks)
  f = _fields(eng, bank)
  assert set(np.unique(f.orientation.cpu().numpy()).tolist()) == {0, 1, 2, 3}
  want = _model(eng, bank)
  _compare_draws(eng, bank, want, geometry.variant_id(variant))
  north = _model(eng, bank, north=True)
  _same(eng.observe_states(bank, E.OBS_LAYER), north, "LAYER of the rows")
  _same(lay, north[-N:], "the bound LAYER")
  _same(eng.observe_ego_layer(), want[-N:], "live worlds")
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 3. the pin to RGB -----------------------------------------------------------------------------
def _stacks_decide_pixels(layer, rgb, avatar_layer):
  """One viewer: over the cells whose avatar-layer entry is 0, do equal [L] stacks have identical
  8 x 8 x 3 pixel blocks?  layer [VH, VW, L], rgb [VH * 8, VW * 8, 3]."""
  VH, VW, _ = layer.shape
  blocks = rgb.reshape(VH, 8, VW, 8, 3).transpose(0, 2, 1, 3, 4).reshape(VH * VW, -1)
  stacks = layer.reshape(VH * VW, -1)
  seen = {}
  for stack, block in zip(stacks, blocks):
    if stack[avatar_layer] != 0:
      continue
    key = stack.tobytes()
    if key in seen and seen[key] != block.tobytes():
      return False
    seen[key] = block.tobytes()
  return True


def test_equal_stacks_have_equal_pixels_and_the_north_window_does_not():
  env = substrate.build("clean_up", roles=("default",) * 7, num_worlds=8, env_seed=SEED)
  env.reset()
  states = env.save_state()
  f = env.state_fields(states)
  P = env.num_players
  facing = (torch.arange(8)[:, None] + torch.arange(P)[None, :]) % 4
  f.orientation.copy_(facing.to(f.orientation.dtype).to(f.orientation.device))
  assert not env.check_states(states).cpu().numpy().any()
  rgb = env.observe_states(states, ("RGB",))["RGB"].cpu().numpy()
  ego = env.observe_ego_layer(states).cpu().numpy()
  north = env.engine.observe_states(states.data, E.OBS_LAYER).cpu().numpy()
  avatar_layer = env.state_layout().avatar_layer
  alive = f.alive.cpu().numpy()
  assert alive.all() and rgb.shape[2:] == (88, 88, 3)
  failed_north = 0
  for r in range(8):
    for p in range(P):
      assert _stacks_decide_pixels(ego[r, p], rgb[r, p], avatar_layer), (r, p, int(facing[r, p]))
      if int(facing[r, p]) == 0:
        assert np.array_equal(ego[r, p], north[r, p])
      else:
        failed_north += not _stacks_decide_pixels(north[r, p], rgb[r, p], avatar_layer)
  assert failed_north > 0   # (the power of the check: the north window does not name what RGB shows)
  env.engine.sync()
  util.no_faults(env.engine)
  env.close()


# ---- 4. the leaf -----------------------------------------------------------------------------------
def _leaf_config(name="clean_up"):
  cfg = substrate.get_config(name)
  cfg.individual_observation_names = list(cfg.individual_observation_names) + ["EGO_LAYER"]
  return cfg


@pytest.mark.parametrize("T", [0, 3])
def test_the_leaf_follows_every_submission(T):
  cfg, plain_cfg = _leaf_config(), substrate.get_config("clean_up")
  kw = dict(roles=cfg.default_player_roles, num_worlds=N, env_seed=SEED)
  if T:
    kw["rollout_length"] = T
  env = substrate.build_from_config(cfg, **kw)
  twin = substrate.build_from_config(plain_cfg, **kw)
  eng = env.engine
  P = env.num_players
  spec = env.observation_spec()[0]["EGO_LAYER"]
  assert spec.shape == substrate.layer_spec(eng.pack_bytes).shape and spec.dtype == np.int32
  assert "EGO_LAYER" in env.state_leaves() and "EGO_LAYER" not in twin.state_leaves()
  stats = env.set_episode_stats(columns=())
  fused = eng.fused
  rng = np.random.default_rng(SEED)
  acts = lambda *shape: torch.from_numpy(util.random_actions(rng, 1, int(np.prod(shape)), P, eng.num_actions)
                                         .reshape(shape + (P,))).to(eng.device)
  history = {}   # ring slot -> the bytes it was given

  def check(ts, what):
    leaf = ts.observation["EGO_LAYER"]
    assert tuple(leaf.shape) == (N, P) + spec.shape and leaf.dtype == torch.int32
    want = _model(eng, env.save_state().data)
    _same(leaf, want, (what, "model"))
    _same(env.observe_ego_layer(), want, (what, "observe_ego_layer"))
    if T:
      assert ts.slot == env.slot
      _same(env.rollout["observation"]["EGO_LAYER"][ts.slot], want, (what, "ring slot"))
      history[ts.slot] = want
      for s, kept in history.items():   # slots written earlier keep their bytes for T submissions
        _same(env.rollout["observation"]["EGO_LAYER"][s], kept, (what, "slot", s))

  check(env.reset(), "reset"); twin.reset()
  a = acts(N)
  check(env.step(a), "step"); twin.step(a)
  if not T:
    a, mask = acts(N), torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=eng.device)
    check(env.step(a, active=mask), "masked step"); twin.step(a, active=mask)
  a = acts(5, N)
  check(env.step_many(a).timestep, "step_many"); twin.step_many(a)
  saved = env.save_state()
  a = acts(N)
  check(env.step(a), "step"); twin.step(a)
  src = [2, -1, 0, 0, -1, 5]
  check(env.load_state(saved, src), "load_state"); twin.load_state(twin_states(twin, saved), src)
  drawn = env.observe_states(saved, ("EGO_LAYER",), rows=[3, 3, 1], players=[0, 6, 2])["EGO_LAYER"]
  _same(drawn, _model(eng, saved.data)[[3, 3, 1], [0, 6, 2]], "observe_states")
  with pytest.raises(ValueError, match=r"states=True.*observe_states"):
    env.step_many(acts(2, N), observations=("EGO_LAYER",))
  # the twin without the leaf ends on identical records and identical other leaves
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  ours, theirs = env.observation(), twin.observation()
  assert set(ours) == set(theirs) | {"EGO_LAYER"}
  for n in theirs:
    assert torch.equal(ours[n], theirs[n]), n
  # (set_episode_stats beside the leaf: both launches follow every submission; no episode has closed)
  length = stats.running["length"].cpu().numpy()
  assert (length[[1, 4]] > 0).all() and (length[[0, 2, 3, 5]] == 0).all() and bool(stats.open.all())   # (loaded: FIRST)
  # clearing the registration: the leaf is written no more, the engine's launches are its own
  frozen = env.rollout["observation"]["EGO_LAYER"].clone() if T else env.observation()["EGO_LAYER"].clone()
  eng.bind_ego_layer(None)
  assert eng.fused == fused == twin.engine.fused
  a = acts(N)
  env.step(a); twin.step(a)
  now = env.rollout["observation"]["EGO_LAYER"] if T else env.observation()["EGO_LAYER"]
  assert torch.equal(now, frozen)
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  for e in (eng, twin.engine):
    e.sync()
    util.no_faults(e)
  env.close()
  twin.close()


def twin_states(twin, saved):
  """`saved` (another substrate's rows of the same pack and seed) as the twin's own WorldStates."""
  return substrate.WorldStates(saved.data, twin.engine.state_fingerprint)


def test_build_substrate_names_the_leaf_beside_pooled_views():
  cfg = substrate.get_config("clean_up")
  env = substrate.build_substrate(lab2d_settings=geometry.settings("clean_up"),
                                  individual_observations=["RGB", "LAYER", "EGO_LAYER"],
                                  global_observations=["WORLD.RGB"], action_table=cfg.action_set, num_worlds=N,
                                  env_seed=SEED, rgb_pool=8, world_rgb_pool=4)
  eng = env.engine
  ts = env.reset()
  A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 6, N, env.num_players, eng.num_actions)).to(eng.device)
  for k in range(6):
    ts = env.step(A[k])
  bank = env.save_state().data
  _same(ts.observation["EGO_LAYER"], _model(eng, bank), "leaf")
  _same(ts.observation["LAYER"], _model(eng, bank, north=True), "LAYER")
  assert tuple(ts.observation["RGB"].shape[2:]) == (11, 11, 3)
  eng.sync()
  util.no_faults(eng)
  env.close()


def test_tune_does_not_write_the_leaf():
  """mp_tune's probe submissions (real steps on an engine nothing was done with, dry launches on one
  in use) leave the registered leaf and the records as they were."""
  for used in (False, True):
    eng = E.Engine(E.load_pack("clean_up"), N, device=0)
    eng.bind(E.OBS_WORLD_RGB)
    leaf = eng.bind_ego_layer(torch.full(eng.ego_layer_shape, -7, dtype=torch.int32, device=eng.device))
    if used:
      eng.reset()
      eng.step(torch.zeros((N, eng.P), dtype=torch.int32, device=eng.device))
      before = (leaf.clone(), eng.save_worlds().clone())
      _same(leaf, _model(eng, before[1]), "before the probe")
    eng.tune()
    if used:
      assert torch.equal(leaf, before[0]) and torch.equal(eng.save_worlds(), before[1])
    else:
      assert bool((leaf == -7).all())
    eng.sync()
    util.no_faults(eng)
    eng.close()


# ---- 5. mixture ------------------------------------------------------------------------------------
def test_a_mixture_shares_one_leaf():
  names = ["collaborative_cooking__cramped", "collaborative_cooking__ring"]
  ind = list(substrate.get_config(names[0]).individual_observation_names) + ["EGO_LAYER"]
  for T in (0, 2):
    kw = dict(rollout_length=T) if T else {}
    mix = substrate.build_mixture(names, num_worlds=[2, 2], individual_observations=ind, env_seed=SEED, **kw)
    P = mix.num_players
    dev = mix._members[0].engine.device
    ts = mix.reset()
    A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 8, 4, P, mix.action_spec()[0].num_values)).to(dev)
    for k in range(8):
      ts = mix.step(A[k])
    leaf = ts.observation["EGO_LAYER"]
    assert tuple(leaf.shape[:2]) == (4, P) and leaf.dtype == torch.int32
    whole = mix.observe_ego_layer()
    assert torch.equal(leaf, whole)
    for i, m in enumerate(mix._members):
      sl = mix.member_slice(i)
      own = m.observe_ego_layer()
      assert torch.equal(leaf[sl], own), (T, i)
      _same(own, _model(m.engine, m.save_state().data), (T, i, "model"))
      m.engine.sync()
      util.no_faults(m.engine)
    assert not torch.equal(leaf[mix.member_slice(0)], leaf[mix.member_slice(1)])
    mix.close()


# ---- 6. bad indices --------------------------------------------------------------------------------
def test_an_index_out_of_range_leaves_its_element_and_is_reported():
  eng = E.Engine(E.load_pack("clean_up"), N, device=0)
  eng.reset()
  bank = eng.save_worlds()
  want = _model(eng, bank)
  P = eng.P
  fill = -7
  out = torch.full((4, P) + want.shape[2:], fill, dtype=torch.int32, device=eng.device)
  eng.observe_ego_layer(bank, rows=[1, N, 0, -1], out=out)
  with pytest.raises(ValueError, match=r"MpEgoLayer: rows\[(1\] = 6|3\] = -1) is not a row"):
    eng.sync()
  got = out.cpu().numpy()
  assert np.array_equal(got[0], want[1]) and np.array_equal(got[2], want[0])
  assert (got[1] == fill).all() and (got[3] == fill).all()
  out = torch.full((3,) + want.shape[2:], fill, dtype=torch.int32, device=eng.device)
  eng.observe_ego_layer(bank, rows=[2, 2, 5], players=[0, P, 6], out=out)
  with pytest.raises(ValueError, match=rf"MpEgoLayer: players\[1\] = {P} is not a player"):
    eng.sync()
  got = out.cpu().numpy()
  assert np.array_equal(got[0], want[2, 0]) and np.array_equal(got[2], want[5, 6]) and (got[1] == fill).all()
  # the live worlds: a world index out of range
  out = torch.full((2, P) + want.shape[2:], fill, dtype=torch.int32, device=eng.device)
  eng.observe_ego_layer(None, rows=[N + 3, 4], out=out)
  with pytest.raises(ValueError, match=r"MpEgoLayer: rows\[0\] = 9"):
    eng.sync()
  got = out.cpu().numpy()
  assert (got[0] == fill).all() and np.array_equal(got[1], want[4])
  # host-side refusals launch nothing, and the engine stays usable
  with pytest.raises(ValueError, match="fingerprint"):
    eng.observe_ego_layer(bank, fingerprint=1)
  with pytest.raises(ValueError, match="without a row list"):
    eng.observe_ego_layer(bank[:2], players=[0, 0, 0])
  with pytest.raises(ValueError, match="device"):
    E.ego_layer_request(eng._L, eng._h, E.MP_EGO_REGISTER, dst=out.cpu().numpy().ctypes.data, dst_bytes=1 << 30)
  fresh = E.Engine(E.load_pack("clean_up"), 2, device=0)
  with pytest.raises(ValueError, match="never been reset"):
    fresh.observe_ego_layer()
  fresh.close()
  eng.step(torch.zeros((N, P), dtype=torch.int32, device=eng.device))
  _same(eng.observe_ego_layer(), _model(eng, eng.save_worlds()), "after the reports")
  eng.sync()
  util.no_faults(eng)
  eng.close()
