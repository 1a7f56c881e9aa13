""""N.LAYER" (avatar_library.lua:246-257; A17) written by the launch that steps the worlds, from
the records while they are in LDS: the stand-alone step kernels when it is bound alone, the frame
launch's feeders beside the pixel views, the rules launch of the two-launch form.  Every int32 is
held against `Oracle.layer_view` — every committed pack, dead and removed avatars (OutOfBounds on
every layer), TORUS maps, forced plans, the benchmarked size — and against mp_observe's own
launch.  It is offered as a rollout ring (mp_bind_output_ring), which mp_tune leaves alone, and
through `Substrate`, `build_substrate`, an edited `SubstrateConfig` and `lab2d_env`.  No fault
word may be set after any of it."""
import os
import pickle

import numpy as np
import pytest
import torch

import util
from meltingpot_amd import builder, engine, lab2d_env, substrate

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(engine.__file__), "assets")
PACKS = sorted(f[:-4] for f in os.listdir(ASSETS) if f.endswith(".mpk"))
POOL_OF = {k: f for f, k in engine.OBS_RGB_POOL.items()}


def _layers(oracles):
  return np.stack([np.stack([o.layer_view(p) for p in range(o.P)]) for o in oracles])


def _oob_rows(pack, lay):
  """(world, player) whose whole window is one value on every layer: an off-grid or dead viewer."""
  flat = lay.reshape(lay.shape[0], lay.shape[1], -1)
  return int((flat == flat[:, :, :1]).all(axis=2).sum())


def _run(name, n, steps, looks, seed=0, pack=None, weights=None, agent=None, world=False,
         world_pool=1, dev=None, unfused=None):
  """LAYER bound (with the per-agent view `agent` and / or WORLD.RGB beside it), n worlds stepped
  with random actions next to n oracles; LAYER, every bound pixel and the state compared after the
  reset and after the steps in `looks`.  Returns how many (world, player) windows were all
  OutOfBounds over the looks."""
  pack = pack or engine.load_pack(name)
  e = engine.Engine(pack, n, device=0, dev=dev, world_pool=world_pool, unfused=unfused)
  lay = e.bind(engine.OBS_LAYER)
  bufs = {}
  if agent is not None:
    bufs[agent] = e.bind(agent)
  if world:
    bufs[engine.OBS_WORLD_RGB] = e.bind(engine.OBS_WORLD_RGB)
  oracles = util.make_oracles(pack, n)
  P, nact = e.P, e.num_actions
  rng = np.random.default_rng(seed)
  acts = util.random_actions(rng, steps, n, P, nact, weights)
  dacts = torch.from_numpy(acts).to(e.device)
  oob = 0
  try:
    e.reset()
    for o in oracles:
      o.reset()
    for s in range(steps + 1):
      if s > 0:
        e.step(dacts[s - 1])
        for w, o in enumerate(oracles):
          o.step(acts[s - 1, w])
      if s not in looks and s != steps:
        continue
      got = lay.cpu().numpy()
      want = _layers(oracles)
      assert got.shape == want.shape, (got.shape, want.shape)
      for w in range(n):
        assert np.array_equal(got[w], want[w]), (name, s, w)
      # ... and what mp_observe's own launch reads from the records
      assert torch.equal(e.observe(engine.OBS_LAYER), lay), (name, s)
      oob += _oob_rows(pack, got)
      if bufs:
        grid, avat, _ = e.dump()
        for w, o in enumerate(oracles):
          og, oa, _ = o.dump()
          assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), (name, s, w)
        if agent is not None:
          host = bufs[agent].cpu().numpy()
          for w, o in enumerate(oracles):
            a = np.stack([o.render_agent(p) for p in range(P)])
            want_a = a if agent == engine.OBS_RGB else engine.pool_rgb(a, POOL_OF[agent])
            assert np.array_equal(host[w], want_a), (name, agent, s, w)
        if world:
          host = bufs[engine.OBS_WORLD_RGB].cpu().numpy()
          for w, o in enumerate(oracles):
            assert np.array_equal(host[w], engine.pool_rgb(o.render_world(), world_pool)), (name, s, w)
      util.no_faults(e)
  finally:
    for o in oracles:
      o.close()
    e.close()
  return oob


@pytest.mark.parametrize("name", PACKS)
def test_every_pack_layer_alone(name):
  """LAYER bound alone (the stand-alone step kernels write it): 7 worlds (a ragged last
  workgroup), 24 random steps with beams, after the reset and at steps 1, 9 and 24."""
  _run(name, 7, 24, looks=(0, 1, 9))


def test_dead_and_removed_avatars_see_out_of_bounds():
  """clean_up with zaps: zapped avatars wait off the grid and see OutOfBounds on every layer (A6)."""
  weights = [1, 1, 1, 1, 1, 1, 1, 12, 1]   # fireZap (index 7) most of the time
  oob = _run("clean_up", 16, 40, looks=tuple(range(0, 41, 2)), seed=11, weights=weights)
  assert oob > 0


@pytest.mark.parametrize("name", ["territory__rooms", "territory__open"])
def test_territory_zaps_and_torus(name):
  """territory: zapped avatars are removed; territory__rooms is a TORUS map (the window wraps)."""
  oob = _run(name, 12, 40, looks=tuple(range(0, 41, 4)), seed=12, weights=[1, 1, 1, 1, 1, 1, 1, 10, 2])
  if name == "territory__rooms":
    from meltingpot_amd import lower
    assert int(util.pack_tables(engine.load_pack(name))["hdr"][lower.HDR_TOPOLOGY]) == 1
  assert oob >= 0


VIEWS = [(engine.OBS_RGB, False, 1), (engine.OBS_RGB_POOL8, False, 1), (None, True, 1),
         (engine.OBS_RGB, True, 1), (engine.OBS_RGB_POOL4, True, 8)]


@pytest.mark.parametrize("name", ["clean_up", "territory__rooms", "coins", "collaborative_cooking__cramped"])
@pytest.mark.parametrize("dev", [
    None,
    {"batch_worlds": 1, "ring_batches": 6, "static_pct": 50, "max_groups": 4},
    {"batch_worlds": 3, "ring_batches": 2, "max_groups": 8, "world_waves": 1},
])
def test_layer_beside_pixel_views_forced_plans(name, dev):
  """The frame launch's feeders write LAYER: beside RGB, RGB_POOL8, WORLD.RGB, both views and
  pooled both; odd world counts and several batches per workgroup."""
  for agent, world, kw in VIEWS:
    _run(name, 37, 5, looks=(0, 1), seed=1, agent=agent, world=world, world_pool=kw, dev=dev)


@pytest.mark.parametrize("name", ["clean_up", "coins", "territory__rooms"])
def test_layer_beside_pixel_views_unfused(name):
  """MpConfig.unfused = 1: the rules launch writes LAYER, the draw-only launches the views."""
  for agent, world, kw in VIEWS[:4]:
    _run(name, 21, 6, looks=(0, 1), seed=3, agent=agent, world=world, world_pool=kw, unfused=True)


def test_tiny_batches():
  for n in (1, 2, 3, 5):
    _run("clean_up", n, 4, looks=(0, 1), seed=n, world=True)
    _run("clean_up", n, 4, looks=(0, 1), seed=n)


def test_benchmarked_size():
  """clean_up 4096 x 7: LAYER + WORLD.RGB under the plan mp_tune keeps, and LAYER alone — every
  world against mp_observe's launch on the same records, sampled worlds against the oracle."""
  name, n, steps = "clean_up", 4096, 3
  pack = engine.load_pack(name)
  rng = np.random.default_rng(9)
  acts = rng.integers(0, 9, size=(steps, n, 7), dtype=np.int32)
  sample = (0, 1, 63, 64, 1000, 2047, 3001, 4094, 4095)
  want = {}
  for w in sample:
    from oracle import oracle as oracle_lib
    o = oracle_lib.Oracle(pack, util.world_seed(w))
    o.reset()
    want[(w, 0)] = (np.stack([o.layer_view(p) for p in range(7)]), o.render_world())
    for s in range(steps):
      o.step(acts[s, w])
      want[(w, s + 1)] = (np.stack([o.layer_view(p) for p in range(7)]), o.render_world())
    o.close()
  dacts = torch.from_numpy(acts).to("cuda")
  for with_world in (True, False):
    e = engine.Engine(pack, n, device=0)
    lay = e.bind(engine.OBS_LAYER)
    wv = e.bind(engine.OBS_WORLD_RGB) if with_world else None
    if with_world:
      e.tune()
    e.reset()
    for s in range(steps + 1):
      if s > 0:
        e.step(dacts[s - 1])
      assert torch.equal(e.observe(engine.OBS_LAYER), lay), (with_world, s)
      for w in sample:
        assert np.array_equal(lay[w].cpu().numpy(), want[(w, s)][0]), (with_world, s, w)
        if with_world:
          assert np.array_equal(wv[w].cpu().numpy(), want[(w, s)][1]), (with_world, s, w)
    util.no_faults(e)
    e.close()
    del lay, wv
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,pixels", [("clean_up", False), ("coins", True), ("territory__rooms", True)])
def test_layer_ring(name, pixels):
  """Engine.bind_ring(OBS_LAYER): submission t writes slot t % T and no other slot; with a tuned
  pixel ring beside it.  mp_tune on an engine in use leaves every LAYER slot as it was."""
  pack = engine.load_pack(name)
  n, T, steps = 9, 3, 7
  e = engine.Engine(pack, n, device=0)
  ring = e.bind_ring(engine.OBS_LAYER, slots=T)
  assert tuple(ring.shape) == (T,) + tuple(e.shapes[engine.OBS_LAYER][0])
  wring = e.bind_ring(engine.OBS_WORLD_RGB, slots=T, tune=True) if pixels else None
  oracles = util.make_oracles(pack, n)
  rng = np.random.default_rng(4)
  acts = rng.integers(0, e.num_actions, size=(steps, n, e.P), dtype=np.int32)
  try:
    e.reset()
    for o in oracles:
      o.reset()
    for t in range(steps + 1):
      if t > 0:
        before = ring.cpu().numpy()
        e.step(torch.from_numpy(acts[t - 1]).to(e.device))
        for w, o in enumerate(oracles):
          o.step(acts[t - 1, w])
        after = ring.cpu().numpy()
        for sl in range(T):
          if sl != t % T:
            assert np.array_equal(after[sl], before[sl]), (t, sl)
      got = ring[t % T].cpu().numpy()
      assert np.array_equal(got, _layers(oracles)), t
      assert e.ring["last"] == t % T
      if pixels:
        world = np.stack([o.render_world() for o in oracles])
        assert np.array_equal(wring[t % T].cpu().numpy(), world), t
    # mp_tune on an engine in use (dry probes): no LAYER slot changes
    before = ring.cpu().numpy()
    e.tune()
    assert np.array_equal(ring.cpu().numpy(), before)
    assert torch.equal(e.observe(engine.OBS_LAYER), ring[e.ring["last"]])
    e.step(torch.from_numpy(acts[0]).to(e.device))
    for w, o in enumerate(oracles):
      o.step(acts[0, w])
    assert np.array_equal(ring[(steps + 1) % T].cpu().numpy(), _layers(oracles))
    util.no_faults(e)
  finally:
    for o in oracles:
      o.close()
    e.close()


def test_layer_ring_tuned_before_use():
  """mp_tune on an untouched engine (stepping probes, state put back) with a LAYER ring beside a
  pixel ring: the first reset and steps land in slots 0, 1, ... as the oracle has them."""
  pack = engine.load_pack("clean_up")
  n, T = 8, 2
  e = engine.Engine(pack, n, device=0)
  ring = e.bind_ring(engine.OBS_LAYER, slots=T)
  e.bind_ring(engine.OBS_RGB, slots=T, tune=False)
  e.tune()
  oracles = util.make_oracles(pack, n)
  e.reset()
  for o in oracles:
    o.reset()
  assert np.array_equal(ring[0].cpu().numpy(), _layers(oracles))
  a = np.full((n, e.P), 7, np.int32)
  e.step(torch.from_numpy(a).to(e.device))
  for w, o in enumerate(oracles):
    o.step(a[w])
  assert np.array_equal(ring[1].cpu().numpy(), _layers(oracles))
  util.no_faults(e)
  for o in oracles:
    o.close()
  e.close()


def _settings():
  here = os.path.dirname(os.path.abspath(__file__))
  with open(os.path.join(here, "golden", "clean_up_modified_settings.pkl"), "rb") as f:
    return pickle.load(f)["lab2d_settings"]


def test_build_substrate_with_layer():
  """build_substrate(individual_observations=["RGB", "LAYER"], num_worlds=64): the leaves, the
  spec and the rollout leaves against the oracle on the run-time pack."""
  from oracle import oracle as oracle_lib
  settings = _settings()
  cfg = substrate.get_config("clean_up")
  _, pack_bytes, _ = builder.lower_settings(settings, action_set=cfg.action_set)
  n = 64
  for T in (0, 3):
    env = substrate.build_substrate(lab2d_settings=settings, individual_observations=["RGB", "LAYER"],
                                    global_observations=["WORLD.RGB"], action_table=cfg.action_set,
                                    num_worlds=n, env_seed=50, rollout_length=T or None)
    refs = [oracle_lib.Oracle(pack_bytes, 50 + w, 7) for w in range(n)]
    try:
      spec = env.observation_spec()[0]
      assert spec["LAYER"] == substrate.layer_spec(pack_bytes)
      ts = env.reset()
      for o in refs:
        o.reset()
      assert set(ts.observation) == {"RGB", "LAYER", "WORLD.RGB", "COLLECTIVE_REWARD"}
      rng = np.random.default_rng(6)
      for s in range(6):
        lay = ts.observation["LAYER"]
        assert tuple(lay.shape) == (n, 7) + spec["LAYER"].shape and lay.dtype == torch.int32
        host = lay.cpu().numpy()
        rgb = ts.observation["RGB"].cpu().numpy()
        for w in range(0, n, 7):
          for p in range(7):
            assert np.array_equal(host[w, p], refs[w].layer_view(p)), (T, s, w, p)
            assert np.array_equal(rgb[w, p], refs[w].render_agent(p)), (T, s, w, p)
        a = rng.integers(0, 9, size=(n, 7)).astype(np.int32)
        ts = env.step(torch.from_numpy(a).to(env.engine.device))
        for w, o in enumerate(refs):
          o.step(a[w])
      if T:
        ring = env.rollout["observation"]["LAYER"]
        assert tuple(ring.shape) == (T, n, 7) + spec["LAYER"].shape
        assert torch.equal(ring[env.slot], ts.observation["LAYER"])
      util.no_faults(env.engine)
    finally:
      env.close()
      for o in refs:
        o.close()


def test_symbolic_only_substrate_beside_pooled_views():
  """A symbolic-only learner (LAYER + scalars, no pixels), and LAYER beside rgb_pool /
  world_rgb_pool as a ring, through edited SubstrateConfigs."""
  from oracle import oracle as oracle_lib
  roles = substrate.get_config("clean_up").default_player_roles
  sym = substrate.get_config("clean_up")
  sym.individual_observation_names = ["LAYER", "READY_TO_SHOOT"]
  sym.global_observation_names = []
  mixed = substrate.get_config("clean_up")
  mixed.individual_observation_names = list(mixed.individual_observation_names) + ["LAYER"]
  pack = engine.load_pack("clean_up")
  n, seed = 16, 77
  oracles = [oracle_lib.Oracle(pack, seed + w, 7) for w in range(n)]
  envs = [substrate.build_from_config(sym, roles=roles, num_worlds=n, env_seed=seed),
          substrate.build_from_config(mixed, roles=roles, num_worlds=n, env_seed=seed, rgb_pool=8,
                                      world_rgb_pool=4, rollout_length=2)]
  try:
    stss = [env.reset() for env in envs]
    for o in oracles:
      o.reset()
    assert set(stss[0].observation) == {"LAYER", "READY_TO_SHOOT", "COLLECTIVE_REWARD"}
    assert envs[1].observation_spec()[0]["LAYER"] == substrate.layer_spec(pack)
    rng = np.random.default_rng(2)
    for s in range(5):
      want = _layers(oracles)
      for env, ts in zip(envs, stss):
        assert np.array_equal(ts.observation["LAYER"].cpu().numpy(), want), s
      world = np.stack([engine.pool_rgb(o.render_world(), 4) for o in oracles])
      assert np.array_equal(stss[1].observation["WORLD.RGB"].cpu().numpy(), world), s
      a = rng.integers(0, 9, size=(n, 7)).astype(np.int32)
      stss = [env.step(torch.from_numpy(a).to("cuda")) for env in envs]
      for w, o in enumerate(oracles):
        o.step(a[w])
    for env in envs:
      util.no_faults(env.engine)
  finally:
    for env in envs:
      env.close()
    for o in oracles:
      o.close()


def test_lab2d_env_n_layer():
  """lab2d_env.Environment(layer=True): "N.LAYER" with the spec (VH, VW, L) int32, equal to the
  oracle's after a reset and steps."""
  from oracle import oracle as oracle_lib
  pack = engine.load_pack("commons_harvest__open")
  roles = substrate.get_config("commons_harvest__open").default_player_roles
  P = len(roles)
  env = lab2d_env.Environment("commons_harvest__open", roles, env_seed=123, layer=True)
  o = oracle_lib.Oracle(pack, 123, P)
  try:
    spec = env.observation_spec()
    for p in range(P):
      assert spec[f"{p + 1}.LAYER"] == substrate.layer_spec(pack).replace(name=f"{p + 1}.LAYER")
    ts = env.reset()
    o.reset()
    for s in range(6):
      assert set(ts.observation) == set(spec)
      for p in range(P):
        assert np.array_equal(ts.observation[f"{p + 1}.LAYER"], o.layer_view(p)), (s, p)
      ts = env.step({"1.move": 1 + s % 4, "2.turn": 1})
      fields = np.zeros((P, len(env._names)), np.int32)
      for p in range(P):
        for a, (n, (lo, hi, default)) in enumerate(zip(env._names, env._ranges)):
          fields[p, a] = default
      fields[0, env._names.index("move")] = 1 + s % 4
      fields[1, env._names.index("turn")] = 1
      o.step_fields(fields)
  finally:
    env.close()
    o.close()
