"""Pooled per-agent RGB on the GPU (MP_OBS_RGB_POOL2/4/8): drawn by the launch that steps the
worlds, every byte equal to the oracle's full image pooled in numpy (`engine.pool_rgb`) — for
every pack, with WORLD.RGB in the same launch under forced plans, at the benchmarked sizes
against a same-seed engine with the full view, through mp_observe, in a rollout ring and
behind the `Substrate(..., rgb_pool=k)` surface.  No fault word may be set after any of it."""
import os

import numpy as np
import pytest
import torch

import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(engine.__file__), "assets")
PACKS = sorted(f[:-4] for f in os.listdir(ASSETS) if f.endswith(".mpk"))
KS = (2, 4, 8)


def _run_against_oracle(name, n, steps, views, dev=None, seed=0, looks=()):
  """Engines (one per entry of `views`: a tuple of kinds bound together) stepped with the same
  random actions as n oracles; state, rewards and every bound view compared at each step in
  `looks` and at the end."""
  pack = engine.load_pack(name)
  engs = [engine.Engine(pack, n, device=0, dev=dev) for _ in views]
  bufs = [{k: e.bind(k) for k in kinds} for e, kinds in zip(engs, views)]
  oracles = util.make_oracles(pack, n)
  for e in engs:
    e.reset()
  for o in oracles:
    o.reset()
  rng = np.random.default_rng(seed)
  P, nact = engs[0].P, engs[0].num_actions
  acts = rng.integers(0, nact, size=(steps, n, P), dtype=np.int32)
  dacts = torch.from_numpy(acts).to(engs[0].device)
  looks = set(looks) | {steps}
  try:
    for s in range(steps):
      for e in engs:
        e.step(dacts[s])
      for w, o in enumerate(oracles):
        o.step(acts[s, w])
      if s + 1 not in looks:
        continue
      full = {w: np.stack([o.render_agent(p) for p in range(P)]) for w, o in enumerate(oracles)}
      for e, b in zip(engs, bufs):
        grid, avat, glob = e.dump()
        rew = e.observe(engine.OBS_REWARD).cpu().numpy()
        host = {k: t.cpu().numpy() for k, t in b.items()}
        for w, o in enumerate(oracles):
          og, oa, ogl = o.dump()
          assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), (name, s, w)
          assert np.array_equal(glob[w], ogl), (name, s, w)
          assert np.array_equal(rew[w], o.rewards()), (name, s, w)
          for k, v in host.items():
            if k == engine.OBS_WORLD_RGB:
              want = o.render_world()
            else:
              pk = {kk: f for f, kk in engine.OBS_RGB_POOL.items()}[k]
              want = engine.pool_rgb(full[w], pk)
            assert np.array_equal(v[w], want), (name, k, s, w)
        util.no_faults(e)
  finally:
    for o in oracles:
      o.close()
    for e in engs:
      e.close()


@pytest.mark.parametrize("name", PACKS)
def test_every_pack_pooled_alone(name):
  """1.  16 worlds x 40 random steps (beams included), each factor bound alone."""
  _run_against_oracle(name, 16, 40, [(engine.OBS_RGB_POOL[k],) for k in KS], looks=(1, 20))


@pytest.mark.parametrize("name", ["clean_up", "territory__rooms"])
@pytest.mark.parametrize("dev", [
    {"batch_worlds": 1, "ring_batches": 6, "static_pct": 50, "max_groups": 4},
    {"batch_worlds": 3, "ring_batches": 2, "max_groups": 8},
    {"max_groups": 5},
])
def test_pooled_with_world_view_forced_plans(name, dev):
  """2.  A pooled view and WORLD.RGB in ONE launch, several batches per workgroup."""
  views = [(engine.OBS_RGB_POOL[k], engine.OBS_WORLD_RGB) for k in KS]
  _run_against_oracle(name, 96, 8, views, dev=dev, seed=1, looks=(1,))


def _pooled_vs_full(name, n, steps, dev_list):
  pack = engine.load_pack(name)
  full = engine.Engine(pack, n, device=0)
  rgb = full.bind(engine.OBS_RGB)
  full.reset()
  rng = np.random.default_rng(5)
  acts = torch.from_numpy(rng.integers(0, full.num_actions, size=(steps, n, full.P),
                                       dtype=np.int32)).to(full.device)
  want = []
  for s in range(steps):
    full.step(acts[s])
    want.append(engine.pool_rgb(rgb.cpu().numpy(), 8))
  util.no_faults(full)
  full.close()
  del rgb
  torch.cuda.empty_cache()
  for dev, tune in dev_list:
    e = engine.Engine(pack, n, device=0, dev=dev)
    out = e.bind(engine.OBS_RGB_POOL8)
    if tune:
      e.tune()
    e.reset()
    for s in range(steps):
      e.step(acts[s])
      assert np.array_equal(out.cpu().numpy(), want[s]), (name, dev, tune, s)
    util.no_faults(e)
    e.close()


@pytest.mark.parametrize("name,n", [("clean_up", 4096), ("territory__rooms", 8192)])
def test_benchmarked_sizes_pooled_equals_pooled_full(name, n):
  """3.  At the benchmarked sizes, under the stock plan, the plan mp_tune keeps, and the plans
  mp_tune chooses among (single-world ring, half of it pooled, XCD teams, half the feeders,
  sc1 stores)."""
  dev_list = [(None, False), (None, True),
              ({"batch_worlds": 1, "ring_batches": 16}, False),
              ({"batch_worlds": 1, "ring_batches": 16, "static_pct": 50}, False),
              ({"batch_worlds": 1, "ring_batches": 16, "team": 1}, False),
              ({"feeders": 4}, False),
              ({"store_sc1": 1}, False)]
  _pooled_vs_full(name, n, 3, dev_list)


@pytest.mark.parametrize("name", ["clean_up", "coins", "collaborative_cooking__cramped",
                                  "prisoners_dilemma_in_the_matrix__repeated"])
def test_observe_pooled_without_a_bound_view(name):
  """4.  mp_observe draws every pooled kind from the records (the render-only kernel)."""
  pack = engine.load_pack(name)
  n, steps = 12, 15
  e = engine.Engine(pack, n, device=0)
  oracles = util.make_oracles(pack, n)
  e.reset()
  for o in oracles:
    o.reset()
  rng = np.random.default_rng(7)
  acts = rng.integers(0, e.num_actions, size=(steps, n, e.P), dtype=np.int32)
  for s in range(steps):
    e.step(torch.from_numpy(acts[s]).to(e.device))
    for w, o in enumerate(oracles):
      o.step(acts[s, w])
  full = np.stack([np.stack([o.render_agent(p) for p in range(e.P)]) for o in oracles])
  for k in KS:
    got = e.observe(engine.OBS_RGB_POOL[k]).cpu().numpy()
    assert np.array_equal(got, engine.pool_rgb(full, k)), (name, k)
  assert np.array_equal(e.observe(engine.OBS_RGB).cpu().numpy(), full)
  util.no_faults(e)
  for o in oracles:
    o.close()
  e.close()


def test_binding_two_agent_views_is_refused():
  e = engine.Engine(engine.load_pack("clean_up"), 4, device=0)
  e.bind(engine.OBS_RGB_POOL8)
  with pytest.raises(ValueError, match="one per-agent view"):
    e.bind(engine.OBS_RGB)
  with pytest.raises(ValueError, match="one per-agent view"):
    e.bind(engine.OBS_RGB_POOL4)
  e.unbind(engine.OBS_RGB_POOL8)
  e.bind(engine.OBS_RGB_POOL4)
  e.close()


def test_rollout_ring_pooled():
  """5.  rollout_length=T with rgb_pool=8: slot t holds what the unringed run shows at step t."""
  T, n, steps = 4, 8, 6
  roles = ("default",) * 7
  a = substrate.build("clean_up", roles=roles, num_worlds=n, rgb_pool=8, rollout_length=T, env_seed=11)
  b = substrate.build("clean_up", roles=roles, num_worlds=n, rgb_pool=8, env_seed=11)
  rng = np.random.default_rng(2)
  a.reset()
  ts = b.reset()
  seen = [ts.observation["RGB"].clone()]
  for s in range(steps):
    act = torch.from_numpy(rng.integers(0, 9, size=(n, 7), dtype=np.int32)).cuda()
    a.step(act)
    seen.append(b.step(act).observation["RGB"].clone())
  ring = a.rollout["observation"]["RGB"]
  for t in range(steps + 1 - T, steps + 1):
    assert np.array_equal(ring[t % T].cpu().numpy(), seen[t].cpu().numpy()), t
  util.no_faults(a.engine)
  util.no_faults(b.engine)
  a.close()
  b.close()


def test_api_shape_and_spec():
  """6.  The drop-in surface."""
  env = substrate.build("clean_up", roles=("default",) * 7, num_worlds=64, rgb_pool=8)
  ts = env.reset()
  rgb = ts.observation["RGB"]
  assert tuple(rgb.shape) == (64, 7, 11, 11, 3)
  spec = env.observation_spec()[0]["RGB"]
  assert spec.shape == (11, 11, 3) and spec.dtype == np.uint8
  assert "WORLD.RGB" in ts.observation
  util.no_faults(env.engine)
  env.close()


def _assert_step_matches_specs(env):
  env.reset()
  action = [int(spec.maximum) for spec in env.action_spec()]
  timestep = env.step(action)
  observation_specs = env.observation_spec()
  assert len(observation_specs) == len(timestep.observation)
  for observation, spec in zip(timestep.observation, observation_specs):
    assert set(spec) == set(observation)
    for key in spec:
      spec[key].validate(observation[key])


@pytest.mark.parametrize("name", sorted(substrate.SUBSTRATES))
def test_conformance_with_rgb_pool(name):
  """6.  The per-substrate conformance check, with rgb_pool=8."""
  factory = substrate.get_factory(name)
  with factory.build(factory.default_player_roles(), rgb_pool=8) as env:
    _assert_step_matches_specs(env)
    rgb = env.observation_spec()[0]["RGB"]
    full = factory.timestep_spec().observation["RGB"]
    assert rgb.shape == (full.shape[0] // 8, full.shape[1] // 8, 3)
    util.no_faults(env.engine)


def test_switching_the_agent_view_beside_a_tuned_ring():
  """A ring of WORLD.RGB tuned with the full RGB bound, then the full view swapped for a pooled
  one (and back): the ring's plans were made for the other LDS layout and are dropped; both views
  stay exact."""
  name, n, steps = "clean_up", 64, 4
  pack = engine.load_pack(name)
  e = engine.Engine(pack, n, device=0)
  ring = e.bind_ring(engine.OBS_WORLD_RGB, slots=2, tune=False)
  e.bind(engine.OBS_RGB)
  e.tune()
  e.unbind(engine.OBS_RGB)
  pooled = e.bind(engine.OBS_RGB_POOL8)
  oracles = util.make_oracles(pack, n)
  e.reset()
  for o in oracles:
    o.reset()
  rng = np.random.default_rng(9)
  acts = rng.integers(0, e.num_actions, size=(steps, n, e.P), dtype=np.int32)
  for s in range(steps):
    e.step(torch.from_numpy(acts[s]).to(e.device))
    for w, o in enumerate(oracles):
      o.step(acts[s, w])
  got, world = pooled.cpu().numpy(), ring[e.ring["last"]].cpu().numpy()
  for w, o in enumerate(oracles):
    full = np.stack([o.render_agent(p) for p in range(e.P)])
    assert np.array_equal(got[w], engine.pool_rgb(full, 8)), w
    assert np.array_equal(world[w], o.render_world()), w
  util.no_faults(e)
  e.unbind(engine.OBS_RGB_POOL8)
  rgb = e.bind(engine.OBS_RGB)
  e.step(torch.from_numpy(acts[0]).to(e.device))
  for w, o in enumerate(oracles):
    o.step(acts[0, w])
  got = rgb.cpu().numpy()
  for w, o in enumerate(oracles):
    assert np.array_equal(got[w], np.stack([o.render_agent(p) for p in range(e.P)])), w
  util.no_faults(e)
  for o in oracles:
    o.close()
  e.close()
