"""`substrate.build_mixture`: several layouts of one level stepped as one batched Substrate.

CPU: the compatibility rules and refusals, the world granule, the layout of the members' worlds,
and — with the oracle standing in for every member's engine (`oracle_engine.OracleBatchEngine`,
as tests/test_every_substrate.py injects it) — the seeding contract: mixture world g is world 0
of a one-world Substrate of its member's name built with world_offset = g and the same env_seed.
The GPU side is tests/test_gpu_mixture.py."""
import numpy as np
import pytest

import util  # noqa: F401
from meltingpot_amd import engine as E, lower, pack as pack_lib, substrate

KITCHENS = tuple(f"collaborative_cooking__{k}" for k in ("asymmetric", "circuit", "cramped", "forced", "ring"))


@pytest.fixture
def oracle_engine(monkeypatch):
  from oracle_engine import OracleBatchEngine, OracleEngine

  def events(self, world=0):
    # (one world's events through the one-world stand-in, which decodes them with the product's
    # own `Engine._decode_events`: the real class, not the patched name)
    single = OracleEngine.__new__(OracleEngine)
    single._o, single.pack_bytes = self._o[world], self.pack_bytes
    return OracleEngine.events(single, 0)

  monkeypatch.setattr(OracleBatchEngine, "events", events)
  monkeypatch.setattr(OracleBatchEngine, "_decode_events", staticmethod(E.Engine._decode_events),
                      raising=False)
  monkeypatch.setattr(substrate.engine_lib, "Engine", OracleBatchEngine)


# -- compatibility and refusals ------------------------------------------------------------

def test_the_five_kitchens_mix(oracle_engine):
  with substrate.build_mixture(KITCHENS, num_worlds=10, env_seed=1) as mix:
    assert mix.members == KITCHENS
    assert mix.num_worlds == 10 and mix.num_players == 2
    spec = mix.observation_spec()
    assert len(spec) == 2
    assert spec[0]["RGB"].shape == (40, 40, 3) and spec[0]["WORLD.RGB"].shape == (40, 72, 3)
    assert set(spec[0]) == {"RGB", "WORLD.RGB", "COLLECTIVE_REWARD"}
    assert mix.action_spec()[0].num_values == 8
    ts = mix.reset()
    assert tuple(ts.observation["RGB"].shape) == (10, 2, 40, 40, 3)
    assert tuple(ts.observation["WORLD.RGB"].shape) == (10, 40, 72, 3)
    assert tuple(ts.reward.shape) == (10, 2) and tuple(ts.discount.shape) == (10,)
    assert ts.step_type.tolist() == [0] * 10
    ts = mix.step(np.zeros((10, 2), np.int64))
    assert ts.step_type.tolist() == [1] * 10


def test_player_counts_must_agree():
  with pytest.raises(ValueError, match="same number of players"):
    substrate.build_mixture(["collaborative_cooking__crowded", "collaborative_cooking__ring"],
                            num_worlds=4)


def test_a_differing_world_view_is_refused_by_name_and_can_be_dropped(oracle_engine):
  names = ["territory__rooms", "territory__open"]
  with pytest.raises(ValueError) as e:
    substrate.build_mixture(names, num_worlds=2)
  msg = str(e.value)
  assert "'WORLD.RGB'" in msg and "territory__rooms" in msg and "territory__open" in msg
  assert "(168, 168, 3)" in msg and "(184, 312, 3)" in msg
  assert "global_observations=()" in msg
  with substrate.build_mixture(names, num_worlds=2, global_observations=(), env_seed=3) as mix:
    assert "WORLD.RGB" not in mix.observation_spec()[0]
    ts = mix.reset()
    assert set(ts.observation) == {"RGB", "READY_TO_SHOOT", "COLLECTIVE_REWARD"}
    assert tuple(ts.observation["RGB"].shape) == (2, 9, 88, 88, 3)


def test_matrix_games_with_the_same_resources_mix(oracle_engine):
  names = ["prisoners_dilemma_in_the_matrix__repeated", "stag_hunt_in_the_matrix__repeated",
           "chicken_in_the_matrix__repeated"]
  with substrate.build_mixture(names, num_worlds=[1, 2, 1], env_seed=9) as mix:
    ts = mix.reset()
    assert tuple(ts.observation["INVENTORY"].shape) == (4, 2, 2)
    assert tuple(ts.observation["INTERACTION_INVENTORIES"].shape) == (4, 2, 2, 2)
    mix.step(np.ones((4, 2), np.int64))


def test_matrix_games_with_other_resources_are_refused_and_narrowed(oracle_engine):
  names = ["prisoners_dilemma_in_the_matrix__repeated", "running_with_scissors_in_the_matrix__repeated"]
  with pytest.raises(ValueError) as e:
    substrate.build_mixture(names, num_worlds=2)
  msg = str(e.value)
  assert "'INVENTORY'" in msg and "'INTERACTION_INVENTORIES'" in msg
  assert names[0] in msg and names[1] in msg and "individual_observations=[...]" in msg
  # WORLD.RGB is the same map: only the inventories differ
  with substrate.build_mixture(names, num_worlds=2, env_seed=1,
                               individual_observations=["RGB", "READY_TO_SHOOT"]) as mix:
    assert set(mix.observation_spec()[0]) == {"RGB", "READY_TO_SHOOT", "WORLD.RGB", "COLLECTIVE_REWARD"}


def test_action_counts_must_agree():
  # coins (7 actions) and a kitchen (8): both 2 players
  with pytest.raises(ValueError, match="action_spec"):
    substrate.build_mixture(["coins", "collaborative_cooking__ring"], num_worlds=2,
                            individual_observations=["RGB"], global_observations=())


def test_roles_must_be_valid_for_every_member():
  names = ["bach_or_stravinsky_in_the_matrix__repeated", "prisoners_dilemma_in_the_matrix__repeated"]
  with pytest.raises(ValueError, match="Invalid roles for prisoners_dilemma"):
    substrate.build_mixture(names, roles=("bach_fan", "stravinsky_fan"), num_worlds=2)


@pytest.mark.parametrize("kwargs, what", [
    ({"names": ["collaborative_cooking__ring", "no_such_substrate"], "num_worlds": 2}, "no_such_substrate"),
    ({"names": [], "num_worlds": 2}, "at least one"),
    ({"names": list(KITCHENS[:2]), "num_worlds": [4, 0]}, "at least one world"),
    ({"names": list(KITCHENS[:2]), "num_worlds": [4, -1]}, "at least one world"),
    ({"names": list(KITCHENS[:2]), "num_worlds": [4]}, "1 world counts for 2 members"),
    ({"names": list(KITCHENS[:2]), "num_worlds": 0}, "positive"),
    ({"names": [KITCHENS[0]], "num_worlds": 1}, "at least two worlds"),
    ({"names": list(KITCHENS[:2]), "num_worlds": 2, "rgb_pool": 3}, "rgb_pool"),
])
def test_refusals(kwargs, what):
  with pytest.raises(ValueError, match=what):
    substrate.build_mixture(kwargs.pop("names"), **kwargs)


def test_unknown_keyword_arguments_are_refused():
  with pytest.raises(TypeError, match="batched"):
    substrate.build_mixture(KITCHENS, num_worlds=5, batched=False)


# -- the world granule ------------------------------------------------------------------------

def _pixel_bytes(name, rgb_pool, world_rgb_pool):
  """Bytes per world of the two pixel views, from the pack's header (what the engine draws)."""
  pack = E.load_pack(name)
  hdr = pack_lib.loads(pack)["hdr"]
  S = int(hdr[lower.HDR_SPRITE])
  vh = (int(hdr[lower.HDR_VF]) + int(hdr[lower.HDR_VB]) + 1) * S
  vw = (int(hdr[lower.HDR_VL]) + int(hdr[lower.HDR_VR]) + 1) * S
  P = len(substrate.get_config(name).default_player_roles)
  return {"RGB": P * (vh // rgb_pool) * (vw // rgb_pool) * 3,
          "WORLD.RGB": (int(hdr[lower.HDR_H]) * S // world_rgb_pool) * (int(hdr[lower.HDR_W]) * S // world_rgb_pool) * 3}


@pytest.mark.parametrize("name", sorted(substrate.SUBSTRATES))
def test_granule_of_every_pooled_and_full_view(name):
  config = substrate.get_config(name)
  pack = E.load_pack(name)
  P = len(config.default_player_roles)
  for k in (1, 2, 4, 8):
    for kw in (k, 1), (1, k), (k, k):
      bpw = substrate.leaf_bytes_per_world(config, pack, P, *kw)
      want = _pixel_bytes(name, *kw)
      assert {n: bpw[n] for n in want} == want, (name, kw)
      g = substrate.world_granule(bpw)
      # every member offset that is a multiple of g starts both views on 16 bytes ...
      assert all(g * b % 16 == 0 for b in want.values()), (name, kw, g)
      # ... and g is the smallest such count
      assert all(any(h * b % 16 for b in want.values()) for h in range(1, g)), (name, kw, g)
      if kw == (1, 1):
        assert g == 1   # full views are multiples of 192 B a world
      for n in ("#reward", "#discount", "#step_type", "COLLECTIVE_REWARD"):
        assert n in bpw


def test_granule_examples():
  cfg, pack = substrate.get_config("clean_up"), E.load_pack("clean_up")
  bpw = substrate.leaf_bytes_per_world(cfg, pack, 7, rgb_pool=8)
  assert bpw["RGB"] == 2541 and substrate.world_granule(bpw) == 16
  kitchen = substrate.get_config(KITCHENS[0]), E.load_pack(KITCHENS[0])
  bpw = substrate.leaf_bytes_per_world(*kitchen, 2, rgb_pool=8, world_rgb_pool=8)
  assert (bpw["RGB"], bpw["WORLD.RGB"]) == (150, 135)
  assert substrate.world_granule({"RGB": 150}) == 8
  assert substrate.world_granule(bpw) == 16


def test_split_worlds():
  assert substrate.split_worlds(4096, 5, 1) == [820, 819, 819, 819, 819]
  assert substrate.split_worlds(4096, 5, 16) == [832, 816, 816, 816, 816]
  assert substrate.split_worlds(10, 5, 16) == [16] * 5             # one granule each at least
  assert substrate.split_worlds(100, 3, 16) == [48, 32, 32]         # 7 granules: 112
  assert substrate.split_worlds([10, 17, 16], 3, 8) == [16, 24, 16]  # each rounded up
  assert substrate.split_worlds([3, 1], 2, 1) == [3, 1]
  for total in range(1, 200):
    for g in (1, 2, 8, 16):
      counts = substrate.split_worlds(total, 5, g)
      assert all(c % g == 0 and c >= g for c in counts)
      assert max(counts) - min(counts) <= g
      assert sum(counts) >= total and sum(counts) - total < g or sum(counts) == 5 * g


# -- layout and the seeding contract (the oracle stands in for the members' engines) --------

def test_member_layout(oracle_engine):
  counts = [2, 1, 3, 1, 2]
  with substrate.build_mixture(KITCHENS, num_worlds=counts, env_seed=0) as mix:
    assert mix.num_worlds == 9
    assert [mix.member_slice(i) for i in range(5)] == [
        slice(0, 2), slice(2, 3), slice(3, 6), slice(6, 7), slice(7, 9)]
    assert mix.member_of_world.dtype == __import__("torch").int32
    assert mix.member_of_world.tolist() == [0, 0, 1, 2, 2, 2, 3, 4, 4]
    for i, eng in enumerate(mix.engines):
      assert eng.N == counts[i]
    # every member writes its slice of the mixture's own leaves
    ts = mix.reset()
    for i, eng in enumerate(mix.engines):
      sl = mix.member_slice(i)
      assert eng._bound[E.OBS_RGB].data_ptr() == ts.observation["RGB"][sl].data_ptr()
      assert eng._bound[E.OBS_STEP_TYPE].data_ptr() == ts.step_type[sl].data_ptr()


def _one_world_reference(names_of_world, env_seed, world_offset=0):
  return [substrate.build(n, roles=("default",) * 2, world_offset=world_offset + g, env_seed=env_seed)
          for g, n in enumerate(names_of_world)]


def _check_world(ts, g, one):
  """Mixture timestep `ts` at world g against the one-world timestep `one`."""
  assert int(ts.step_type[g]) == int(one.step_type)
  assert float(ts.discount[g]) == float(one.discount)
  assert np.array_equal(ts.reward[g].numpy(), np.asarray(one.reward))
  for p, obs in enumerate(one.observation):
    for n, v in obs.items():
      got = ts.observation[n][g] if n in ("WORLD.RGB", "COLLECTIVE_REWARD") else ts.observation[n][g, p]
      assert np.array_equal(got.numpy(), np.asarray(v)), (g, p, n)


@pytest.mark.parametrize("rollout_length", [0, 8])
def test_world_g_is_the_one_world_substrate_at_offset_g(oracle_engine, rollout_length):
  counts = [2, 1, 2, 1, 1]
  of_world = [KITCHENS[i] for i, c in enumerate(counts) for _ in range(c)]
  seed, offset = 12345, 40
  mix = substrate.build_mixture(KITCHENS, num_worlds=counts, env_seed=seed, world_offset=offset,
                                rollout_length=rollout_length)
  singles = _one_world_reference(of_world, seed, offset)
  rng = np.random.default_rng(7)
  ts, ones = mix.reset(), [s.reset() for s in singles]
  kept = []
  for step in range(50):
    for g, one in enumerate(ones):
      _check_world(ts, g, one)
    if rollout_length:
      kept.append((ts, ones))
    a = rng.integers(0, 8, size=(7, 2))
    ts, ones = mix.step(a), [s.step(a[g]) for g, s in enumerate(singles)]
  if rollout_length:
    # the last T timesteps handed out are still what they were: slots of the ring
    for old, old_ones in kept[-rollout_length + 1:]:
      for g, one in enumerate(old_ones):
        _check_world(old, g, one)
  assert mix.engines[0].N == 2
  mix.close()
  for s in singles:
    s.close()


def test_a_ring_slot_of_seven_worlds_is_padded(oracle_engine):
  # 7 worlds: "#discount" is 56 B a slot, "#step_type" 28 B — padded to 256-byte slots
  with substrate.build_mixture(KITCHENS, num_worlds=[2, 1, 2, 1, 1], env_seed=0,
                               rollout_length=4) as mix:
    ring = mix.rollout
    assert tuple(ring["discount"].shape) == (4, 7) and ring["discount"].stride() == (32, 1)
    assert tuple(ring["step_type"].shape) == (4, 7) and ring["step_type"].stride() == (64, 1)
    rgb = ring["observation"]["RGB"]   # 9600 B a world: 7 x 9600 = 67200 = 262.5 x 256
    assert rgb.stride(0) == 67328 and tuple(rgb.shape) == (4, 7, 2, 40, 40, 3)
    ts = mix.reset()
    assert ts.slot == 0 and tuple(ts.discount.shape) == (7,)
    for s in range(1, 6):
      ts = mix.step(np.zeros((7, 2), np.int64))
      assert ts.slot == s % 4 == mix.slot
      assert ts.step_type.data_ptr() == ring["step_type"][s % 4].data_ptr()


def test_host_and_tensor_actions_and_their_shape(oracle_engine):
  import torch
  with substrate.build_mixture(KITCHENS[:2], num_worlds=[1, 2], env_seed=0) as mix:
    mix.reset()
    mix.step(torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
      mix.step(np.zeros((2, 2), np.int64))


def test_events_and_observables_use_mixture_worlds(oracle_engine):
  with substrate.build_mixture(KITCHENS[:2], num_worlds=[1, 2], env_seed=0) as mix:
    seen = []
    mix.observables().events_batched.subscribe(on_next=seen.append)
    steps = []
    mix.observables().timestep.subscribe(on_next=steps.append)
    mix.reset()
    assert len(steps) == 1
    assert {w for w, _ in seen} <= {0, 1, 2}
    assert mix.events(2) == mix.engines[1].events(1)
    with pytest.raises(IndexError):
      mix.events(3)
    done = []
    mix.observables().timestep.subscribe(on_completed=lambda: done.append(1))
  assert done == [1]


def test_a_custom_action_table_is_shared(oracle_engine):
  table = [{"move": 0, "turn": 0, "interact": 0}, {"move": 1, "turn": 0, "interact": 0}]
  with substrate.build_mixture(KITCHENS[:2], num_worlds=2, env_seed=0, action_table=table) as mix:
    assert mix.action_spec()[0].num_values == 2
    mix.reset()
    mix.step(np.ones((2, 2), np.int64))
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
      mix.step(np.full((2, 2), 2, np.int64))

