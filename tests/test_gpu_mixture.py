"""`substrate.build_mixture` on the HIP engine: several layouts of one level as ONE batched
substrate whose members write slices of shared leaves.

Every check holds the mixture against what a user gets without it — one `Substrate` per member,
built with the member's world offset and the same env_seed, stepped with the same actions — and
against the CPU oracle replayed under a world's global seed."""
import numpy as np
import pytest

from meltingpot_amd import engine as E, substrate

pytestmark = pytest.mark.gpu

KITCHENS = tuple(f"collaborative_cooking__{k}" for k in ("asymmetric", "circuit", "cramped", "forced", "ring"))
UNEVEN = [16, 32, 48, 16, 64]
MATRIX = ("prisoners_dilemma_in_the_matrix__repeated", "chicken_in_the_matrix__repeated",
          "stag_hunt_in_the_matrix__repeated")


def _separate(mix, seed, **kw):
  """One Substrate per member: the worlds of member i, created at its offset in the mixture."""
  return [substrate.build(name, roles=("default",) * mix.num_players,
                          num_worlds=mix.member_slice(i).stop - mix.member_slice(i).start,
                          world_offset=mix.member_slice(i).start, env_seed=seed, **kw)
          for i, name in enumerate(mix.members)]


def _leaves(ts):
  out = {"#step_type": ts.step_type, "#reward": ts.reward, "#discount": ts.discount}
  out.update(ts.observation)
  return out


def _assert_same(mix, ts, separate, tss, where):
  got = _leaves(ts)
  for i, (sub, one) in enumerate(zip(separate, tss)):
    sl = mix.member_slice(i)
    want = _leaves(one)
    assert set(want) == set(got)
    for n, v in want.items():
      assert v.shape == got[n][sl].shape, (where, i, n)
      assert bool((got[n][sl] == v).all()), (where, mix.members[i], n)
    assert bool((mix.engines[i].observe(E.OBS_EVENTS) == sub.engine.observe(E.OBS_EVENTS)).all()), (where, i)


def _counters_match(mix, separate):
  total = {}
  for i, sub in enumerate(separate):
    c = sub.engine.counters()
    assert mix.engines[i].counters() == c, mix.members[i]
    for k, v in c.items():
      total[k] = total.get(k, 0) + v
  assert mix.counters() == total


@pytest.mark.parametrize("pool", [1, 8])
def test_equivalence_with_separate_substrates(pool):
  import torch
  kw = {"rgb_pool": pool, "world_rgb_pool": pool}
  mix = substrate.build_mixture(KITCHENS, num_worlds=UNEVEN, env_seed=77, **kw)
  assert mix.num_worlds == 176 and [mix.member_slice(i).start for i in range(5)] == [0, 16, 48, 96, 112]
  separate = _separate(mix, 77, **kw)
  if pool == 8:
    assert mix.observation_spec()[0]["RGB"].shape == (5, 5, 3)
    assert mix.observation_spec()[0]["WORLD.RGB"].shape == (5, 9, 3)
  ts, tss = mix.reset(), [s.reset() for s in separate]
  _assert_same(mix, ts, separate, tss, "reset")
  gen = torch.Generator(device="cuda").manual_seed(pool)
  for step in range(400):
    a = torch.randint(0, 8, (176, 2), dtype=torch.int32, device="cuda", generator=gen)
    ts = mix.step(a)
    tss = [s.step(a[mix.member_slice(i)]) for i, s in enumerate(separate)]
    _assert_same(mix, ts, separate, tss, step)
  torch.cuda.synchronize()
  _counters_match(mix, separate)
  assert int(mix.counters()["world_steps"]) == 176 * 400
  for i, eng in enumerate(mix.engines):
    assert not eng.fault_words()[:6].any(), mix.members[i]
  mix.close()
  for s in separate:
    s.close()


def test_oracle_parity_at_global_seeds():
  """Sampled worlds of every member replayed by the oracle, seeded as the mixture seeds them:
  env_seed + world_offset + g (the Substrate API's seeds; tests/util.py's replay harness
  replays the engine's default seeds, so the replay is done here)."""
  import torch
  from oracle import oracle
  seed, offset, steps = 1000, 5, 200
  mix = substrate.build_mixture(KITCHENS, num_worlds=UNEVEN, env_seed=seed, world_offset=offset)
  rng = np.random.default_rng(3)
  acts = rng.integers(0, 8, size=(steps, mix.num_worlds, 2), dtype=np.int32)
  dacts = torch.from_numpy(acts).cuda()
  ts = mix.reset()
  for s in range(steps):
    ts = mix.step(dacts[s])
  torch.cuda.synchronize()
  rgb, world = ts.observation["RGB"].cpu().numpy(), ts.observation["WORLD.RGB"].cpu().numpy()
  reward = ts.reward.cpu().numpy()
  checked = 0
  for i, name in enumerate(mix.members):
    sl = mix.member_slice(i)
    pack = E.load_pack(name)
    grid, avat, glob = mix.engines[i].dump()
    ev = mix.engines[i].observe(E.OBS_EVENTS).cpu().numpy()
    for g in (sl.start, sl.start + 7, sl.stop - 1):
      w = g - sl.start
      o = oracle.Oracle(pack, seed + offset + g, 2)
      o.reset()
      for s in range(steps):
        o.step(acts[s, g])
      og, oa, ogl = o.dump()
      assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), (name, g)
      assert np.array_equal(glob[w], ogl), (name, g)
      assert np.array_equal(reward[g], o.rewards()), (name, g)
      got = sorted(tuple(int(v) for v in r[:3]) for r in ev[w, 1:1 + int(ev[w, 0, 0])])
      assert got == sorted(tuple(int(v) for v in e) for e in o.events()), (name, g)
      assert np.array_equal(world[g], o.render_world()), (name, g)
      for p in range(2):
        assert np.array_equal(rgb[g, p], o.render_agent(p)), (name, g, p)
      o.close()
      checked += 1
  assert checked == 15
  mix.close()


@pytest.mark.parametrize("auto_reset", [True, False])
def test_episode_ends(auto_reset):
  """The matrix games' episodes end at random after frame 1000: step types, discounts and the
  FIRST observations of the restarted worlds match the separate substrates'."""
  import torch
  mix = substrate.build_mixture(MATRIX, num_worlds=[32, 64, 32], env_seed=4, auto_reset=auto_reset)
  separate = _separate(mix, 4, auto_reset=auto_reset)
  ts, tss = mix.reset(), [s.reset() for s in separate]
  gen = torch.Generator(device="cuda").manual_seed(11)
  lasts = firsts = 0
  for step in range(1500):
    if not auto_reset and step == 1450:
      ts, tss = mix.reset(), [s.reset() for s in separate]
    else:
      a = torch.randint(0, 8, (128, 2), dtype=torch.int32, device="cuda", generator=gen)
      ts = mix.step(a)
      tss = [s.step(a[mix.member_slice(i)]) for i, s in enumerate(separate)]
    _assert_same(mix, ts, separate, tss, step)
    if step > 0:
      lasts += int((ts.step_type == 2).sum())
      firsts += int((ts.step_type == 0).sum())
  # (one chance in ten per 100 steps after frame 1000: about 50 of the 128 worlds end)
  assert lasts >= 8, lasts
  assert firsts >= (8 if auto_reset else 128), firsts
  _counters_match(mix, separate)
  mix.close()
  for s in separate:
    s.close()


@pytest.mark.parametrize("pool", [1, 8])
def test_rings_wrap_and_pad(pool):
  import torch
  kw = {"rgb_pool": pool, "world_rgb_pool": pool, "rollout_length": 32}
  mix = substrate.build_mixture(KITCHENS, num_worlds=UNEVEN, env_seed=21, **kw)
  separate = _separate(mix, 21, **kw)
  ring = mix.rollout
  leaves = {"step_type": ring["step_type"], "reward": ring["reward"], "discount": ring["discount"],
            **ring["observation"]}
  padded = [n for n, v in leaves.items()
            if v.stride(0) != int(np.prod(v.shape[1:]))]
  # 176 worlds: an 8-byte discount is 1408 B a slot, the slot 1536 B apart
  assert "discount" in padded and "step_type" in padded, padded
  for n, v in leaves.items():
    assert (v.stride(0) * v.element_size()) % 256 == 0 and tuple(v[0].shape)[0] == 176, n
  kept, kept_sep = [mix.reset()], [[s.reset() for s in separate]]
  gen = torch.Generator(device="cuda").manual_seed(5)
  for step in range(40):
    a = torch.randint(0, 8, (176, 2), dtype=torch.int32, device="cuda", generator=gen)
    kept.append(mix.step(a))
    kept_sep.append([s.step(a[mix.member_slice(i)]) for i, s in enumerate(separate)])
  assert [t.slot for t in kept] == [s % 32 for s in range(41)]
  # the last 32 timesteps handed out, untouched, slot by slot
  for ts, tss in zip(kept[-32:], kept_sep[-32:]):
    assert all(one.slot == ts.slot for one in tss)
    _assert_leaves_only(mix, ts, tss)
  # and the whole rings
  for i, s in enumerate(separate):
    sl = mix.member_slice(i)
    theirs = s.rollout
    assert bool((ring["step_type"][:, sl] == theirs["step_type"]).all())
    assert bool((ring["reward"][:, sl] == theirs["reward"]).all())
    assert bool((ring["discount"][:, sl] == theirs["discount"]).all())
    for n in ring["observation"]:
      assert bool((ring["observation"][n][:, sl] == theirs["observation"][n]).all()), (i, n)
  mix.close()
  for s in separate:
    s.close()


def _assert_leaves_only(mix, ts, tss):
  got = _leaves(ts)
  for i, one in enumerate(tss):
    sl = mix.member_slice(i)
    for n, v in _leaves(one).items():
      assert bool((got[n][sl] == v).all()), (ts.slot, mix.members[i], n)


def test_4096_worlds_tuned_members_against_sampled_worlds():
  """The five kitchens at 4096 worlds (every member's plan tuned to its slices by mp_tune); a
  block of worlds of each member against a Substrate built for that block alone, at its
  global world offset."""
  import torch
  mix = substrate.build_mixture(KITCHENS, num_worlds=4096, env_seed=8)
  assert mix.num_worlds == 4096
  assert [mix.member_slice(i).stop - mix.member_slice(i).start for i in range(5)] == [820, 819, 819, 819, 819]
  blocks = []
  for i in range(5):
    sl = mix.member_slice(i)
    g0 = sl.start + (sl.stop - sl.start) // 2 - 4
    blocks.append((g0, substrate.build(mix.members[i], roles=("default",) * 2, num_worlds=8,
                                       world_offset=g0, env_seed=8)))
  ts = mix.reset()
  tbs = [b.reset() for _, b in blocks]
  gen = torch.Generator(device="cuda").manual_seed(2)
  for step in range(64):
    a = torch.randint(0, 8, (4096, 2), dtype=torch.int32, device="cuda", generator=gen)
    ts = mix.step(a)
    tbs = [b.step(a[g0:g0 + 8]) for g0, b in blocks]
  got = _leaves(ts)
  for (g0, b), tb in zip(blocks, tbs):
    for n, v in _leaves(tb).items():
      assert bool((got[n][g0:g0 + 8] == v).all()), (g0, n)
  assert mix.counters()["world_steps"] == 4096 * 64
  for eng in mix.engines:
    assert not eng.fault_words()[:6].any()
  mix.close()
  for _, b in blocks:
    b.close()
