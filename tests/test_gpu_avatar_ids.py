"""AVATAR_IDS_IN_VIEW and AVATAR_IDS_IN_RANGE_TO_ZAP on the GPU (MpAvatarIds;
Engine.observe_avatar_ids / bind_avatar_ids, Substrate's named leaves, observe_avatar_ids and
observe_states, MixtureSubstrate's): both kernels byte for byte against the library's host twin
(which tests/test_avatar_ids_cpu.py holds to the numpy model) on rows of random play with beams
and on the hand-placed rows of tests/avatar_ids_rows.py; waves that take several elements in turn;
indices out of range; the registered leaves behind every kind of submission, with and without a
rollout ring, and in a mixture; and IN_RANGE held to the engine's own beam: on a pack whose beam
blockers all live on the avatars' layer, the targets of a zap fired now are exactly IN_RANGE's."""
import functools

import numpy as np
import pytest
import torch

import avatar_ids_rows as HR
import situations
import states_recipe as R
import util
from meltingpot_amd import engine, substrate
from meltingpot_amd import pack as pack_lib

pytestmark = pytest.mark.gpu

E = engine
N = 64
SEED = 5
FILL = 0x5A5A5A5A
VIEW, ZAP = substrate.AVATAR_IDS_NAMES
PLAYERS = {"clean_up": 7, "commons_harvest__open": 16, "territory__rooms": 9, "externality_mushrooms__dense": 5}


def _same(got, want, what):
  got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
  want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
  assert got.shape == want.shape and got.dtype == want.dtype == np.int32, (what, got.shape, want.shape)
  assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def _filled(eng, *shape):
  return torch.full(shape, FILL, dtype=torch.int32, device=eng.device)


def _actions(rng, eng, *shape):
  w = np.ones(eng.num_actions)
  w[min(7, eng.num_actions - 1)] = 4   # (the beam, four times as likely as another action)
  a = util.random_actions(rng, 1, int(np.prod(shape)), eng.P, eng.num_actions, w)
  return torch.from_numpy(a.reshape(shape + (eng.P,))).to(eng.device)


@functools.lru_cache(maxsize=None)
def case(name):
  """(bank uint8 [R, S] on the device, the host twin's (in_view, in_range) of it, the index of the
  first hand-placed row): 64 worlds after every 10th of 200 random steps with beams, then the
  hand-placed rows.  Computed once and shared; treat it as read-only."""
  pack = R.pack(name)
  eng = E.Engine(pack, N, device=0)
  assert eng.P == PLAYERS[name]
  eng.reset()
  res = eng.step_many(_actions(np.random.default_rng(SEED), eng, 200, N), states=True)
  played = res["states"][9::10].reshape(-1, eng.info.world_state_bytes)
  assert played.shape[0] == 20 * N
  hand = torch.from_numpy(HR.hand_rows(name)[0]).to(eng.device)
  bank = torch.cat([played, hand]).contiguous()
  eng.sync()
  util.no_faults(eng)
  eng.close()
  host = E.avatar_ids_host(pack, bank.cpu().numpy())
  alive = substrate.StateFields(played.cpu(), substrate.SubstrateStateLayout(E.state_layout(pack), pack_lib.loads(pack))).alive
  if name != "territory__rooms":   # (zapped and respawning avatars occur, and somebody is in range)
    assert bool((alive == 0).any()) and host[1][:20 * N].any()
  return bank, host, 20 * N


# ---- 1. both kernels against the host twin -----------------------------------------------------------
@pytest.mark.parametrize("name", HR.LEVELS)
def test_both_kernels_equal_the_host_twin(name):
  bank, (want_v, want_z), _ = case(name)
  eng = E.Engine(R.pack(name), 4, device=0)
  R_, P = bank.shape[0], eng.P
  rows = torch.arange(R_, dtype=torch.int32, device=eng.device).repeat_interleave(P)
  players = torch.arange(P, dtype=torch.int32, device=eng.device).repeat(R_)
  for view, zap in ((True, True), (True, False), (False, True)):
    # the rows kernel, into tensors prefilled with something that is neither 0 nor 1
    out = (_filled(eng, R_, P, P) if view else None, _filled(eng, R_, P, P) if zap else None)
    got = eng.observe_avatar_ids(bank, view=view, zap=zap, out=out)
    assert (got[0] is out[0]) and (got[1] is out[1])
    if view:
      _same(got[0], want_v, (name, "rows kernel, IN_VIEW", view, zap))
    if zap:
      _same(got[1], want_z, (name, "rows kernel, IN_RANGE", view, zap))
    # the views kernel over every (row, player)
    out = (_filled(eng, R_ * P, P) if view else None, _filled(eng, R_ * P, P) if zap else None)
    got = eng.observe_avatar_ids(bank, rows=rows, players=players, view=view, zap=zap, out=out)
    if view:
      _same(got[0], want_v.reshape(R_ * P, P), (name, "views kernel, IN_VIEW", view, zap))
    if zap:
      _same(got[1], want_z.reshape(R_ * P, P), (name, "views kernel, IN_RANGE", view, zap))
  # rows and (row, player) pairs with repeats, out of order
  rng = np.random.default_rng(SEED)
  r = rng.integers(0, R_, size=300).astype(np.int32)
  p = rng.integers(0, P, size=300).astype(np.int32)
  r[1], p[1] = r[0], p[0]
  got = eng.observe_avatar_ids(bank, rows=r)
  _same(got[0], want_v[r], (name, "repeated rows")); _same(got[1], want_z[r], (name, "repeated rows, zap"))
  got = eng.observe_avatar_ids(bank, rows=r, players=p)
  _same(got[0], want_v[r, p], (name, "sampled views")); _same(got[1], want_z[r, p], (name, "sampled views, zap"))
  eng.sync()
  util.no_faults(eng)
  eng.close()


def test_waves_that_take_several_elements_in_turn():
  """20000 repeated rows of commons_harvest__open (P * nc = 144 > 64: three rounds a row): every
  wave takes many elements, and a [P][P] block left in its LDS by the element before would show."""
  name = "commons_harvest__open"
  bank, (want_v, want_z), _ = case(name)
  eng = E.Engine(R.pack(name), 4, device=0)
  P = eng.P
  r = np.random.default_rng(SEED + 1).integers(0, bank.shape[0], size=20000).astype(np.int32)
  # (neighbours in the list differ: a busy row next to an empty one)
  busy = np.argsort(want_z.sum(axis=(1, 2)))
  r[0:2000:2], r[1:2000:2] = busy[-1000:], busy[:1000]
  out = (_filled(eng, r.size, P, P), _filled(eng, r.size, P, P))
  eng.observe_avatar_ids(bank, rows=r, out=out)
  _same(out[0], want_v[r], "IN_VIEW"); _same(out[1], want_z[r], "IN_RANGE")
  assert want_z[r[0]].sum() > 0 and want_z[r[1]].sum() == 0
  p = np.random.default_rng(SEED + 2).integers(0, P, size=r.size).astype(np.int32)
  out = (_filled(eng, r.size, P), _filled(eng, r.size, P))
  eng.observe_avatar_ids(bank, rows=r, players=p, out=out)
  _same(out[0], want_v[r, p], "IN_VIEW, views"); _same(out[1], want_z[r, p], "IN_RANGE, views")
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 2. bad indices, refusals ------------------------------------------------------------------------
def test_an_index_out_of_range_is_skipped_and_reported():
  bank, (want_v, want_z), _ = case("clean_up")
  eng = E.Engine(R.pack("clean_up"), 6, device=0)
  eng.reset()
  P, M = eng.P, bank.shape[0]
  out = (_filled(eng, 5, P, P), _filled(eng, 5, P, P))
  eng.observe_avatar_ids(bank, rows=[1, M, 0, -1, M + 40], out=out)
  with pytest.raises(ValueError, match=rf"MpAvatarIds: rows\[(1\] = {M}|3\] = -1|4\] = {M + 40}) is not a row"):
    eng.sync()
  for got, want in zip(out, (want_v, want_z)):
    got = got.cpu().numpy()
    assert np.array_equal(got[0], want[1]) and np.array_equal(got[2], want[0]) and (got[[1, 3, 4]] == FILL).all()
  out = (_filled(eng, 4, P), _filled(eng, 4, P))
  eng.observe_avatar_ids(bank, rows=[2, 2, 5, 1], players=[0, P, 6, -1], out=out)
  with pytest.raises(ValueError, match=rf"MpAvatarIds: players\[(1\] = {P}|3\] = -1) is not a player"):
    eng.sync()
  for got, want in zip(out, (want_v, want_z)):
    got = got.cpu().numpy()
    assert np.array_equal(got[0], want[2, 0]) and np.array_equal(got[2], want[5, 6]) and (got[[1, 3]] == FILL).all()
  # the live worlds: a world index out of range
  live = E.avatar_ids_host(eng.pack_bytes, eng.save_worlds().cpu().numpy())
  out = (_filled(eng, 2, P, P), _filled(eng, 2, P, P))
  eng.observe_avatar_ids(None, rows=[6 + 3, 4], out=out)
  with pytest.raises(ValueError, match=r"MpAvatarIds: rows\[0\] = 9"):
    eng.sync()
  for got, want in zip(out, live):
    got = got.cpu().numpy()
    assert (got[0] == FILL).all() and np.array_equal(got[1], want[4])
  # host-side refusals launch nothing, and the engine stays usable
  with pytest.raises(ValueError, match="neither view nor zap"):
    eng.observe_avatar_ids(bank, view=False, zap=False)
  with pytest.raises(ValueError, match="fingerprint"):
    eng.observe_avatar_ids(bank, fingerprint=1)
  with pytest.raises(ValueError, match="without a row list"):
    eng.observe_avatar_ids(bank[:2], players=[0, 0, 0])
  with pytest.raises(ValueError, match="out must be a contiguous int32 tensor"):
    eng.observe_avatar_ids(bank, out=(torch.zeros((M, P, P), dtype=torch.int64, device=eng.device), None))
  good = _filled(eng, M, P, P)
  req = dict(fingerprint=eng.state_fingerprint, bank=bank.data_ptr(), bank_rows=M, count=M, dst=good.data_ptr(),
             dst_bytes=good.numel() * 4)
  with pytest.raises(ValueError, match="NULL dst and NULL dst_zap"):
    E.avatar_ids_request(eng._L, eng._h, E.MP_AVATARIDS_DRAW, **dict(req, dst=None))
  with pytest.raises(ValueError, match=rf"need {good.numel() * 4} bytes, dst has {good.numel() * 4 - 1}"):
    E.avatar_ids_request(eng._L, eng._h, E.MP_AVATARIDS_DRAW, **dict(req, dst_zap=good.data_ptr(),
                                                                       dst_zap_bytes=good.numel() * 4 - 1))
  with pytest.raises(ValueError, match="4-byte aligned"):
    E.avatar_ids_request(eng._L, eng._h, E.MP_AVATARIDS_DRAW, **dict(req, dst=good.data_ptr() + 2))
  with pytest.raises(ValueError, match="device"):
    E.avatar_ids_request(eng._L, eng._h, E.MP_AVATARIDS_REGISTER, dst_zap=good.cpu().numpy().ctypes.data,
                         dst_zap_bytes=6 * P * P * 4)
  assert bool((good == FILL).all())
  fresh = E.Engine(R.pack("clean_up"), 2, device=0)
  with pytest.raises(ValueError, match="never been reset"):
    fresh.observe_avatar_ids()
  fresh.close()
  eng.step(torch.zeros((6, P), dtype=torch.int32, device=eng.device))
  now = E.avatar_ids_host(eng.pack_bytes, eng.save_worlds().cpu().numpy())
  got = eng.observe_avatar_ids()
  _same(got[0], now[0], "after the reports"); _same(got[1], now[1], "after the reports, zap")
  eng.sync()
  util.no_faults(eng)
  eng.close()


@pytest.mark.parametrize("name", ["coins", "collaborative_cooking__cramped"])
def test_a_level_without_a_zapper(name):
  cfg = substrate.get_config(name)
  env = substrate.build_from_config(cfg, roles=cfg.default_player_roles, num_worlds=6, env_seed=SEED)
  eng = env.engine
  env.reset()
  A = _actions(np.random.default_rng(SEED), eng, 6, 6)
  for k in range(6):
    env.step(A[k])
  with pytest.raises(ValueError, match="has no Zapper"):
    eng.observe_avatar_ids()
  with pytest.raises(ValueError, match=rf"'{name}' has no Zapper"):
    env.observe_avatar_ids(zap=True)
  got_v, none = env.observe_avatar_ids()
  assert none is None
  want_v, _ = E.avatar_ids_host(eng.pack_bytes, env.save_state().data.cpu().numpy(), zap=False)
  _same(got_v, want_v, name)
  assert want_v[:, np.arange(eng.P), np.arange(eng.P)].all()
  leafy = substrate.get_config(name)
  leafy.individual_observation_names = list(leafy.individual_observation_names) + [ZAP]
  with pytest.raises(ValueError, match=rf"'{name}' has no Zapper"):
    substrate.build_from_config(leafy, roles=cfg.default_player_roles, num_worlds=6, env_seed=SEED)
  eng.sync()
  util.no_faults(eng)
  env.close()


# ---- 3. the registered leaves -------------------------------------------------------------------------
def _leaf_config(name="clean_up"):
  cfg = substrate.get_config(name)
  cfg.individual_observation_names = list(cfg.individual_observation_names) + [VIEW, ZAP]
  return cfg


def _twin(eng):
  """The host twin's (in_view, in_range) of the engine's worlds as they are now."""
  return E.avatar_ids_host(eng.pack_bytes, eng.save_worlds().cpu().numpy(), fingerprint=eng.state_fingerprint,
                           num_players=eng.P)


@pytest.mark.parametrize("T", [0, 4])
def test_the_leaves_follow_every_submission(T):
  cfg, plain_cfg = _leaf_config(), substrate.get_config("clean_up")
  kw = dict(roles=cfg.default_player_roles, num_worlds=N, env_seed=SEED)
  if T:
    kw["rollout_length"] = T
  env = substrate.build_from_config(cfg, **kw)
  twin = substrate.build_from_config(plain_cfg, **kw)
  eng = env.engine
  P = env.num_players
  for n in (VIEW, ZAP):
    spec = env.observation_spec()[0][n]
    assert spec.shape == (P,) and spec.dtype == np.int32 and spec.name == n
    assert n in env.state_leaves() and n not in twin.state_leaves() and n not in twin.observation_spec()[0]
  fused = eng.fused
  rng = np.random.default_rng(SEED)
  history = {}   # ring slot -> what it was given

  def check(ts, what):
    want = _twin(eng)
    got = env.observe_avatar_ids()
    for n, w, g in zip((VIEW, ZAP), want, got):
      leaf = ts.observation[n]
      assert tuple(leaf.shape) == (N, P, P) and leaf.dtype == torch.int32
      _same(leaf, w, (what, n, "leaf")); _same(g, w, (what, n, "observe_avatar_ids"))
      if T:
        assert ts.slot == env.slot
        _same(env.rollout["observation"][n][ts.slot], w, (what, n, "ring slot"))
        history[(n, ts.slot)] = w
    for (n, s), kept in history.items():   # slots written earlier keep what they held
      _same(env.rollout["observation"][n][s], kept, (what, n, "slot", s))

  check(env.reset(), "reset"); twin.reset()
  if T:
    for k in range(9):   # every slot of the ring, twice and once more
      a = _actions(rng, eng, N)
      check(env.step(a), ("step", k)); twin.step(a)
  else:
    a = _actions(rng, eng, N)
    check(env.step(a), "step"); twin.step(a)
    a, mask = _actions(rng, eng, N), torch.from_numpy((np.arange(N) % 3 != 1).astype(np.uint8)).to(eng.device)
    check(env.step(a, active=mask), "step(active=mask)"); twin.step(a, active=mask)
    worlds = [4, 0, 63, 17]
    a = _actions(rng, eng, 3, len(worlds))
    check(env.step_many(a, worlds=worlds).timestep, "step_many(worlds=list)"); twin.step_many(a, worlds=worlds)
  a = _actions(rng, eng, 5, N)
  res = env.step_many(a, states=not T); twin.step_many(a)   # (per-step states beside a ring: not this test's)
  check(res.timestep, "step_many(K = 5)")
  saved = env.save_state()
  a = _actions(rng, eng, N)
  check(env.step(a), "step"); twin.step(a)
  src = [(w * 7) % N if w % 5 else -1 for w in range(N)]
  check(env.load_state(saved, src), "load_state")
  twin.load_state(substrate.WorldStates(saved.data, twin.engine.state_fingerprint), src)
  # saved rows and step_many(states=True) rows through observe_states, with and without players
  for states in (saved,) if T else (saved, res.states):
    every = env.observe_states(states, (VIEW, ZAP))
    want = E.avatar_ids_host(eng.pack_bytes, states.data.cpu().numpy(), fingerprint=eng.state_fingerprint)
    _same(every[VIEW], want[0], "observe_states"); _same(every[ZAP], want[1], "observe_states, zap")
    r = np.random.default_rng(SEED).integers(0, len(states), size=40).astype(np.int32)
    p = np.random.default_rng(SEED + 1).integers(0, P, size=40).astype(np.int32)
    all_rows = env.observe_states(states, (VIEW, ZAP), rows=r)
    drawn = env.observe_states(states, (VIEW, ZAP), rows=r, players=p)
    for n in (VIEW, ZAP):
      assert tuple(drawn[n].shape) == (40, P)
      assert torch.equal(drawn[n], all_rows[n][torch.arange(40), torch.from_numpy(p).long()])
    pair = env.observe_avatar_ids(states, rows=r, players=p)
    assert torch.equal(pair[0], drawn[VIEW]) and torch.equal(pair[1], drawn[ZAP])
  assert set(env.observe_states(saved)) >= {VIEW, ZAP}   # (the default: this substrate's own leaves)
  with pytest.raises(ValueError, match=r"states=True.*observe_states"):
    env.step_many(_actions(rng, eng, 2, N), observations=(VIEW,))
  # the twin without the leaves ends on identical records and identical other leaves
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  ours, theirs = env.observation(), twin.observation()
  assert set(ours) == set(theirs) | {VIEW, ZAP}
  for n in theirs:
    assert torch.equal(ours[n], theirs[n]), n
  # clearing the registration: the leaves are written no more, the engine's launches are its own
  now = (lambda n: env.rollout["observation"][n]) if T else (lambda n: env.observation()[n])
  frozen = {n: now(n).clone() for n in (VIEW, ZAP)}
  assert eng.bind_avatar_ids(None) == (None, None)
  assert eng.fused == fused == twin.engine.fused
  a = _actions(rng, eng, N)
  env.step(a); twin.step(a)
  for n in (VIEW, ZAP):
    assert torch.equal(now(n), frozen[n])
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  for e in (eng, twin.engine):
    e.sync()
    util.no_faults(e)
  env.close()
  twin.close()


def test_one_leaf_alone_and_build_substrate():
  import geometry
  cfg = substrate.get_config("clean_up")
  env = substrate.build_substrate(lab2d_settings=geometry.settings("clean_up"),
                                  individual_observations=["RGB", VIEW], global_observations=[],
                                  action_table=cfg.action_set, num_worlds=6, env_seed=SEED)
  eng = env.engine
  ts = env.reset()
  A = _actions(np.random.default_rng(SEED), eng, 6, 6)
  for k in range(6):
    ts = env.step(A[k])
  assert ZAP not in ts.observation
  _same(ts.observation[VIEW], _twin(eng)[0], "the view leaf alone")
  with pytest.raises(ValueError, match="need a batched substrate"):
    substrate.build_from_config(_leaf_config(), roles=cfg.default_player_roles, num_worlds=1)
  eng.sync()
  util.no_faults(eng)
  env.close()


def test_tune_does_not_write_the_registered_leaves():
  eng = E.Engine(R.pack("clean_up"), 6, device=0)
  eng.bind(E.OBS_WORLD_RGB)
  view, zap = eng.bind_avatar_ids(_filled(eng, *eng.avatar_ids_shape), _filled(eng, *eng.avatar_ids_shape))
  eng.tune()
  assert bool((view == FILL).all()) and bool((zap == FILL).all())
  eng.reset()
  want = _twin(eng)
  _same(view, want[0], "after the reset"); _same(zap, want[1], "after the reset, zap")
  eng.sync()
  util.no_faults(eng)
  eng.close()


def test_a_mixture_of_two_commons_harvest_layouts_shares_the_leaves():
  names = ["commons_harvest__open", "commons_harvest__closed"]
  for T in (0, 2):
    kw = dict(rollout_length=T) if T else {}
    mix = substrate.build_mixture(names, num_worlds=[3, 4], env_seed=SEED, global_observations=(),
                                  individual_observations=("READY_TO_SHOOT", VIEW, ZAP), **kw)
    P = mix.num_players
    dev = mix._members[0].engine.device
    mix.reset()
    A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 5, 7, P, mix.action_spec()[0].num_values)).to(dev)
    for k in range(5):
      ts = mix.step(A[k])
    whole = mix.observe_avatar_ids()
    for n, w in zip((VIEW, ZAP), whole):
      leaf = mix.rollout["observation"][n][mix.slot] if T else ts.observation[n]
      assert tuple(leaf.shape) == (7, P, P) and leaf.dtype == torch.int32
      _same(leaf, w, (T, n, "registered"))
    for i, m in enumerate(mix._members):
      sl = mix.member_slice(i)
      want = _twin(m.engine)
      _same(whole[0][sl], want[0], (T, i, "the member's slice")); _same(whole[1][sl], want[1], (T, i, "the member's slice, zap"))
      m.engine.sync()
      util.no_faults(m.engine)
    mix.close()


# ---- 4. held to the engine's own beam ----------------------------------------------------------------
def _qualifies(pack):
  """Every state that blocks the zap's hit lives on the avatars' layer, and every state of that
  layer that is no avatar's blocks it: the beam and IN_RANGE's rays then stop at the same cells."""
  t = pack_lib.loads(pack)
  hits = [n.decode() for n in bytes(t["hit_names"]).split(b"\0")[:-1]]
  bit = 1 << hits.index("zapHit")
  block = np.asarray(t["state_hit_block"]).reshape(-1).astype(np.int64)
  layer = np.asarray(t["state_layer"]).reshape(-1)
  from meltingpot_amd import lower
  al = int(t["hdr"][lower.HDR_AVATAR_LAYER])
  avatars = {int(s) for s in np.asarray(t["avatar_alive_state"]).reshape(-1)}
  if "avatar_extra_alive" in t:
    avatars |= {int(s) for s in np.asarray(t["avatar_extra_alive"]).reshape(-1, 2)[:, 0]}
  n = min(len(block), len(layer))
  blockers_on_layer = all(layer[s] == al for s in range(1, n) if block[s] & bit)
  layer_blocks = all(block[s] & bit for s in range(1, n) if layer[s] == al and s not in avatars)
  return blockers_on_layer and layer_blocks


def test_in_range_is_who_a_zap_fired_now_hits():
  pack = R.pack("clean_up")
  assert _qualifies(pack), "clean_up does not qualify: " + str([n for n in HR.LEVELS if _qualifies(R.pack(n))])
  rows, what, tags = HR.hand_rows("clean_up")
  use = tags["alive"]   # (every avatar on the map: nobody waits to respawn within the step)
  P = PLAYERS["clean_up"]
  in_range = E.avatar_ids_host(pack, rows)[1][use]
  eng = E.Engine(pack, len(use) * P, device=0, auto_reset=False)
  eng.reset()
  bank = torch.from_numpy(rows[use]).to(eng.device)
  fields = substrate.StateFields(bank, substrate.SubstrateStateLayout(eng.state_layout(), pack_lib.loads(pack)))
  fields.ztimer[:] = 0   # the zap cooldown: ready
  _same(eng.observe_avatar_ids(bank, view=False)[1], in_range, "the device's IN_RANGE of the rows")
  ids = situations.action_ids("clean_up")
  src = np.repeat(np.arange(len(use), dtype=np.int32), P)   # fork p of row r is world r * P + p
  eng.load_worlds(bank, src)
  actions = np.full((len(use), P, P), ids["NOOP"], np.int32)
  actions[:, np.arange(P), np.arange(P)] = ids["fireZap"]
  eng.step(torch.from_numpy(actions.reshape(-1, P)).to(eng.device))
  events = eng.events_all()
  some, shadowed = 0, 0
  for i, r in enumerate(use):
    for p in range(P):
      hit = {int(e["target"]) - 1 for n, e in events[i * P + p] if n == "zap" and int(e["source"]) == p + 1}
      others = [e for n, e in events[i * P + p] if n == "zap" and int(e["source"]) != p + 1]
      assert not others, (what[r], p, others)
      assert hit == set(np.flatnonzero(in_range[i, p]).tolist()), (what[r], p, hit, in_range[i, p])
      some += bool(hit)
    shadowed += r in tags["shadow"] and in_range[i, 0, 1] == 1 and in_range[i, 0, 2] == 0
  assert some >= len(tags["footprint"]) and shadowed == len(tags["shadow"]) == 4
  eng.sync()
  util.no_faults(eng)
  eng.close()
