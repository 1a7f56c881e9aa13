"""Action sequences: `step_many` runs K steps of every world in one launch and hands back the
transition of every step.  It IS the sequential loop: per-step rows, final scalars, records,
counters, views and ring slots are byte-identical to K calls of `step` on a twin engine — on every
pack, through auto-resets and frozen worlds, with repeated actions, raw fields, custom action
tables, strided tensors and mixtures — and the oracle stepped with the same actions agrees without
the single-step path.  Every refusal happens on the host, before any launch."""
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
SCALARS = (E.OBS_REWARD, E.OBS_READY_TO_SHOOT, E.OBS_AUX0, E.OBS_STEP_TYPE, E.OBS_DISCOUNT,
           E.OBS_COLLECTIVE_REWARD, E.OBS_POSITION, E.OBS_ORIENTATION, E.OBS_EVENTS)
OPTIONAL = (E.OBS_ZAP_MATRIX, E.OBS_AUX1, E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES,
            E.OBS_MATRIX_CUMULANTS, E.OBS_INTERACTION_REWARDS)
# the five per-step kinds, by the name step_many returns them under
FIVE = {"reward": E.OBS_REWARD, "collective_reward": E.OBS_COLLECTIVE_REWARD,
        "step_type": E.OBS_STEP_TYPE, "discount": E.OBS_DISCOUNT, "events": E.OBS_EVENTS}


def _engine(pack, n, kinds=SCALARS, **kw):
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


def _same_bufs(a, b, what):
  for k in a:
    if k == E.OBS_EVENTS:
      _same_events(a[k], b[k], what)
    else:
      assert torch.equal(a[k], b[k]), (what, k, (a[k] != b[k]).nonzero()[:4].tolist())


def _loop(e, bufs, A, fields=False):
  """K calls of step on e; returns the five kinds cloned after every step."""
  rows = {name: [] for name in FIVE}
  for k in range(A.shape[0]):
    (e.step_fields if fields else e.step)(A[k])
    for name, kind in FIVE.items():
      rows[name].append(bufs[kind].clone())
  return {name: torch.stack(v) for name, v in rows.items()}


def _same_rows(got, ref, what):
  for name in got:
    if name == "events":
      for k in range(ref[name].shape[0]):
        _same_events(got[name][k], ref[name][k], (what, "row", k))
    else:
      assert torch.equal(got[name], ref[name]), (what, name, (got[name] != ref[name]).nonzero()[:4].tolist())


def _same_engines(a, abufs, b, bbufs, what):
  _same_bufs(abufs, bbufs, what)
  assert torch.equal(a.save_worlds(), b.save_worlds()), what
  assert a.counters() == b.counters(), what
  util.no_faults(a); util.no_faults(b)


def _supported(pack):
  probe = engine.Engine(pack, 1, device=0, debug_observations=True)
  extra = tuple(k for k in OPTIONAL if probe._L.mp_obs_bytes(probe._h, k) > 0)
  probe.close()
  return extra


# ---- 1. every pack ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PACKS)
def test_every_pack_equals_the_sequential_loop(name):
  pack = engine.load_pack(name)
  kinds = SCALARS + _supported(pack)
  n = 64
  for dev in (None, {"no_next_orders": 1}):
    kw = {"debug_observations": True}
    if dev:
      kw["dev"] = dev
    a, abufs = _engine(pack, n, kinds, **kw)
    b, bbufs = _engine(pack, n, kinds, **kw)
    P, nact = a.P, a.num_actions
    rng = np.random.default_rng(11)
    warm = torch.from_numpy(util.random_actions(rng, 20, n, P, nact)).to(a.device)
    a.reset(); b.reset()
    for s in range(20):
      a.step(warm[s]); b.step(warm[s])
    for K in (1, 7, 33):
      A = torch.from_numpy(util.random_actions(rng, K, n, P, nact)).to(a.device)
      got = a.step_many(A, events=True)
      ref = _loop(b, bbufs, A)
      _same_rows(got, ref, (name, dev, K))
      _same_engines(a, abufs, b, bbufs, (name, dev, K))
    a.close(); b.close()


# ---- 2. against the oracle, without the single-step path ---------------------------------------
@pytest.mark.parametrize("name", ["clean_up", "commons_harvest__open", "territory__rooms",
                                  "prisoners_dilemma_in_the_matrix__arena",
                                  "collaborative_cooking__cramped"])
def test_sixty_steps_in_one_launch_match_the_oracle(name):
  pack = engine.load_pack(name)
  n, K = 8, 60
  e, bufs = _engine(pack, n, (E.OBS_REWARD,))
  A = util.random_actions(np.random.default_rng(12), K, n, e.P, e.num_actions)
  e.reset()
  got = e.step_many(torch.from_numpy(A).to(e.device), keep=("reward",))
  rew = got["reward"].cpu().numpy()
  grid, avat, glob = e.dump()
  oracles = util.make_oracles(pack, n)
  for w, o in enumerate(oracles):
    o.reset()
    for k in range(K):
      o.step(A[k, w])
      assert np.array_equal(rew[k, w], o.rewards()), (name, w, k)
    og, oa, ogl = o.dump()
    assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), (name, w)
    assert np.array_equal(glob[w], ogl), (name, w)
    o.close()
  assert np.array_equal(bufs[E.OBS_REWARD].cpu().numpy(), rew[K - 1])
  util.no_faults(e)
  e.close()


# ---- 3. episodes that end inside a sequence ----------------------------------------------------
@pytest.mark.parametrize("auto", [True, False])
def test_episodes_end_inside_the_sequence(auto):
  """MAXFRAMES = 9 and K = 33 right after a reset: every world is LAST at row 8.  With auto_reset it
  is FIRST at row 9 and so on every ten rows; without, it is frozen from row 9 on (row 8 is the
  episode's own last step, with whatever it paid and reported: LAST, discount 0), and reports LAST,
  zero reward, zero discount and an empty event header to the end.  The row patterns are asserted
  here, so the test cannot pass on sequences in which nothing ended."""
  pack = util.patch_pack(engine.load_pack("clean_up"), MAXFRAMES=9)
  n, K = 16, 33
  a, abufs = _engine(pack, n, auto_reset=auto)
  b, bbufs = _engine(pack, n, auto_reset=auto)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(13), K, n, a.P, a.num_actions)).to(a.device)
  a.reset(); b.reset()
  got = a.step_many(A, events=True)
  ref = _loop(b, bbufs, A)
  st = got["step_type"].cpu().numpy()
  if auto:
    for last in (8, 18, 28):
      assert (st[last] == 2).all() and (st[last + 1] == 0).all(), (last, st[last], st[last + 1])
    others = [k for k in range(K) if k not in (8, 18, 28, 9, 19, 29)]
    assert (st[others] == 1).all()
  else:
    assert (st[:8] == 1).all() and (st[8:] == 2).all()
    assert (got["reward"][9:] == 0).all() and (got["collective_reward"][9:] == 0).all()
    assert (got["discount"][8:] == 0).all()
    assert (got["events"][9:, :, 0, :] == 0).all()   # an empty header from the first frozen step on
  _same_rows(got, ref, ("episodes", auto))
  _same_engines(a, abufs, b, bbufs, ("episodes", auto))
  assert a.counters()["episodes"] == b.counters()["episodes"] == (n * 4 if auto else n)
  a.close(); b.close()


# ---- 4. views and rings ------------------------------------------------------------------------
@pytest.mark.parametrize("views", [(E.OBS_RGB, E.OBS_WORLD_RGB, E.OBS_LAYER),
                                   (E.OBS_RGB_POOL8, E.OBS_WORLD_RGB, E.OBS_LAYER)])
def test_views_after_the_sequence_are_the_loops(views):
  pack = engine.load_pack("clean_up")
  n, K = 24, 9
  kw = {"world_pool": 8} if E.OBS_RGB_POOL8 in views else {}
  a, abufs = _engine(pack, n, SCALARS + views, **kw)
  b, bbufs = _engine(pack, n, SCALARS + views, **kw)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(14), K, n, a.P, a.num_actions)).to(a.device)
  a.reset(); b.reset()
  for _ in range(2):
    got = a.step_many(A)
    ref = _loop(b, bbufs, A)
    _same_rows(got, {k: ref[k] for k in got}, "views")
    _same_engines(a, abufs, b, bbufs, ("views", views))
  a.close(); b.close()


def test_substrate_ring_takes_one_slot():
  roles = substrate.get_config("clean_up").default_player_roles
  n, K, T = 6, 5, 4
  env = substrate.build("clean_up", roles=roles, num_worlds=n, rollout_length=T, env_seed=31)
  twin = substrate.build("clean_up", roles=roles, num_worlds=n, rollout_length=T, env_seed=31)
  dev = env.engine.device
  A = torch.from_numpy(util.random_actions(np.random.default_rng(15), K, n, env.num_players,
                                           env.action_spec()[0].num_values)).to(dev)
  env.reset(); twin.reset()
  env.step(A[0]); twin.step(A[0])
  before = env.slot
  ring = env.rollout
  kept = {s: {k: v[s].clone() for k, v in ring["observation"].items()} for s in range(T)}
  res = env.step_many(A)
  assert isinstance(res, substrate.StepManyResult) and isinstance(res.timestep, substrate.RolloutTimeStep)
  assert env.slot == (before + 1) % T == res.timestep.slot
  for k in range(K):
    last = twin.step(A[k])
  assert torch.equal(res.timestep.step_type, last.step_type)
  assert torch.equal(res.timestep.reward, last.reward) and torch.equal(res.reward[K - 1], last.reward)
  for name, leaf in last.observation.items():
    assert torch.equal(res.timestep.observation[name], leaf), name
  for s in range(T):
    if s != env.slot:
      for name, v in kept[s].items():
        assert torch.equal(ring["observation"][name][s], v), (s, name)
  one = substrate.build("clean_up", roles=roles, num_worlds=1)
  with pytest.raises(ValueError, match="num_worlds"):
    one.step_many(np.zeros((3, 1, one.num_players), np.int32))
  env.close(); twin.close(); one.close()


# ---- 5. repeat and fields ----------------------------------------------------------------------
def test_repeat_fields_and_custom_action_tables():
  pack = engine.load_pack("clean_up")
  n, K = 16, 12
  a, abufs = _engine(pack, n)
  b, bbufs = _engine(pack, n)
  rng = np.random.default_rng(16)
  P, nact = a.P, a.num_actions
  a.reset(); b.reset()
  block = torch.from_numpy(util.random_actions(rng, 1, n, P, nact)[0]).to(a.device)
  got = a.step_many(block, repeat=K, events=True)
  ref = _loop(b, bbufs, block.expand(K, n, P))
  _same_rows(got, ref, "repeat")
  _same_engines(a, abufs, b, bbufs, "repeat")
  # raw fields: the rows of the stock ACTION_SET, one out-of-range field among them (a counted NOOP)
  table = np.asarray(util.pack_tables(pack)["action_table"], np.int32).reshape(-1, 4)
  nf = int(a.info.num_action_fields)
  F = table[util.random_actions(rng, K, n, P, nact)][..., :nf].copy()
  F[3, 2, 1, 0] = 99
  F = torch.from_numpy(np.ascontiguousarray(F)).to(a.device)
  got = a.step_many(F, fields=True, events=True)
  ref = _loop(b, bbufs, F, fields=True)
  _same_rows(got, ref, "fields")
  _same_engines(a, abufs, b, bbufs, "fields")
  assert a.counters()["bad_actions"] == b.counters()["bad_actions"] >= 1
  # a host array is uploaded once
  H = util.random_actions(rng, K, n, P, nact)
  got = a.step_many(H)
  ref = _loop(b, bbufs, torch.from_numpy(H).to(b.device))
  _same_rows(got, {k: ref[k] for k in got}, "host")
  a.close(); b.close()
  # a Substrate with a custom action_table: its own step loop
  cfg = substrate.get_config("clean_up")
  custom = [dict(cfg.action_set[i]) for i in (0, 3, 1, 7, 8, 5)]
  env = substrate.build("clean_up", roles=cfg.default_player_roles, num_worlds=n, action_table=custom, env_seed=32)
  twin = substrate.build("clean_up", roles=cfg.default_player_roles, num_worlds=n, action_table=custom, env_seed=32)
  A = torch.from_numpy(util.random_actions(rng, K, n, env.num_players, len(custom))).to(env.engine.device)
  env.reset(); twin.reset()
  res = env.step_many(A)
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.reward[k], ts.reward) and torch.equal(res.step_type[k], ts.step_type), k
    assert torch.equal(res.discount[k], ts.discount), k
  for name, leaf in ts.observation.items():
    assert torch.equal(res.timestep.observation[name], leaf), name
  assert torch.equal(env.engine.save_worlds(), twin.engine.save_worlds())
  env.close(); twin.close()


# ---- 6. strides --------------------------------------------------------------------------------
def test_column_slices_of_wider_tensors():
  pack = engine.load_pack("clean_up")
  n, K = 12, 10
  a, abufs = _engine(pack, n)
  b, bbufs = _engine(pack, n)
  P, nact = a.P, a.num_actions
  dev = a.device
  off = n
  wide = torch.full((K, 3 * n, P), -77, dtype=torch.int32, device=dev)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(17), K, n, P, nact)).to(dev)
  wide[:, off:off + n] = A
  shapes = {"reward": ((K, 3 * n, P), torch.float64), "collective_reward": ((K, 3 * n), torch.float64),
            "step_type": ((K, 3 * n), torch.int32), "discount": ((K, 3 * n), torch.float64),
            "events": ((K, 3 * n, E.EVENT_ROWS, 4), torch.int32)}
  outs = {k: torch.full(s, 123, dtype=d, device=dev) for k, (s, d) in shapes.items()}
  a.reset(); b.reset()
  got = a.step_many(wide[:, off:off + n], events=True, out={k: v[:, off:off + n] for k, v in outs.items()})
  ref = _loop(b, bbufs, A)
  _same_rows(got, ref, "strides")
  _same_engines(a, abufs, b, bbufs, "strides")
  for k, v in outs.items():
    assert got[k].data_ptr() == v[:, off:off + n].data_ptr()
    assert (v[:, :off] == 123).all() and (v[:, off + n:] == 123).all(), k   # the neighbours survive
  assert (wide[:, :off] == -77).all() and (wide[:, off + n:] == -77).all()
  with pytest.raises(ValueError, match="along K only"):
    a.step_many(torch.zeros((K, n, 2 * P), dtype=torch.int32, device=dev)[:, :, :P])
  a.close(); b.close()


def test_mixture_of_the_two_player_kitchens():
  names = tuple(f"collaborative_cooking__{k}" for k in ("asymmetric", "circuit", "cramped", "forced", "ring"))
  K = 14
  mix = substrate.build_mixture(names, num_worlds=40, env_seed=33)
  twin = substrate.build_mixture(names, num_worlds=40, env_seed=33)
  n, P = mix.num_worlds, mix.num_players
  A = torch.from_numpy(util.random_actions(np.random.default_rng(18), K, n, P,
                                           mix.action_spec()[0].num_values)).to(mix.engines[0].device)
  mix.reset(); twin.reset()
  res = mix.step_many(A, events=True)
  assert tuple(res.reward.shape) == (K, n, P) and tuple(res.events.shape) == (K, n, E.EVENT_ROWS, 4)
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.reward[k], ts.reward) and torch.equal(res.step_type[k], ts.step_type), k
    assert torch.equal(res.discount[k], ts.discount), k
    assert torch.equal(res.collective_reward[k], ts.observation["COLLECTIVE_REWARD"]), k
  for name, leaf in ts.observation.items():
    assert torch.equal(res.timestep.observation[name], leaf), name
  for x, y in zip(mix.engines, twin.engines):
    assert torch.equal(x.save_worlds(), y.save_worlds())
  assert mix.counters() == twin.counters()
  mix.close(); twin.close()


# ---- 7. forks ----------------------------------------------------------------------------------
def test_forks_of_one_state_run_different_sequences():
  pack = engine.load_pack("clean_up")
  n, K = 64, 25
  src, sbufs = _engine(pack, n, (E.OBS_REWARD,))
  fork, _ = _engine(pack, n, (E.OBS_REWARD,))
  P, nact = src.P, src.num_actions
  rng = np.random.default_rng(19)
  A = torch.from_numpy(util.random_actions(rng, 40, n, P, nact)).to(src.device)
  B = torch.from_numpy(util.random_actions(rng, K, n, P, nact)).to(src.device)
  src.reset(); fork.reset()
  for s in range(40):
    src.step(A[s])
  bank = src.save_worlds()
  fork.load_worlds(bank, np.full(n, 3, np.int32))
  got = fork.step_many(B, keep=("reward",))["reward"]
  for j in (0, 3, 9, 17, 31, 40, 55, 63):
    # the source world continued sequentially under fork j's sequence
    src.load_worlds(bank, np.arange(n, dtype=np.int32))
    for k in range(K):
      acts = A[0].clone()
      acts[3] = B[k, j]
      src.step(acts)
      assert torch.equal(sbufs[E.OBS_REWARD][3], got[k, j]), (j, k)
  util.no_faults(src); util.no_faults(fork)
  src.close(); fork.close()


# ---- 8. geometry and size ----------------------------------------------------------------------
def test_the_largest_map_steps_two_worlds_per_workgroup():
  pack = geometry.pack("clean_up", width=64, height=64)
  n, K = 10, 12
  a, abufs = _engine(pack, n)
  b, bbufs = _engine(pack, n)
  A = torch.from_numpy(util.random_actions(np.random.default_rng(20), K, n, a.P, a.num_actions)).to(a.device)
  a.reset(); b.reset()
  got = a.step_many(A, events=True)
  ref = _loop(b, bbufs, A)
  _same_rows(got, ref, "64 x 64")
  _same_engines(a, abufs, b, bbufs, "64 x 64")
  a.close(); b.close()


def test_at_size_sampled_worlds_match_the_oracle():
  pack = engine.load_pack("clean_up")
  n, K = 4096, 64
  e, bufs = _engine(pack, n, (E.OBS_REWARD,))
  A = util.random_actions(np.random.default_rng(21), K, n, e.P, e.num_actions)
  e.reset()
  rew = e.step_many(torch.from_numpy(A).to(e.device), keep=("reward",))["reward"].cpu().numpy()
  grid, avat, glob = e.dump()
  for w in range(5, n, 128):   # 32 worlds
    o = util.make_oracles(pack, 1, offset=w)[0]
    o.reset()
    for k in range(K):
      o.step(A[k, w])
      assert np.array_equal(rew[k, w], o.rewards()), (w, k)
    og, oa, ogl = o.dump()
    assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa) and np.array_equal(glob[w], ogl), w
    o.close()
  util.no_faults(e)
  e.close()


# ---- 9. refusals -------------------------------------------------------------------------------
def _request(e, **fields):
  """The return code of one raw MpStepMany request on engine e (through mp_restore)."""
  req = engine.MpStepMany(ctypes.sizeof(engine.MpStepMany), 1)
  for k, v in fields.items():
    if k.startswith("row"):        # row2=(ptr, distance): per_step[2]
      req.per_step[int(k[3:])], req.per_step_bytes[int(k[3:])] = v
    else:
      setattr(req, k, v)
  return e._L.mp_restore(e._h, ctypes.addressof(req), ctypes.sizeof(req))


def test_refusals_launch_nothing_and_leave_the_engine_as_it_was():
  pack = engine.load_pack("clean_up")
  n, K = 8, 6
  e, bufs = _engine(pack, n)
  L = e._L
  P, nact = e.P, e.num_actions
  dev = e.device
  A = torch.from_numpy(util.random_actions(np.random.default_rng(22), K, n, P, nact)).to(dev)
  ablock = n * P * 4

  def refused(word, **fields):
    assert _request(e, **fields) == engine.MP_ERR_INVALID, fields
    assert word.encode() in L.mp_last_error(), (word, L.mp_last_error())

  refused("never been reset", steps=K, actions=A.data_ptr(), actions_step_bytes=ablock)
  e.reset()
  e.step(A[0])
  state, ctr = e.save_worlds().clone(), e.counters()
  scal = {k: v.clone() for k, v in bufs.items()}
  ok = dict(steps=K, actions=A.data_ptr(), actions_step_bytes=ablock)
  refused("NULL", steps=K, actions=None)
  assert L.mp_restore(None, ctypes.addressof(engine.MpStepMany(ctypes.sizeof(engine.MpStepMany), 1)),
                      ctypes.sizeof(engine.MpStepMany)) == engine.MP_ERR_INVALID
  refused("steps", **dict(ok, steps=0))
  refused("steps", **dict(ok, steps=engine.STEP_MANY_MAX + 1))
  refused("struct_size", **dict(ok, struct_size=8))
  refused("fields", **dict(ok, fields=2))
  refused("actions_step_bytes", **dict(ok, actions_step_bytes=ablock - 4))
  refused("actions_step_bytes", **dict(ok, actions_step_bytes=ablock + 2))
  rew = torch.zeros((K, n, P), dtype=torch.float64, device=dev)
  st = torch.zeros((K, n), dtype=torch.int32, device=dev)
  ev = torch.zeros((K, n, E.EVENT_ROWS, 4), dtype=torch.int32, device=dev)
  evb = n * E.EVENT_ROWS * 16
  refused("REWARD", **dict(ok, row0=(rew.data_ptr(), n * P * 8 - 8)))      # smaller than a step's rows
  refused("REWARD", **dict(ok, row0=(rew.data_ptr(), n * P * 8 + 4)))      # not a multiple of 8
  refused("STEP_TYPE", **dict(ok, row2=(st.data_ptr(), n * 4 + 2)))
  refused("EVENTS", **dict(ok, row4=(ev.data_ptr(), evb + 8)))             # rows are int4: 16 bytes
  refused("aligned", **dict(ok, row4=(ev.data_ptr() + 4, evb)))            # a misaligned EVENTS base
  # memory the device cannot be trusted with: a host numpy array, pinned host memory
  host = np.zeros((K, n, P), np.int32)
  refused("host", **dict(ok, actions=host.ctypes.data))
  pinned = torch.zeros((K, n, P), dtype=torch.float64).pin_memory()
  refused("host", **dict(ok, row0=(pinned.data_ptr(), n * P * 8)))
  # buffers too short by one row: K rows end exactly where the device allocation ends (torch's
  # caching allocator hands out parts of larger allocations, so the end is the runtime's answer)
  # and the request asks for K + 1
  hip = ctypes.CDLL("libamdhip64.so")
  def end_of_allocation(tensor):
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size),
                                     ctypes.c_void_p(tensor.data_ptr())) == 0
    return base.value + size.value
  short = dict(ok, steps=K + 1)
  refused("allocation", **dict(short, actions=end_of_allocation(A) - K * ablock))
  refused("allocation", **dict(short, row0=(end_of_allocation(rew) - K * n * P * 8, n * P * 8)))
  refused("allocation", **dict(short, row4=(end_of_allocation(ev) - K * evb, evb)))
  with pytest.raises(ValueError):
    e.step_many(A.to(torch.int64))
  with pytest.raises(ValueError):
    e.step_many(A[:, :, :P - 1])
  # nothing was launched: the engine is as it was, and goes on like a twin
  assert torch.equal(e.save_worlds(), state) and e.counters() == ctr
  for k, v in bufs.items():
    assert torch.equal(v, scal[k]), k
  twin, tb = _engine(pack, n)
  twin.reset()
  twin.step(A[0])
  got = e.step_many(A, events=True)
  ref = _loop(twin, tb, A)
  _same_rows(got, ref, "after refusals")
  _same_engines(e, bufs, twin, tb, "after refusals")
  e.close(); twin.close()


# ---- 10. the raw request ------------------------------------------------------------------------
def test_a_raw_request_equals_engine_step_many():
  """Engine.step_many sends an MpStepTrajectory; an MpStepMany request as a C caller sends it
  (all five rows; a block of actions per step, then one block repeated) gives the same rows and
  leaves the same engine."""
  pack = engine.load_pack("clean_up")
  n, K = 16, 9
  e, bufs = _engine(pack, n)
  twin, tb = _engine(pack, n)
  P, nact = e.P, e.num_actions
  A = torch.from_numpy(util.random_actions(np.random.default_rng(23), K, n, P, nact)).to(e.device)
  e.reset(); twin.reset()
  e.step(A[0]); twin.step(A[0])
  e.use_current_stream()
  for repeat in (False, True):
    ref = twin.step_many(A[1], repeat=K, events=True) if repeat else twin.step_many(A, events=True)
    got = {name: torch.zeros_like(v) for name, v in ref.items()}
    rows = {f"row{i}": (got[name].data_ptr(), got[name][0].numel() * got[name].element_size())
            for i, name in enumerate(FIVE)}
    assert _request(e, steps=K, actions=(A[1] if repeat else A).data_ptr(),
                    actions_step_bytes=0 if repeat else n * P * 4, **rows) == 0, e._L.mp_last_error()
    _same_rows(got, ref, ("raw", repeat))
    _same_engines(e, bufs, twin, tb, ("raw", repeat))
  e.close(); twin.close()
