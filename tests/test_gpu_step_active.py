"""Stepping some of the worlds (MpStepActive; Engine.step / Engine.step_many with active=): in step k
world w runs only where active[k, w] is non-zero and is not touched otherwise.  On the recipe's packs
(one per level kernel, episodes of 16 frames, five worlds, 24 seeded steps): all ones against the
unmasked request, all zeros, the K-step request against the loop of masked single steps, the worlds'
independence against an UNMASKED twin (the anchor that does not lean on the new code), the CPU
oracle's model, bound views and fusing, registered episode starts, the refusals, and the Substrate
and mixture surface.

The mask of the K = 24 tests is fixed: world 0 is active throughout (it passes an episode boundary),
world 1 never, world 2 on even k (it ends mid-episode), world 3 for k < 16 and again from k = 20 (it
is paused on LAST, in front of its reset, for k = 16 .. 19), world 4 with p = 0.6 from a seeded
generator."""
import ctypes

import numpy as np
import pytest
import torch

import states_recipe as R
import util
from engine_model import ModelEngine
from meltingpot_amd import engine, substrate
from test_gpu_episode_starts import PIXEL_PACKS, _plan, _same_as_model, _same_events

pytestmark = pytest.mark.gpu

E = engine
N, K = R.N, R.STEPS
FIVE = (("reward", E.OBS_REWARD), ("collective_reward", E.OBS_COLLECTIVE_REWARD),
        ("step_type", E.OBS_STEP_TYPE), ("discount", E.OBS_DISCOUNT), ("events", E.OBS_EVENTS))
KITCHEN = "collaborative_cooking__cramped"


def _mask():
  m = np.zeros((K, N), np.uint8)
  m[:, 0] = 1
  m[0::2, 2] = 1
  m[:16, 3] = 1
  m[20:, 3] = 1
  m[:, 4] = np.random.default_rng(21).random(K) < 0.6
  return m


MASK = _mask()


def _obs_kinds(name):
  """Every non-pixel kind of the level beyond the five, the debug kinds included."""
  probe = engine.Engine(R.pack(name), 1, device=0, debug_observations=True)
  obs = tuple(k for k in E.STEP_ROW_KINDS
              if k not in [kind for _, kind in FIVE] and probe._L.mp_obs_bytes(probe._h, k) > 0)
  probe.close()
  return obs


def _engine(name, **kw):
  e = engine.Engine(R.pack(name), N, device=0, debug_observations=True, **kw)
  e.reset()
  return e


def _actions(e):
  return torch.from_numpy(R.actions(e.P, e.num_actions)).to(e.device)


def _keys(obs):
  """(key of step_many's result, kind) of every row kind but the states and the hashes."""
  return FIVE + tuple((k, k) for k in obs)


def _leaves(e, obs):
  return {key: e.observe(kind).clone() for key, kind in _keys(obs)}


def _same(a, b, key, what):
  """Two blocks [n, ...] of one kind."""
  if key == "events":
    _same_events(a.cpu().numpy(), b.cpu().numpy(), (what, key))
  else:
    assert torch.equal(a, b), (what, key)


def _same_leaves(a, b, obs, what):
  for key, kind in _keys(obs):
    _same(a.observe(kind), b[key] if isinstance(b, dict) else b.observe(kind), key, what)


def _same_engines(a, b, obs, what):
  assert torch.equal(a.save_worlds(), b.save_worlds()), what
  assert a.counters() == b.counters(), what
  _same_leaves(a, b, obs, what)


def _all_rows(obs):
  return dict(events=True, observations=obs, states=True, hashes=True)


def _close(*engines):
  for e in engines:
    util.no_faults(e, sync=True)
    e.close()


# ---- 1. all ones ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_all_ones_is_the_unmasked_request(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  ones = torch.ones((K, N), dtype=torch.uint8, device=a.device)
  got = a.step_many(A, active=ones, **_all_rows(obs))
  ref = b.step_many(A, **_all_rows(obs))
  assert set(got) == set(ref)
  for key in ref:
    for k in range(K) if key == "events" else (slice(None),):
      _same(got[key][k], ref[key][k], key, (name, k))
  _same_engines(a, b, obs, name)
  # ... and the masked single step
  a.step(A[3], active=ones[0]); b.step(A[3])
  _same_engines(a, b, obs, (name, "step"))
  a.step(A[4].cpu().numpy(), active=[True] * N); b.step(A[4])
  _same_engines(a, b, obs, (name, "host step"))
  _close(a, b)


# ---- 2. all zeros ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_all_zeros_touches_nothing(name):
  obs = _obs_kinds(name)
  e = _engine(name)
  A = _actions(e)
  e.step_many(A[:3])
  saved, hashed, leaves, counters = e.save_worlds().clone(), e.hash_worlds().clone(), _leaves(e, obs), e.counters()
  zeros = torch.zeros((K, N), dtype=torch.uint8, device=e.device)
  for mask in (zeros, zeros[0], zeros[:, :1].expand(K, N).contiguous().bool()):
    got = e.step_many(A, active=mask, **_all_rows(obs))
    assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, name
    _same_leaves(e, leaves, obs, name)
    for key, _ in _keys(obs):
      for k in range(K):
        _same(got[key][k], leaves[key], key, (name, k))
    assert torch.equal(got["states"], saved[None].expand(K, -1, -1)), name
    assert torch.equal(got["hashes"], hashed[None].expand(K, -1)), name
  # (without a row that is a function of the record, such a world does not even load its record)
  light = tuple(k for k in obs if k != E.OBS_LAYER)
  got = e.step_many(A, active=zeros, events=True, observations=light)
  for key, _ in _keys(light):
    for k in range(K):
      _same(got[key][k], leaves[key], key, (name, "light", k))
  assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, name
  _same_leaves(e, leaves, obs, (name, "light"))
  e.step(A[3], active=zeros[0])
  assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, name
  _same_leaves(e, leaves, obs, (name, "step"))
  _close(e)


# ---- 3. the K-step request is the loop of masked single steps -------------------------------------
def _masked_loop(b, A, M, obs):
  """The loop of K masked single steps on `b`: per step a clone of every leaf, the records and
  their hashes."""
  rows = []
  for k in range(A.shape[0]):
    b.step(A[k], active=M[k])
    row = _leaves(b, obs)
    row["states"], row["hashes"] = b.save_worlds().clone(), b.hash_worlds().clone()
    rows.append(row)
  return rows


def _same_rows(got, rows, what):
  for k, row in enumerate(rows):
    for key in got:
      _same(got[key][k], row[key], key, (what, k))


def _mask_covers(types, name):
  """The fixed mask did what it is there for (`types`: the masked run's step types [K, N])."""
  types = types.cpu().numpy()
  assert (types[15:20, 3] == 2).all() and types[20, 3] == 0, (name, types[:, 3])   # paused on LAST, then its reset
  assert types[15, 0] == 2 and types[16, 0] == 0, (name, types[:, 0])              # over an episode boundary
  assert types[K - 1, 2] == 1, (name, types[:, 2])                                  # mid-episode in the end
  assert (types[:, 1] == 0).all(), (name, types[:, 1])                              # never ran: FIRST as reset left it


@pytest.mark.parametrize("name", R.PACKS)
def test_step_many_is_the_loop_of_masked_steps(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  got = a.step_many(A, active=M, **_all_rows(obs))
  rows = _masked_loop(b, A, M, obs)
  _same_rows(got, rows, name)
  _same_engines(a, b, obs, name)
  _mask_covers(got["step_type"], name)
  _close(a, b)


def test_step_many_rows_one_family_at_a_time():
  """The one family serves every combination of rows: none, the five only, LAYER only, states only,
  hashes only — each equal to the columns of the request that names them all."""
  name = "clean_up"
  full = _engine(name)
  A = _actions(full)
  M = torch.from_numpy(MASK).to(full.device)
  ref = full.step_many(A, active=M, observations=(E.OBS_LAYER,), states=True, hashes=True)
  for kw in ({}, {"keep": ()}, {"observations": (E.OBS_LAYER,)}, {"states": True}, {"hashes": True},
             {"keep": (), "observations": (E.OBS_POSITION,)}):
    e = _engine(name)
    got = e.step_many(A, active=M, **kw)
    for key, value in got.items():
      if key in ref:
        assert torch.equal(value, ref[key]), (kw, key)
    assert torch.equal(e.save_worlds(), full.save_worlds()) and e.counters() == full.counters(), kw
    _close(e)
  _close(full)


# ---- 4. worlds are independent: the masked run against an UNMASKED twin ----------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_a_masked_world_is_the_unmasked_world_of_its_own_steps(name):
  """World w of the masked run IS world w of an unmasked run of the compacted actions A'[j, w] =
  A[k_j(w), w] (k_j(w): the j-th active step of w; padded with action 0): with c_w(k) the number of
  active steps of w up to and including k, row k of w equals the twin's row c_w(k) - 1, or the
  buffer as it was before the request where c_w(k) = 0; the final record is the twin's state row
  c_w(K - 1) - 1.  The twin runs k_step_hashes_*, which this feature does not touch."""
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  count = MASK.astype(np.int64).cumsum(0)                      # c_w(k)
  compact = torch.zeros_like(A)
  for w in range(N):
    steps = np.nonzero(MASK[:, w])[0]
    compact[:len(steps), w] = A[torch.from_numpy(steps).to(A.device), w]
  before = _leaves(a, obs)
  before["states"], before["hashes"] = a.save_worlds().clone(), a.hash_worlds().clone()
  got = a.step_many(A, active=torch.from_numpy(MASK).to(a.device), **_all_rows(obs))
  twin = b.step_many(compact, **_all_rows(obs))
  final = a.save_worlds()
  for w in range(N):
    at = torch.from_numpy(count[:, w] - 1).to(a.device)
    ran = at >= 0
    for key in got:
      want = twin[key][at.clamp(min=0), w]
      want[~ran] = before[key][w]
      _same(got[key][:, w], want, key, (name, w))
    last = int(count[K - 1, w])
    assert torch.equal(final[w], twin["states"][last - 1, w] if last else before["states"][w]), (name, w)
  _mask_covers(got["step_type"], name)
  _close(a, b)


# ---- 5. against the oracle ------------------------------------------------------------------------
# (the model under a mask is ModelEngine's own: tests/engine_model.py)
@pytest.mark.parametrize("name", R.PACKS)
def test_step_and_step_many_against_the_oracle(name):
  views = (E.OBS_RGB, E.OBS_WORLD_RGB, E.OBS_LAYER) if name in PIXEL_PACKS else ()
  for many in (False, True):
    e = engine.Engine(R.pack(name), N, device=0)
    m = ModelEngine(R.pack(name), N, auto_reset=True)
    for kind in views:
      e.bind(kind).zero_()
      m.bind(kind)
    e.reset(); m.reset()
    A = R.actions(e.P, e.num_actions)
    dA = torch.from_numpy(A).to(e.device)
    dM = torch.from_numpy(MASK).to(e.device)
    record = tuple(k for k in m.record_scalars)
    if many:
      got = e.step_many(dA, active=dM, events=True, observations=record)
      ref = m.step_many(A, active=MASK, events=True, observations=record)
      for key in ("reward", "collective_reward", "step_type", "discount") + record:
        assert np.array_equal(got[key].cpu().numpy(), ref[key]), (name, key)
      for k in range(K):
        _same_events(got["events"][k].cpu().numpy(), ref["events"][k], (name, "row", k))
      _same_as_model(e, m, (name, "step_many"), views)
      _mask_covers(got["step_type"], name)
    else:
      for k in range(K):
        e.step(dA[k], active=dM[k])
        m.step(A[k], active=MASK[k])
        _same_as_model(e, m, (name, "step", k), views)
    _close(e)
    m.close()


# ---- 6. views and fusing --------------------------------------------------------------------------
def test_views_are_redrawn_and_the_engine_stays_fused():
  name = "clean_up"
  views = (E.OBS_RGB, E.OBS_WORLD_RGB)
  a = engine.Engine(R.pack(name), N, device=0)
  b = engine.Engine(R.pack(name), N, device=0)
  for e in (a, b):
    for kind in views:
      e.bind(kind).zero_()
    e.reset()
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  fused = a.fused
  assert fused
  for k in range(4):
    a.step(A[k], active=M[k])
    bank = a.save_worlds()
    for kind in views:
      assert torch.equal(a._bound[kind], a.observe_states(bank, kind)), (k, kind)
    assert a.fused == fused
  a.step_many(A[4:12], active=M[4:12])
  bank = a.save_worlds()
  for kind in views:
    assert torch.equal(a._bound[kind], a.observe_states(bank, kind)), kind
  assert a.fused == fused
  # the twin joins a where it is now; the next unmasked step is the step it was
  b.load_worlds(bank, np.arange(N, dtype=np.int32))
  a.step(A[12]); b.step(A[12])
  assert torch.equal(a.hash_worlds(), b.hash_worlds())
  for kind in views:
    assert torch.equal(a._bound[kind], b._bound[kind]), kind
  _close(a, b)


# ---- 7. registered episode starts -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", KITCHEN])
def test_episode_starts_under_a_mask(name):
  obs = _obs_kinds(name)
  a, b, c = _engine(name), _engine(name), _engine(name)
  bank, rows, info = _plan(a, name)
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  drows = [torch.from_numpy(rows).to(e.device) for e in (a, b, c)]
  for e, r in zip((a, b, c), drows):
    e.set_episode_starts(bank, r)
  got = a.step_many(A, active=M, **_all_rows(obs))
  _same_rows(got, _masked_loop(b, A, M, obs), name)
  _same_engines(a, b, obs, name)
  # worlds 0 and 3 started from their rows, world 3 in the first step after its pause
  hashes = a.hash_states(bank)
  assert got["hashes"][16, 0] == hashes[rows[0]] and got["hashes"][20, 3] == hashes[rows[3]], name
  assert torch.equal(got["hashes"][15:20, 3], got["hashes"][15, 3].expand(5)), name
  # the loop form: rows[3] rewritten while world 3 is paused on LAST; it starts from the row written last
  first, last = [r for r in (info["mid"] + 1, info["mid"] + 2, info["mid"] + 4) if r != rows[3]][:2]   # after step 8
  assert len({int(hashes[first]), int(hashes[last]), int(hashes[rows[3]])}) == 3
  for k in range(K):
    if k == 17:
      drows[2][3] = first
    if k == 19:
      drows[2][3] = last
    c.step(A[k], active=M[k])
    if k == 20:
      assert c.hash_worlds()[3] == hashes[last], name
      assert int(c.observe(E.OBS_STEP_TYPE)[3]) == 0, name
  # -1 everywhere is the level's own reset: the masked request of an engine without a registration
  d, plain = _engine(name), _engine(name)
  minus = torch.full((N,), -1, dtype=torch.int32, device=d.device)
  d.set_episode_starts(bank, minus)
  got = d.step_many(A, active=M, **_all_rows(obs))
  ref = plain.step_many(A, active=M, **_all_rows(obs))
  for key in ref:
    for k in range(K) if key == "events" else (slice(None),):
      _same(got[key][k], ref[key][k], key, (name, "-1", k))
  _same_engines(d, plain, obs, (name, "-1"))
  _close(a, b, c, d, plain)


# ---- 8. refusals ----------------------------------------------------------------------------------
def test_refusals():
  name = "coins"
  e = _engine(name)
  A = _actions(e)
  e.step_many(A[:3])
  ones = torch.ones((K, N), dtype=torch.uint8, device=e.device)
  hashed, counters = e.hash_worlds().clone(), e.counters()

  def raw(eng, size=None, **kw):
    req = E.MpStepActive(ctypes.sizeof(E.MpStepActive), K, 0, 0)
    req.actions, req.actions_step_bytes = A.data_ptr(), A.stride(0) * 4
    req.active, req.active_step_bytes = ones.data_ptr(), N
    for key, value in kw.items():
      setattr(req, key, value)
    return eng._L.mp_restore(eng._h, ctypes.addressof(req), ctypes.sizeof(req) if size is None else size)

  def untouched(what):
    assert torch.equal(e.hash_worlds(), hashed) and e.counters() == counters, what

  assert raw(e, struct_size=88) == E.MP_ERR_INVALID                      # a wrong struct_size
  assert b"MpStepActive: struct_size" in e._L.mp_last_error()
  assert raw(e, active=None) == E.MP_ERR_INVALID
  assert raw(e, active_step_bytes=N - 1) == E.MP_ERR_INVALID             # rows that overlap
  assert b"active_step_bytes" in e._L.mp_last_error()
  host = np.ones((K, N), np.uint8)
  assert raw(e, active=host.ctypes.data) == E.MP_ERR_INVALID             # a host pointer
  assert raw(e, reserved=(ctypes.c_uint64 * 5)(0, 0, 1, 0, 0)) == E.MP_ERR_INVALID
  assert b"reserved" in e._L.mp_last_error()
  assert raw(e, steps=0) == E.MP_ERR_INVALID and raw(e, steps=E.STEP_MANY_MAX + 1) == E.MP_ERR_INVALID
  untouched("invalid requests")
  # an extent that runs past its allocation: K - 1 rows of device memory, `stride` apart, asked for K
  # steps (one allocation of the library's own: no caching allocator rounds it up)
  stride, steps = 2 << 20, 3
  ptr = ctypes.c_void_p()
  assert e._L.mp_alloc_output(e.device.index or 0, (steps - 1) * stride, 0, ctypes.byref(ptr)) == 0
  try:
    short = dict(active=ptr.value, active_step_bytes=stride)
    assert raw(e, steps=steps, **short) == E.MP_ERR_INVALID
    assert b"MpStepActive (active)" in e._L.mp_last_error() and b"past the end" in e._L.mp_last_error()
    untouched("a short mask")
  finally:
    e._L.mp_free_output(e.device.index or 0, ptr)
  with pytest.raises(ValueError, match="active="):                        # the Python check, before the library
    e.step_many(A, active=ones[:K - 1])
  with pytest.raises(ValueError, match="lives on"):
    e.step_many(A, active=ones.cpu())
  untouched("the Python checks")
  # a ring bound
  e.bind_ring(E.OBS_REWARD, slots=4, tune=False)
  assert raw(e) == -5 and b"ring" in e._L.mp_last_error()                 # MP_ERR_UNSUPPORTED
  with pytest.raises(engine.EngineError, match="ring"):
    e.step(A[0], active=ones[0])
  untouched("a ring")
  assert e.ring["next"] == 0
  _close(e)
  # an engine that promised one launch a step, with a view
  one = engine.Engine(R.pack(name), N, device=0, unfused=False)
  one.reset()
  assert raw(one) == 0                                                    # no view: the step kernels alone
  one.bind(E.OBS_WORLD_RGB)
  before = one.hash_worlds().clone()
  assert raw(one) == -5 and b"unfused" in one._L.mp_last_error()
  assert torch.equal(one.hash_worlds(), before)
  _close(one)
  # an engine never reset
  fresh = engine.Engine(R.pack(name), N, device=0)
  assert raw(fresh) == E.MP_ERR_INVALID and b"never been reset" in fresh._L.mp_last_error()
  _close(fresh)


# ---- 9. the Substrate surface and a mixture -------------------------------------------------------
def test_substrate_lengths_masks_and_refusals():
  name = KITCHEN
  roles = substrate.get_config(name).default_player_roles
  kw = dict(roles=roles, num_worlds=4, env_seed=5)
  envs = [substrate.build(name, **kw) for _ in range(4)]
  a, b, c, d = envs
  for env in envs:
    env.reset()
  n, P = 4, len(roles)
  rng = np.random.default_rng(3)
  A = rng.integers(0, a.action_spec()[0].num_values, size=(8, n, P)).astype(np.int32)
  lengths = torch.tensor([8, 0, 3, 5], device=a.engine.device)
  mask = torch.arange(8, device=a.engine.device)[:, None] < lengths[None]
  ra = a.step_many(A, lengths=lengths)
  rb = b.step_many(A, active=mask)                                   # bool
  rc = c.step_many(A, active=mask.to(torch.uint8) * 255)             # uint8 holding 0 / 255
  rd = d.step_many(A, active=mask.cpu().numpy())                     # a host array, uploaded once
  for other, r in ((b, rb), (c, rc), (d, rd)):
    assert torch.equal(a.hash_worlds(), other.hash_worlds())
    assert torch.equal(ra.reward, r.reward) and torch.equal(ra.step_type, r.step_type)
    assert a.engine.counters() == other.engine.counters()
  assert a.engine.counters()["world_steps"] == b.engine.counters()["world_steps"]
  # the rewards of skipped steps repeat: the return is summed under the mask
  returns = (ra.reward * mask[:, :, None]).sum(0)
  assert returns.shape == (n, P) and bool((returns[1] == 0).all())
  # the masked single step returns the usual TimeStep; a skipped world's elements are what they were
  before = ra.timestep.step_type.clone()
  assert before.tolist() == [1, 0, 1, 1]                             # world 1 never ran: FIRST
  ts = a.step(A[0], active=[False, True, False, False])
  tb = b.step(A[0], active=torch.tensor([0, 1, 0, 0], dtype=torch.uint8, device=b.engine.device))
  assert torch.equal(a.hash_worlds(), b.hash_worlds())
  assert torch.equal(ts.reward, tb.reward) and torch.equal(ts.step_type, tb.step_type)
  assert ts.step_type.tolist() == [1, 1, 1, 1]
  with pytest.raises(ValueError, match="not both"):
    a.step_many(A, active=mask, lengths=lengths)
  with pytest.raises(ValueError, match="lengths="):
    a.step_many(A, lengths=lengths[:3])
  with pytest.raises(ValueError, match="lengths="):
    a.step_many(A, lengths=lengths.double())
  with pytest.raises(ValueError, match="active="):
    a.step_many(A, active=mask.long())
  for env in envs:
    assert not env.engine.fault_words()[:6].any()
    env.close()
  single = substrate.build(name, roles=roles)
  single.reset()
  with pytest.raises(ValueError, match="num_worlds"):
    single.step([0] * P, active=[1])
  single.close()
  ring = substrate.build(name, rollout_length=4, **kw)
  ring.reset()
  with pytest.raises(ValueError, match="rollout ring"):
    ring.step_many(A, active=mask)
  with pytest.raises(ValueError, match="rollout ring"):
    ring.step(A[0], active=mask[0])
  with pytest.raises(ValueError, match="rollout ring"):
    ring.step_many(A, lengths=lengths)
  ring.close()


def test_a_mixture_hands_each_member_its_columns():
  names = (KITCHEN, "collaborative_cooking__asymmetric")
  kw = dict(num_worlds=16, env_seed=3, individual_observations=("POSITION",), global_observations=())
  mix = substrate.build_mixture(names, **kw)
  plain = substrate.build_mixture(names, **kw)
  mix.reset(); plain.reset()
  n, P = mix.num_worlds, mix.num_players
  rng = np.random.default_rng(11)
  dev = mix.engines[0].device
  A = torch.from_numpy(rng.integers(0, mix.action_spec()[0].num_values, size=(8, n, P)).astype(np.int32)).to(dev)
  M = torch.from_numpy(rng.random((8, n)) < 0.5).to(dev)
  M[:, 0], M[:, n - 1] = True, False
  r = mix.step_many(A, active=M, hashes=True)
  alone = []
  for i, member in enumerate(plain._members):
    sl = plain.member_slice(i)
    alone.append(member.step_many(A[:, sl], active=M[:, sl], hashes=True))
  assert torch.equal(mix.hash_worlds(), plain.hash_worlds())
  for i, part in enumerate(alone):
    sl = mix.member_slice(i)
    assert torch.equal(r.reward[:, sl], part.reward) and torch.equal(r.step_type[:, sl], part.step_type)
    assert torch.equal(r.hashes[:, sl], part.hashes)
  assert mix.counters() == plain.counters()
  # the masked single step, and lengths=
  ts = mix.step(A[0], active=M[0])
  for i, member in enumerate(plain._members):
    sl = plain.member_slice(i)
    member.step(A[0, sl], active=M[0, sl])
  assert torch.equal(mix.hash_worlds(), plain.hash_worlds())
  assert tuple(ts.step_type.shape) == (n,)
  lengths = torch.from_numpy(rng.integers(0, 9, size=n)).to(dev)
  mix.step_many(A, lengths=lengths)
  plain.step_many(A, active=torch.arange(8, device=dev)[:, None] < lengths[None])
  assert torch.equal(mix.hash_worlds(), plain.hash_worlds())
  with pytest.raises(ValueError, match="not both"):
    mix.step_many(A, active=M, lengths=lengths)
  for e in mix.engines + plain.engines:
    e.sync()
    assert not e.fault_words()[:6].any()
  mix.close(); plain.close()
