"""Stepping the worlds a device index list names (MpStepListed; Engine.step / Engine.step_many and
Substrate.step / Substrate.step_many with worlds=): the launch has one wave per ENTRY of the list, and
every per-call tensor has one column per entry.  The defining identity is the masked request over all
N worlds on a twin engine, with mask[k][worlds[i]] = active[k][i] and full_actions[k][worlds[i]] =
actions[k][i]: the records, counters, leaves and `stopped` are equal, and every per-call tensor is
the gather of the twin's.  On the recipe's packs (one per level kernel, episodes of 16 frames, five
worlds — two workgroups of the full launch, and a list of three is one partial workgroup — 24 seeded
steps).

Results of the checks that set bounds: none — every comparison here is for equal bits."""
import ctypes

import numpy as np
import pytest
import torch

import states_recipe as R
import util
from engine_model import ModelEngine
from meltingpot_amd import engine, substrate
from test_gpu_episode_starts import PIXEL_PACKS, _plan, _same_as_model, _same_events
from test_gpu_step_active import (KITCHEN, _actions, _all_rows, _close, _engine, _keys, _leaves,
                                  _obs_kinds, _same, _same_engines, _same_leaves)

pytestmark = pytest.mark.gpu

E = engine
N, K = R.N, R.STEPS
LAST, REWARD = E.MP_STOP_LAST, E.MP_STOP_REWARD
COMMONS = "commons_harvest__open"
WORLDS = [3, 0, 4]   # unsorted, and spanning the two workgroups of the twin's launch
NEW = ("stopped", "ran", "returns")


def _full(A, worlds, mask=None):
  """The twin's request of a listed one: actions [K, N, P] with A's columns scattered to their
  worlds (0 elsewhere) and the mask [K, N] (`mask`: active [K, M], None: all ones)."""
  full = torch.zeros((A.shape[0], N) + tuple(A.shape[2:]), dtype=A.dtype, device=A.device)
  active = torch.zeros((A.shape[0], N), dtype=torch.uint8, device=A.device)
  idx = torch.as_tensor(worlds, device=A.device, dtype=torch.long)
  full[:, idx] = A
  active[:, idx] = 1 if mask is None else mask.to(torch.uint8)
  return full, active


def _gathered(got, ref, worlds, what):
  """Every per-step tensor of `got` is the gather of the twin's."""
  idx = torch.as_tensor(worlds, device=next(iter(ref.values())).device, dtype=torch.long)
  for key in ref:
    if key in NEW:
      continue
    assert got[key].shape[:2] == (ref[key].shape[0], len(worlds)), (what, key, got[key].shape)
    for k in range(ref[key].shape[0]) if key == "events" else (slice(None),):
      want = ref[key][k][idx] if key == "events" else ref[key][:, idx]
      _same(got[key][k], want, key, (what, k))


def _snapshot(e, obs):
  s = _leaves(e, obs)
  s["states"], s["hashes"] = e.save_worlds().clone(), e.hash_worlds().clone()
  return s


def _untouched(e, before, obs, worlds, what):
  """Worlds `worlds` of `e` are byte-identical to the snapshot `before`: record, hash, leaves, events."""
  now = _snapshot(e, obs)
  idx = torch.as_tensor(worlds, device=e.device, dtype=torch.long)
  for key in now:
    _same(now[key][idx], before[key][idx], key, (what, "untouched"))


# ---- 1. identity with the masked twin, every level --------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_a_listed_request_is_the_gather_of_the_masked_twin(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  for e in (a, b):
    e.step_many(A[:3])           # (the in-place buffers hold something to carry)
  before = _snapshot(a, obs)
  counters = a.counters()
  mine = A[:, WORLDS].contiguous()
  full, mask = _full(mine, WORLDS)
  got = a.step_many(mine, worlds=torch.tensor(WORLDS, dtype=torch.int32, device=a.device), **_all_rows(obs))
  ref = b.step_many(full, active=mask, **_all_rows(obs))
  assert set(got) == set(ref), name
  assert tuple(got["states"].shape) == (K, 3, a.info.world_state_bytes) and tuple(got["hashes"].shape) == (K, 3)
  _gathered(got, ref, WORLDS, name)
  _same_engines(a, b, obs, name)
  _untouched(a, before, obs, [1, 2], name)
  assert a.counters() != counters, name
  # the worlds crossed an episode end, so a reset ran inside the call
  types = got["step_type"].cpu().numpy()
  assert (types[12] == 2).all() and (types[13] == 0).all(), (name, types[:, 0])
  _close(a, b)


# ---- 2. M = N and M = 1 -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", R.MATRIX])
def test_a_permutation_is_the_unmasked_request_and_one_entry(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  perm = [4, 2, 0, 3, 1]
  got = a.step_many(A[:, perm].contiguous(), worlds=perm, **_all_rows(obs))   # (a host list is uploaded once)
  ref = b.step_many(A, **_all_rows(obs))
  _gathered(got, ref, perm, name)
  _same_engines(a, b, obs, name)
  before = _snapshot(a, obs)
  one = A[:8, 2:3].contiguous()
  full, mask = _full(one, [2])
  got = a.step_many(one, worlds=np.array([2]), **_all_rows(obs))
  ref = b.step_many(full, active=mask, **_all_rows(obs))
  assert tuple(got["reward"].shape) == (8, 1, a.P)
  _gathered(got, ref, [2], (name, "one"))
  _same_engines(a, b, obs, (name, "one"))
  _untouched(a, before, obs, [0, 1, 3, 4], (name, "one"))
  _close(a, b)


# ---- 3. the loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", KITCHEN])
def test_step_many_is_the_loop_of_listed_steps(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  mine = A[:, WORLDS].contiguous()
  w = torch.tensor(WORLDS, dtype=torch.int32, device=a.device)
  idx = w.long()
  got = a.step_many(mine, worlds=w, **_all_rows(obs))
  for k in range(K):
    b.step(mine[k] if k % 2 else mine[k].cpu().numpy(), worlds=w if k % 3 else WORLDS)
    row = _snapshot(b, obs)
    for key in got:
      _same(got[key][k], row[key][idx], key, (name, k))
  _same_engines(a, b, obs, name)
  _close(a, b)


# ---- 4. with a mask, stop conditions, sums and `stopped` -------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", COMMONS, R.MATRIX])
def test_mask_until_returns_and_stopped_against_the_twin(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  dev = a.device
  worlds = [3, 0, 4, 1]
  mine = A[:, worlds].contiguous()
  active = torch.from_numpy((np.random.default_rng(4).random((K, 4)) < 0.7).astype(np.uint8)).to(dev)
  active[:, 0] = 1                      # (entry 0, world 3: every step, so it stops on LAST)
  entry = torch.tensor([0, 2, 1, 0, 0], dtype=torch.uint8, device=dev)   # world 1 listed, world 2 unlisted
  full, mask = _full(mine, worlds, active)
  sa, sb = entry.clone(), entry.clone()
  kw = dict(until=("last", "reward"), returns=True, gamma=0.99)
  got = a.step_many(mine, worlds=worlds, active=active, stopped=sa, **kw, **_all_rows(obs))
  ref = b.step_many(full, active=mask, stopped=sb, **kw, **_all_rows(obs))
  assert set(got) == set(ref) and got["stopped"] is sa
  _gathered(got, ref, worlds, name)
  _same_engines(a, b, obs, name)
  idx = torch.tensor(worlds, device=dev)
  assert tuple(got["ran"].shape) == (4,) and tuple(got["returns"].shape) == (4, a.P) and tuple(sa.shape) == (N,)
  assert torch.equal(got["ran"], ref["ran"][idx]), (name, got["ran"], ref["ran"])
  assert torch.equal(got["returns"].view(torch.int64), ref["returns"][idx].view(torch.int64)), name
  assert torch.equal(sa, sb), (name, sa, sb)
  # `stopped` is by world: the bytes on entry are kept (world 1 ran nothing), the unlisted world's too,
  # and only listed worlds that stopped were written
  s = sa.tolist()
  assert s[1] == 2 and s[2] == 1 and int(got["ran"][3]) == 0, (name, s, got["ran"])
  assert s[3] != 0 and int(got["ran"][0]) >= 1, (name, s)
  _close(a, b)


@pytest.mark.parametrize("name", ["clean_up", R.MATRIX])
def test_an_entry_that_runs_nothing_carries_its_rows_to_its_own_column(name):
  """Eight worlds, worlds = [5, 2, 7], K = 3, entry 1's column of the mask all zero, and no row that
  needs the record (the five kinds, the level's kinds of READY_TO_SHOOT, AUX0, POSITION and
  ORIENTATION, and on the matrix pack one level kind): the wave of entry 1 loads no record and writes
  column 1 of every row from world 2's in-place buffers — where the shifted row bases and the level
  copy's column meet with no step run."""
  n, worlds, steps = 8, [5, 2, 7], 3
  obs = _obs_kinds(name)
  fin = tuple(k for k in (E.OBS_READY_TO_SHOOT, E.OBS_AUX0, E.OBS_POSITION, E.OBS_ORIENTATION) if k in obs)
  level = tuple(k for k in (E.OBS_INTERACTION_REWARDS,) if k in obs)
  assert fin and (level or name != R.MATRIX), (name, obs)
  a, b = [engine.Engine(R.pack(name), n, device=0, debug_observations=True) for _ in range(2)]
  A = torch.from_numpy(R.actions(a.P, a.num_actions, n=n)).to(a.device)
  for e in (a, b):
    e.reset()
    e.step_many(A[:3])           # (the in-place buffers hold something to carry)
  before = _snapshot(a, obs)
  idx = torch.tensor(worlds, device=a.device)
  mine = A[3:3 + steps, idx].contiguous()
  active = torch.ones((steps, 3), dtype=torch.uint8, device=a.device)
  active[:, 1] = 0
  full = torch.zeros_like(A[:steps])
  full[:, idx] = mine
  mask = torch.zeros((steps, n), dtype=torch.uint8, device=a.device)
  mask[:, idx] = active
  got = a.step_many(mine, worlds=worlds, active=active, events=True, observations=fin + level)
  ref = b.step_many(full, active=mask, events=True, observations=fin + level)
  assert set(got) == set(ref) and all(key in got for key, _ in _keys(fin + level)), (name, sorted(map(str, got)))
  _gathered(got, ref, worlds, name)
  for key, _ in _keys(fin + level):     # (and without the twin: every row of entry 1 is world 2's buffer)
    for k in range(steps):
      _same(got[key][k][1:2], before[key][2:3], key, (name, "carried", k))
  _same_engines(a, b, obs, name)
  _untouched(a, before, obs, [0, 1, 2, 3, 4, 6], name)
  _close(a, b)


def test_seventy_steps_with_lengths_through_the_substrate():
  """K = 70 by repeat=70: steps past 64 are the second bit of a lane's part of the mask column."""
  config = substrate.get_config(COMMONS)
  roles = config.default_player_roles
  a, b = [substrate.Substrate(config, roles, R.pack(COMMONS), num_worlds=N, env_seed=5) for _ in range(2)]
  a.reset(); b.reset()
  dev = a.engine.device
  P = len(roles)
  block = torch.from_numpy(R.actions(P, a.action_spec()[0].num_values)[0]).to(dev)
  mine = block[WORLDS].contiguous()
  lengths = torch.tensor([70, 66, 9], device=dev)
  full = torch.zeros((N, P), dtype=block.dtype, device=dev)
  full[WORLDS] = mine
  every = torch.zeros(N, dtype=torch.int64, device=dev)
  every[WORLDS] = lengths
  r = a.step_many(mine, repeat=70, lengths=lengths, worlds=WORLDS, returns=True, gamma=0.99, hashes=True)
  t = b.step_many(full, repeat=70, lengths=every, returns=True, gamma=0.99, hashes=True)
  assert isinstance(r, substrate.StepManyUntil)
  assert tuple(r.reward.shape) == (70, 3, P) and tuple(r.hashes.shape) == (70, 3)
  assert r.ran.tolist() == [70, 66, 9] and torch.equal(r.ran, t.ran[WORLDS])
  assert torch.equal(r.returns.view(torch.int64), t.returns[WORLDS].view(torch.int64))
  for field in ("step_type", "reward", "discount", "collective_reward"):
    assert torch.equal(getattr(r, field), getattr(t, field)[:, WORLDS]), field
  assert torch.equal(r.hashes, t.hashes[:, WORLDS])
  assert bool((r.hashes[65] != r.hashes[64])[:2].all()) and r.hashes[66, 1] == r.hashes[65, 1]
  assert torch.equal(a.hash_worlds(), b.hash_worlds()) and a.engine.counters() == b.engine.counters()
  assert tuple(r.timestep.step_type.shape) == (N,) and torch.equal(r.timestep.reward, t.timestep.reward)
  for env in (a, b):
    util.no_faults(env.engine, sync=True)
    env.close()


# ---- 5. registered episode starts -------------------------------------------------------------------
@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("name", ["clean_up", KITCHEN])
def test_registered_episode_starts_against_the_twin(name, fresh):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  bank, rows, info = _plan(a, name)
  A = _actions(a)
  for e in (a, b):
    e.set_episode_starts(bank, torch.from_numpy(rows).to(e.device), fresh=fresh)   # (rows [N]: by world)
  mine = A[:, WORLDS].contiguous()
  full, mask = _full(mine, WORLDS)
  got = a.step_many(mine, worlds=WORLDS, **_all_rows(obs))
  ref = b.step_many(full, active=mask, **_all_rows(obs))
  _gathered(got, ref, WORLDS, (name, fresh))
  _same_engines(a, b, obs, (name, fresh))
  # the listed worlds crossed an episode end and started from their own rows (worlds 3, 0, 4)
  assert (got["step_type"][15] == 2).all() and rows[3] >= 0 and rows[0] >= 0
  if not fresh:
    hashes = a.hash_states(bank)
    assert got["hashes"][16, 0] == hashes[rows[3]] and got["hashes"][16, 1] == hashes[rows[0]], name
  _close(a, b)


# ---- 6. an anchor that does not lean on the GPU twin ------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up"])
def test_a_listed_run_against_the_oracle(name):
  e = engine.Engine(R.pack(name), N, device=0)
  m = ModelEngine(R.pack(name), N, auto_reset=True)
  e.reset(); m.reset()
  A = R.actions(e.P, e.num_actions)
  mine = np.ascontiguousarray(A[:, WORLDS])
  mask = np.zeros((K, N), np.uint8)
  mask[:, WORLDS] = 1
  full = np.zeros_like(A)
  full[:, WORLDS] = mine
  record = tuple(k for k in m.record_scalars)
  got = e.step_many(torch.from_numpy(mine).to(e.device), worlds=WORLDS, events=True, observations=record)
  ref = m.step_many(full, active=mask, events=True, observations=record)
  for key in ("reward", "collective_reward", "step_type", "discount") + record:
    assert np.array_equal(got[key].cpu().numpy(), ref[key][:, WORLDS]), (name, key)
  for k in range(K):
    _same_events(got["events"][k].cpu().numpy(), ref["events"][k][WORLDS], (name, "row", k))
  _same_as_model(e, m, name)
  _close(e)
  m.close()


# ---- 7. bad entries ---------------------------------------------------------------------------------
def test_bad_entries_run_nothing_and_are_reported_once():
  name = "clean_up"
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  dev = a.device
  worlds = torch.tensor([2, 7, 2, -1, 1], dtype=torch.int32, device=dev)
  good = [0, 4]                                         # entries 0 and 4: worlds 2 and 1
  mine = A[:, [2, 0, 3, 4, 1]].contiguous()
  before = _snapshot(a, obs)
  # every per-call tensor pre-filled with a sentinel (a third engine's call gives the shapes)
  c = _engine(name)
  shapes = c.step_many(mine, worlds=[0, 1, 2, 3, 4], returns=True, **_all_rows(obs))
  out = {key: torch.full_like(tensor, 77) for key, tensor in shapes.items() if key != "stopped"}
  _close(c)
  sentinel = {key: tensor.clone() for key, tensor in out.items()}
  got = a.step_many(mine, worlds=worlds, returns=out["returns"], out=out, **_all_rows(obs))
  full = torch.zeros_like(A)
  full[:, [2, 1]] = mine[:, good]
  mask = torch.zeros((K, N), dtype=torch.uint8, device=dev)
  mask[:, [2, 1]] = 1
  ref = b.step_many(full, active=mask, returns=True, **_all_rows(obs))
  with pytest.raises(ValueError, match="MpStepListed") as info:
    a.sync()
  assert "worlds[" in str(info.value), info.value
  a.sync()                                              # reported once
  assert not a.fault_words()[:10].any()
  for key in ref:
    if key == "stopped":
      continue
    g, r = got[key], ref[key]
    assert g is out[key], key
    if key in ("ran", "returns"):
      assert torch.equal(g[good], r[[2, 1]]), key
      assert torch.equal(g[1:4], sentinel[key][1:4]), key
    else:
      for k in range(K) if key == "events" else (slice(None),):
        _same(g[k][good] if key == "events" else g[:, good], r[k][[2, 1]] if key == "events" else r[:, [2, 1]],
              key, ("bad entries", k))
      assert torch.equal(g[:, 1:4], sentinel[key][:, 1:4]), key
  _same_engines(a, b, obs, "bad entries")
  _untouched(a, before, obs, [0, 3, 4], "bad entries")
  # the engine stays usable: the next listed call runs
  nxt = a.step_many(mine[:2, :3].contiguous(), worlds=WORLDS)
  full, mask = _full(mine[:2, :3].contiguous(), WORLDS)
  ref = b.step_many(full, active=mask)
  _gathered(nxt, ref, WORLDS, "next")
  _same_engines(a, b, obs, "next")
  _close(a, b)


# ---- 8. views ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PIXEL_PACKS)
def test_views_are_redrawn_and_the_engine_stays_fused(name):
  views = (E.OBS_RGB, E.OBS_WORLD_RGB)
  a = engine.Engine(R.pack(name), N, device=0)
  b = engine.Engine(R.pack(name), N, device=0)
  for e in (a, b):
    for kind in views:
      e.bind(kind).zero_()
    e.reset()
  A = _actions(a)
  mine = A[:, WORLDS].contiguous()
  full, mask = _full(mine, WORLDS)
  fused = a.fused
  a.step(mine[0], worlds=WORLDS); b.step(full[0], active=mask[0])
  for kind in views:
    assert torch.equal(a._bound[kind], b._bound[kind]), (name, kind, "step")
  a.step_many(mine[1:9], worlds=WORLDS); b.step_many(full[1:9], active=mask[1:9])
  for kind in views:
    assert torch.equal(a._bound[kind], b._bound[kind]), (name, kind)
  assert a.fused == fused
  # the next unlisted step is the step it was
  a.step(A[9]); b.step(A[9])
  assert torch.equal(a.hash_worlds(), b.hash_worlds())
  for kind in views:
    assert torch.equal(a._bound[kind], b._bound[kind]), (name, kind, "after")
  _close(a, b)


# ---- 9. refusals ------------------------------------------------------------------------------------
def test_refusals():
  name = "coins"
  e = _engine(name)
  A = _actions(e)
  e.step_many(A[:3])
  dev = e.device
  M = 3
  mine = A[:, WORLDS].contiguous()
  w = torch.tensor(WORLDS, dtype=torch.int32, device=dev)
  ones = torch.ones((K, M), dtype=torch.uint8, device=dev)
  stopped = torch.zeros(N, dtype=torch.uint8, device=dev)
  ran = torch.zeros(M, dtype=torch.int32, device=dev)
  ret = torch.zeros((M, e.P), dtype=torch.float64, device=dev)
  saved, counters = e.save_worlds().clone(), e.counters()

  def raw(eng, **kw):
    req = E.MpStepListed(ctypes.sizeof(E.MpStepListed), K, 0, 0)
    req.actions, req.actions_step_bytes = mine.data_ptr(), mine.stride(0) * 4
    req.active, req.active_step_bytes = ones.data_ptr(), M
    req.stop, req.gamma = LAST, 1.0
    req.stopped, req.ran, req.returns = stopped.data_ptr(), ran.data_ptr(), ret.data_ptr()
    req.worlds, req.count = w.data_ptr(), M
    for key, value in kw.items():
      setattr(req, key, value)
    return eng._L.mp_restore(eng._h, ctypes.addressof(req), ctypes.sizeof(req))

  def untouched(what):
    assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, what
    assert not stopped.any() and not ran.any() and not ret.any(), what

  def invalid(field, **kw):
    assert raw(e, **kw) == E.MP_ERR_INVALID, kw
    message = e._L.mp_last_error()
    assert b"MpStepListed" in message and field in message, (kw, message)

  invalid(b"NULL worlds", worlds=None)
  invalid(b"count", count=0)
  invalid(b"count", count=N + 1)
  invalid(b"4-byte", worlds=w.data_ptr() + 2)
  invalid(b"(worlds)", worlds=np.array(WORLDS, np.int32).ctypes.data)     # host memory
  invalid(b"reserved", reserved2=1)
  invalid(b"reserved", reserved3=(ctypes.c_uint64 * 3)(0, 1, 0))
  invalid(b"pad", pad=1)
  invalid(b"stop", stop=4)
  invalid(b"gamma", gamma=float("inf"))
  invalid(b"overlaps", worlds=ran.data_ptr())
  invalid(b"overlaps", ran=w.data_ptr())
  invalid(b"overlaps", stopped=w.data_ptr())
  rows = (E.MpStepRow * 1)()
  rows[0].kind, rows[0].rows, rows[0].step_bytes = E.OBS_STEP_TYPE, w.data_ptr(), 4 * M
  invalid(b"overlaps", rows=rows, num_rows=1, steps=1)
  # extents sized for M where the list is longer: actions of 3 columns for a count of 5 run past their end
  size = 2 << 20
  ptr = ctypes.c_void_p()
  assert e._L.mp_alloc_output(dev.index or 0, size, 0, ctypes.byref(ptr)) == 0
  try:
    end = ptr.value + size
    for field, kw in ((b"(ran)", dict(ran=end - 4 * M + 4)), (b"(returns)", dict(returns=end - 8)),
                      (b"(worlds)", dict(worlds=end - 4)), (b"(active)", dict(active=end - M + 1, active_step_bytes=0,
                                                                                    steps=1)),
                      (b"(actions)", dict(actions=end - mine[0].numel() * 4 + 4, steps=1))):
      invalid(field, **kw)
    untouched("short extents")
  finally:
    e._L.mp_free_output(dev.index or 0, ptr)
  untouched("invalid requests")
  # the Python checks, before the library
  for kw, match in ((dict(worlds=w.float()), "worlds="), (dict(worlds=w[None]), "worlds="),
                    (dict(worlds=[]), "names no world"), (dict(worlds=[0, 1, 2, 3, 4, 0]), "more entries"),
                    (dict(worlds=w.cpu()), "lives on"), (dict(worlds=w, active=torch.ones((K, N), dtype=torch.uint8,
                                                                                          device=dev)), "active="),
                    (dict(worlds=w, returns=torch.zeros((N, e.P), dtype=torch.float64, device=dev)), "returns="),
                    (dict(worlds=w, out={"reward": torch.zeros((K, N, e.P), dtype=torch.float64, device=dev)}),
                     "out")):
    with pytest.raises(ValueError, match=match):
      e.step_many(mine, **kw)
  with pytest.raises(ValueError, match="shape"):
    e.step_many(A, worlds=w)              # actions sized for N
  with pytest.raises(ValueError, match="shape"):
    e.step(A[0], worlds=w)
  untouched("the Python checks")
  # an int64 list of the device is converted once, as save_worlds does
  e.step_many(mine[:1], worlds=w.long())
  assert not torch.equal(e.save_worlds(), saved)
  saved, counters = e.save_worlds().clone(), e.counters()
  # a ring bound
  e.bind_ring(E.OBS_REWARD, slots=4, tune=False)
  assert raw(e) == -5 and b"ring" in e._L.mp_last_error() and b"MpStepListed" in e._L.mp_last_error()
  with pytest.raises(engine.EngineError, match="ring"):
    e.step_many(mine, worlds=w)
  untouched("a ring")
  _close(e)
  # an engine that promised one launch a step, with a view
  one = engine.Engine(R.pack(name), N, device=0, unfused=False)
  one.reset()
  one.bind(E.OBS_WORLD_RGB)
  before = one.hash_worlds().clone()
  assert raw(one) == -5 and b"unfused" in one._L.mp_last_error()
  assert torch.equal(one.hash_worlds(), before) and not stopped.any()
  _close(one)
  # a one-world substrate, a substrate with a ring, and a mixture
  config = substrate.get_config(COMMONS)
  roles = config.default_player_roles
  single = substrate.Substrate(config, roles, R.pack(COMMONS))
  single.reset()
  with pytest.raises(ValueError, match="num_worlds"):
    single.step([0] * len(roles), worlds=[0])
  with pytest.raises(ValueError, match="num_worlds"):
    single.step_many(np.zeros((2, 1, len(roles)), np.int32), worlds=[0])
  single.close()
  ring = substrate.Substrate(config, roles, R.pack(COMMONS), num_worlds=N, rollout_length=4)
  ring.reset()
  with pytest.raises(ValueError, match="rollout ring"):
    ring.step_many(np.zeros((2, 3, len(roles)), np.int32), worlds=WORLDS)
  ring.close()
  mix = substrate.build_mixture((KITCHEN, "collaborative_cooking__asymmetric"), num_worlds=8, env_seed=3,
                                individual_observations=("POSITION",), global_observations=())
  mix.reset()
  hashed = mix.hash_worlds().clone()
  acts = np.zeros((2, 3, mix.num_players), np.int32)
  with pytest.raises(ValueError, match="mixture"):
    mix.step_many(acts, worlds=WORLDS)
  with pytest.raises(ValueError, match="mixture"):
    mix.step(acts[0], worlds=WORLDS)
  assert torch.equal(mix.hash_worlds(), hashed)
  mix.close()


# ---- 10. the Substrate surface ----------------------------------------------------------------------
def test_substrate_surface():
  config = substrate.get_config(COMMONS)
  roles = config.default_player_roles
  a, b = [substrate.Substrate(config, roles, R.pack(COMMONS), num_worlds=N, env_seed=5) for _ in range(2)]
  a.reset(); b.reset()
  dev = a.engine.device
  P = len(roles)
  A = torch.from_numpy(R.actions(P, a.action_spec()[0].num_values)).to(dev)
  mine = A[:, WORLDS].contiguous()
  full, mask = _full(mine, WORLDS)
  w = torch.tensor(WORLDS, dtype=torch.int32, device=dev)
  ts = a.step(mine[0], worlds=w)
  ref = b.step(full[0], active=mask[0])
  assert tuple(ts.step_type.shape) == (N,) and tuple(ts.reward.shape) == (N, P)
  assert torch.equal(ts.step_type, ref.step_type) and torch.equal(ts.reward, ref.reward)
  for leaf in ts.observation:
    assert torch.equal(ts.observation[leaf], ref.observation[leaf]), leaf
  assert ts.step_type.tolist() == [1, 0, 0, 1, 1]
  r = a.step_many(mine[1:9], worlds=WORLDS, states=True, hashes=True, observations=("READY_TO_SHOOT",))
  t = b.step_many(full[1:9], active=mask[1:9], states=True, hashes=True, observations=("READY_TO_SHOOT",))
  assert isinstance(r, substrate.StepManyTrajectory) and not isinstance(r, substrate.StepManyUntil)
  assert tuple(r.reward.shape) == (8, 3, P) and tuple(r.observation["READY_TO_SHOOT"].shape)[:2] == (8, 3)
  assert torch.equal(r.reward, t.reward[:, WORLDS]) and torch.equal(r.hashes, t.hashes[:, WORLDS])
  assert torch.equal(r.observation["READY_TO_SHOOT"], t.observation["READY_TO_SHOOT"][:, WORLDS])
  assert tuple(r.timestep.step_type.shape) == (N,) and torch.equal(r.timestep.reward, t.timestep.reward)
  assert len(r.states) == 8 * 3
  # step k of entry i is row k * M + i: it loads with load_state and draws with observe_states
  rows = [5 * 3 + 0, 5 * 3 + 2]                         # after step 5 of the call: worlds 3 and 4
  picked = r.states[rows]
  assert torch.equal(picked.data, t.states.data[[5 * N + 3, 5 * N + 4]])
  drawn, want = a.observe_states(picked), b.observe_states(t.states[[5 * N + 3, 5 * N + 4]])
  assert drawn and set(drawn) == set(want)
  for leaf in drawn:
    assert torch.equal(drawn[leaf], want[leaf]), leaf
  b.load_state(picked, [-1, 0, 1, -1, -1])
  assert torch.equal(b.hash_worlds()[[1, 2]], r.hashes[5, [0, 2]])
  for env in (a, b):
    util.no_faults(env.engine, sync=True)
    env.close()
