"""Stopping worlds inside step_many (MpStepUntil; Engine.step_many with until=, stopped=, returns=,
gamma=): a world that a step leaves on LAST, or pays, stops there for the rest of the call.  The
defining identity is the loop of the merged masked single step, step(A[k], active=M[k] & ~done), on a
twin engine, with `done` updated on the host from what each step left.  On the recipe's packs (one per
level kernel, episodes of 16 frames, five worlds, 24 seeded steps) under the fixed mask of
test_gpu_step_active: world 0 is active throughout (it stops on LAST at step 15), world 1 never,
world 2 on even k (12 steps, it never stops), world 3 for k < 16 and from k = 20 (it stops at step 15
and so skips the steps from 20 on, in which the plain masked request resets it), world 4 at random.

Results of the checks that set bounds: none — every comparison here is for equal bits."""
import ctypes

import numpy as np
import pytest
import torch

import states_recipe as R
from engine_model import ModelEngine
from meltingpot_amd import engine, substrate
from test_gpu_episode_starts import PIXEL_PACKS, _plan, _same_as_model, _same_events
from test_gpu_step_active import (KITCHEN, MASK, _actions, _all_rows, _close, _engine, _keys,
                                  _leaves, _obs_kinds, _same, _same_engines, _same_leaves, _same_rows)

pytestmark = pytest.mark.gpu

E = engine
N, K = R.N, R.STEPS
LAST, REWARD = E.MP_STOP_LAST, E.MP_STOP_REWARD
COMMONS, MUSHROOMS = "commons_harvest__open", "externality_mushrooms__dense"
NEW = ("stopped", "ran", "returns")


def _rows_equal(got, ref, what):
  """Every per-step tensor of `ref` against `got`'s."""
  for key in ref:
    if key in NEW:
      continue
    for k in range(ref[key].shape[0]) if key == "events" else (slice(None),):
      _same(got[key][k], ref[key][k], key, (what, k))


def _until_loop(b, A, M, obs, stop, stopped=None):
  """The identity's right-hand side on `b`: the loop of the merged step(A[k], active=m_k) with m_k =
  M[k] & (stopped == 0), `stopped` updated after every step from STEP_TYPE and REWARD of the worlds
  that ran it.  Returns (rows as _masked_loop gives them, ran, stopped)."""
  dev = b.device
  stopped = torch.zeros(N, dtype=torch.uint8, device=dev) if stopped is None else stopped.clone()
  ran = torch.zeros(N, dtype=torch.int32, device=dev)
  rows = []
  for k in range(A.shape[0]):
    m = stopped == 0
    if M is not None:
      m = m & (M[k] != 0)
    b.step(A[k], active=m)
    row = _leaves(b, obs)
    row["states"], row["hashes"] = b.save_worlds().clone(), b.hash_worlds().clone()
    rows.append(row)
    reason = torch.zeros(N, dtype=torch.uint8, device=dev)
    if stop & LAST:
      reason |= (m & (row["step_type"] == 2)).to(torch.uint8) * LAST
    if stop & REWARD:
      reason |= (m & (row["reward"] != 0).any(1)).to(torch.uint8) * REWARD
    stopped = torch.where(reason != 0, reason, stopped)
    ran += m.to(torch.int32)
  return rows, ran, stopped


def _definition(reward, steps, gamma):
  """returns by its definition, in numpy float64: `reward` [K, N, P]; `steps`: bool [K, N], the steps
  that ran."""
  ret = np.zeros(reward.shape[1:], np.float64)
  for w in range(reward.shape[1]):
    g = np.float64(1.0)
    for k in range(reward.shape[0]):
      if steps[k, w]:
        ret[w] = ret[w] + g * reward[k, w]
        g = g * np.float64(gamma)
  return ret


def _same_bits(got, ref, what):
  got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
  assert got.dtype == np.float64 and ref.dtype == np.float64 and got.shape == ref.shape, what
  assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (what, got, ref)


def _ran_steps(M, ran):
  """bool [K, N]: the steps that ran, given the mask (None: all ones) and how many ran — a world runs
  its active steps in order until it stops."""
  M = np.ones((K, N), bool) if M is None else np.asarray(M) != 0
  return M & (M.cumsum(0) <= np.asarray(ran)[None])


# ---- 1. nothing to stop on: the masked request ------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_nothing_to_stop_on_is_the_masked_request(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  stopped = torch.zeros(N, dtype=torch.uint8, device=a.device)
  got = a.step_many(A, active=M, stopped=stopped, returns=True, **_all_rows(obs))
  ref = b.step_many(A, active=M, **_all_rows(obs))
  assert set(got) == set(ref) | set(NEW)
  _rows_equal(got, ref, name)
  _same_engines(a, b, obs, name)
  assert got["stopped"] is stopped and not stopped.any(), name
  assert got["ran"].dtype == torch.int32 and got["ran"].tolist() == MASK.sum(0).tolist(), name
  _same_bits(got["returns"], _definition(ref["reward"].cpu().numpy(), MASK != 0, 1.0), name)
  _close(a, b)


def test_no_mask_is_the_unmasked_request_and_a_long_mask_column():
  name = "clean_up"
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  got = a.step_many(A, returns=True, **_all_rows(obs))           # active=None: all ones
  ref = b.step_many(A, **_all_rows(obs))
  _rows_equal(got, ref, name)
  _same_engines(a, b, obs, name)
  assert got["ran"].tolist() == [K] * N and not got["stopped"].any()
  # K = 72: the mask column spans two 64-bit words of a lane
  long_actions = A.repeat(3, 1, 1)
  mask = torch.from_numpy((np.random.default_rng(72).random((3 * K, N)) < 0.5).astype(np.uint8)).to(a.device)
  got = a.step_many(long_actions, active=mask, returns=True, **_all_rows(obs))
  ref = b.step_many(long_actions, active=mask, **_all_rows(obs))
  _rows_equal(got, ref, (name, 72))
  _same_engines(a, b, obs, (name, 72))
  assert got["ran"].tolist() == mask.sum(0).tolist()
  assert int(mask[64:].sum()) > 0 and int((mask[64:] == 0).sum()) > 0
  _close(a, b)


# ---- 2. the identity --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_until_last_is_the_loop_of_masked_steps(name):
  obs = _obs_kinds(name)
  a, b, plain = _engine(name), _engine(name), _engine(name)
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  got = a.step_many(A, active=M, until="last", **_all_rows(obs))
  rows, ran, stopped = _until_loop(b, A, M, obs, LAST)
  _same_rows({k: v for k, v in got.items() if k not in NEW}, rows, name)
  _same_engines(a, b, obs, name)
  assert torch.equal(got["ran"], ran) and torch.equal(got["stopped"], stopped), (name, got["ran"], got["stopped"])
  # the coverage this test is there for
  types = got["step_type"].cpu().numpy()
  ran, stopped = ran.tolist(), stopped.tolist()
  assert ran[0] == 16 and stopped[0] == LAST and (types[15:, 0] == 2).all(), (name, types[:, 0])
  masked = plain.step_many(A, active=M)["step_type"].cpu().numpy()
  assert types[20, 3] == 2 and masked[20, 3] == 0 and stopped[3] == LAST, (name, types[:, 3], masked[:, 3])
  assert ran[2] == 12 and stopped[2] == 0 and ran[1] == 0 and stopped[1] == 0, (name, ran, stopped)
  _close(a, b, plain)


# ---- 3. until="reward" ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [COMMONS, MUSHROOMS])
def test_until_reward_is_the_loop_of_masked_steps(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  got = a.step_many(A, until="reward", **_all_rows(obs))
  rows, ran, stopped = _until_loop(b, A, None, obs, REWARD)
  _same_rows({k: v for k, v in got.items() if k not in NEW}, rows, name)
  _same_engines(a, b, obs, name)
  assert torch.equal(got["ran"], ran) and torch.equal(got["stopped"], stopped), (name, got["ran"], got["stopped"])
  ran, stopped = ran.tolist(), stopped.tolist()
  print(name, "ran", ran, "stopped", stopped)
  assert sum(1 for w in range(N) if stopped[w] == REWARD and ran[w] < K) >= 2, (name, ran, stopped)
  assert sum(1 for w in range(N) if stopped[w] == 0 and ran[w] == K) >= 1, (name, ran, stopped)
  # a stopped world stands on the step that paid it
  reward = got["reward"].cpu().numpy()
  for w in range(N):
    if stopped[w]:
      assert (reward[ran[w] - 1:, w] == reward[ran[w] - 1, w]).all() and (reward[ran[w] - 1, w] != 0).any(), (name, w)
      assert (reward[:ran[w] - 1, w] == 0).all(), (name, w)
  # both conditions together
  c, d = _engine(name), _engine(name)
  got = c.step_many(A, until=("last", "reward"), **_all_rows(obs))
  rows, ran, stopped = _until_loop(d, A, None, obs, LAST | REWARD)
  _same_rows({k: v for k, v in got.items() if k not in NEW}, rows, (name, "both"))
  _same_engines(c, d, obs, (name, "both"))
  assert torch.equal(got["ran"], ran) and torch.equal(got["stopped"], stopped), (name, got["ran"], got["stopped"])
  for w in range(N):
    assert int(stopped[w]) == (REWARD if int(ran[w]) < 16 else LAST), (name, ran, stopped)
  _close(a, b, c, d)


# ---- 4. returns -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1.0, 0.97])
def test_returns_are_the_definition_bit_for_bit(gamma):
  for until in (None, "last"):
    e = _engine(COMMONS)
    A = _actions(e)
    got = e.step_many(A, until=until, returns=True, gamma=gamma)
    reward, ran = got["reward"].cpu().numpy(), got["ran"].cpu().numpy()
    if until is None:
      assert ran.tolist() == [K] * N
      # (the discount shows only where a world is paid more than once)
      assert int(((reward != 0).any(2).sum(0) >= 2).sum()) >= 3, (reward != 0).any(2).sum(0)
    else:
      assert ran.tolist() == [16] * N and got["stopped"].tolist() == [LAST] * N
    _same_bits(got["returns"], _definition(reward, _ran_steps(None, ran), gamma), (gamma, until))
    _close(e)
  # under the mask, gamma = 1: the masked sum
  e = _engine(COMMONS)
  got = e.step_many(A, active=torch.from_numpy(MASK).to(e.device), returns=True, gamma=gamma)
  reward = got["reward"].cpu().numpy()
  _same_bits(got["returns"], _definition(reward, MASK != 0, gamma), (gamma, "mask"))
  if gamma == 1.0:
    _same_bits(got["returns"], (reward * MASK[:, :, None]).sum(0), "the masked sum")
  # a tensor of the caller's is written in place
  _close(e)
  e = _engine(COMMONS)
  mine = torch.full((N, e.P), float("nan"), dtype=torch.float64, device=e.device)
  again = e.step_many(A, active=torch.from_numpy(MASK).to(e.device), returns=mine, gamma=gamma)
  assert again["returns"] is mine and torch.equal(mine, got["returns"])
  _close(e)


# ---- 5. `stopped` persists --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", COMMONS])
def test_chunks_sharing_stopped_are_the_one_call(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  stop = ("last", "reward") if name == COMMONS else "last"
  whole = a.step_many(A, active=M, until=stop, returns=True)
  stopped = torch.zeros(N, dtype=torch.uint8, device=b.device)
  ran = torch.zeros(N, dtype=torch.int32, device=b.device)
  ret = torch.zeros((N, b.P), dtype=torch.float64, device=b.device)
  for lo in range(0, K, 8):
    part = b.step_many(A[lo:lo + 8], active=M[lo:lo + 8], until=stop, stopped=stopped, returns=True)
    assert part["stopped"] is stopped
    ran += part["ran"]
    ret += part["returns"]
  _same_engines(a, b, obs, name)
  assert torch.equal(stopped, whole["stopped"]) and torch.equal(ran, whole["ran"]), (name, stopped, ran)
  assert torch.equal(ret, whole["returns"]), name   # (gamma = 1, rewards that are small integers: exact)
  assert int(stopped[0]) != 0
  if name == "clean_up":
    # world 0, released, takes its reset in its first step
    assert int(b.observe(E.OBS_STEP_TYPE)[0]) == 2
    stopped[0] = 0
    entry = stopped.tolist()
    nxt = b.step_many(A[:2], until=stop, stopped=stopped)
    assert nxt["step_type"][:, 0].tolist() == [0, 1], nxt["step_type"][:, 0]
    assert nxt["ran"].tolist() == [0 if s else 2 for s in entry], (nxt["ran"], entry)   # (world 3 stays stopped)
    assert entry[3] == LAST and stopped.tolist()[3] == LAST
  _close(a, b)


@pytest.mark.parametrize("name", R.PACKS)
def test_everything_stopped_touches_nothing(name):
  obs = _obs_kinds(name)
  e = _engine(name)
  A = _actions(e)
  e.step_many(A[:3])
  saved, hashed, leaves, counters = e.save_worlds().clone(), e.hash_worlds().clone(), _leaves(e, obs), e.counters()
  stopped = torch.tensor([1, 2, 3, 255, 1], dtype=torch.uint8, device=e.device)
  ones = torch.ones((K, N), dtype=torch.uint8, device=e.device)
  for mask in (None, ones):
    ret = torch.full((N, e.P), float("nan"), dtype=torch.float64, device=e.device)
    got = e.step_many(A, active=mask, until=("last", "reward"), stopped=stopped, returns=ret, **_all_rows(obs))
    assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, name
    _same_leaves(e, leaves, obs, name)
    for key, _ in _keys(obs):
      for k in range(K):
        _same(got[key][k], leaves[key], key, (name, k))
    assert torch.equal(got["states"], saved[None].expand(K, -1, -1)), name
    assert torch.equal(got["hashes"], hashed[None].expand(K, -1)), name
    assert stopped.tolist() == [1, 2, 3, 255, 1] and got["ran"].tolist() == [0] * N, name
    assert torch.equal(ret, torch.zeros_like(ret)), name
  # (without a row that is a function of the record, such a world does not even load its record)
  light = tuple(k for k in obs if k != E.OBS_LAYER)
  got = e.step_many(A, until="last", stopped=stopped, returns=True, events=True, observations=light)
  for key, _ in _keys(light):
    for k in range(K):
      _same(got[key][k], leaves[key], key, (name, "light", k))
  assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, name
  _same_leaves(e, leaves, obs, (name, "light"))
  assert got["ran"].tolist() == [0] * N and not got["returns"].any(), name
  got = e.step_many(A, until="last", stopped=stopped, returns=True, keep=())   # no row at all
  assert torch.equal(e.save_worlds(), saved) and e.counters() == counters, name
  _same_leaves(e, leaves, obs, (name, "no rows"))
  assert got["ran"].tolist() == [0] * N and not got["returns"].any(), name
  _close(e)


# ---- 6. against the oracle --------------------------------------------------------------------------
# (the model with a stop state is ModelEngine's own: tests/engine_model.py)
@pytest.mark.parametrize("name", R.PACKS)
def test_step_many_against_the_oracle(name):
  views = (E.OBS_RGB, E.OBS_WORLD_RGB, E.OBS_LAYER) if name in PIXEL_PACKS else ()
  e = engine.Engine(R.pack(name), N, device=0)
  m = ModelEngine(R.pack(name), N, auto_reset=True)
  for kind in views:
    e.bind(kind).zero_()
    m.bind(kind)
  e.reset(); m.reset()
  fused = e.fused
  A = R.actions(e.P, e.num_actions)
  dA = torch.from_numpy(A).to(e.device)
  dM = torch.from_numpy(MASK).to(e.device)
  record = tuple(k for k in m.record_scalars)
  got = e.step_many(dA, active=dM, until=("last", "reward"), returns=True, gamma=0.97, events=True,
                    observations=record)
  ref = m.step_many(A, active=MASK, stop=LAST | REWARD, returns=True, gamma=0.97, events=True,
                    observations=record)
  for key in ("reward", "collective_reward", "step_type", "discount") + record:
    assert np.array_equal(got[key].cpu().numpy(), ref[key]), (name, key)
  for k in range(K):
    _same_events(got["events"][k].cpu().numpy(), ref["events"][k], (name, "row", k))
  assert got["ran"].tolist() == ref["ran"].tolist() and got["stopped"].tolist() == ref["stopped"].tolist(), name
  _same_bits(got["returns"], ref["returns"], name)
  _same_as_model(e, m, (name, "step_many"), views)
  assert e.fused == fused
  assert got["stopped"][0] != 0 and got["stopped"][1] == 0, (name, got["stopped"])
  # the next call, with the same bytes: the stopped worlds stay where they are, the others go on
  second = e.step_many(dA[:8], until=("last", "reward"), stopped=got["stopped"], events=True)
  ref2 = m.step_many(A[:8], stop=LAST | REWARD, stopped=ref["stopped"], events=True)
  assert second["ran"].tolist() == ref2["ran"].tolist() and second["stopped"].tolist() == ref2["stopped"].tolist()
  assert np.array_equal(second["step_type"].cpu().numpy(), ref2["step_type"]), name
  _same_as_model(e, m, (name, "second"), views)
  _close(e)
  m.close()


# ---- 7. row families one at a time ------------------------------------------------------------------
def test_step_many_rows_one_family_at_a_time():
  name = "clean_up"
  full = _engine(name)
  A = _actions(full)
  M = torch.from_numpy(MASK).to(full.device)
  ref = full.step_many(A, active=M, until="last", returns=True, observations=(E.OBS_LAYER,), states=True, hashes=True)
  for kw in ({}, {"keep": ()}, {"observations": (E.OBS_LAYER,)}, {"states": True}, {"hashes": True},
             {"keep": (), "observations": (E.OBS_POSITION,)}):
    e = _engine(name)
    got = e.step_many(A, active=M, until="last", returns=True, **kw)
    assert set(NEW) <= set(got), kw
    for key, value in got.items():
      if key in ref:
        assert torch.equal(value, ref[key]), (kw, key)
    assert torch.equal(e.save_worlds(), full.save_worlds()) and e.counters() == full.counters(), kw
    _close(e)
  _close(full)


# ---- 8. registered episode starts -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", KITCHEN])
def test_episode_starts_wait_for_a_stopped_world(name):
  obs = _obs_kinds(name)
  a, b = _engine(name), _engine(name)
  bank, rows, info = _plan(a, name)
  A = _actions(a)
  M = torch.from_numpy(MASK).to(a.device)
  for e in (a, b):
    e.set_episode_starts(bank, torch.from_numpy(rows).to(e.device))
  stopped = torch.zeros(N, dtype=torch.uint8, device=a.device)
  got = a.step_many(A, active=M, until="last", stopped=stopped, **_all_rows(obs))
  loop, ran, ref_stopped = _until_loop(b, A, M, obs, LAST)
  _same_rows({k: v for k, v in got.items() if k not in NEW}, loop, name)
  _same_engines(a, b, obs, name)
  assert torch.equal(got["ran"], ran) and torch.equal(stopped, ref_stopped), name
  # worlds 0 and 3 stopped on LAST and kept their hash through the call: no start was taken
  hashes = a.hash_states(bank)
  assert stopped.tolist()[0] == LAST and stopped.tolist()[3] == LAST
  for w in (0, 3):
    assert torch.equal(got["hashes"][15:, w], got["hashes"][15, w].expand(K - 15)), (name, w)
    assert got["hashes"][15, w] != hashes[rows[w]], (name, w)
  # ... and start from their rows in the first step of the next call that lets them run
  stopped.zero_()
  nxt = a.step_many(A[:2], until="last", stopped=stopped, hashes=True)
  assert rows[0] >= 0 and rows[3] >= 0
  assert nxt["hashes"][0, 0] == hashes[rows[0]] and nxt["hashes"][0, 3] == hashes[rows[3]], name
  _close(a, b)


# ---- 9. refusals ------------------------------------------------------------------------------------
def test_refusals():
  name = "coins"
  e = _engine(name)
  A = _actions(e)
  e.step_many(A[:3])
  dev = e.device
  ones = torch.ones((K, N), dtype=torch.uint8, device=dev)
  stopped = torch.zeros(N, dtype=torch.uint8, device=dev)
  ran = torch.zeros(N, dtype=torch.int32, device=dev)
  ret = torch.zeros((N, e.P), dtype=torch.float64, device=dev)
  hashed, counters = e.hash_worlds().clone(), e.counters()

  def raw(eng, size=None, **kw):
    req = E.MpStepUntil(ctypes.sizeof(E.MpStepUntil), K, 0, 0)
    req.actions, req.actions_step_bytes = A.data_ptr(), A.stride(0) * 4
    req.active, req.active_step_bytes = ones.data_ptr(), N
    req.stop, req.gamma = LAST, 1.0
    req.stopped, req.ran, req.returns = stopped.data_ptr(), ran.data_ptr(), ret.data_ptr()
    for key, value in kw.items():
      setattr(req, key, value)
    return eng._L.mp_restore(eng._h, ctypes.addressof(req), ctypes.sizeof(req) if size is None else size)

  def untouched(what):
    assert torch.equal(e.hash_worlds(), hashed) and e.counters() == counters, what
    assert not stopped.any() and not ran.any() and not ret.any(), what

  def invalid(field, **kw):
    assert raw(e, **kw) == E.MP_ERR_INVALID, kw
    message = e._L.mp_last_error()
    assert b"MpStepUntil" in message and field in message, (kw, message)

  invalid(b"struct_size", struct_size=96)
  invalid(b"stop", stop=4)
  invalid(b"stop", stop=LAST | REWARD | 8)
  invalid(b"pad", pad=1)
  invalid(b"reserved", reserved=(ctypes.c_uint64 * 5)(0, 0, 0, 0, 1))
  invalid(b"gamma", gamma=float("nan"))
  invalid(b"active_step_bytes", active=None)          # NULL is all ones, and takes no row distance
  host8, host32, host64 = np.zeros(N, np.uint8), np.zeros(N, np.int32), np.zeros((N, e.P), np.float64)
  invalid(b"(active)", active=np.ones((K, N), np.uint8).ctypes.data)
  invalid(b"(stopped)", stopped=host8.ctypes.data)
  invalid(b"(ran)", ran=host32.ctypes.data)
  invalid(b"(returns)", returns=host64.ctypes.data)
  invalid(b"8-byte", returns=ret.data_ptr() + 4)
  invalid(b"4-byte", ran=ran.data_ptr() + 2)
  assert raw(e, steps=0) == E.MP_ERR_INVALID and raw(e, steps=E.STEP_MANY_MAX + 1) == E.MP_ERR_INVALID
  # the three outputs overlap nothing else the request names
  invalid(b"overlaps", ran=ret.data_ptr())
  invalid(b"overlaps", returns=A.data_ptr())
  invalid(b"overlaps", stopped=ones.data_ptr() + N)
  invalid(b"overlaps", stopped=ran.data_ptr())
  untouched("invalid requests")
  # extents that run past their allocation: the last bytes of one allocation of the library's own (no
  # caching allocator rounds it up), of a size every allocation granularity divides
  size = 2 << 20
  ptr = ctypes.c_void_p()
  assert e._L.mp_alloc_output(dev.index or 0, size, 0, ctypes.byref(ptr)) == 0
  try:
    end = ptr.value + size
    for field, kw in ((b"(stopped)", dict(stopped=end - 1)), (b"(ran)", dict(ran=end - 4)),
                      (b"(returns)", dict(returns=end - 8)), (b"(returns)", dict(returns=end - N * e.P * 8 + 8)),
                      (b"(active)", dict(active=end - N, active_step_bytes=N))):
      invalid(field, **kw)
      assert b"past the end" in e._L.mp_last_error(), kw
    untouched("short extents")
  finally:
    e._L.mp_free_output(dev.index or 0, ptr)
  # the Python checks, before the library
  for kw, match in ((dict(until="first"), "until="), (dict(until=("last", "paid")), "until="),
                    (dict(until="last", stopped=stopped[:N - 1]), "stopped="),
                    (dict(stopped=stopped.bool()), "stopped="), (dict(stopped=stopped.cpu()), "lives on"),
                    (dict(returns=ret[:, :1]), "returns="), (dict(returns=ret.float()), "returns="),
                    (dict(returns=ret.cpu()), "lives on"), (dict(returns=True, gamma=float("inf")), "gamma="),
                    (dict(returns=True, out={"ran": ran.long()}), "ran="), (dict(gamma=0.9), "gamma=")):
    with pytest.raises(ValueError, match=match):
      e.step_many(A, **kw)
  untouched("the Python checks")
  # a ring bound
  e.bind_ring(E.OBS_REWARD, slots=4, tune=False)
  assert raw(e) == -5 and b"ring" in e._L.mp_last_error() and b"MpStepUntil" in e._L.mp_last_error()
  assert raw(e, active=None, active_step_bytes=0) == -5 and b"ring" in e._L.mp_last_error()
  with pytest.raises(engine.EngineError, match="ring"):
    e.step_many(A, until="last")
  untouched("a ring")
  assert e.ring["next"] == 0
  _close(e)
  # an engine that promised one launch a step, with a view
  one = engine.Engine(R.pack(name), N, device=0, unfused=False)
  one.reset()
  assert raw(one) == 0                                                    # no view: the step kernels alone
  one.sync()
  assert ran.tolist() == [16] * N and stopped.tolist() == [LAST] * N
  stopped.zero_(); ran.zero_()
  one.bind(E.OBS_WORLD_RGB)
  before = one.hash_worlds().clone()
  assert raw(one) == -5 and b"unfused" in one._L.mp_last_error()
  assert torch.equal(one.hash_worlds(), before) and not stopped.any()
  _close(one)
  # an engine never reset
  fresh = engine.Engine(R.pack(name), N, device=0)
  assert raw(fresh) == E.MP_ERR_INVALID and b"never been reset" in fresh._L.mp_last_error()
  _close(fresh)


# ---- 10. the Substrate surface and a mixture --------------------------------------------------------
def test_substrate_named_results_and_lengths():
  config = substrate.get_config(COMMONS)
  roles = config.default_player_roles
  envs = [substrate.Substrate(config, roles, R.pack(COMMONS), num_worlds=N, env_seed=5) for _ in range(2)]
  a, b = envs
  for env in envs:
    env.reset()
  dev = a.engine.device
  P = len(roles)
  A = torch.from_numpy(R.actions(P, a.action_spec()[0].num_values)).to(dev)
  lengths = torch.tensor([24, 0, 20, 9, 24], device=dev)
  M = torch.arange(K, device=dev)[:, None] < lengths[None]
  r = a.step_many(A, lengths=lengths, until=("last", "reward"), returns=True, gamma=0.97, hashes=True)
  assert isinstance(r, substrate.StepManyUntil) and isinstance(r, substrate.StepManyTrajectory)
  assert isinstance(r, substrate.StepManyResult) and r.observation == {} and r.states is None
  assert tuple(r.ran.shape) == (N,) and r.ran.dtype == torch.int32
  assert tuple(r.stopped.shape) == (N,) and r.stopped.dtype == torch.uint8
  assert tuple(r.returns.shape) == (N, P) and r.returns.dtype == torch.float64
  kept = r._replace(events=None)
  assert kept.ran is r.ran and kept.stopped is r.stopped and kept.returns is r.returns and kept.hashes is r.hashes
  # the host loop of the masked step on the twin
  stopped = torch.zeros(N, dtype=torch.uint8, device=dev)
  ran = torch.zeros(N, dtype=torch.int32, device=dev)
  steps = np.zeros((K, N), bool)
  for k in range(K):
    m = M[k] & (stopped == 0)
    ts = b.step(A[k], active=m)
    reason = (m & (ts.step_type == 2)).to(torch.uint8) * LAST | (m & (ts.reward != 0).any(1)).to(torch.uint8) * REWARD
    stopped = torch.where(reason != 0, reason, stopped)
    ran += m.to(torch.int32)
    steps[k] = m.cpu().numpy()
    assert torch.equal(r.hashes[k], b.hash_worlds()), k
  assert torch.equal(a.hash_worlds(), b.hash_worlds()) and a.engine.counters() == b.engine.counters()
  assert torch.equal(r.ran, ran) and torch.equal(r.stopped, stopped), (r.ran, r.stopped)
  assert bool((r.ran <= lengths).all()) and r.ran[1] == 0 and int((r.stopped != 0).sum()) >= 2, (r.ran, r.stopped)
  _same_bits(r.returns, _definition(r.reward.cpu().numpy(), steps, 0.97), "substrate")
  assert torch.equal(r.timestep.step_type, r.step_type[K - 1])
  # the closed loop without the host: K = 1 calls sharing `stopped`
  for env in envs:
    env.reset()
  stopped = torch.zeros(N, dtype=torch.uint8, device=dev)
  total = torch.zeros(N, dtype=torch.int32, device=dev)
  for k in range(K):
    total += a.step_many(A[k:k + 1], until="last", stopped=stopped).ran
  whole = b.step_many(A, until="last")
  assert torch.equal(a.hash_worlds(), b.hash_worlds()) and torch.equal(total, whole.ran)
  assert torch.equal(stopped, whole.stopped) and stopped.tolist() == [LAST] * N
  # a call without the new arguments returns what it returned
  assert type(b.step_many(A[:2])) is substrate.StepManyResult
  with pytest.raises(ValueError, match="until="):
    a.step_many(A, until="sometimes")
  with pytest.raises(ValueError, match="stopped="):
    a.step_many(A, stopped=stopped[:2])
  with pytest.raises(ValueError, match="gamma="):
    a.step_many(A, gamma=0.5)
  for env in envs:
    assert not env.engine.fault_words()[:6].any()
    env.close()
  single = substrate.Substrate(config, roles, R.pack(COMMONS))
  single.reset()
  with pytest.raises(ValueError, match="num_worlds"):
    single.step_many(A[:, :1], until="last")
  single.close()
  ring = substrate.Substrate(config, roles, R.pack(COMMONS), num_worlds=N, rollout_length=4)
  ring.reset()
  with pytest.raises(ValueError, match="rollout ring"):
    ring.step_many(A, until="last")
  with pytest.raises(ValueError, match="rollout ring"):
    ring.step_many(A, returns=True)
  ring.close()


def test_a_mixture_hands_each_member_its_rows():
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
  entry = torch.from_numpy((rng.random(n) < 0.3).astype(np.uint8) * 2).to(dev)
  entry[0], entry[1], entry[n - 2] = 0, 1, 3
  stopped = entry.clone()
  ret = torch.full((n, P), float("nan"), dtype=torch.float64, device=dev)
  r = mix.step_many(A, active=M, until=("last", "reward"), stopped=stopped, returns=ret, gamma=0.9, hashes=True)
  assert r.stopped is stopped and r.returns is ret and tuple(r.ran.shape) == (n,)
  for i, member in enumerate(plain._members):
    sl = plain.member_slice(i)
    mine = entry[sl].clone()
    part = member.step_many(A[:, sl], active=M[:, sl], until=("last", "reward"), stopped=mine, returns=True,
                            gamma=0.9, hashes=True)
    assert torch.equal(r.ran[sl], part.ran) and torch.equal(stopped[sl], mine), i
    _same_bits(ret[sl], part.returns.cpu().numpy(), i)
    assert torch.equal(r.reward[:, sl], part.reward) and torch.equal(r.hashes[:, sl], part.hashes), i
  assert torch.equal(mix.hash_worlds(), plain.hash_worlds()) and mix.counters() == plain.counters()
  # a world stopped on entry ran nothing and kept its byte; the others ran their active steps
  want = torch.where(entry != 0, torch.zeros_like(entry, dtype=torch.int64), M.sum(0))
  paid = (r.reward != 0).any(2).any(0)
  assert torch.equal(r.ran.long()[~paid], want[~paid]), (r.ran, want)
  assert torch.equal(stopped[entry != 0], entry[entry != 0]) and not torch.isnan(ret).any()
  for e in mix.engines + plain.engines:
    e.sync()
    assert not e.fault_words()[:6].any()
  mix.close(); plain.close()
