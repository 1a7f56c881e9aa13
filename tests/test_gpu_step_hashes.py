"""Per-step state hashes in step_many (MP_STEP_ROW_HASH, Engine.step_many(hashes=True)): row k of
the hash rows is the hash of what the state rows' row k holds, and what hash_worlds() gives after
the k-th call of the loop of single steps — over the step that ends an episode, the auto-reset step
behind it and the frozen steps of an engine without auto-reset — on one pack per level kernel.  A
world never reset writes none, the row rides beside the state rows and LAYER in one launch, it
changes nothing else the launch leaves behind, and a mixture gets one [K, N_total] tensor."""
import ctypes

import numpy as np
import pytest
import torch

import states_recipe as R
import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

E = engine
N, K = R.N, 6
AHEAD = 13          # single launch in front: the K steps are steps 14 .. 19 of the recipe's actions,
END = 16 - AHEAD - 1  # so row END is the episode's LAST step (16) and row END + 1 the step behind it
SENTINEL = -0x0123456789ABCDEF


def _engines(name, count, **kw):
  """`count` engines of the recipe's pack, each AHEAD steps into the recipe's actions."""
  out = []
  for _ in range(count):
    e = engine.Engine(R.pack(name), N, device=0, **kw)
    e.reset()
    out.append(e)
  A = torch.from_numpy(R.actions(out[0].P, out[0].num_actions)).to(out[0].device)
  for e in out:
    e.step_many(A[:AHEAD])
  return out, A[AHEAD:AHEAD + K].contiguous()


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("name", R.PACKS)
def test_hash_rows_equal_the_hashes_of_the_state_rows_and_of_the_loop(name, auto):
  (a, b, c), A = _engines(name, 3, auto_reset=auto)
  got = a.step_many(A, hashes=True)
  assert got["hashes"].shape == (K, N) and got["hashes"].dtype == torch.int64
  ref = b.step_many(A, states=True)
  for key in ("reward", "step_type", "discount", "collective_reward"):
    assert torch.equal(got[key], ref[key]), (name, auto, key)
  for k in range(K):
    assert torch.equal(got["hashes"][k], b.hash_states(ref["states"][k])), (name, auto, k)
    c.step(A[k])
    assert torch.equal(got["hashes"][k], c.hash_worlds()), (name, auto, k)
  # the sequence crosses an episode's end: LAST, then FIRST (auto-reset) or frozen
  types = got["step_type"].cpu().numpy()
  assert (types[END] == 2).all() and (types[END + 1] == (0 if auto else 2)).all(), (name, auto)
  assert torch.equal(a.save_worlds(), b.save_worlds()) and torch.equal(a.save_worlds(), c.save_worlds())
  assert a.counters() == b.counters() == c.counters()
  for e in (a, b, c):
    e.sync()
    util.no_faults(e)
    e.close()


def test_one_step():
  (a, b), A = _engines("coins", 2)
  got = a.step_many(A[:1], hashes=True)
  b.step(A[0])
  assert got["hashes"].shape == (1, N) and torch.equal(got["hashes"][0], b.hash_worlds())
  a.close(); b.close()


def test_a_world_never_reset_writes_no_hash_rows():
  a = engine.Engine(R.pack("clean_up"), N, device=0)
  b = engine.Engine(R.pack("clean_up"), N, device=0)
  mask = np.ones(N, np.uint8)
  mask[3] = 0
  a.reset(mask=mask); b.reset(mask=mask)
  A = torch.from_numpy(R.actions(a.P, a.num_actions)).to(a.device)[:K]
  out = torch.full((K, N), SENTINEL, dtype=torch.int64, device=a.device)
  got = a.step_many(A, out={"hashes": out})
  assert got["hashes"].data_ptr() == out.data_ptr()
  assert bool((out[:, 3] == SENTINEL).all())
  live = [0, 1, 2, 4]
  for k in range(K):
    b.step(A[k])
    assert torch.equal(out[k, live], b.hash_worlds(live)), k
  a.sync()
  util.no_faults(a)
  a.close(); b.close()


@pytest.mark.parametrize("name", ["clean_up", R.MATRIX])
def test_hashes_states_and_layer_in_one_call_are_the_separate_calls(name):
  (a, b, c, d), A = _engines(name, 4)
  both = a.step_many(A, hashes=True, states=True, observations=(E.OBS_LAYER,), events=True)
  hashes = b.step_many(A, hashes=True)["hashes"]
  states = c.step_many(A, states=True)["states"]
  layer = d.step_many(A, observations=(E.OBS_LAYER,))[E.OBS_LAYER]
  assert torch.equal(both["hashes"], hashes) and torch.equal(both["states"], states)
  assert torch.equal(both[E.OBS_LAYER], layer)
  assert torch.equal(a.hash_states(both["states"].view(K * N, -1)).view(K, N), hashes)
  for e in (a, b, c, d):
    e.sync()
    util.no_faults(e)
    e.close()


def test_the_hash_row_changes_nothing_else():
  name = "clean_up"
  # (not EVENTS: rows beyond a header's count are not written, so a bound buffer holds what it held)
  bound = (E.OBS_REWARD, E.OBS_STEP_TYPE, E.OBS_READY_TO_SHOOT, E.OBS_POSITION, E.OBS_LAYER, E.OBS_WORLD_RGB)
  (a, b), A = _engines(name, 2)
  abufs, bbufs = {k: a.bind(k) for k in bound}, {k: b.bind(k) for k in bound}
  with_row = a.step_many(A, hashes=True, observations=(E.OBS_POSITION,))
  without = b.step_many(A, observations=(E.OBS_POSITION,))
  for key in without:
    assert torch.equal(with_row[key], without[key]), key
  assert torch.equal(a.save_worlds(), b.save_worlds()) and a.counters() == b.counters()
  for kind in bound:
    assert torch.equal(abufs[kind], bbufs[kind]), kind
  for e in (a, b):
    e.sync()
    util.no_faults(e)
    e.close()


def test_substrate_and_mixture_hashes():
  name = "clean_up"
  cfg = substrate.get_config(name)
  n = 4
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=5)
  P, nact = env.num_players, env.action_spec()[0].num_values
  A = util.random_actions(np.random.default_rng(9), 5, n, P, nact)
  env.reset()
  res = env.step_many(A, hashes=True, states=True)
  assert isinstance(res, substrate.StepManyTrajectory) and tuple(res.hashes.shape) == (5, n)
  assert torch.equal(env.hash_states(res.states).view(5, n), res.hashes)
  assert torch.equal(env.hash_worlds(), res.hashes[4]) and res._replace(events=None).hashes is res.hashes
  plain = env.step_many(A)
  assert type(plain) is substrate.StepManyResult
  env.close()
  # two kitchens: one [K, N_total] tensor, each member writing its columns
  names = ("collaborative_cooking__cramped", "collaborative_cooking__asymmetric")
  kw = dict(num_worlds=16, env_seed=3, individual_observations=("POSITION",), global_observations=())
  mix, twin = substrate.build_mixture(names, **kw), substrate.build_mixture(names, **kw)
  Km = 4
  B = util.random_actions(np.random.default_rng(2), Km, mix.num_worlds, mix.num_players, mix.action_spec()[0].num_values)
  mix.reset(); twin.reset()
  res = mix.step_many(B, hashes=True)
  assert tuple(res.hashes.shape) == (Km, mix.num_worlds) and res.hashes.dtype == torch.int64
  assert torch.equal(mix.hash_worlds(), res.hashes[Km - 1])
  dB = torch.from_numpy(B).to(res.hashes.device)
  for i, member in enumerate(twin._members):   # each member's own Engine.step_many(hashes=True), on the twin
    cols = twin.member_slice(i)
    own = member._submit_many(dB[:, cols], None, False, None, hashes=True)["hashes"]
    assert tuple(own.shape) == (Km, cols.stop - cols.start) and torch.equal(res.hashes[:, cols], own), i
  pick = [mix.num_worlds - 1, 0, 1, mix.num_worlds - 1, 9]   # both members, out of order, a repeat
  assert torch.equal(mix.hash_worlds(pick), res.hashes[Km - 1][pick])
  with pytest.raises(ValueError, match="no per-step states"):
    mix.step_many(B, states=True)
  mix.close(); twin.close()


def test_hash_row_refusals_launch_nothing():
  """The hash row is checked by step_request like every other row: element size 8."""
  (e, twin), A = _engines("clean_up", 2)
  L = e._L
  Ks = 4
  A = A[:Ks].contiguous()
  block = N * 8
  buf = torch.full((Ks * block + 64,), 0x5C, dtype=torch.uint8, device=e.device)
  state, ctr = e.save_worlds().clone(), e.counters()
  HASH = E.STEP_ROW_HASH

  def request(rows):
    arr = (E.MpStepRow * len(rows))()
    for i, (kind, ptr, dist) in enumerate(rows):
      arr[i].kind, arr[i].rows, arr[i].step_bytes = kind, ptr, dist
    req = E.MpStepTrajectory(ctypes.sizeof(E.MpStepTrajectory), Ks, 0, len(rows))
    req.actions, req.actions_step_bytes, req.rows = A.data_ptr(), N * e.P * 4, arr
    return L.mp_restore(e._h, ctypes.addressof(req), ctypes.sizeof(req)), L.mp_last_error().decode()

  def refused(word, rows):
    rc, msg = request(rows)
    assert rc == E.MP_ERR_INVALID and "MpStepTrajectory" in msg and word in msg, (word, rc, msg)

  refused("step_bytes of HASH", [(HASH, buf.data_ptr(), block - 8)])        # shorter than N hashes
  refused("step_bytes of HASH", [(HASH, buf.data_ptr(), block + 4)])        # no multiple of 8
  refused("aligned", [(HASH, buf.data_ptr() + 4, block)])
  refused("no buffer", [(HASH, None, block)])
  refused("named twice", [(HASH, buf.data_ptr(), block), (HASH, buf.data_ptr(), block)])
  hip = ctypes.CDLL("libamdhip64.so")
  base, size = ctypes.c_void_p(), ctypes.c_size_t()
  assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(buf.data_ptr())) == 0
  end = (base.value + size.value) & ~7
  refused("allocation", [(HASH, end - (Ks - 1) * block - 8, block)])          # the last row leaves the allocation
  e.sync()
  assert bool((buf == 0x5C).all())
  assert torch.equal(e.save_worlds(), state) and e.counters() == ctr
  # the same request, well-formed, runs; a distance larger than a block leaves the gap alone
  assert request([(HASH, buf.data_ptr(), block + 8)])[0] == 0
  rows = buf[:Ks * (block + 8)].view(torch.int64).view(Ks, N + 1)
  for k in range(Ks):
    twin.step(A[k])
    assert torch.equal(rows[k, :N], twin.hash_worlds()), k
  assert bool((buf[:Ks * (block + 8)].view(Ks, block + 8)[:, block:] == 0x5C).all())
  with pytest.raises(ValueError, match="hashes"):
    e.step_many(A, out={"hashes": torch.zeros((Ks, N + 1), dtype=torch.int64, device=e.device)})
  for eng in (e, twin):
    eng.sync()
    util.no_faults(eng)
    eng.close()
