"""Per-step world states in step_many (MP_STEP_ROW_STATE, Engine.step_many(states=True)): row k
of the state rows is, byte for byte, what save_worlds() gives after the k-th call of the loop of
single steps — counters and the cached visiting orders included, over the steps that end an
episode, the auto-reset steps behind them and the frozen steps of an engine without auto-reset —
on one pack per level kernel.  The rows load and draw like any saved state, a world never reset
writes none, two engines share one [K, 2N, S] tensor by columns, and every refusal happens on the
host."""
import ctypes

import numpy as np
import pytest
import torch

import states_recipe as recipe
import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

E = engine
N, K = recipe.N, recipe.STEPS
ENV_SEED = 0x5EED0123456789AB


def _pair(name, kinds=(), **kw):
  a = engine.Engine(recipe.pack(name), N, device=0, **kw)
  b = engine.Engine(recipe.pack(name), N, device=0, **kw)
  return a, b, {k: a.bind(k) for k in kinds}, {k: b.bind(k) for k in kinds}


# 7. state rows equal the loop's saves
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("name", recipe.PACKS)
def test_state_rows_equal_the_saves_of_the_loop(name, auto):
  bound = (E.OBS_REWARD, E.OBS_STEP_TYPE, E.OBS_READY_TO_SHOOT, E.OBS_POSITION, E.OBS_LAYER)
  a, b, abufs, bbufs = _pair(name, bound, auto_reset=auto)
  plain = engine.Engine(recipe.pack(name), N, device=0, auto_reset=auto)
  A = torch.from_numpy(recipe.actions(a.P, a.num_actions)).to(a.device)
  fields = name == "clean_up" and auto   # once: the raw action surface
  if fields:
    table = torch.from_numpy(util.pack_tables(recipe.pack(name))["action_table"].reshape(-1, 4)[:, :a.info.num_action_fields].astype(np.int32)).to(a.device)
    F = table[A.long()].contiguous()
  for eng in (a, b, plain):
    eng.reset()
  rows = (E.OBS_LAYER, E.OBS_POSITION)
  got = a.step_many(F if fields else A, fields=fields, observations=rows, events=True, states=True)
  ref = plain.step_many(F if fields else A, fields=fields, observations=rows, events=True)   # the same request without states
  S = a.info.world_state_bytes
  assert got["states"].shape == (K, N, S) and got["states"].dtype == torch.uint8
  types = []
  for k in range(K):
    b.step_fields(F[k]) if fields else b.step(A[k])
    saved = b.save_worlds()
    assert torch.equal(got["states"][k], saved), (name, auto, k, (got["states"][k] != saved).nonzero()[:4].tolist())
    types.append(bbufs[E.OBS_STEP_TYPE].cpu().numpy().copy())
  # the sequence crosses an episode's end: LAST at step 16, then FIRST (auto-reset) or frozen
  assert (types[15] == 2).all() and (types[16] == (0 if auto else 2)).all(), (name, auto)
  for key in ref:   # the other rows, and what the request leaves in place
    if key == "events":
      continue   # (rows beyond a header's count are not written)
    assert torch.equal(got[key], ref[key]), (name, auto, key)
  for kind in bound:
    assert torch.equal(abufs[kind], bbufs[kind]), (name, auto, kind)
  assert torch.equal(a.save_worlds(), b.save_worlds()) and torch.equal(a.save_worlds(), plain.save_worlds())
  assert a.counters() == b.counters() == plain.counters()
  for eng in (a, b, plain):
    util.no_faults(eng)
    eng.close()


# 8. worlds never reset
def test_a_world_never_reset_writes_no_state_rows():
  a, b, _, _ = _pair("clean_up")
  mask = np.ones(N, np.uint8)
  mask[3] = 0
  a.reset(mask=mask); b.reset(mask=mask)
  A = torch.from_numpy(recipe.actions(a.P, a.num_actions)).to(a.device)[:6]
  out = torch.full((6, N, a.info.world_state_bytes), 0x5C, dtype=torch.uint8, device=a.device)
  got = a.step_many(A, out={"states": out})
  assert got["states"].data_ptr() == out.data_ptr()
  assert bool((out[:, 3] == 0x5C).all())
  live = [0, 1, 2, 4]
  for k in range(6):
    b.step(A[k])
    assert torch.equal(out[k, live], b.save_worlds(live)), k
  util.no_faults(a)
  a.close(); b.close()


# 9. round trips
@pytest.mark.parametrize("name", ["clean_up", recipe.MATRIX])
def test_state_rows_draw_what_the_observation_rows_hold(name):
  e = engine.Engine(recipe.pack(name), N, device=0)
  A = torch.from_numpy(recipe.actions(e.P, e.num_actions)).to(e.device)
  kinds = (E.OBS_LAYER, E.OBS_POSITION, E.OBS_READY_TO_SHOOT) + ((E.OBS_INVENTORY,) if e.info.num_resources else ())
  e.reset()
  got = e.step_many(A, observations=kinds, states=True)
  bank = got["states"].view(K * N, -1)
  for kind in kinds:
    drawn = e.observe_states(bank, kind)
    assert torch.equal(drawn.view(got[kind].shape), got[kind]), (name, kind)
    rows = [k * N + w for k, w in ((16, 2), (3, 4), (15, 0), (23, 1))]
    picked = torch.stack([got[kind][k, w] for k, w in ((16, 2), (3, 4), (15, 0), (23, 1))])
    assert torch.equal(e.observe_states(bank, kind, rows=rows), picked), (name, kind, "rows")
  e.sync()
  util.no_faults(e)
  e.close()


def test_substrate_states_load_and_continue_like_the_loop():
  name = "clean_up"
  cfg = substrate.get_config(name)
  n = 4
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=ENV_SEED)
  twin = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=ENV_SEED)
  P, nact = env.num_players, env.action_spec()[0].num_values
  A = util.random_actions(np.random.default_rng(9), 20, n, P, nact)
  env.reset(); twin.reset()
  res = env.step_many(A, states=True)
  assert isinstance(res, substrate.StepManyTrajectory) and len(res) == 6 and res.observation == {}
  assert isinstance(res.states, substrate.WorldStates) and len(res.states) == 20 * n
  assert res._replace(events=None).states is res.states
  loop = []   # (a batched substrate's leaves are overwritten in place: clone what is compared later)
  for k in range(20):
    ts = twin.step(A[k])
    loop.append((ts.reward.clone(), ts.step_type.clone(),
                 {leaf: v.clone() for leaf, v in ts.observation.items()} if k in (7, 19) else None))
  final = twin.save_state()
  assert torch.equal(res.states[19 * n:].data, final.data)
  # the views of step 8's rows and of the last step's, then back to step 8 and on with the remaining actions
  at8 = res.states[7 * n:8 * n]
  for states, k in ((at8, 7), (res.states[19 * n:], 19)):
    seen = env.observe_states(states)
    assert set(seen) == set(env.state_leaves()) & set(loop[k][2]) and "RGB" in seen and "READY_TO_SHOOT" in seen
    for leaf, value in seen.items():
      assert torch.equal(value, loop[k][2][leaf]), (leaf, k)
  some = env.observe_states(res.states, ("LAYER", "POSITION"), rows=[7 * n + 2, 19 * n])
  assert tuple(some) == ("LAYER", "POSITION") and some["POSITION"].shape == (2, P, 2)
  assert torch.equal(some["LAYER"][0], env.observe_states(at8, "LAYER")["LAYER"][2])
  env.load_state(at8, list(range(n)))
  for k in range(8, 20):
    ts = env.step(A[k])
    assert torch.equal(ts.reward, loop[k][0]) and torch.equal(ts.step_type, loop[k][1]), k
  keep = _tail_mask(final.data)
  assert torch.equal(env.save_state().data[:, keep], final.data[:, keep])
  with pytest.raises(ValueError, match="COLLECTIVE_REWARD.*transition"):
    env.observe_states(at8, ("COLLECTIVE_REWARD",))
  env.close(); twin.close()


def _tail_mask(rows):
  """Every byte of a record but WorldTail::ctr[] and reward_fx (a load keeps the destination's)."""
  seed = np.frombuffer(np.uint64(ENV_SEED).tobytes(), np.uint8)   # world 0's seed is the env_seed itself
  row = rows[0].cpu().numpy()
  at = [i for i in range(0, row.size - 8, 8) if (row[i:i + 8] == seed).all()]
  assert len(at) == 1, at
  keep = torch.ones(row.size, dtype=torch.bool, device=rows.device)
  keep[at[0] + 8:at[0] + 8 + 36] = False
  return keep


# 10. column slices
def test_two_engines_share_one_state_tensor_by_columns():
  name = "clean_up"
  a, b, _, _ = _pair(name)
  c = engine.Engine(recipe.pack(name), N, device=0, world_offset=N)
  d = engine.Engine(recipe.pack(name), N, device=0, world_offset=N)
  S = a.info.world_state_bytes
  wide = torch.full((K, 2 * N + 1, S), 0x5C, dtype=torch.uint8, device=a.device)
  A = torch.from_numpy(recipe.actions(a.P, a.num_actions, n=2 * N)).to(a.device)
  for eng in (a, b, c, d):
    eng.reset()
  a.step_many(A[:, :N], out={"states": wide[:, :N]})
  c.step_many(A[:, N:], out={"states": wide[:, N:2 * N]})
  for k in range(K):
    b.step(A[k, :N].contiguous()); d.step(A[k, N:].contiguous())
    assert torch.equal(wide[k, :N], b.save_worlds()) and torch.equal(wide[k, N:2 * N], d.save_worlds()), k
  assert bool((wide[:, 2 * N] == 0x5C).all())   # the neighbour survives
  for eng in (a, b, c, d):
    eng.close()


# 11. refusals
def _request(e, rows, **fields):
  arr = (E.MpStepRow * max(len(rows), 1))()
  for i, (kind, ptr, dist) in enumerate(rows):
    arr[i].kind, arr[i].rows, arr[i].step_bytes = kind, ptr, dist
  req = E.MpStepTrajectory(ctypes.sizeof(E.MpStepTrajectory), 1)
  req.num_rows = len(rows)
  req.rows = arr
  for k, v in fields.items():
    setattr(req, k, v)
  return e._L.mp_restore(e._h, ctypes.addressof(req), ctypes.sizeof(req))


def test_state_row_refusals_launch_nothing():
  e = engine.Engine(recipe.pack("clean_up"), N, device=0)
  L = e._L
  e.reset()
  Ks = 4
  A = torch.from_numpy(recipe.actions(e.P, e.num_actions)).to(e.device)[:Ks].contiguous()
  S = e.info.world_state_bytes
  block = N * S
  assert block % 16 == 0
  buf = torch.full((Ks * block + 64,), 0x5C, dtype=torch.uint8, device=e.device)
  state, ctr = e.save_worlds().clone(), e.counters()
  ok = dict(steps=Ks, actions=A.data_ptr(), actions_step_bytes=N * e.P * 4)
  ST = E.STEP_ROW_STATE

  def refused(word, rows, **fields):
    assert _request(e, rows, **dict(ok, **fields)) == E.MP_ERR_INVALID, (word, L.mp_last_error())
    assert b"MpStepTrajectory" in L.mp_last_error() and word.encode() in L.mp_last_error(), (word, L.mp_last_error())

  refused("step_bytes of STATE", [(ST, buf.data_ptr(), block - 16)])        # shorter than N records
  refused("step_bytes of STATE", [(ST, buf.data_ptr(), block + 8)])         # no multiple of 16
  refused("aligned", [(ST, buf.data_ptr() + 8, block)])
  refused("no buffer", [(ST, None, block)])
  refused("named twice", [(ST, buf.data_ptr(), block), (ST, buf.data_ptr(), block)])
  hip = ctypes.CDLL("libamdhip64.so")
  base, size = ctypes.c_void_p(), ctypes.c_size_t()
  assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(buf.data_ptr())) == 0
  end = (base.value + size.value) & ~15
  refused("allocation", [(ST, end - (Ks - 1) * block - 16, block)])            # the last row leaves the allocation
  refused("no observation kind", [(ST + 1, buf.data_ptr(), block)])
  refused("no observation kind", [(24, buf.data_ptr(), block)])
  e.sync()
  assert bool((buf == 0x5C).all())
  assert torch.equal(e.save_worlds(), state) and e.counters() == ctr
  # every observation kind and the state row in one request: MP_OBS_KINDS + 1 rows are not too many to name
  assert _request(e, [(ST, buf.data_ptr(), block)] * (E.OBS_RGB_POOL8 + 3), **ok) == E.MP_ERR_INVALID
  assert b"num_rows" in L.mp_last_error()
  # the same request, well-formed, runs
  assert _request(e, [(ST, buf.data_ptr(), block)], **ok) == 0
  twin = engine.Engine(recipe.pack("clean_up"), N, device=0)
  twin.reset()
  for k in range(Ks):
    twin.step(A[k])
    assert torch.equal(buf[k * block:(k + 1) * block].view(N, S), twin.save_worlds()), k
  with pytest.raises(ValueError, match="states"):
    e.step_many(A, out={"states": torch.zeros((Ks, N, S + 1), dtype=torch.uint8, device=e.device)})
  util.no_faults(e)
  e.close(); twin.close()


def test_a_mixture_says_that_it_has_no_state_rows():
  mix = substrate.build_mixture(("collaborative_cooking__cramped", "collaborative_cooking__asymmetric"),
                                num_worlds=16, env_seed=3, individual_observations=("POSITION",),
                                global_observations=())
  A = np.zeros((2, mix.num_worlds, mix.num_players), np.int32)
  with pytest.raises(ValueError, match="mixture has no per-step states"):
    mix.step_many(A, states=True)
  mix.close()
