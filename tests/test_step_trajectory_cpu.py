"""Action sequences with per-step rows of the observations (MpStepTrajectory) on the host side
(the request's layout, wrapper and kernels: tests/test_request_abi_cpu.py): a NULL engine is refused under the request's name, the kind and shape rules hold
without an engine, and `Substrate.step_many(observations=...)` runs on the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from meltingpot_amd import engine, substrate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = engine


def _header():
  return open(os.path.join(ROOT, "include", "mp_engine.h")).read()


def test_header_structs_equal_the_ctypes_structs_and_abi_stays_8():
  """Where the request sits in the header, and its wrapper's signature.  (What it held of the layout and the ABI version: tests/test_request_abi_cpu.py.)"""
  text = _header()
  # the new text sits behind the MpStepMany typedef, which is as it was
  assert text.index("} MpStepMany;") < text.index("sizeof(MpStepTrajectory)")
  wrapper = open(os.path.join(ROOT, "include", "mp_step_trajectory.h")).read()
  assert re.search(r"static inline int mp_step_trajectory\(MpEngine\* eng, const int32_t\* actions_device", wrapper)


def test_the_request_adds_no_exported_symbol():
  """(tests/test_cabi_cpu.py holds ABI_SYMBOLS to what the library exports.)"""
  assert "mp_step_trajectory" not in E.ABI_SYMBOLS


def test_null_engine_is_invalid_under_the_requests_name():
  L = E.load_library()
  req = E.MpStepTrajectory(ctypes.sizeof(E.MpStepTrajectory), 4)
  req.actions = 0x1000   # (never dereferenced: there is no engine)
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"MpStepTrajectory" in L.mp_last_error()
  # an MpStepMany request still answers under its own name
  old = E.MpStepMany(ctypes.sizeof(E.MpStepMany), 4)
  old.actions = 0x1000
  assert L.mp_restore(None, ctypes.addressof(old), ctypes.sizeof(old)) == E.MP_ERR_INVALID
  assert b"MpStepMany" in L.mp_last_error()


def test_kind_and_shape_rules_hold_without_an_engine():
  check = E.check_step_rows
  assert check(()) == ()
  assert check([E.OBS_LAYER, E.OBS_READY_TO_SHOOT, np.int32(E.OBS_POSITION)]) == (
      E.OBS_LAYER, E.OBS_READY_TO_SHOOT, E.OBS_POSITION)
  assert set(E.STEP_ROW_KINDS) == set(range(2, 21)) and not set(E.STEP_ROW_KINDS) & set(E.PIXEL_KINDS)
  for pixel in E.PIXEL_KINDS:
    with pytest.raises(ValueError, match="pixel kind.*rollout ring"):
      check([E.OBS_LAYER, pixel])
  with pytest.raises(ValueError, match="named twice"):
    check([E.OBS_LAYER, E.OBS_LAYER])
  with pytest.raises(ValueError, match="named twice"):      # keep= stacks REWARD already
    check([E.OBS_REWARD], taken=[E.OBS_REWARD])
  for bad in (99, -1, "LAYER", True, 2.0):
    with pytest.raises(ValueError, match="step_many"):
      check([bad])
  K, N, P = 5, 6, 3
  shapes = {E.OBS_POSITION: ((N, P, 2), torch.int32), E.OBS_READY_TO_SHOOT: ((N, P), torch.float64)}
  good = {E.OBS_POSITION: torch.zeros((K, N, P, 2), dtype=torch.int32)}
  assert check([E.OBS_POSITION, E.OBS_READY_TO_SHOOT], steps=K, shapes=shapes, out=good) == (
      E.OBS_POSITION, E.OBS_READY_TO_SHOOT)
  wide = torch.zeros((K, 3 * N, P, 2), dtype=torch.int32)
  check([E.OBS_POSITION], steps=K, shapes=shapes, out={E.OBS_POSITION: wide[:, N:2 * N]})   # a column slice
  bad_outs = [torch.zeros((K, N, P, 2), dtype=torch.int64),          # wrong dtype
              torch.zeros((K, N, P, 2), dtype=torch.float64),
              torch.zeros((K + 1, N, P, 2), dtype=torch.int32),      # wrong K
              torch.zeros((K, N, P), dtype=torch.int32),             # wrong rank
              torch.zeros((K, N + 1, P, 2), dtype=torch.int32),      # wrong N
              np.zeros((K, N, P, 2), np.int32)]                      # no tensor
  for buf in bad_outs:
    with pytest.raises(ValueError, match="step_many"):
      check([E.OBS_POSITION], steps=K, shapes=shapes, out={E.OBS_POSITION: buf})
  with pytest.raises(ValueError, match="along K only"):
    check([E.OBS_POSITION], steps=K, shapes=shapes,
          out={E.OBS_POSITION: torch.zeros((K, N, 2 * P, 2), dtype=torch.int32)[:, :, :P]})
  with pytest.raises(ValueError, match="overlap"):
    check([E.OBS_POSITION], steps=K, shapes=shapes,
          out={E.OBS_POSITION: torch.zeros((1, N, P, 2), dtype=torch.int32).expand(K, N, P, 2)})
  with pytest.raises(ValueError, match="overlap"):
    check([E.OBS_POSITION], steps=K, shapes=shapes,
          out={E.OBS_POSITION: torch.zeros(K * N * P * 2, dtype=torch.int32).as_strided((K, N, P, 2), (N * P, P * 2, 2, 1))})


# ---- the Substrate layer on the oracle ----------------------------------------------------------
@pytest.fixture
def oracle_engine(monkeypatch):
  from oracle_engine import OracleBatchEngine

  class ManyOracleEngine(OracleBatchEngine):
    """The stand-in with a step_many: the loop of step, `_value(kind)` stacked per step."""

    def step_many(self, actions, *, repeat=None, fields=False,
                  keep=("reward", "collective_reward", "step_type", "discount"), events=False,
                  observations=(), out=None):
      assert not events, "the stand-in has no raw event rows"
      a = np.asarray(actions.cpu() if hasattr(actions, "cpu") else actions)
      A = int(self.info.num_action_fields) if fields else None
      K = E.check_step_many(a.shape, a.dtype, self.N, self.P, repeat=repeat, num_fields=A)
      five = {n: E._STEP_MANY_KIND_OF[n] for n in E.STEP_MANY_KINDS[:4] if n in keep}
      kinds = E.check_step_rows(observations, taken=list(five.values()))
      wanted = dict(five)
      wanted.update({k: k for k in kinds})
      rows = {key: [] for key in wanted}
      for k in range(K):
        (self.step_fields if fields else self.step)(a if repeat is not None else a[k])
        for key, kind in wanted.items():
          rows[key].append(torch.from_numpy(np.ascontiguousarray(self._value(kind))).view(self.shapes[kind][0]))
      result = {}
      for key, kind in wanted.items():
        stacked = torch.stack(rows[key]).to(self.shapes[kind][1])
        if out is not None and out.get(key) is not None:
          out[key].copy_(stacked)
          stacked = out[key]
        result[key] = stacked
      return result

  monkeypatch.setattr(substrate.engine_lib, "Engine", ManyOracleEngine)


def _actions(rng, K, n, P, nact):
  return rng.integers(0, nact, size=(K, n, P)).astype(np.int32)


def test_substrate_observations_on_the_oracle(oracle_engine):
  cfg = substrate.get_config("clean_up")
  n, K = 3, 6
  env = substrate.build("clean_up", roles=cfg.default_player_roles, num_worlds=n, env_seed=41)
  twin = substrate.build("clean_up", roles=cfg.default_player_roles, num_worlds=n, env_seed=41)
  P, nact = env.num_players, env.action_spec()[0].num_values
  A = _actions(np.random.default_rng(5), K, n, P, nact)
  env.reset(); twin.reset()
  offered = env.step_leaves()
  assert "RGB" not in offered and "WORLD.RGB" not in offered
  aux0 = cfg.aux0_name
  asked = tuple(x for x in ("READY_TO_SHOOT", "POSITION", "ORIENTATION", aux0) if x in offered)
  assert "READY_TO_SHOOT" in asked and aux0 in asked
  res = env.step_many(A, observations=asked)
  assert isinstance(res, substrate.StepManyTrajectory) and isinstance(res, substrate.StepManyResult)
  assert len(res) == 6 and res.events is None
  assert tuple(res.observation) == asked
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.reward[k], ts.reward) and torch.equal(res.step_type[k], ts.step_type), k
    for name in asked:
      assert torch.equal(res.observation[name][k], ts.observation[name]), (name, k)
  for name in asked:
    leaf = ts.observation[name]
    assert tuple(res.observation[name].shape) == (K,) + tuple(leaf.shape), name
    assert res.observation[name].dtype == leaf.dtype, name
    assert torch.equal(res.timestep.observation[name], leaf), name
  # True: every non-pixel leaf, COLLECTIVE_REWARD (one of the five: the tensor the call stacks anyway) included
  res = env.step_many(A, observations=True)
  assert set(res.observation) == set(offered)
  assert res.observation["COLLECTIVE_REWARD"] is res.collective_reward
  for k in range(K):
    ts = twin.step(A[k])
    for name in offered:
      assert torch.equal(res.observation[name][k], ts.observation[name]), (name, k)
  # without observations: what the call has always returned
  plain = env.step_many(A)
  assert type(plain) is substrate.StepManyResult and not hasattr(plain, "observation")
  assert type(env.step_many(A, observations=())) is substrate.StepManyResult
  for k in range(2 * K):
    twin.step(A[k % K])
  # refusals: a pixel leaf, a name that is no leaf, a name twice
  with pytest.raises(ValueError, match="pixel leaf.*READY_TO_SHOOT"):
    env.step_many(A, observations=("RGB",))
  with pytest.raises(ValueError, match="no leaf of this substrate.*READY_TO_SHOOT"):
    env.step_many(A, observations=("INVENTORY",))
  with pytest.raises(ValueError, match="named twice"):
    env.step_many(A, observations=("READY_TO_SHOOT", "READY_TO_SHOOT"))
  # (a refused call stepped nothing)
  ts = twin.step(A[0])
  got = env.step_many(A[:1], observations="READY_TO_SHOOT")   # (one name as a string)
  assert torch.equal(got.observation["READY_TO_SHOOT"][0], ts.observation["READY_TO_SHOOT"])
  env.close(); twin.close()


def test_substrate_inventories_on_the_oracle(oracle_engine):
  name = "prisoners_dilemma_in_the_matrix__repeated"
  cfg = substrate.get_config(name)
  n, K = 2, 5
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=42)
  twin = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=42)
  A = _actions(np.random.default_rng(6), K, n, env.num_players, env.action_spec()[0].num_values)
  env.reset(); twin.reset()
  res = env.step_many(A, observations=("INVENTORY", "READY_TO_SHOOT"))
  R = env.engine.info.num_resources
  assert tuple(res.observation["INVENTORY"].shape) == (K, n, env.num_players, R)
  assert res.observation["INVENTORY"].dtype == torch.float64
  for k in range(K):
    ts = twin.step(A[k])
    assert torch.equal(res.observation["INVENTORY"][k], ts.observation["INVENTORY"]), k
    assert torch.equal(res.observation["READY_TO_SHOOT"][k], ts.observation["READY_TO_SHOOT"]), k
  env.close(); twin.close()
