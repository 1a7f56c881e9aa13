"""Observations of saved world states (MpStatesObserve) and the per-step state rows
(MP_STEP_ROW_STATE) on the host side (the request's layout, wrapper and kernels:
tests/test_request_abi_cpu.py): NULL and empty requests are refused before a device is looked for, and
`Substrate.observe_states` checks its names before any engine call."""
import ctypes
import os
import re

import pytest
import torch

from meltingpot_amd import engine, substrate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = engine


def _header():
  return open(os.path.join(ROOT, "include", "mp_engine.h")).read()


def test_header_declares_the_request_with_the_ctypes_fields_and_keeps_the_abi():
  """The wrapper's signature, and the kinds the Python layer offers.  (What it held of the layout and the ABI version: tests/test_request_abi_cpu.py.)"""
  wrapper = open(os.path.join(ROOT, "include", "mp_states_observe.h")).read()
  assert re.search(r"static inline int mp_observe_states\(MpEngine\* eng, MpObsKind kind, const void\* bank_device", wrapper)
  # the kinds the Python layer offers are the header's record functions
  assert set(E.STATE_OBS_KINDS) == set(E.PIXEL_KINDS) | {E.OBS_LAYER, E.OBS_READY_TO_SHOOT, E.OBS_POSITION,
                                                        E.OBS_ORIENTATION, E.OBS_INVENTORY}


def test_the_request_adds_no_exported_symbol():
  """The request rides mp_snapshot.  (tests/test_cabi_cpu.py holds ABI_SYMBOLS to what the library
  exports; the request's kernels: tests/test_request_abi_cpu.py.)"""
  assert "mp_observe_states" not in E.ABI_SYMBOLS


def test_null_and_empty_requests_are_invalid_without_a_device():
  L = E.load_library()
  req = E.MpStatesObserve(ctypes.sizeof(E.MpStatesObserve), E.OBS_POSITION)
  assert L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"MpStatesObserve" in L.mp_last_error()
  assert L.mp_snapshot(None, None, ctypes.sizeof(req)) == E.MP_ERR_INVALID
  # the request does not ride mp_restore
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  # a state row named without an engine: refused under the trajectory request's name
  rows = (E.MpStepRow * 1)()
  rows[0].kind, rows[0].rows, rows[0].step_bytes = E.STEP_ROW_STATE, 0x1000, 4096
  many = E.MpStepTrajectory(ctypes.sizeof(E.MpStepTrajectory), 4, 0, 1)
  many.actions, many.rows = 0x1000, rows
  assert L.mp_restore(None, ctypes.addressof(many), ctypes.sizeof(many)) == E.MP_ERR_INVALID
  assert b"MpStepTrajectory" in L.mp_last_error()


@pytest.fixture
def oracle_engine(monkeypatch):
  from oracle_engine import OracleBatchEngine

  class NoStatesEngine(OracleBatchEngine):
    """The oracle stand-in has no saved states: reaching it is the failure."""

    @property
    def state_fingerprint(self):
      raise AssertionError("an engine call")

    def observe_states(self, *args, **kw):
      raise AssertionError("an engine call")

    def step_many(self, *args, **kw):
      raise AssertionError("an engine call")

  monkeypatch.setattr(substrate.engine_lib, "Engine", NoStatesEngine)


def test_substrate_checks_names_before_any_engine_call(oracle_engine):
  cfg = substrate.get_config("clean_up")
  env = substrate.build("clean_up", roles=cfg.default_player_roles, num_worlds=2, env_seed=3)
  states = substrate.WorldStates(torch.zeros((2, 64), dtype=torch.uint8), 7)
  offered = env.state_leaves()
  assert set(offered) == {"RGB", "WORLD.RGB", "LAYER", "READY_TO_SHOOT", "POSITION", "ORIENTATION"}
  assert offered["RGB"] == E.OBS_RGB and offered["LAYER"] == E.OBS_LAYER
  for leaf in ("COLLECTIVE_REWARD", cfg.aux0_name, "INTERACTION_INVENTORIES"):
    with pytest.raises(ValueError, match=f"{leaf}.*transition leaf"):
      env.observe_states(states, (leaf,))
  with pytest.raises(ValueError, match="'NO_SUCH_LEAF' is no leaf of this substrate"):
    env.observe_states(states, ("RGB", "NO_SUCH_LEAF"))
  with pytest.raises(ValueError, match="'INVENTORY' is no leaf of this substrate"):   # clean_up has none
    env.observe_states(states, "INVENTORY")
  with pytest.raises(ValueError, match="WorldStates"):
    env.observe_states(torch.zeros((2, 64), dtype=torch.uint8), ("RGB",))
  with pytest.raises(AssertionError, match="an engine call"):   # good names do reach the engine
    env.observe_states(states, ("RGB",))
  env.close()
  name = "prisoners_dilemma_in_the_matrix__repeated"
  mx = substrate.build(name, roles=substrate.get_config(name).default_player_roles, num_worlds=2, env_seed=3)
  assert "INVENTORY" in mx.state_leaves()
  mx.close()


def test_a_mixture_refuses_states_by_name(oracle_engine):
  names = ("collaborative_cooking__cramped", "collaborative_cooking__asymmetric")
  mix = substrate.build_mixture(names, num_worlds=16, env_seed=3, individual_observations=("POSITION",),
                                global_observations=())
  import numpy as np
  with pytest.raises(ValueError, match="mixture has no per-step states"):
    mix.step_many(np.zeros((2, mix.num_worlds, mix.num_players), np.int32), states=True)
  mix.close()


def test_check_step_rows_keeps_refusing_what_is_no_observation_kind():
  for bad in (E.STEP_ROW_STATE, 24, -1):
    with pytest.raises(ValueError, match="no observation kind"):
      E.check_step_rows([bad])
