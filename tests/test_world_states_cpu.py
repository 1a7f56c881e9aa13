"""World states as device data (mp_state_fingerprint / mp_save_worlds / mp_load_worlds) on the
host side: the header declares the entry points (the request's layout and the wrappers' answers:
tests/test_request_abi_cpu.py), NULL and empty
arguments are refused before a device is looked for, and `substrate.WorldStates` checks what it
holds and selects rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from meltingpot_amd import engine
from meltingpot_amd.substrate import WorldStates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
  return open(os.path.join(ROOT, "include", "mp_engine.h")).read()


def test_header_declares_the_world_state_request_and_keeps_abi_8():
  """The wrappers' header declares the three entry points.  (What it held of the layout and the ABI version: tests/test_request_abi_cpu.py.)"""
  wrappers = open(os.path.join(ROOT, "include", "mp_world_states.h")).read()
  assert re.search(r"static inline uint64_t mp_state_fingerprint\(MpEngine\* eng\)", wrappers)
  assert re.search(r"static inline int mp_save_worlds\(MpEngine\* eng, const int32_t\* worlds_device, "
                   r"int32_t count,\s*void\* dst_device, uint64_t dst_bytes\)", wrappers)
  assert re.search(r"static inline int mp_load_worlds\(MpEngine\* eng, const void\* bank_device, "
                   r"int32_t bank_rows,\s*const int32_t\* src_device, uint64_t fingerprint\)", wrappers)


def test_the_world_states_add_no_exported_symbol():
  """The operations ride on mp_snapshot / mp_restore: they are no symbols of the ABI (which
  tests/test_cabi_cpu.py holds to what the library exports)."""
  assert not {"mp_state_fingerprint", "mp_save_worlds", "mp_load_worlds"} & set(engine.ABI_SYMBOLS)


def test_header_lists_every_observation_kind_in_exactly_one_load_group():
  """The header's comment on MP_STATES_LOAD names each kind once: (A) functions of the record,
  (B) transition kinds."""
  text = _header()
  doc = text[text.index("MP_STATES_LOAD (mp_restore): ONE launch"):text.index("enum { MP_STATES_FINGERPRINT")]
  a = doc[doc.index("(A)"):doc.index("(B)")]
  b = doc[doc.index("(B)"):]
  kinds = sorted(set(re.findall(r"\b(MP_OBS_[A-Z_0-9]+)\s*=", text)) - {"MP_OBS_KINDS"})
  def names(part):
    found = set(re.findall(r"\bMP_OBS_[A-Z_0-9]+\b", part))
    for m in re.finditer(r"\b(MP_OBS_[A-Z_]+?)(\d)\.\.(\d)\b", part):   # MP_OBS_AUX1..4
      found |= {f"{m.group(1)}{k}" for k in range(int(m.group(2)), int(m.group(3)) + 1)}
    for m in re.finditer(r"\b(MP_OBS_[A-Z_]+?)(\d)/(\d)/(\d)\b", part):   # MP_OBS_RGB_POOL2/4/8
      found |= {f"{m.group(1)}{m.group(k)}" for k in (2, 3, 4)}
    return found & set(kinds)
  assert names(a) | names(b) == set(kinds), set(kinds) - names(a) - names(b)
  assert not names(a) & names(b), names(a) & names(b)
  assert {"MP_OBS_POSITION", "MP_OBS_LAYER", "MP_OBS_WORLD_RGB"} <= names(a)
  assert {"MP_OBS_STEP_TYPE", "MP_OBS_EVENTS", "MP_OBS_ZAP_MATRIX"} <= names(b)


def test_null_and_empty_arguments_are_invalid_without_a_device():
  L = engine.load_library()
  req = engine.MpWorldStates(ctypes.sizeof(engine.MpWorldStates), engine.MP_STATES_SAVE)
  assert L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)) == engine.MP_ERR_INVALID
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == engine.MP_ERR_INVALID
  assert L.mp_snapshot(None, None, ctypes.sizeof(req)) == engine.MP_ERR_INVALID


def test_world_states_refuse_wrong_dtype_shape_and_fingerprint():
  rows = torch.arange(3 * 64, dtype=torch.int32).to(torch.uint8).reshape(3, 64)
  with pytest.raises(ValueError):
    WorldStates(rows.to(torch.int32), 5)
  with pytest.raises(ValueError):
    WorldStates(rows.reshape(-1), 5)
  with pytest.raises(ValueError):
    WorldStates(rows[:0], 5)
  with pytest.raises(ValueError):
    WorldStates(np.zeros((3, 64), np.uint8), 5)
  with pytest.raises(ValueError):
    WorldStates(rows, -1)
  with pytest.raises(ValueError):
    WorldStates(rows, 1 << 64)
  s = WorldStates(rows, 0xFEDCBA9876543210)
  s.check(0xFEDCBA9876543210, 64)
  with pytest.raises(ValueError, match="fingerprint"):
    s.check(0xFEDCBA9876543211, 64)
  with pytest.raises(ValueError, match="bytes"):
    s.check(0xFEDCBA9876543210, 128)


def test_world_states_select_rows():
  rows = (torch.arange(5 * 32, dtype=torch.int64) % 251).to(torch.uint8).reshape(5, 32)
  s = WorldStates(rows, 42)
  assert len(s) == 5 and s.row_bytes == 32
  one = s[3]
  assert isinstance(one, WorldStates) and tuple(one.data.shape) == (1, 32) and one.fingerprint == 42
  assert torch.equal(one.data[0], rows[3])
  assert torch.equal(s[-1].data[0], rows[4])
  assert torch.equal(s[1:4].data, rows[1:4])
  picked = s[[4, 0, 0, 2]]
  assert torch.equal(picked.data, rows[[4, 0, 0, 2]]) and picked.data.is_contiguous()
  assert torch.equal(s[torch.tensor([2, 1])].data, rows[[2, 1]])
  assert torch.equal(s[np.array([1, 3])].data, rows[[1, 3]])
  with pytest.raises(ValueError):
    s[torch.tensor([True, False, True, False, True])]
  with pytest.raises(IndexError):
    s[7]
