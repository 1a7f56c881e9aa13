"""Stepping some of the worlds (MpStepActive) without a GPU: include/mp_step_active.h compiles as
C99 and as C++17 and its request has the size and the offsets the library and the ctypes mirror
expect, distinct from every other request's; the mask check of Engine.step / Engine.step_many
refuses bad dtypes, ranks, shapes and strides; the library exports what it exported; the new kernel
family is in the code object; a request without an engine is refused by the library's own checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from meltingpot_amd import _build, engine

E = engine
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = ("clean_up", "commons", "coins", "territory", "matrix", "coop", "gift", "cook", "mushroom")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "mp_step_active.h"
int main(void) {
  /* (no engine: both wrappers answer MP_ERR_INVALID with the library's message) */
  int a = mp_step_many_active(NULL, NULL, 4, 0, 0, NULL, 0, NULL, 0);
  int b = mp_step_active(NULL, NULL, 0, NULL);
  printf("%u %u %u %u %d %d\n", (unsigned)sizeof(MpStepActive), (unsigned)offsetof(MpStepActive, active),
         (unsigned)offsetof(MpStepActive, active_step_bytes), (unsigned)offsetof(MpStepActive, reserved), a, b);
  return 0;
}
'''


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cc")])
def test_the_header_compiles_and_has_the_size_of_the_mirror(tmp_path, compiler, std, suffix):
  src = tmp_path / f"active.{suffix}"
  src.write_text(PROGRAM)
  exe = tmp_path / "active"
  subprocess.run([compiler, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                  _build.build_engine(), f"-Wl,-rpath,{os.path.dirname(_build.LIB_PATH)}"], check=True)
  out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
  M = E.MpStepActive
  assert out == [str(ctypes.sizeof(M)), str(M.active.offset), str(M.active_step_bytes.offset),
                 str(M.reserved.offset), str(E.MP_ERR_INVALID), str(E.MP_ERR_INVALID)]


def test_the_mirror_has_the_documented_layout():
  M = E.MpStepActive
  assert ctypes.sizeof(M) == 96
  offsets = {name: getattr(M, name).offset for name, _ in M._fields_}
  assert offsets == {"struct_size": 0, "steps": 4, "fields": 8, "num_rows": 12, "actions": 16,
                     "actions_step_bytes": 24, "rows": 32, "active": 40, "active_step_bytes": 48, "reserved": 56}
  # the seven fields in front are MpStepTrajectory's
  T = E.MpStepTrajectory
  for name, _ in T._fields_:
    assert getattr(T, name).offset == offsets[name] and getattr(T, name).size == getattr(M, name).size, name


def test_request_size_differs_from_every_other_request():
  others = [ctypes.sizeof(c) for c in (E.MpStatesHash, E.MpStateLayout, E.MpStatesCheck, E.MpStatesObserve,
                                       E.MpStatesView, E.MpKernelVariant, E.MpWorldStates, E.MpStepMany,
                                       E.MpStepTrajectory, E.MpEpisodeStarts)]
  assert sorted(others) == [40, 48, 56, 64, 72, 80, 88, 104, 112, 120]
  mine = ctypes.sizeof(E.MpStepActive)
  assert mine == 96 and mine not in others and mine < 448   # (a snapshot is >= 448 bytes)


def test_the_library_exports_what_it_exported():
  assert len(E.ABI_SYMBOLS) == 30   # (the request rides mp_restore)
  out = subprocess.run(["nm", "-D", "--defined-only", _build.build_engine()], capture_output=True, text=True,
                       check=True).stdout
  exported = sorted(line.split()[-1] for line in out.splitlines()
                    if line.split() and line.split()[-2] in ("T", "D", "B", "R"))
  assert exported == sorted(E.ABI_SYMBOLS)


def test_the_new_kernel_family_is_in_the_code_object():
  blob = open(_build.build_engine(), "rb").read()
  for level in LEVELS:
    assert f"k_many_active_{level}".encode() in blob, level


def test_the_mask_check_without_a_gpu():
  K, N = 6, 5
  check = E.check_step_active
  full = torch.ones((K, N), dtype=torch.uint8)
  for mask, step in ((full, N), (full.bool(), N), (full[0], 0), (full[0].bool(), 0),
                     (torch.ones((K, 3 * N), dtype=torch.uint8)[:, N:2 * N], 3 * N),
                     (torch.ones((K, 3 * N), dtype=torch.bool)[:, 2 * N:], 3 * N)):
    got, distance = check(mask, K, N)
    assert got is mask and distance == step
  assert check(full[:1], 1, N)[1] == N              # K = 1: one row
  # host data is handed back as a contiguous uint8 array of 0 / 1
  for host in (np.ones((K, N), np.uint8) * 255, np.ones((K, N), bool), [[True] * N] * K, [[0, 3, 1, 0, 1]] * K):
    got, distance = check(host, K, N)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (K, N) and distance == N
    assert got.flags["C_CONTIGUOUS"] and got.max() == 1
  got, distance = check([1, 0, 0, 1, 1], K, N)
  assert got.tolist() == [1, 0, 0, 1, 1] and distance == 0
  bad = [
      full.to(torch.int32), full.to(torch.int8), full.float(), full.long(),          # dtypes
      np.ones((K, N), np.int64), np.ones((K, N), np.float32), [[0.5] * N] * K,
      full[:, :N - 1], full[:K - 1], full.t(), torch.ones((N, K), dtype=torch.uint8),   # shapes
      full[None], torch.ones((), dtype=torch.uint8), torch.ones((N + 1,), dtype=torch.uint8),   # ranks
      np.ones((K, N, 1), np.uint8), [1] * (N - 1),
      torch.ones((K, 2 * N), dtype=torch.uint8)[:, ::2],                             # a row that is not contiguous
      torch.ones((2 * N,), dtype=torch.uint8)[::2],
      torch.ones((N,), dtype=torch.uint8).expand(K, N),                              # rows 0 < N apart
      torch.ones((K + N,), dtype=torch.uint8).as_strided((K, N), (1, 1)),            # overlapping rows
      torch.ones((K, N), dtype=torch.uint8).as_strided((K, N), (N - 1, 1)),          # a stride smaller than N
  ]
  for mask in bad:
    with pytest.raises(ValueError, match="active="):
      check(mask, K, N)


def test_the_library_refuses_a_request_without_an_engine():
  L = E.load_library()
  req = E.MpStepActive(ctypes.sizeof(E.MpStepActive), 1)
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"MpStepActive" in L.mp_last_error()
  # a buffer of that size with another struct_size is this request, refused as such
  host = np.zeros(ctypes.sizeof(req), np.uint8)
  assert L.mp_restore(None, host.ctypes.data, host.size) == E.MP_ERR_INVALID
  assert b"MpStepActive: struct_size" in L.mp_last_error()
  # ... and so are non-zero reserved words
  req.reserved[4] = 1
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"reserved" in L.mp_last_error()
