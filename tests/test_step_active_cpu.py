"""Stepping some of the worlds (MpStepActive) without a GPU: the mask check of Engine.step /
Engine.step_many refuses bad dtypes, ranks, shapes and strides; a request without an engine is
refused by the library's own checks.  (The request's layout, wrappers and kernels:
tests/test_request_abi_cpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from meltingpot_amd import engine

E = engine
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
