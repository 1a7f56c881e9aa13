"""Registered episode starts without a GPU: the Python argument check refuses bad shapes, dtypes
and devices; a request without a device is refused by the library's own checks.  (The request's
layout, wrappers and kernels: tests/test_request_abi_cpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from meltingpot_amd import engine

E = engine
def test_the_argument_check_without_a_gpu():
  N, S, M = 5, 64, 7
  cpu = torch.device("cpu")
  bank = torch.zeros((M, S), dtype=torch.uint8)
  rows = torch.full((N,), -1, dtype=torch.int32)
  verdicts = torch.zeros((M, 2), dtype=torch.int32)
  check = E.check_episode_starts
  assert check(bank, rows, None, N, S, cpu) == M
  assert check(bank, rows, verdicts, N, S, cpu) == M
  bad = [
      (dict(bank=bank.numpy()), "bank"),                              # no tensor
      (dict(bank=bank.to(torch.int8)), "bank"),                       # dtype
      (dict(bank=bank.view(-1)), "bank"),                             # one dimension
      (dict(bank=torch.zeros((M, S + 16), dtype=torch.uint8)), "bank"),   # another row size
      (dict(bank=torch.zeros((M, 2 * S), dtype=torch.uint8)[:, :S]), "bank"),   # not contiguous
      (dict(bank=bank[:0]), "no rows"),
      (dict(rows=rows.long()), "rows"),
      (dict(rows=rows[:N - 1]), "rows"),
      (dict(rows=torch.zeros((N, 1), dtype=torch.int32)), "rows"),
      (dict(rows=torch.zeros((2 * N,), dtype=torch.int32)[::2]), "rows"),
      (dict(rows=[-1] * N), "rows"),
      (dict(verdicts=verdicts.long()), "verdicts"),
      (dict(verdicts=verdicts[:M - 1]), "verdicts"),
      (dict(verdicts=torch.zeros((M,), dtype=torch.int32)), "verdicts"),
      (dict(verdicts=torch.zeros((M, 4), dtype=torch.int32)[:, ::2]), "verdicts"),
  ]
  for change, message in bad:
    args = dict(bank=bank, rows=rows, verdicts=verdicts)
    args.update(change)
    with pytest.raises(ValueError, match=message):
      check(args["bank"], args["rows"], args["verdicts"], N, S, cpu)
  # host tensors for an engine on a GPU: each of the three is named
  for device in ("cuda:0", torch.device("cuda", 1)):
    with pytest.raises(ValueError, match="bank lives on cpu"):
      check(bank, rows, verdicts, N, S, device)
  meta = torch.device("meta")
  with pytest.raises(ValueError, match="rows lives on cpu"):
    check(bank.to(meta), rows, None, N, S, meta)
  with pytest.raises(ValueError, match="verdicts lives on cpu"):
    check(bank.to(meta), rows.to(meta), verdicts, N, S, meta)


def test_the_library_refuses_a_request_without_an_engine():
  L = E.load_library()
  req = E.MpEpisodeStarts(ctypes.sizeof(E.MpEpisodeStarts))
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"MpEpisodeStarts" in L.mp_last_error()
  # and a buffer of that size with another struct_size is this request, refused as such
  host = np.zeros(ctypes.sizeof(req), np.uint8)
  assert L.mp_restore(None, host.ctypes.data, host.size) == E.MP_ERR_INVALID
