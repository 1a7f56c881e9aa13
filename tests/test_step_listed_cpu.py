"""Stepping a device list of worlds (MpStepListed) without a GPU: the argument check of worlds=
accepts and refuses what it should; a request without an engine is refused by the library's own
checks.  (The request's layout, wrappers and kernels: tests/test_request_abi_cpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from meltingpot_amd import engine

E = engine
def test_the_argument_check_without_a_gpu():
  N, P, M, K = 5, 3, 3, 4
  check = E.check_step_listed
  shapes = {E.OBS_REWARD: ((N, P), "torch.float64"), E.OBS_STEP_TYPE: ((N,), "torch.int32"),
            E.OBS_POSITION: ((N, P, 2), "torch.int32")}
  # the list: 1-D integers, a tensor, an array or a list; the values are the device's to check
  for worlds in ([3, 0, 4], (3, 0, 4), np.array([3, 0, 4]), np.array([3, 0, 4], np.int32),
                 torch.tensor([3, 0, 4]), torch.tensor([3, 0, 4], dtype=torch.int32), [2, 7, 2]):
    assert check(worlds, N, P) == M
  assert check([0], N, P) == 1 and check([4, 2, 0, 3, 1], N, P) == N
  for bad in ([[3, 0, 4]], np.zeros((3, 1), np.int32), torch.zeros((1, 3), dtype=torch.int32), 3,
              [0.0, 1.0], np.array([1.0, 2.0]), torch.tensor([1.0]), [True, False], "012"):
    with pytest.raises(ValueError, match="worlds= must be 1-D integers"):
      check(bad, N, P)
  with pytest.raises(ValueError, match="names no world"):
    check([], N, P)
  with pytest.raises(ValueError, match="names no world"):
    check(torch.zeros((0,), dtype=torch.int32), N, P)
  with pytest.raises(ValueError, match="more entries than worlds"):
    check([0, 1, 2, 3, 4, 0], N, P)
  # everything per world has M columns
  w = [3, 0, 4]
  actions = np.zeros((K, M, P), np.int32)
  assert check(w, N, P, actions=actions) == M
  assert check(w, N, P, actions=torch.zeros((M, P), dtype=torch.int32), repeat=K) == M
  assert check(w, N, P, actions=np.zeros((K, M, P, 2), np.int32), num_fields=2) == M
  for bad in (np.zeros((K, N, P), np.int32), np.zeros((K, M, P + 1), np.int32), np.zeros((M, P), np.int32)):
    with pytest.raises(ValueError, match="one column per entry"):
      check(w, N, P, actions=bad)
  with pytest.raises(ValueError, match="one column per entry"):
    check(w, N, P, actions=np.zeros((N, P), np.int32), repeat=K)
  assert check(w, N, P, actions=actions, active=np.ones((K, M), np.uint8)) == M
  assert check(w, N, P, actions=actions, active=torch.ones((M,), dtype=torch.bool)) == M
  for bad in (np.ones((K, N), np.uint8), np.ones((N,), np.uint8), torch.ones((K, N), dtype=torch.uint8)):
    with pytest.raises(ValueError, match="active="):
      check(w, N, P, actions=actions, active=bad)
  assert check(w, N, P, lengths=torch.tensor([1, 2, 3])) == M
  assert check(w, N, P, lengths=np.array([1, 2, 3])) == M
  for bad in (torch.tensor([1, 2, 3, 4, 5]), np.arange(N), torch.tensor([1.0, 2.0, 3.0])):
    with pytest.raises(ValueError, match="lengths="):
      check(w, N, P, lengths=bad)
  good = {"reward": torch.zeros((K, M, P), dtype=torch.float64), "step_type": torch.zeros((K, M), dtype=torch.int32),
          E.OBS_POSITION: torch.zeros((K, M, P, 2), dtype=torch.int32), "ran": torch.zeros((M,), dtype=torch.int32),
          "returns": torch.zeros((M, P), dtype=torch.float64), "hashes": torch.zeros((K, M), dtype=torch.int64),
          "states": torch.zeros((K, M, 64), dtype=torch.uint8),
          "stopped": torch.zeros((N,), dtype=torch.uint8)}   # (by world)
  assert check(w, N, P, actions=actions, out=good, shapes=shapes) == M
  sized_for_n = {"reward": torch.zeros((K, N, P), dtype=torch.float64),
                 "step_type": torch.zeros((K, N), dtype=torch.int32),
                 E.OBS_POSITION: torch.zeros((K, N, P, 2), dtype=torch.int32),
                 "ran": torch.zeros((N,), dtype=torch.int32), "returns": torch.zeros((N, P), dtype=torch.float64),
                 "hashes": torch.zeros((K, N), dtype=torch.int64), "states": torch.zeros((K, N, 64), dtype=torch.uint8)}
  for key, tensor in sized_for_n.items():
    with pytest.raises(ValueError, match="out"):
      check(w, N, P, actions=actions, out={key: tensor}, shapes=shapes)


def test_the_library_refuses_a_request_without_an_engine():
  L = E.load_library()

  def refused(**kw):
    req = E.MpStepListed(ctypes.sizeof(E.MpStepListed), 1)
    req.gamma = 1.0
    req.count = 1
    for key, value in kw.items():
      setattr(req, key, value)
    assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) in (E.MP_ERR_INVALID, E.MP_ERR_NO_DEVICE), kw
    message = L.mp_last_error()
    assert b"MpStepListed" in message, (kw, message)
    return message

  assert b"NULL engine" in refused()
  assert b"MpStepListed: struct_size" in refused(struct_size=136)
  # a buffer of that size with another struct_size is this request, refused as such
  host = np.zeros(ctypes.sizeof(E.MpStepListed), np.uint8)
  assert L.mp_restore(None, host.ctypes.data, host.size) == E.MP_ERR_INVALID
  assert b"MpStepListed: struct_size" in L.mp_last_error()
  assert b"pad" in refused(pad=1)
  assert b"reserved2" in refused(reserved2=1)
  for i in range(5):
    words = [0] * 5
    words[i] = 1
    assert b"reserved" in refused(reserved=(ctypes.c_uint64 * 5)(*words))
  for i in range(3):
    words = [0] * 3
    words[i] = 1
    assert b"reserved" in refused(reserved3=(ctypes.c_uint64 * 3)(*words))
  assert b"stop" in refused(stop=4)
  assert b"gamma" in refused(gamma=float("nan"))
