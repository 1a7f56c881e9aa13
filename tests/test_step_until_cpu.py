"""Stopping worlds inside step_many (MpStepUntil) without a GPU: the argument check of
Engine.step_many's until=, stopped=, returns= and gamma= accepts and refuses what it should; a
request without an engine is refused by the library's own checks.  (The request's layout, wrappers
and kernels: tests/test_request_abi_cpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from meltingpot_amd import engine

E = engine
def test_the_argument_check_without_a_gpu():
  N, P = 5, 3
  check = E.check_step_until
  stopped = torch.zeros((N,), dtype=torch.uint8)
  ran = torch.zeros((N,), dtype=torch.int32)
  returns = torch.zeros((N, P), dtype=torch.float64)
  assert check(N, P) == 0
  assert check(N, P, until="last") == 1 and check(N, P, until="reward") == 2
  for both in (("last", "reward"), ["reward", "last"], {"last", "reward"}, iter(("last", "reward", "last"))):
    assert check(N, P, until=both) == 3
  assert check(N, P, until=()) == 0
  assert check(N, P, until="last", stopped=stopped, ran=ran, returns=returns, gamma=0.97) == 1
  assert check(N, P, returns=True) == 0 and check(N, P, returns=False, gamma=0) == 0
  assert check(N, P, stopped=stopped, device=torch.device("cpu")) == 0
  # rows [a, b) of a wider tensor are contiguous: what a mixture hands its members
  assert check(N, P, stopped=torch.zeros((3 * N,), dtype=torch.uint8)[N:2 * N],
               ran=torch.zeros((3 * N,), dtype=torch.int32)[2 * N:],
               returns=torch.zeros((3 * N, P), dtype=torch.float64)[N:2 * N]) == 0
  for until in ("first", "LAST", ("last", "paid"), 1, ("last", 2), "last,reward"):
    with pytest.raises(ValueError, match="until="):
      check(N, P, until=until)
  for bad in (stopped.bool(), stopped.to(torch.int8), stopped.to(torch.int32), stopped[:N - 1], stopped[None],
              torch.zeros((2 * N,), dtype=torch.uint8)[::2], np.zeros((N,), np.uint8), [0] * N):
    with pytest.raises(ValueError, match="stopped="):
      check(N, P, stopped=bad)
  for bad in (ran.long(), ran.to(torch.uint8), ran[:N - 1], torch.zeros((2 * N,), dtype=torch.int32)[::2],
              np.zeros((N,), np.int32)):
    with pytest.raises(ValueError, match="ran="):
      check(N, P, ran=bad)
  for bad in (returns.float(), returns.long(), returns[:, :P - 1], returns[:N - 1], returns.reshape(-1),
              returns.t(), torch.zeros((P, N), dtype=torch.float64).t(), np.zeros((N, P)), 1, "yes"):
    with pytest.raises(ValueError, match="returns="):
      check(N, P, returns=bad)
  for bad in (float("nan"), float("inf"), -float("inf"), None, "x"):
    with pytest.raises(ValueError, match="gamma="):
      check(N, P, returns=True, gamma=bad)
  for kw in (dict(stopped=stopped), dict(ran=ran), dict(returns=returns)):
    with pytest.raises(ValueError, match="lives on"):
      check(N, P, device=torch.device("cuda", 0), **kw)


def test_the_library_refuses_a_request_without_an_engine():
  L = E.load_library()

  def refused(**kw):
    req = E.MpStepUntil(ctypes.sizeof(E.MpStepUntil), 1)
    req.gamma = 1.0
    for key, value in kw.items():
      setattr(req, key, value)
    assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID, kw
    message = L.mp_last_error()
    assert b"MpStepUntil" in message, (kw, message)
    return message

  assert b"NULL engine" in refused()
  assert b"MpStepUntil: struct_size" in refused(struct_size=96)
  # a buffer of that size with another struct_size is this request, refused as such
  host = np.zeros(ctypes.sizeof(E.MpStepUntil), np.uint8)
  assert L.mp_restore(None, host.ctypes.data, host.size) == E.MP_ERR_INVALID
  assert b"MpStepUntil: struct_size" in L.mp_last_error()
  assert b"pad" in refused(pad=1)
  for i in range(5):
    words = [0] * 5
    words[i] = 1
    assert b"reserved" in refused(reserved=(ctypes.c_uint64 * 5)(*words))
  assert b"stop" in refused(stop=4)
  assert b"stop" in refused(stop=7)
  assert b"gamma" in refused(gamma=float("nan"))
  assert b"gamma" in refused(gamma=float("inf"))
