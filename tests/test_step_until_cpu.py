"""Stopping worlds inside step_many (MpStepUntil) without a GPU: include/mp_step_until.h compiles as
C99 and as C++17 and its request has the size and the offsets the library and the ctypes mirror
expect, its leading fields at MpStepActive's offsets and its size distinct from every other
request's; the argument check of Engine.step_many's until=, stopped=, returns= and gamma= accepts
and refuses what it should; the library exports what it exported; the new kernel family is in the
code object; a request without an engine is refused by the library's own checks."""
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
TAIL = ("stop", "pad", "stopped", "ran", "returns", "gamma", "reserved")

PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "mp_step_until.h"
int main(void) {
  /* (no engine: both wrappers answer MP_ERR_INVALID with the library's message) */
  int a = mp_step_many_until(NULL, NULL, 4, 0, 0, NULL, 0, NULL, 0, MP_STOP_LAST | MP_STOP_REWARD, NULL, NULL,
                             NULL, 0.97);
  int b = mp_step_until(NULL, NULL, 0, MP_STOP_LAST, NULL);
  printf("%u %u %u %u %u %u %u %u %u %u %d %d\n", (unsigned)sizeof(MpStepUntil),
         (unsigned)offsetof(MpStepUntil, active), (unsigned)offsetof(MpStepUntil, active_step_bytes),
         (unsigned)offsetof(MpStepUntil, stop), (unsigned)offsetof(MpStepUntil, pad),
         (unsigned)offsetof(MpStepUntil, stopped), (unsigned)offsetof(MpStepUntil, ran),
         (unsigned)offsetof(MpStepUntil, returns), (unsigned)offsetof(MpStepUntil, gamma),
         (unsigned)offsetof(MpStepUntil, reserved), a, b);
  return MP_STOP_LAST == 1 && MP_STOP_REWARD == 2 ? 0 : 1;
}
'''


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cc")])
def test_the_header_compiles_and_has_the_size_of_the_mirror(tmp_path, compiler, std, suffix):
  src = tmp_path / f"until.{suffix}"
  src.write_text(PROGRAM)
  exe = tmp_path / "until"
  subprocess.run([compiler, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                  _build.build_engine(), f"-Wl,-rpath,{os.path.dirname(_build.LIB_PATH)}"], check=True)
  out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
  M = E.MpStepUntil
  assert out == [str(ctypes.sizeof(M)), str(M.active.offset), str(M.active_step_bytes.offset)] + \
      [str(getattr(M, name).offset) for name in TAIL] + [str(E.MP_ERR_INVALID), str(E.MP_ERR_INVALID)]


def test_the_mirror_has_the_documented_layout():
  M, A = E.MpStepUntil, E.MpStepActive
  assert ctypes.sizeof(M) == 136
  offsets = {name: getattr(M, name).offset for name, _ in M._fields_}
  assert offsets == {"struct_size": 0, "steps": 4, "fields": 8, "num_rows": 12, "actions": 16,
                     "actions_step_bytes": 24, "rows": 32, "active": 40, "active_step_bytes": 48, "stop": 56,
                     "pad": 60, "stopped": 64, "ran": 72, "returns": 80, "gamma": 88, "reserved": 96}
  # the fields in front are MpStepActive's, at its offsets; the new ones begin where its reserved words do
  for name, _ in A._fields_:
    if name != "reserved":
      assert getattr(A, name).offset == offsets[name] and getattr(A, name).size == getattr(M, name).size, name
  assert A.reserved.offset == offsets["stop"]
  assert (E.MP_STOP_LAST, E.MP_STOP_REWARD) == (1, 2)


def test_request_size_differs_from_every_other_request():
  others = [ctypes.sizeof(c) for c in (E.MpStatesHash, E.MpStateLayout, E.MpStatesCheck, E.MpStatesObserve,
                                       E.MpStatesView, E.MpKernelVariant, E.MpWorldStates, E.MpStepMany,
                                       E.MpStepTrajectory, E.MpEpisodeStarts, E.MpStepActive)]
  assert sorted(others) == [40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120]
  mine = ctypes.sizeof(E.MpStepUntil)
  assert mine not in others and mine < 448   # (a snapshot is >= 448 bytes)


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
    assert f"k_many_until_{level}".encode() in blob, level
    assert f"k_many_active_{level}".encode() in blob, level   # (an MpStepActive request keeps its own)


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
