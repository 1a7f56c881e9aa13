"""Registered episode starts without a GPU: include/mp_episode_starts.h compiles as C99 and as
C++17 and its request has the size the library and the ctypes mirror expect, distinct from every
other request's; the Python argument check refuses bad shapes, dtypes and devices; the library
exports what it exported; the new kernel families are in the code object; a request without a
device is refused by the library's own checks."""
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
#include <stdio.h>
#include "mp_episode_starts.h"
int main(void) {
  /* (no engine: both wrappers answer MP_ERR_INVALID with the library's message) */
  int a = mp_set_episode_starts(NULL, NULL, 1, NULL, NULL, 0, 0);
  int b = mp_clear_episode_starts(NULL);
  printf("%u %d %d\n", (unsigned)sizeof(MpEpisodeStarts), a, b);
  return 0;
}
'''


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cc")])
def test_the_header_compiles_and_has_the_size_of_the_mirror(tmp_path, compiler, std, suffix):
  src = tmp_path / f"starts.{suffix}"
  src.write_text(PROGRAM)
  exe = tmp_path / "starts"
  subprocess.run([compiler, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                  _build.build_engine(), f"-Wl,-rpath,{os.path.dirname(_build.LIB_PATH)}"], check=True)
  out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
  assert out == [str(ctypes.sizeof(E.MpEpisodeStarts)), str(E.MP_ERR_INVALID), str(E.MP_ERR_INVALID)]


def test_request_size_differs_from_every_other_request():
  others = [ctypes.sizeof(c) for c in (E.MpStatesHash, E.MpStateLayout, E.MpStatesCheck, E.MpStatesObserve,
                                       E.MpKernelVariant, E.MpWorldStates, E.MpStepMany, E.MpStepTrajectory)]
  mine = ctypes.sizeof(E.MpEpisodeStarts)
  assert mine == 72 and mine not in others and mine < 448   # (a snapshot is >= 448 bytes)


def test_the_library_exports_what_it_exported():
  assert len(E.ABI_SYMBOLS) == 30   # (the request rides mp_restore)
  out = subprocess.run(["nm", "-D", "--defined-only", _build.build_engine()], capture_output=True, text=True,
                       check=True).stdout
  exported = sorted(line.split()[-1] for line in out.splitlines()
                    if line.split() and line.split()[-2] in ("T", "D", "B", "R"))
  assert exported == sorted(E.ABI_SYMBOLS)


def test_the_new_kernel_families_are_in_the_code_object():
  blob = open(_build.build_engine(), "rb").read()
  for level in LEVELS:
    assert f"k_step_starts_{level}".encode() in blob, level
    assert f"k_many_starts_{level}".encode() in blob, level


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
