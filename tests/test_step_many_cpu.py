"""Action sequences (MpStepMany: K steps of every world in one submission) on the host side: the
header's struct equals the ctypes one next to an unchanged ABI, the library exports what it
exported and contains the nine K-step kernels, NULL and empty requests are refused before a device
is looked for, the C wrapper compiles and links, and the shape rules hold without an engine."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from meltingpot_amd import _build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("k_step_many_clean_up", "k_step_many_commons", "k_step_many_coins", "k_step_many_coop",
           "k_step_many_gift", "k_step_many_cook", "k_step_many_mushroom", "k_step_many_matrix",
           "k_step_many_territory")


def _header():
  return open(os.path.join(ROOT, "include", "mp_engine.h")).read()


def test_header_struct_equals_the_ctypes_struct_and_abi_stays_8():
  text = _header()
  body = text[text.index("typedef struct {\n  uint32_t struct_size;        /* = sizeof(MpStepMany)"):]
  body = body[:body.index("} MpStepMany;")]
  fields = re.findall(r"^\s+(?:const\s+)?\w+\*?\s+(\w+)(?:\[5\])?;", body, re.M)
  assert fields == [f for f, _ in engine.MpStepMany._fields_]
  size = ctypes.sizeof(engine.MpStepMany)
  assert size != ctypes.sizeof(engine.MpWorldStates) == 56 and size < 448
  assert engine.MpStepMany.per_step.size == 40 and engine.MpStepMany.per_step_bytes.size == 40
  assert re.search(r"#define MP_ABI_VERSION 8\b", text)
  assert re.search(rf"#define MP_STEP_MANY_MAX {engine.STEP_MANY_MAX}\b", text)
  assert engine.load_library().mp_abi_version() == engine.MP_ABI_VERSION == 8
  # the new text sits behind the MpWorldStates typedef (the load groups' comment ends at its enum)
  assert text.index("} MpWorldStates;") < text.index("sizeof(MpStepMany)")
  wrapper = open(os.path.join(ROOT, "include", "mp_step_many.h")).read()
  assert re.search(r"static inline int mp_step_many\(MpEngine\* eng, const int32_t\* actions_device", wrapper)


def test_the_request_adds_no_exported_symbol():
  out = subprocess.run(["nm", "-D", "--defined-only", _build.build_engine()], capture_output=True,
                       text=True, check=True).stdout
  names = {line.split()[-1] for line in out.splitlines()
           if line.split() and line.split()[-2] in ("T", "D", "B", "R")}
  assert names == set(engine.ABI_SYMBOLS) and len(names) == 30
  assert "mp_step_many" not in names


def test_null_engine_and_zero_steps_are_invalid_without_a_device():
  L = engine.load_library()
  req = engine.MpStepMany(ctypes.sizeof(engine.MpStepMany), 4)
  req.actions = 0x1000   # (never dereferenced: there is no engine)
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == engine.MP_ERR_INVALID
  assert b"MpStepMany" in L.mp_last_error()
  req.steps = 0
  assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == engine.MP_ERR_INVALID
  assert L.mp_restore(None, None, ctypes.sizeof(req)) == engine.MP_ERR_INVALID


def test_the_c_wrapper_compiles_and_links_against_the_library(tmp_path):
  lib = _build.build_engine()
  src = tmp_path / "m.c"
  src.write_text('#include <stdio.h>\n#include "mp_step_many.h"\n'
                 "int main(void) {\n"
                 "  void* rows[5] = {0, 0, 0, 0, 0};\n"
                 "  uint64_t dist[5] = {0, 0, 0, 0, 0};\n"
                 '  printf("%d %d %d %d\\n", mp_step_many(NULL, NULL, 4, 0, 0, rows, dist),\n'
                 "         mp_step_many(NULL, NULL, 0, 0, 0, NULL, NULL), (int)sizeof(MpStepMany),\n"
                 "         MP_STEP_MANY_MAX);\n"
                 "  return 0;\n}\n")
  exe = tmp_path / "m"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                  "-o", str(exe), lib, f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
  out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
  assert out == [str(engine.MP_ERR_INVALID), str(engine.MP_ERR_INVALID),
                 str(ctypes.sizeof(engine.MpStepMany)), str(engine.STEP_MANY_MAX)]


def test_library_contains_the_nine_k_step_kernels():
  path = _build.build_engine()
  out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", path],
                       capture_output=True, text=True).stdout
  assert "gfx950" in out
  blob = open(path, "rb").read()
  for kernel in KERNELS:
    assert kernel.encode() in blob, kernel


def test_shape_rules_hold_without_an_engine():
  N, P = 6, 3
  check = engine.check_step_many
  assert check((5, N, P), torch.int32, N, P) == 5
  assert check((5, N, P), np.dtype(np.int64), N, P) == 5
  assert check((N, P), torch.int32, N, P, repeat=9) == 9
  assert check((2, N, P, 4), torch.int32, N, P, num_fields=4) == 2
  assert check((engine.STEP_MANY_MAX, N, P), torch.int32, N, P) == engine.STEP_MANY_MAX
  bad = [dict(shape=(N, P)),                                   # wrong rank
         dict(shape=(5, N, P, 1)),
         dict(shape=(5, N + 1, P)),                            # wrong N
         dict(shape=(5, N, P + 1)),                            # wrong P
         dict(shape=(5, N, P), dtype=torch.float32),           # float dtype
         dict(shape=(5, N, P), dtype=np.dtype(np.float64)),
         dict(shape=(5, N, P), repeat=5),                      # repeat with a [K, N, P] tensor
         dict(shape=(N, P), repeat=0),
         dict(shape=(N, P), repeat=engine.STEP_MANY_MAX + 1),  # K above the maximum
         dict(shape=(engine.STEP_MANY_MAX + 1, N, P)),
         dict(shape=(0, N, P)),
         dict(shape=(5, N, P), num_fields=4),                  # fields without the field axis
         dict(shape=(5, N, P, 3), num_fields=4)]
  for case in bad:
    with pytest.raises(ValueError, match="step_many"):
      check(case["shape"], case.get("dtype", torch.int32), N, P, repeat=case.get("repeat"),
            num_fields=case.get("num_fields"))
