"""The MpStatesView request without a GPU: its C struct as a C compiler lays it out against the
ctypes mirror, its size against every other request's (mp_snapshot tells them apart by size), the
library's exported symbols, and the call without an engine.  (What the request draws is held to the
step launches where an engine runs: tests/test_gpu_observe_views.py.)"""
import ctypes
import os
import subprocess

from meltingpot_amd import _build
from meltingpot_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "kind", "fingerprint", "bank", "rows", "players", "dst", "dst_bytes",
          "bank_rows", "count", "reserved")


def test_the_c_struct_is_the_ctypes_mirror(tmp_path):
  src = tmp_path / "view.c"
  prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(MpStatesView, {f}));' for f in FIELDS)
  src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mp_states_view.h"\n'
                 "int main(void) {\n"
                 '  printf("sizeof %zu\\n", sizeof(MpStatesView));\n' + prints + "\n"
                 "  /* (the wrapper compiles and refuses a NULL engine on the host) */\n"
                 '  printf("rc %d\\n", mp_observe_views(NULL, MP_OBS_RGB, NULL, 0, NULL, NULL, 0, NULL, 0, 0));\n'
                 "  return 0;\n}\n")
  exe = tmp_path / "view"
  _build.build_engine()
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                  _build.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_build.LIB_PATH)}"], check=True)
  out = dict(line.split() for line in
             subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(E.MpStatesView) == 80
  assert [f for f, _ in E.MpStatesView._fields_] == list(FIELDS)
  for f in FIELDS:
    assert int(out[f]) == getattr(E.MpStatesView, f).offset, f
  assert int(out["rc"]) == E.MP_ERR_INVALID


def test_its_size_is_no_other_request_s():
  others = (E.MpStatesObserve, E.MpStatesHash, E.MpStateLayout, E.MpStatesCheck, E.MpKernelVariant,
            E.MpWorldStates, E.MpStepMany, E.MpStepTrajectory, E.MpEpisodeStarts)
  sizes = [ctypes.sizeof(c) for c in others]
  assert ctypes.sizeof(E.MpStatesView) not in sizes and len(set(sizes)) == len(sizes)
  assert ctypes.sizeof(E.MpStatesView) < 448   # (no engine's snapshot is that small)


def test_the_library_still_exports_its_thirty_symbols():
  out = subprocess.run(["nm", "-D", "--defined-only", _build.build_engine()], capture_output=True, text=True,
                       check=True).stdout
  names = {line.split()[-1] for line in out.splitlines()
           if line.split() and line.split()[-2] in ("T", "D", "B", "R")}
  assert names == set(E.ABI_SYMBOLS) and len(names) == 30
  blob = open(_build.build_engine(), "rb").read()
  assert b"k_state_view" in blob and b"k_view_scalar" in blob   # (the request's own kernels are in it)


def test_without_an_engine_the_request_is_refused():
  L = E.load_library()
  req = E.MpStatesView(ctypes.sizeof(E.MpStatesView))
  assert L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"MpStatesView" in L.mp_last_error()
