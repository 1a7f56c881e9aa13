"""The MpStatesView request without a GPU: the call without an engine.  (Its struct, wrapper and
kernels: tests/test_request_abi_cpu.py; what the request draws is held to the step launches where an
engine runs: tests/test_gpu_observe_views.py.)"""
import ctypes

from meltingpot_amd import engine as E


def test_without_an_engine_the_request_is_refused():
  L = E.load_library()
  req = E.MpStatesView(ctypes.sizeof(E.MpStatesView))
  assert L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"MpStatesView" in L.mp_last_error()
