"""Which handler, if any, a (carrier, buffer size) pair reaches: every one of the 18 requests' sizes
through mp_snapshot and through mp_restore with a NULL engine, a size no request has, and a NULL
buffer, against tests/golden/request_dispatch.json, which
tests/tools/make_state_request_refusals.py recorded: return code and message.  No device."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import make_state_request_refusals as T  # noqa: E402


@pytest.fixture(scope="module")
def golden():
  with open(T.DISPATCH) as f:
    return json.load(f)


def test_dispatch_is_the_recorded_one(golden):
  cases = T.dispatch_cases()
  assert len({name for name, *_ in cases}) == len(cases) == 2 * (18 + 2)
  got = T.replay_dispatch(T.E.load_library(), cases)
  assert set(got) == set(golden)
  wrong = {n: (v, golden[n]) for n, v in got.items() if v != golden[n]}
  assert not wrong, wrong


def test_the_table_says_what_it_should(golden):
  """Entries by hand, so that a fixture recorded from a broken library does not pass."""
  # a request reaches its handler through its own carrier only; through the other it is no request
  assert golden["MpStatesObserve/mp_snapshot"] == [-1, "MpStatesObserve: NULL engine"]
  assert golden["MpStatesObserve/mp_restore"] == [-1, "mp_restore: bad buffer"]
  assert golden["MpStepListed/mp_restore"] == [-1, "MpStepListed: NULL engine or actions"]
  assert golden["MpStepListed/mp_snapshot"] == [-1, "mp_snapshot: bad buffer"]
  # MpWorldStates goes through both, and through neither without an engine
  assert golden["MpWorldStates/mp_snapshot"] == [-1, "mp_snapshot: bad buffer"]
  assert golden["MpWorldStates/mp_restore"] == [-1, "mp_restore: bad buffer"]
  # the host forms are reached without an engine
  assert golden["MpViewHash/mp_snapshot"] == [-1, "MpViewHash: unknown op 0"]
  assert golden["MpKernelVariant/mp_snapshot"] == [-1, "mp_create: bad MpConfig (struct_size)"]
  for carrier in T.CARRIERS:
    assert golden[f"odd_size/{carrier}"] == golden[f"null_buffer/{carrier}"] == [-1, f"{carrier}: bad buffer"]
  reached = sorted(n for n, (_, text) in golden.items() if "bad buffer" not in text)
  assert len(reached) == 17 and all(golden[n][0] == -1 for n in golden)
