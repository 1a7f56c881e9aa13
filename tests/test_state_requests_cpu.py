"""The refusals of the saved-state requests that need no device — the NULL-engine refusals and the
host forms (MP_CHECK_HOST, MP_HASH_HOST, MP_HASH_MASK, MP_EGO_HOST, MP_VIEWHASH_HOST,
MP_EGOPLANES_HOST) — against tests/golden/state_request_refusals.json, which
tests/tools/make_state_request_refusals.py recorded: return code and message, byte for byte up to
pointers."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import make_state_request_refusals as T  # noqa: E402


@pytest.fixture(scope="module")
def golden():
  with open(T.GOLDEN) as f:
    return json.load(f)


def test_host_refusals_are_the_recorded_ones(golden):
  c = T.HostCtx()
  cases = T.cpu_cases(c)
  assert len({name for name, *_ in cases}) == len(cases) >= 100
  got = T.replay(c.L, cases)
  assert not [n for n in got if n not in golden], "a case the fixture lacks: record it"
  wrong = {n: (v, golden[n]) for n, v in got.items() if v != golden[n]}
  assert not wrong, wrong


def test_the_table_says_what_it_should(golden):
  """A few entries by hand, so that a fixture recorded from a broken library does not pass."""
  assert golden["observe/null_engine"] == [-1, "MpStatesObserve: NULL engine"]
  assert golden["hash_mask/counts_not_validated"] == [0, ""]
  assert golden["check_host/fingerprint"][1].endswith("is not this pack's (6f8038d69e9d1fc6)")
  assert golden["view_hash_host/no_rows_count_over"] == [
      -1, "MpViewHash: without a row list rows 0 .. count - 1 are hashed (count 4, there are 3 rows)"]
  assert golden["hash_host/no_rows_count_over"] == [
      -1, "MpStatesHash: without a row list rows 0 .. count - 1 are hashed (count 4, the bank has 3 rows)"]
  assert golden["load/null_engine"] == [-1, "mp_restore: bad buffer"]


def test_normalise():
  assert T.normalise("X (bank): [0x7f00aa, +16 bytes) runs past the end of its allocation (0x7f0000, 32 bytes)") == \
      "X (bank): [PTR, +16 bytes) runs past the end of its allocation"
  assert T.normalise("rows (nil) and out 0xdeadbeef must be 4-byte aligned") == \
      "rows (nil) and out PTR must be 4-byte aligned"
