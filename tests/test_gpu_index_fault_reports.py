"""The deferred reports of an index a launch skipped: every case of
tests/tools/make_index_fault_reports.py — one request with one entry of its rows[], players[],
worlds[], src[] or classes[] out of range, then mp_sync — against
tests/golden/index_fault_reports.json (return code and message, byte for byte).  The kernels skip
the element and write the fault words by design; nothing faults."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import make_index_fault_reports as T  # noqa: E402

pytestmark = pytest.mark.gpu


def test_deferred_reports_are_the_recorded_ones():
  with open(T.GOLDEN) as f:
    golden = json.load(f)
  c = T.Ctx()
  got = T.replay(c, T.cases(c))
  for eng in (c.eng, c.short):   # each reported once: a report clears the word that claims it (the others stay)
    assert not eng.fault_words()[[0, 8, 9, 12, 32]].any(), eng.fault_words()[:40]
  c.close()
  assert set(got) == set(golden) == set(T.CODES)
  wrong = {n: (v, golden[n]) for n, v in got.items() if v != golden[n]}
  assert not wrong, wrong
