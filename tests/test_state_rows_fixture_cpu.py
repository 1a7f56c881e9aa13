"""Real rows through the host-only check: tests/golden/state_rows.npz holds records an engine
saved on a GPU (tests/tools/make_state_rows_fixture.py: per recipe pack, worlds 0 and 4 after
steps 1 (MID), 16 (LAST) and 17 (FIRST), and a row with a dead avatar where the recipe has one).
Every one of them is well-formed, the mutations of test_state_check_cpu.py get their exact
verdicts on them too, and the bytes nobody judges take any value."""
import functools
import os

import numpy as np
import pytest

import states_recipe as R
import test_state_check_cpu as C
from meltingpot_amd import engine as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_rows.npz")


@functools.lru_cache(maxsize=None)
def golden():
  return dict(np.load(GOLDEN))


def rows_of(name):
  return golden()[name + "/rows"]


def dead_row(name):
  return 6 if name in R.DEAD_AVATARS else None


@pytest.mark.parametrize("name", R.PACKS)
def test_every_fixture_row_is_well_formed(name):
  rows, lay = rows_of(name), C.layout(name)
  assert lay.fingerprint == int(golden()[name + "/fingerprint"][0]), "the record layout changed: regenerate the fixture"
  assert rows.shape == (6 if dead_row(name) is None else 7, lay.world_stride)
  v = C.verdicts(name, rows)
  assert not v.any(), [lay.describe(*x) for x in v]
  f = C.fields(name, rows)
  assert [int(s) for s in f.step[:6]] == [1, 1, 16, 16, 0, 0] and [int(d) for d in f.done[:6]] == [0, 0, 1, 1, 0, 0]
  if dead_row(name) is not None:
    assert bool((f.alive[6] == 0).any())
  with pytest.raises(ValueError, match="fingerprint"):
    E.check_states_host(R.pack(name), rows, fingerprint=lay.fingerprint ^ 1)


@pytest.mark.parametrize("name", R.PACKS)
def test_mutations_of_real_rows_get_their_exact_verdict(name):
  lay, rows = C.layout(name), rows_of(name)
  muts = C.all_mutations(name, rows, dead_row(name))
  bank = np.concatenate([C.apply(name, m, rows) for m in muts])
  for m, v in zip(muts, C.verdicts(name, bank)):
    assert tuple(int(x) for x in v) == m[2], (name, m[0], lay.describe(*v), "wanted", lay.describe(*m[2]))


@pytest.mark.parametrize("name", R.PACKS)
def test_unjudged_bytes_of_real_rows_take_any_value(name):
  lay = C.layout(name)
  rows = C.junk_unjudged(name, rows_of(name))
  v = C.verdicts(name, rows)
  assert not v.any(), [lay.describe(*x) for x in v]
