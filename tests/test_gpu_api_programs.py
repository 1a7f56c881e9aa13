"""One engine driven through a long, seeded, arbitrary sequence of API calls — resets, masked
re-seeds, device / host / raw-field steps, step_many with and without rows, saves, loads, snapshots,
restores and views bound and unbound in between — against the oracle-backed model of
tests/engine_model.py after EVERY call (records, transition kinds, record-function kinds, step_many's
rows, bad_actions, every bound view and ring slot), and against a twin engine of the other launch
form (unfused, generic kernels, no view bound) on every output kind the level produces and on the
saved records: tests/api_programs.py.  One program per committed (seed, profile): three per level
(n = 5, 13, 37; one with a rollout ring, one with WORLD.RGB pooled by 8) on packs whose episodes
end after 17 frames, and two on the committed clean_up pack, where the kernels with its constants
compiled in run.

The second test runs the STATE programs (api_programs.STATE_COMMITTED): the same thirteen classes
plus masked steps, masked and stopping K-step calls with a persistent `stopped`, per-step state rows
that become banks, registered episode starts whose `rows` are rewritten on the device, and reads of
saved states (observe_states, observe_views, the hashes, check_states) — two programs per level with
6 and 23 worlds (a last workgroup of 2 and of 3) on the levels' variants that pay often, and one on
the committed clean_up pack.  There the twin runs the other form of every new K-step call, the host
loop of masked single steps, and performs a registration's defining identity with load_worlds.

The third test runs the UNIT programs (api_programs.UNIT_COMMITTED): the state classes plus listed
steps (with entries that are no world and entries that repeat one, in tensors filled beforehand),
episode statistics registered, re-registered and cleared, and the three view units (EGO_LAYER, the
view hashes, the planes) registered in any subset, in place or as rings, and read from bank rows and
live worlds.  After every op the statistics tensors equal the model's fold bit for bit and the
library's host fold of what the twin's single steps left; every registered tensor equals the model's
function of all N records and the library's host form of save_worlds(), and changes only behind a
submission.  The twin registers nothing, so everything it is compared on shows that a registration
changes no record and no output."""
import pytest

import api_programs as ap
from meltingpot_amd import engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,profile", ap.COMMITTED, ids=[p["name"] for _, p in ap.COMMITTED])
def test_program(seed, profile):
  program = ap.make_program(seed, profile)
  eng, twin = ap.make_engines(profile)
  model = ap.make_model(profile)
  try:
    if profile["stock"]:
      assert eng.plan["stock"] == engine.KERNEL_STOCK
      assert twin.plan["stock"] == engine.KERNEL_GENERIC
    else:
      assert eng.plan["stock"] == engine.KERNEL_GENERIC
    assert ap.run_program(program, eng, model, twin) == len(program)
    if profile["ring"]:
      assert eng.ring["slots"] == ap.RING_SLOTS
  finally:
    eng.close(); twin.close(); model.close()


@pytest.mark.parametrize("seed,profile", ap.STATE_COMMITTED, ids=[p["name"] for _, p in ap.STATE_COMMITTED])
def test_state_program(seed, profile):
  program = ap.make_program(seed, profile)
  eng, twin = ap.make_engines(profile)
  model = ap.make_model(profile)
  try:
    if profile["stock"]:
      assert eng.plan["stock"] == engine.KERNEL_STOCK
      assert twin.plan["stock"] == engine.KERNEL_GENERIC
    else:
      assert eng.plan["stock"] == engine.KERNEL_GENERIC
    assert ap.run_program(program, eng, model, twin) == len(program)
  finally:
    eng.close(); twin.close(); model.close()


@pytest.mark.parametrize("seed,profile", ap.UNIT_COMMITTED, ids=[p["name"] for _, p in ap.UNIT_COMMITTED])
def test_unit_program(seed, profile):
  import collections
  program = ap.make_program(seed, profile)
  eng, twin = ap.make_engines(profile)
  model = ap.make_model(profile)
  cover = collections.Counter()
  try:
    if profile["stock"]:
      assert eng.plan["stock"] == engine.KERNEL_STOCK
      assert twin.plan["stock"] == engine.KERNEL_GENERIC
    else:
      assert eng.plan["stock"] == engine.KERNEL_GENERIC
    assert ap.run_program(program, eng, model, twin, cover=cover) == len(program)
    print("cover", profile["name"], dict(sorted(cover.items())))
    if profile["ring"]:
      assert eng.ring["slots"] == ap.RING_SLOTS
    # (the runner has stopped on any other word after every op: only a bad entry's report was ever set)
    words = eng.fault_words()[:18].copy()
    if any(op.get("bad") and not op.get("refused") for op in program):
      assert (words[11] & 255) in ap.LISTED_FAULTS + (0,), words
      words[9:12] = 0
    assert not words.any(), eng.fault_words()[:18]
    assert not twin.fault_words()[:18].any()
  finally:
    eng.close(); twin.close(); model.close()
