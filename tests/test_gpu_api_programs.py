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
loop of masked single steps, and performs a registration's defining identity with load_worlds."""
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
