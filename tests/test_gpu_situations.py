"""The step kernels against the oracle on enumerated small situations (tests/situations.py): every
world of one batched launch is another hand-built position — pairs and triples of movers that
want one cell, swaps, moves into a cell vacated in the same frame, across the seam of a torus,
beams at every cell of their footprint and among the dirt, walls and resources of the stock maps,
respawns onto taken spawn points, and the scripted scenes of the oracle's own CPU tests — stated once and applied to both sides, the engine's through `state_fields`-style edits of saved
rows.  Each scope runs through the stand-alone step kernels and through the fused launch with
one view bound; clean_up's pairs also through step_many(K = 1) and step(active = all ones).

Before any step the bridge itself is checked (check_states all zero, a checked load, equal dumps):
a failure there is a situations.ConstructionError, not a parity failure.  Everything is bit-exact."""
import numpy as np
import pytest

import situations as S

pytestmark = pytest.mark.gpu

LEVELS = ("clean_up", "commons_harvest__open", "territory__rooms")
TWO_FORMS = ("standalone", "fused")


def _hold(builder, args, form):
  scope, ref = S.reference(builder, *args)
  assert scope.n == scope.count, (scope.name, scope.n, scope.count)   # nothing sampled away
  assert ref["accepted"].all(), scope.name
  compared = S.run_engine(scope, ref, form)
  assert compared == scope.count
  return scope, ref


@pytest.mark.parametrize("level,form", [(l, f) for l in LEVELS for f in TWO_FORMS] +
                         [("clean_up", "step_many"), ("clean_up", "active")])
def test_pairs_of_movers(level, form):
  scope, ref = _hold(S.pair_scope, (level,), form)
  assert scope.count == 4800
  won = S.pair_outcomes(scope, ref)
  # the seeds differ between worlds, so the shuffled visiting order does: both orders occur
  assert len(won["A"]) and len(won["B"]) and len(won["neither"]) and not len(won["both"]), won


@pytest.mark.parametrize("level,half,form", [(l, h, f) for l in LEVELS for h in (0, 1) for f in TWO_FORMS])
def test_three_movers_around_one_cell(level, half, form):
  scope, ref = _hold(S.triple_half, (level, half), form)
  assert scope.count == 3456
  # where two or three enter, exactly one arrives, and each of the three does somewhere
  centre = S.PATCHES[level][1]
  on_centre = (ref["avat"][1][:, :, :2] == np.array(centre)).all(2)
  crowd = scope.tags["entering"] >= 2
  assert (on_centre[crowd].sum(1) == 1).all()
  assert on_centre[crowd].any(0).all()


@pytest.mark.parametrize("form", TWO_FORMS)
def test_pairs_of_movers_across_the_seam(form):
  scope, ref = _hold(S.pair_scope, ("clean_up", "seam"), form)
  assert scope.count == 4800
  H, W = ref["grid"].shape[-2:]
  xy = ref["avat"][1][:, :, :2]
  for corner in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W - 2, 0), (0, H - 2), (2, 0), (0, 2)):
    assert (xy == np.array(corner)).all(2).any(), corner   # moves ended on both sides of both edges


@pytest.mark.parametrize("level,form", [(l, f) for l in LEVELS for f in TWO_FORMS])
def test_beams_at_every_cell_of_their_footprint(level, form):
  """clean_up: zap and clean; commons_harvest__open: zap, on through the removal to the respawn;
  territory__rooms: zap (twice: mark, then remove) and claim.  Targets standing, shielded by a
  nearer avatar (A4), leaving, arriving, and zapping in the same step."""
  scope, ref = _hold(S.beam_scope, (level,), form)
  assert scope.count == {"clean_up": 1702, "commons_harvest__open": 852, "territory__rooms": 624}[level]
  dead = [(ref["avat"][s][:, :, 3] == 0).any() for s in range(scope.steps + 1)]
  assert not dead[0] and any(dead)                       # somebody is removed ...
  if level == "commons_harvest__open":
    assert not dead[-1]                                  # ... and there everybody is back at the end


@pytest.mark.parametrize("form", TWO_FORMS)
def test_respawn_onto_taken_spawn_points(form):
  scope, ref = _hold(S.respawn_scope, (), form)
  assert scope.count == 1600
  alive = np.stack([ref["avat"][s][:, :, 3].sum(1) for s in range(scope.steps + 1)])
  assert (alive[:5] == 3).all()                          # the timer of 4 frames
  back = alive[5:] == 4
  assert back[0].any() and not back[0].all()             # some land at once, some on a taken point ...
  assert (back[-1] & ~back[0]).any()                     # ... and land in a later frame


@pytest.mark.parametrize("form", TWO_FORMS)
def test_pairs_of_movers_with_a_on_an_apple(form):
  """commons_harvest__open with A standing on a live apple: a move of A's into standing B is
  blocked and enters A's own cell again (A3b), which eats the apple."""
  scope, ref = _hold(S.pair_scope, ("commons_harvest__open", "apple"), form)
  blocked = scope.tags["conflict"] == 5
  assert (ref["rewards"][0][blocked, 0] == 1.0).all() and blocked.sum() == 64


@pytest.mark.parametrize("form", TWO_FORMS)
def test_coop_minings_scripted_scenes(form):
  """The scenes tests/test_oracle_coop_cpu.py holds to hand-computed values: two miners on one
  gold ore inside the window and just outside it, one miner alone, two on one iron ore."""
  scope, ref = _hold(S.coop_scope, (), form)
  assert scope.count == 24
  paid = ref["rewards"].sum(0)                           # [n, P] over the steps
  assert (paid[scope.tags["scene"] == 0] == [8.0, 8.0, 0.0]).all()
  assert not paid[scope.tags["scene"] == 1].any()
  assert (paid[scope.tags["scene"] == 2] == [1.0, 1.0, 0.0]).all()


@pytest.mark.parametrize("form", TWO_FORMS)
def test_two_cooks_at_one_counter(form):
  """tests/test_oracle_cook_cpu.py's scene: both interact with one stocked counter in one frame and
  the first in the frame's visiting order is served — either of them, over the worlds."""
  scope, ref = _hold(S.cook_scope, (), form)
  assert scope.count == 16
  assert len(S.cook_served(scope, ref)) == 2


@pytest.mark.parametrize("level,form", [(l, f) for l in LEVELS for f in TWO_FORMS])
def test_beams_stopped_by_cells_of_the_map(level, form):
  """The shooter on every free cell of a band of the STOCK map: clean_up's dirty river and its
  wall (the clean beam is stopped by dirt and cleans it), a room of territory__rooms with its
  resource and resource walls (the claim beam claims), commons_harvest__open's top wall."""
  scope, ref = _hold(S.blocked_beam_scope, (level,), form)
  assert scope.count == {"clean_up": 3408, "commons_harvest__open": 472, "territory__rooms": 320}[level]
  types = {e[0] for events in ref["events"][0] for e in events}
  assert types >= {"clean_up": {1, 3}, "commons_harvest__open": {1}, "territory__rooms": {1, 4}}[level]


@pytest.mark.parametrize("form", TWO_FORMS)
def test_gift_refinements_scripted_chain(form):
  scope, ref = _hold(S.gift_scope, (), form)
  assert scope.count == 8 and (ref["rewards"].sum(0) == [4.0, 5.0]).all()


@pytest.mark.parametrize("form", TWO_FORMS)
def test_the_matrix_scripted_interaction(form):
  """Two placed avatars collect, are placed face to face and interact (either of them): freeze,
  payout, removal, respawn; and the refused interaction of two who have collected nothing."""
  scope, ref = _hold(S.matrix_scope, (), form)
  assert scope.count == 24
  paid = ref["rewards"].sum(0)
  assert (paid[scope.tags["scene"] < 2] > 0).all() and not paid[scope.tags["scene"] == 2].any()


@pytest.mark.parametrize("form", TWO_FORMS)
def test_the_scripted_soup(form):
  """collaborative_cooking.c:266-279 on the GPU: the delivered soup pays both players 20."""
  scope, ref = _hold(S.soup_scope, (), form)
  assert scope.count == 8 and (ref["rewards"].sum(0) == [20.0, 20.0]).all()
