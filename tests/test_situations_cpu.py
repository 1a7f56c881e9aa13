"""The enumerated situations of tests/situations.py on the CPU, oracle against oracle: the
generators' counts, every placement accepted, every ordered outcome present — and proof that the
scopes discriminate: with ONE engine assumption switched (`Oracle.set_option`) the switched side
differs from the stock side in at least one situation of the scope that is there to hold it."""
import numpy as np
import pytest

import situations as S

LEVELS = ("clean_up", "commons_harvest__open", "territory__rooms")


def _differs(ref, other):
  """Worlds in which two oracle runs of one scope differ after some step (state or rewards)."""
  bad = np.zeros(len(ref["accepted"]), bool)
  for name in ("grid", "avat", "glob", "rewards"):
    a, b = ref[name], other[name]
    bad |= (a != b).reshape(a.shape[0], a.shape[1], -1).any(2).any(0)
  return np.flatnonzero(bad)


def _stock(builder, *args):
  scope, ref = S.reference(builder, *args)
  assert scope.n == scope.count
  assert ref["accepted"].all(), scope.name                        # place_avatar refused nothing
  assert not _differs(ref, ref).size
  return scope, ref


@pytest.mark.parametrize("level", LEVELS)
def test_pairs_of_movers(level):
  scope, ref = _stock(S.pair_scope, level)
  assert scope.count == 4 * 12 * 4 * 25 == 4800
  # 192 same-cell conflicts, 64 swaps, 192 + 192 moves into a vacated cell, 64 + 64 into a standing avatar
  assert np.bincount(scope.tags["conflict"]).tolist() == [4032, 192, 64, 192, 192, 64, 64]
  won = S.pair_outcomes(scope, ref)
  assert len(won["A"]) > 0 and len(won["B"]) > 0 and len(won["A"]) + len(won["B"]) == 192
  assert len(won["neither"]) == 64 and not len(won["both"])
  # the patch holds nothing but floor: nobody is paid, and a lone mover always arrives
  assert not ref["rewards"].any()
  # A1: without the shuffle the avatars are visited in index order and A wins every conflict
  fixed = S.run_oracle(scope, options=(("A1_shuffle_order", 0),), stride=0)
  bad = _differs(ref, fixed)
  assert (scope.tags["conflict"][bad] == 1).any()
  assert len(S.pair_outcomes(scope, fixed)["B"]) == 0 and len(S.pair_outcomes(scope, fixed)["A"]) == 192


@pytest.mark.parametrize("level", LEVELS)
def test_three_movers_around_one_cell(level):
  halves = [_stock(S.triple_half, level, h) for h in (0, 1)]
  assert sum(scope.count for scope, _ in halves) == 4 * 64 * 27 == 6912
  differs = 0
  for scope, ref in halves:
    centre = np.array(S.PATCHES[level][1])
    on_centre = (ref["avat"][1][:, :, :2] == centre).all(2)
    crowd = scope.tags["entering"] >= 2
    assert (on_centre[crowd].sum(1) == 1).all() and on_centre[crowd].any(0).all()
    assert (on_centre[scope.tags["entering"] == 0].sum(1) == 0).all()
    fixed = S.run_oracle(scope, options=(("A1_shuffle_order", 0),), stride=0)
    bad = _differs(ref, fixed)
    differs += int(crowd[bad].sum())
  assert differs


def test_pairs_across_the_seam():
  scope, ref = _stock(S.pair_scope, "clean_up", "seam")
  assert scope.count == 4800
  H, W = ref["grid"].shape[-2:]
  assert {tuple(p) for p in scope.places[:, 1, :2]} >= {(W - 2, 0), (W - 1, H - 1), (0, H - 2), (1, 1)}
  won = S.pair_outcomes(scope, ref)
  assert len(won["A"]) and len(won["B"]) and len(won["neither"]) == 64
  fixed = S.run_oracle(scope, options=(("A1_shuffle_order", 0),), stride=0)
  assert _differs(ref, fixed).size


@pytest.mark.parametrize("level", LEVELS)
def test_beams(level):
  scope, ref = _stock(S.beam_scope, level)
  assert scope.count == {"clean_up": 1702, "commons_harvest__open": 852, "territory__rooms": 624}[level]
  assert np.bincount(scope.tags["kind"]).all()           # every kind of case is there
  dead = [(ref["avat"][s][:, :, 3] == 0).any() for s in range(scope.steps + 1)]
  assert not dead[0] and any(dead)
  # A4: a blocked cell without its beam sprite shows wherever somebody stands in a beam
  off = S.run_oracle(scope, options=(("A4_beam_marks_blocked", 0),), stride=0)
  bad = _differs(ref, off)
  assert (scope.tags["kind"][bad] == 1).any()            # the shielded cases tell the two apart
  # the zap's footprint is where an avatar is hit: a target on each cell of the 7 x 7 patch
  (cx, cy), ids = S.PATCHES[level][1], S.action_ids(level)
  park = S.BEAMS[level][2]
  taken = S._avatar_layer_cells(scope.pack)   # (territory's patch has wall corners in its ring)
  cells = [(x, y) for y in range(cy - 3, cy + 4) for x in range(cx - 3, cx + 4)
           if (x, y) != (cx, cy) and not taken[y, x]]
  assert len(cells) >= 46
  places = [[[cx, cy, o, 1], [x, y, 0, 1], [park[0], park[1], 0, 1]] for o in range(4) for x, y in cells]
  acts = np.array([[ids["fireZap"], ids["NOOP"], ids["NOOP"]]] * len(places))[None]
  probe = S.Scope("zap probe", level, scope.pack, 3, places, acts, lambda w: str(places[w]), len(places))
  hit = S.run_oracle(probe, stride=0)
  assert hit["accepted"].all()
  for o in range(4):
    want = set(S.beam_footprint(level, "fireZap", o))
    got = {c for i, c in enumerate(cells)
           if any(e == (1, 1, 2) for e in hit["events"][0][o * len(cells) + i])}   # 'zap', source 1, target 2
    assert got == want, (level, o)


def test_respawn_onto_taken_spawn_points():
  scope, ref = _stock(S.respawn_scope)
  assert scope.count == (4 + 6) * 4 * S.RESPAWN_SEEDS == 1600
  alive = np.stack([ref["avat"][s][:, :, 3].sum(1) for s in range(scope.steps + 1)])
  assert (alive[:5] == 3).all() and (alive[5] == 4).any() and not (alive[5] == 4).all()
  # nobody ever shares a cell
  for s in range(scope.steps + 1):
    a = ref["avat"][s]
    for w in np.flatnonzero(a[:, :, 3].sum(1) == 4):
      assert len({(x, y) for x, y in a[w, :, :2]}) == 4
  # A5: picking among the FREE points only, every dead avatar lands at the first attempt
  free_only = S.run_oracle(scope, options=(("A5_teleport_free_only", 1),), stride=0)
  assert (free_only["avat"][5][:, :, 3].sum(1) == 4).all() and _differs(ref, free_only).size


def test_a_blocked_move_reenters_the_cell_a_stands_on():
  """A3b, where onEnter does something: A stands on a live apple of commons_harvest__open."""
  scope, ref = _stock(S.pair_scope, "commons_harvest__open", "apple")
  blocked = scope.tags["conflict"] == 5
  assert blocked.sum() == 64 and (ref["rewards"][0][blocked, 0] == 1.0).all()
  off = S.run_oracle(scope, options=(("A3b_blocked_move_reenters", 0),), stride=0)
  bad = _differs(ref, off)
  assert bad.size and not off["rewards"][0][blocked, 0].any()
  # on bare floor the switch is invisible: the apple is what makes the scope see it
  floor, fref = _stock(S.pair_scope, "commons_harvest__open")
  assert not _differs(fref, S.run_oracle(floor, options=(("A3b_blocked_move_reenters", 0),), stride=0)).size


def test_coop_minings_scripted_scenes():
  scope, ref = _stock(S.coop_scope)
  assert scope.count == 3 * S.COOP_SEEDS == 24
  paid = ref["rewards"].sum(0)
  assert (paid[scope.tags["scene"] == 0] == [8.0, 8.0, 0.0]).all()     # inside the window
  assert not paid[scope.tags["scene"] == 1].any()                      # B one frame too late
  assert (paid[scope.tags["scene"] == 2] == [1.0, 1.0, 0.0]).all()     # iron: each hit pays
  # late: B's hit found the ore raw again and opened a window of its own
  t = S.util.pack_tables(scope.pack)
  s_part = int(t["cm_states"][4])
  late = np.flatnonzero(scope.tags["scene"] == 1)
  assert (ref["grid"][5][late] == s_part).any((1, 2, 3)).all()


def test_two_cooks_at_one_counter():
  scope, ref = _stock(S.cook_scope)
  assert scope.count == S.COOK_SEEDS == 16
  assert S.cook_served(scope, ref) == {0, 1}             # exactly one is served, either of them
  fixed = S.run_oracle(scope, options=(("A1_shuffle_order", 0),), stride=0)
  assert S.cook_served(scope, fixed) == {0}


@pytest.mark.parametrize("level", LEVELS)
def test_beams_stopped_by_cells_of_the_map(level):
  scope, ref = _stock(S.blocked_beam_scope, level)
  assert scope.count == {"clean_up": 3408, "commons_harvest__open": 472, "territory__rooms": 320}[level]
  types = {e[0] for events in ref["events"][0] for e in events}
  # zap; clean_up: player_cleaned (a dirty cell stopped the clean beam); territory: claimed_resource
  assert types >= {"clean_up": {1, 3}, "commons_harvest__open": {1}, "territory__rooms": {1, 4}}[level]
  # A4, where the blocker is a CELL: the lone shots (kind 0) differ without the blocked cell's sprite
  off = S.run_oracle(scope, options=(("A4_beam_marks_blocked", 0),), stride=0)
  bad = _differs(ref, off)
  assert (scope.tags["kind"][bad] == 0).any()


def test_the_imported_scenes_pay_what_their_cpu_tests_compute():
  scope, ref = _stock(S.gift_scope)
  assert scope.count == S.SCENE_SEEDS and (ref["rewards"].sum(0) == [4.0, 5.0]).all()
  scope, ref = _stock(S.soup_scope)
  assert scope.count == S.SCENE_SEEDS and (ref["rewards"].sum(0) == [20.0, 20.0]).all()
  assert all((17, 1, 3) in ref["events"][-2][w] for w in range(scope.n))   # receiver_accepted_item: soup
  scope, ref = _stock(S.matrix_scope)
  assert scope.count == 3 * S.SCENE_SEEDS
  paid, scene = ref["rewards"].sum(0), scope.tags["scene"]
  assert (paid[scene < 2] > 0).all() and not paid[scene == 2].any()
  assert (paid[scene == 0] == paid[scene == 1]).all()    # the payout does not depend on who zaps here
  for w in np.flatnonzero(scene < 2):
    assert any(e[0] == 11 for e in ref["events"][1][w])  # 'interaction'
  assert not any(e[0] == 11 for w in np.flatnonzero(scene == 2) for e in ref["events"][0][w])
  assert (ref["avat"][-1][:, :, 3] == 1).all()           # everybody is back at the end
