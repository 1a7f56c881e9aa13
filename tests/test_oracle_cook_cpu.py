"""collaborative_cooking (lua/levels/collaborative_cooking/components.lua,
configs/substrates/collaborative_cooking.py + seven layout modules): the committed packs against
the reference configs, and the oracle's restatement of the rules — a scripted soup from the
first tomato to the shared reward, and conservation of items over rollouts on stocked kitchens."""

import numpy as np
import pytest

import util
import refdata
from meltingpot_amd import engine, lower, pack
from oracle import oracle

LAYOUTS = ("asymmetric", "circuit", "cramped", "crowded", "figure_eight", "forced", "ring")
ACCEPTED, DROPPED, COLLECTED = 17, 18, 19
EMPTY, TOMATO, DISH, SOUP = range(4)
INTERACT_HEAVY = [1, 3, 1, 1, 1, 3, 3, 6]     # weights over the ACTION_SET: a third of the actions interact


def stocked(pack_bytes, cooking_time=3):
  """The pack with something on every counter (tomato, dish, soup in turn) and a short cooking
  time: random play then meets every rule — filling and emptying pots, soups delivered — within
  a few hundred frames."""
  t = pack.loads(pack_bytes)
  ci = t["cc_container_i32"].reshape(-1, 2).copy()
  k = 0
  for row in ci:
    if not row[1]:
      row[0] = (TOMATO, DISH, SOUP)[k % 3]; k += 1
  i32 = t["cc_i32"].copy(); i32[1] = cooking_time
  return util.patch_pack(pack_bytes, tables={"cc_container_i32": ci, "cc_i32": i32}, MAXFRAMES=5000)


def _names(t):
  return [n.decode() for n in bytes(t["state_names"]).split(b"\0")]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_committed_pack_is_what_the_reference_config_lowers_to(layout):
  name = f"collaborative_cooking__{layout}"
  mod = refdata.load_config_module(name)
  roles = tuple(mod.get_config().default_player_roles)
  settings, _, config = refdata.build_settings(name, roles)
  base = refdata.load_config_module("collaborative_cooking")
  committed = engine.load_pack(name)
  assert pack.dumps(lower.lower(name, settings, base.ACTION_SET)) == committed, "run tools/make_packs.py"
  t = pack.loads(committed)
  hdr = t["hdr"]
  rows = [r for r in mod.ASCII_MAP.split("\n") if r]
  assert (hdr[lower.HDR_H], hdr[lower.HDR_W]) == (len(rows), max(map(len, rows)))
  assert hdr[lower.HDR_MAXFRAMES] == 1000 and hdr[lower.HDR_P] == len(roles)       # :937
  assert len(t["cc_container_cells"]) == sum(mod.ASCII_MAP.count(c) for c in "#OD")
  assert len(t["cc_pot_cells"]) == mod.ASCII_MAP.count("C") and len(t["cc_receiver_cells"]) == mod.ASCII_MAP.count("T")
  names = _names(t)
  wait, plain0, off0, dir0 = (int(x) for x in t["cc_inv_states"])
  assert [names[plain0 + k] for k in range(4)] == [f"inventory.{i}" for i in ("empty", "tomato", "dish", "soup")]
  assert [names[off0 + k] for k in range(4)] == [f"inventory.{i}_offset" for i in ("empty", "tomato", "dish", "soup")]
  assert names[dir0] == "inventory.empty_offset.E" and names[dir0 + 11] == "inventory.soup_offset.W"
  assert [names[s] for s in t["cc_pot_states"]] == [
      "cooking_pot.cooking_pot_empty_empty_empty", "cooking_pot.cooking_pot_tomato_empty_empty",
      "cooking_pot.cooking_pot_tomato_tomato_empty", "cooking_pot.cooking_pot_tomato_tomato_tomato",
      "cooking_pot.cooking_pot_cooked"]
  assert list(t["cc_i32"]) == [1, base.COOKING_TIME, base.COOKING_TIME // 10]       # cooldown, :39, bar interval
  assert list(t["cc_receiver_i32"].reshape(-1, 2)[0]) == [SOUP, 1] and t["cc_receiver_f64"][0] == 20.0   # :688-692
  assert list(t["cc_f64"]) == [0.0]
  # dispensers keep what they hold; counters start empty
  ci = t["cc_container_i32"].reshape(-1, 2)
  chars = [rows[c // hdr[lower.HDR_W]][c % hdr[lower.HDR_W]] for c in t["cc_container_cells"]]
  assert [tuple(r) for r in ci] == [{"#": (EMPTY, 0), "O": (TOMATO, 1), "D": (DISH, 1)}[ch] for ch in chars]


def _held(o, t, p):
  grid, avat, _ = o.dump()
  s = int(grid[int(t["state_layer"][t["cc_inv_states"][1]]), avat[p, 1], avat[p, 0]])
  plain0, off0, dir0 = (int(x) for x in t["cc_inv_states"][1:])
  if plain0 <= s < plain0 + 4: return s - plain0
  if off0 <= s < off0 + 4: return s - off0
  if dir0 <= s < dir0 + 12: return (s - dir0) & 3
  return -1


def soup_ops():
  """The script of test_a_scripted_soup, stated once (the test below plays exactly these, and
  tests/situations.py runs them on the GPU): ("place", p, x, y, orient) and ("step", interact of
  player 0, interact of player 1)."""
  ops = [("place", 1, 5, 2, 0)]
  for rep in range(3):
    ops += [("place", 0, 3, 1, 3), ("step", 1, 0), ("place", 0, 4, 1, 0), ("step", 0, 0), ("step", 1, 0),
            ("step", 0, 0)]
  ops += [("step", 0, 0)] * 23
  ops += [("place", 0, 3, 2, 2), ("step", 0, 0), ("step", 1, 0), ("place", 0, 4, 1, 0), ("step", 0, 0),
          ("step", 1, 0), ("place", 1, 3, 1, 0), ("place", 0, 5, 2, 2), ("step", 0, 0), ("step", 1, 0),
          ("step", 0, 0)]
  return ops


def test_a_scripted_soup():
  """cramped: three tomatoes from the dispenser into the pot, one at a time; the pot cooks for 20
  ticks while its bar fills; a dish from the dish dispenser takes the soup; the delivery location
  pays BOTH players 20 — with the events of every transfer and the states a viewer sees."""
  pk = engine.load_pack("collaborative_cooking__cramped")
  t = pack.loads(pk)
  names = _names(t)
  o = oracle.Oracle(pk, util.world_seed(0), 2); o.reset()
  F = lambda move=0, turn=0, interact=0: [move, turn, interact]
  ops = iter(soup_ops())

  def step(a0, a1=F()):
    assert next(ops) == ("step", a0[2], a1[2]) and not (a0[0] or a0[1] or a1[0] or a1[1])
    return o.step_fields(np.array([a0, a1], np.int32))

  def place(*where):
    assert next(ops) == ("place",) + where
    return o.place_avatar(*where)
  pot_state = lambda: names[int(o.dump()[0][4, 0, 4])]
  bar_state = lambda: names[int(o.dump()[0][5, 0, 4])]
  assert place(1, 5, 2, 0)
  for rep in range(3):
    assert place(0, 3, 1, 3)            # facing W: the tomato dispenser at (2, 1)
    step(F(interact=1))
    assert _held(o, t, 0) == TOMATO and o.events() == []
    assert place(0, 4, 1, 0)            # facing N: the pot at (4, 0)
    step(F())                                    # (the beam's cooldown of one frame)
    step(F(interact=1))
    assert _held(o, t, 0) == EMPTY and o.events() == [(DROPPED, 1, TOMATO)]
    assert pot_state().endswith(("tomato_empty_empty", "tomato_tomato_empty", "tomato_tomato_tomato")[rep])
    step(F())
  bars = []
  for i in range(23):
    step(F())
    bars.append(bar_state())
  assert pot_state().endswith("cooked") and bars[-1].endswith("loading_bar_10")
  assert bars[0].endswith("loading_bar_0") and bars[5].endswith("loading_bar_3")
  # the dispenser still holds its tomato; a second interaction in one frame finds a container used
  assert place(0, 3, 2, 2)              # facing S: the dish dispenser at (3, 3)
  step(F()); step(F(interact=1))
  assert _held(o, t, 0) == DISH
  assert place(0, 4, 1, 0)
  step(F()); step(F(interact=1))
  assert _held(o, t, 0) == SOUP and o.events() == [(COLLECTED, 1, SOUP)]
  assert pot_state().endswith("empty_empty_empty")
  assert place(1, 3, 1, 0) and place(0, 5, 2, 2)   # facing S: the delivery location at (5, 3)
  step(F()); step(F(interact=1))
  assert o.rewards().tolist() == [20.0, 20.0] and o.events() == [(ACCEPTED, 1, SOUP)]
  assert _held(o, t, 0) == EMPTY
  step(F())
  assert o.rewards().tolist() == [0.0, 0.0]
  assert next(ops, None) is None


# The scene of test_two_avatars_one_counter_in_one_frame, stated once (tests/situations.py runs it
# on the GPU): circuit's island counters (3, 2) .. (6, 2) are reachable from above and below;
# player 0 above counter (4, 2) facing S, player 1 below it facing N: (x, y, orient)
COUNTER_LAYOUT = "collaborative_cooking__circuit"
COUNTER_PLACES = ((4, 1, 2), (4, 3, 0))


def test_two_avatars_one_counter_in_one_frame():
  """Container._usedThisStep: of two avatars that interact with the same counter in one frame
  only the first in the frame's visiting order is served."""
  pk = stocked(engine.load_pack("collaborative_cooking__cramped"))
  t = pack.loads(pk)
  served = set()
  for seed in range(12):
    o = oracle.Oracle(pk, util.world_seed(seed), 2); o.reset()
    # the counter at (4, 3) between them: player 0 above it facing S ... no: both next to (2, 2)?
    # counter (4, 3) has free cells only above; use the counter at (2, 2): reachable from (3, 2) only.
    # Two avatars can face one counter in `circuit`; here: check the served one holds, the other not,
    # on the counter (4, 3) reached from (4, 2) by one and ... skip unless both can stand.
    break
  # circuit: the island counters (3, 2) .. (6, 2) are reachable from above and below
  pk = stocked(engine.load_pack(COUNTER_LAYOUT))
  t = pack.loads(pk)
  for seed in range(16):
    o = oracle.Oracle(pk, util.world_seed(seed), 2); o.reset()
    assert all(o.place_avatar(p, *place) for p, place in enumerate(COUNTER_PLACES))
    before = [_held(o, t, p) for p in range(2)]
    assert before == [EMPTY, EMPTY]
    o.step_fields(np.array([[0, 0, 1], [0, 0, 1]], np.int32))
    after = [_held(o, t, p) for p in range(2)]
    assert sorted(after)[0] == EMPTY and sorted(after)[1] != EMPTY, after   # exactly one was served
    served.add(after.index(max(after)))
  assert served == {0, 1}      # (the visiting order is shuffled per frame and per world)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_items_are_conserved_on_a_stocked_kitchen(layout):
  """Rollouts with something on every counter: a soup only ever comes out of a cooked pot, a pot
  only ever takes tomatoes, every delivery pays every player 20 and nothing else pays; every event
  names a player that interacted this frame; the bars follow the pots."""
  pk = stocked(engine.load_pack(f"collaborative_cooking__{layout}"))
  t = pack.loads(pk)
  P = int(t["hdr"][lower.HDR_P])
  rng = np.random.default_rng(5)
  seen = {ACCEPTED: 0, DROPPED: 0, COLLECTED: 0}
  for seed in range(3):
    o = oracle.Oracle(pk, util.world_seed(seed), P); o.reset()
    timer = np.zeros(P, int)
    for step in range(1500):
      acts = rng.choice(8, size=P, p=np.array(INTERACT_HEAVY) / sum(INTERACT_HEAVY)).astype(np.int32)
      fired = set()
      for p in range(P):                          # InteractBeam (components.lua:79-100)
        if timer[p] > 0: timer[p] -= 1
        elif acts[p] == 7: timer[p] = 1; fired.add(p)
      before = [_held(o, t, p) for p in range(P)]
      o.step(acts)
      after = [_held(o, t, p) for p in range(P)]
      ev = o.events()
      deliveries = 0
      for ty, a, b in ev:
        seen[ty] += 1
        assert a - 1 in fired
        if ty == ACCEPTED:
          assert b == SOUP and before[a - 1] == SOUP and after[a - 1] == EMPTY; deliveries += 1
        if ty == DROPPED:
          assert b == TOMATO and before[a - 1] == TOMATO and after[a - 1] == EMPTY
        if ty == COLLECTED:
          assert b == SOUP and before[a - 1] == DISH and after[a - 1] == SOUP
      assert o.rewards().tolist() == [20.0 * deliveries] * P
      for p in range(P):
        if p not in fired:
          assert after[p] == before[p]            # an inventory only changes by its avatar's own beam
      assert np.array_equal(o.dump()[1][:, 4], timer)
  # (random play is a poor cook: `forced` separates its two players from what they need)
  assert sum(seen.values()) >= (0 if layout == "forced" else 3), seen
  TOTAL.update({k: TOTAL.get(k, 0) + v for k, v in seen.items()})


TOTAL = {}


def test_every_kind_of_event_was_met():
  """(after the rollouts above) over the seven kitchens: ingredients dropped, soups collected,
  soups delivered."""
  if len(TOTAL) == 0:
    pytest.skip("runs behind test_items_are_conserved_on_a_stocked_kitchen")
  assert TOTAL[DROPPED] >= 20 and TOTAL[COLLECTED] >= 2 and TOTAL[ACCEPTED] >= 5, TOTAL
