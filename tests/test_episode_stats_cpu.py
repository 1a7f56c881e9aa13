"""Episode statistics (MpEpisodeStats) without a GPU (the request's layout and wrappers:
tests/test_request_abi_cpu.py): the new kernel is in the code object; requests without an
engine are refused by the library's own checks; column names parse; and the rule's host form —
the library's own functions compiled for the host — equals the numpy model
(tests/episode_stats_model.py) on oracle trajectories with several episodes per world, under a
random mask, and on crafted event rows at the count boundaries."""
import ctypes
import functools
import os

import numpy as np
import pytest

from meltingpot_amd import _build, engine
from oracle import oracle as oracle_lib
from tests import episode_stats_model as model
from tests import util

E = engine
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "meltingpot_amd", "assets")
PACKS = sorted(f[:-4] for f in os.listdir(ASSETS) if f.endswith(".mpk"))
def test_the_new_kernel_is_in_the_code_object():
  blob = open(_build.build_engine(), "rb").read()
  assert b"k_episode_stats" in blob
  assert "episode_stats.hip" in _build.SOURCES and "episode_stats.h" in _build.HEADERS


def test_the_library_refuses_requests_without_an_engine():
  L = E.load_library()

  def refused(**kw):
    req = E.MpEpisodeStats(ctypes.sizeof(E.MpEpisodeStats), E.MP_STATS_REGISTER)
    for key, value in kw.items():
      setattr(req, key, value)
    assert L.mp_restore(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID, kw
    message = L.mp_last_error()
    assert b"MpEpisodeStats" in message, (kw, message)
    return message

  assert b"NULL engine" in refused()
  assert b"NULL engine" in refused(op=E.MP_STATS_CLEAR)
  assert b"NULL engine" in refused(op=E.MP_STATS_TALLY)
  assert b"struct_size" in refused(struct_size=176)
  host = np.zeros(ctypes.sizeof(E.MpEpisodeStats), np.uint8)   # a buffer of that size is this request
  assert L.mp_restore(None, host.ctypes.data, host.size) == E.MP_ERR_INVALID
  assert b"MpEpisodeStats: struct_size" in L.mp_last_error()
  assert b"unknown op" in refused(op=0) and b"unknown op" in refused(op=5)
  assert b"reserved" in refused(op=E.MP_STATS_HOST, reserved=1)
  assert b"reserved" in refused(op=E.MP_STATS_HOST, reserved2=(ctypes.c_uint64 * 2)(0, 1))
  # the host form: counts over the limits, bad columns, missing rows and tensors
  H = E.MP_STATS_HOST
  assert b"num_columns" in refused(op=H, num_columns=33) and b"num_columns" in refused(op=H, num_columns=-1)
  assert b"num_pairs" in refused(op=H, num_pairs=5)
  assert b"NULL columns" in refused(op=H, num_columns=1)
  col = E.MpEventColumn()
  col.type = 1
  bad = dict(player_payload=2, filter_payload=3, player_shift=32, filter_shift=40, other_shift=32, reserved2=1)
  for key, value in bad.items():
    c = E.MpEventColumn.from_buffer_copy(col)
    setattr(c, key, value)
    message = refused(op=H, num_columns=1, columns=ctypes.addressof(c))
    assert b"columns[0]" in message, (key, message)
  assert b"steps" in refused(op=H, steps=0, count=1, num_players=2)
  assert b"steps" in refused(op=H, steps=1, count=0, num_players=2)
  assert b"num_players" in refused(op=H, steps=1, count=1, num_players=0)
  assert b"num_players" in refused(op=H, steps=1, count=1, num_players=17)
  assert b"NULL events" in refused(op=H, steps=1, count=1, num_players=2, num_columns=1, columns=ctypes.addressof(col))
  assert b"NULL open" in refused(op=H, steps=1, count=1, num_players=2)


def test_column_names():
  col, pair = E.parse_event_column("zap.source")
  assert (col.type, col.player_payload, col.player_shift, col.player_mask, col.filter_payload, pair) == \
      (1, 0, 0, 0xFFFFFFFF, 0, False)
  col, pair = E.parse_event_column("zap.target")
  assert (col.type, col.player_payload, pair) == (1, 1, False)
  col, pair = E.parse_event_column("mining.player[ore_type=2]")
  assert (col.type, col.player_payload, col.filter_payload, col.filter_shift, col.filter_mask, col.filter_value) == \
      (13, 0, 2, 0, 0xFFFFFFFF, 2)
  col, pair = E.parse_event_column("zap.source>target")
  assert pair and (col.player_payload, col.other_shift, col.other_mask) == (0, 0, 0xFFFFFFFF)
  col, pair = E.parse_event_column("extraction_pair.player_b>player_a[ore_type=2]")   # type 15's packed payload
  assert pair and (col.type, col.player_payload, col.player_shift, col.player_mask) == (15, 1, 2, 0x3FFFFFFF)
  assert (col.filter_payload, col.filter_shift, col.filter_mask, col.filter_value) == (2, 0, 3, 2)
  col, pair = E.parse_event_column("gift.receipient_index[source_type=1]")           # type 16's
  assert (col.type, col.player_payload, col.player_shift, col.player_mask) == (16, 1, 0, 15)
  assert (col.filter_payload, col.filter_shift, col.filter_value) == (1, 4, 1)
  col, pair = E.parse_event_column("coin_consumed.player_index[coin_type=1]")
  assert (col.filter_payload, col.filter_shift, col.filter_mask) == (2, 0, 1)
  for bad in ("zap", "zap.", "zap.nobody", "nothing.source", "zap.source[", "zap.source[x=1]", "zap.source>source",
              "mining.ore_type", "mining.player>ore_type", "coin_consumed.player_index[coin_type=2]",
              "AvatarStarted.x", 3, None, "zap.source[target=-1]"):
    with pytest.raises(ValueError):
      E.parse_event_column(bad)
  with pytest.raises(ValueError, match="pair"):
    E._column_array(("zap.source>target",), 32, False, "t")
  with pytest.raises(ValueError, match="pair"):
    E._column_array(("zap.source",), 4, True, "t")
  with pytest.raises(ValueError, match="at most 32"):
    E._column_array(("zap.source",) * 33, 32, False, "t")
  # the default set of a level: one unfiltered column per player-valued key, no pair columns
  assert E.level_event_columns(1) == ("zap.source", "zap.target", "edible_consumed.player_index",
                                      "player_cleaned.player_index")
  for sub in E.LEVEL_EVENT_TYPES:
    names = E.level_event_columns(sub)
    assert 0 < len(names) <= 32 and all(not E.parse_event_column(n)[1] for n in names)


# -- the host form against the numpy model ------------------------------------------------------

CLEAN_SLOTS = np.array([1, 1, 2, 3, 4, 5, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8], np.int32)   # zaps and cleans
K, WORLDS, MAXFRAMES = 40, 3, 12
# pack -> (columns, pair columns, event types the trajectory must really contain)
CASES = {
    "clean_up": (("zap.source", "zap.target", "edible_consumed.player_index", "player_cleaned.player_index"),
                 ("zap.source>target",), (1, 3)),
    "commons_harvest__open": (("zap.source", "zap.target", "edible_consumed.player_index"),
                              ("zap.source>target", "zap.target>source"), (1,)),
    "prisoners_dilemma_in_the_matrix__repeated": (
        ("interaction.row_player_idx", "interaction.col_player_idx", "collected_resource.player_index",
         "collected_resource.player_index[class=1]"), ("interaction.row_player_idx>col_player_idx",), (11, 12)),
    "coop_mining": (("mining.player", "mining.player[ore_type=2]", "extraction.player", "extraction_pair.player_a",
                     "extraction_pair.player_b", "extraction_pair.player_b[ore_type=2]"),
                    ("extraction_pair.player_a>player_b",), (13, 14, 15)),
    "gift_refinements": (("gift.gifter_index", "gift.receipient_index", "gift.gifter_index[source_type=1]",
                          "zap.source"), ("gift.gifter_index>receipient_index",), (16,)),
}


def _rows_of(events):
  """An oracle's [(type, a, b)] as one world-step's raw rows int32 [EVENT_ROWS, 4]."""
  rows = np.zeros((E.EVENT_ROWS, 4), np.int32)
  rows[0, 0] = len(events)
  for i, (t, a, b) in enumerate(events):
    rows[1 + i, :3] = (t, a, b)
  return rows


# pack -> (generator of tests/situations.py, its worlds to take): the scripted scenes of the
# oracle's own CPU tests, played at the start of the first episode — random play does not reach an
# extraction pair, a gift or an interaction inside episodes of 12 frames
SCENES = {
    "coop_mining": ("coop_scope", (0, 1, 2 * 8)),                       # gold twice, iron
    "gift_refinements": ("gift_scope", (0, 1, 2)),
    "prisoners_dilemma_in_the_matrix__repeated": ("matrix_scope", (0, 8, 16)),   # either interacts, nobody collected
}
SCRIPTED_STEPS = 8


@functools.lru_cache(maxsize=None)
def trajectory(name, steps=K, worlds=WORLDS, seed=7):
  """`steps` steps of `worlds` oracle worlds with auto-reset, as an engine reports them: step_type
  [K, n], reward [K, n, P], events [K, n, EVENT_ROWS, 4]; row 0 is the reset.  Actions are the
  beam-heavy hashed ones, behind the level's scripted scene where SCENES names one."""
  from tests import situations
  scope, picks, pack, players = None, None, E.load_pack(name), 0
  if name in SCENES:
    builder, picks = SCENES[name]
    scope = getattr(situations, builder)()
    pack, players = scope.pack, scope.players
  pack = util.patch_pack(pack, MAXFRAMES=MAXFRAMES)
  oracles = [oracle_lib.Oracle(pack, seed + w, players) for w in range(worlds)]
  P = oracles[0].P
  nact = len(oracles[0].tables["action_table"]) // 4
  slots = CLEAN_SLOTS if name == "clean_up" else util.ZAP_HEAVY_SLOTS
  st = np.zeros((steps, worlds), np.int32)
  rw = np.zeros((steps, worlds, P), np.float64)
  ev = np.zeros((steps, worlds, E.EVENT_ROWS, 4), np.int32)

  def place(o, places):
    for p in range(P):
      x, y, ori, alive = (int(v) for v in places[p])
      if x >= 0:
        assert o.place_avatar(p, x, y, ori, bool(alive))

  for k in range(steps):
    a = np.minimum(util.hashed_actions(range(worlds), k, P, slots=slots), nact - 1)
    for w, o in enumerate(oracles):
      scripted = scope is not None and 1 <= k <= min(scope.steps, SCRIPTED_STEPS)
      if k == 0 or o.done:
        o.reset()
        st[k, w] = 0
        if k == 0 and scope is not None:
          i = picks[w]
          for places in scope.rounds:
            place(o, places[i])
          for layer, x, y, state in scope.cells[i]:
            if layer >= 0:
              assert o.set_cell_state(int(layer), int(x), int(y), int(state))
      else:
        st[k, w] = 1 if o.step(scope.actions[k - 1, picks[w]] if scripted else a[w]) else 2
        rw[k, w] = o.rewards()
      ev[k, w] = _rows_of(list(o.events()))
      if scripted and k in scope.later:
        for places in scope.later[k]:
          place(o, places[picks[w]])
  for o in oracles:
    o.close()
  return st, rw, ev


def _host_against_model(st, rw, ev, columns, pairs, active=None, ran=None, chunks=(None,)):
  Kk, n, P = rw.shape
  stats = E.numpy_episode_stats(n, P, len(columns), len(pairs))
  want = model.Model(n, P, columns, pairs)
  lo = 0
  for hi in [Kk if c is None else c for c in chunks]:
    sl = slice(lo, hi)
    E.episode_stats_host(stats, st[sl], rw[sl], ev[sl] if ev is not None else None, columns, pairs,
                         active=None if active is None else active[sl], ran=ran if lo == 0 and hi == Kk else None)
    left = None if ran is None else np.array(ran)
    for k in range(lo, hi):
      mask = np.ones(n, bool) if active is None else active[k] != 0
      if left is not None:
        mask &= left > 0
        left -= mask
      want.step(st[k], rw[k], None if ev is None else ev[k], mask)
    model.assert_equal(stats, want.arrays(), (lo, hi))
    lo = hi
  return stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_form_equals_the_model_on_oracle_trajectories(name):
  columns, pairs, must = CASES[name]
  st, rw, ev = trajectory(name)
  n, P = rw.shape[1:]
  # the case really holds what it is there for: the event types, an episode end, several episodes
  types = set(int(t) for t in ev[:, :, 1:, 0].reshape(-1)) - {0}
  assert set(must) <= types, (name, types)
  assert (st == 2).sum(axis=0).min() >= 3, "at least three episodes a world"
  stats = _host_against_model(st, rw, ev, columns, pairs)
  assert stats["episodes"].min() >= 3 and stats["total"]["counts"].sum() > 0 and stats["total"]["pairs"].sum() > 0
  if name == "commons_harvest__open":
    assert P == 16 and stats["total"]["pairs"].shape[1:] == (2, 16, 16)
  if name == "clean_up":
    assert P == 7
  # under a random mask, in two chunks (the statistics carry over calls), and with ran
  rng = np.random.default_rng(11)
  active = (rng.random((K, n)) < 0.7).astype(np.uint8)
  _host_against_model(st, rw, ev, columns, pairs, active=active, chunks=(17, None))
  _host_against_model(st, rw, ev, columns, pairs, active=active, ran=np.array([0, 9, 1000], np.int32))
  # returns and lengths only
  none = _host_against_model(st, rw, None, (), ())
  assert none["total"]["returns"].tobytes() == stats["total"]["returns"].tobytes()


def crafted_rows(P=5, seed=3):
  """[6, EVENT_ROWS, 4]: header counts 0, 1, 63, 64, 65 and 127, dropped = 3; zaps among P players
  (some with players outside [1, P]: nobody's), rows beyond the count hold junk that must not count."""
  rng = np.random.default_rng(seed)
  counts = (0, 1, 63, 64, 65, 127)
  rows = np.zeros((len(counts), E.EVENT_ROWS, 4), np.int32)
  rows[:, 1:, 0] = 1                                         # junk beyond the count is a zap too
  rows[:, 1:, 1] = rng.integers(0, P + 2, (len(counts), E.EVENT_ROWS - 1))
  rows[:, 1:, 2] = rng.integers(0, P + 2, (len(counts), E.EVENT_ROWS - 1))
  rows[:, 1::3, 0] = 2                                       # every third row another type
  rows[:, 0, 0] = counts
  rows[:, 0, 1] = 3
  return rows


def test_host_form_on_crafted_count_boundaries():
  P = 5
  rows = crafted_rows(P)
  n = rows.shape[0]
  columns, pairs = ("zap.source", "zap.target", "edible_consumed.player_index"), ("zap.source>target",)
  ev = np.stack([rows, rows])                                # a FIRST step and a MID step
  st = np.stack([np.zeros(n, np.int32), np.ones(n, np.int32)])
  rw = np.ones((2, n, P))
  stats = _host_against_model(st, rw, ev, columns, pairs)
  assert (stats["dropped"] == 6).all() and (stats["running"]["length"] == 1).all()
  for i, count in enumerate((0, 1, 63, 64, 65, 127)):
    zaps = rows[i, 1:1 + count]
    zaps = zaps[(zaps[:, 0] == 1) & (zaps[:, 1] >= 1) & (zaps[:, 1] <= P)]
    assert stats["running"]["counts"][i, 0].sum() == 2 * len(zaps)


@pytest.mark.parametrize("name", PACKS)
def test_a_level_emits_no_event_type_outside_its_default_columns(name):
  pack = E.load_pack(name)
  oracles = [oracle_lib.Oracle(pack, 5 + w) for w in range(2)]
  from meltingpot_amd import lower
  sub = int(oracles[0].tables["hdr"][lower.HDR_SUBSTRATE])
  allowed = {E.parse_event_column(n)[0].type for n in E.level_event_columns(sub)} | {9}   # 9: AvatarStarted, nobody's
  assert allowed == set(E.LEVEL_EVENT_TYPES[sub])
  P = oracles[0].P
  nact = len(oracles[0].tables["action_table"]) // 4
  seen = set()
  for o in oracles:
    o.reset()
    seen |= {t for t, _, _ in o.events()}
  for k in range(200):
    a = util.hashed_actions(range(2), k, P, num_actions=nact)
    for w, o in enumerate(oracles):
      if o.done:
        o.reset()
      else:
        o.step(a[w])
      seen |= {t for t, _, _ in o.events()}
  for o in oracles:
    o.close()
  assert seen <= allowed, (name, seen - allowed)
