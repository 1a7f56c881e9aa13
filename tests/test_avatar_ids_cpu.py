"""AVATAR_IDS_IN_VIEW and AVATAR_IDS_IN_RANGE_TO_ZAP (the MpAvatarIds request) without a GPU (its
struct, wrappers and kernels: tests/test_request_abi_cpu.py): the
library's host twin held to the numpy model (tests/avatar_ids_model.py) on real rows (the fixture
of tests/states_recipe.py's recipe, and CPU-oracle worlds under random play with beams) and on the
hand-placed rows of tests/avatar_ids_rows.py, whose expected bits are also stated here one by one.
IN_VIEW is tied to EGO_LAYER: q is in p's view exactly when q's avatar sprite shows on the avatar
layer of p's `ego_layer_host`.  Every comparison is exact equality."""
import ctypes
import functools
import re

import numpy as np
import pytest

import avatar_ids_model as M
import avatar_ids_rows as HR
import states_recipe as R
import view_hash_model as VM
from meltingpot_amd import substrate
from meltingpot_amd import engine as E
from meltingpot_amd import pack as pack_lib

LEVELS = HR.LEVELS
PLAYERS = {"clean_up": 7, "commons_harvest__open": 16, "territory__rooms": 9, "externality_mushrooms__dense": 5}
NO_ZAPPER = ("coins", "collaborative_cooking__cramped")


@functools.lru_cache(maxsize=None)
def real_rows(name):
  """The fixture's rows of a level, then one CPU-oracle world after 8, 16, ... 48 random steps with beams."""
  pack = R.pack(name)
  more, _, _ = VM.oracle_rows(pack, len(substrate.get_config(name).action_set), 1, 48, (8, 16, 24, 32, 40, 48))
  return np.concatenate([HR.golden_rows(name), more])


# ---- structure ---------------------------------------------------------------------------------
def test_the_model_s_footprint_and_the_levels():
  """9 cells for the stock Zapper (length 3, radius 1), 6 for territory's (length 2): P * nc > 64
  on commons_harvest__open, so a wave takes several rounds there."""
  for name in LEVELS:
    pack = R.pack(name)
    assert E.state_layout(pack).P == PLAYERS[name] and E.has_zapper(pack)
    foot = M.footprint(pack)
    assert len(foot) == (6 if name == "territory__rooms" else 9)
    assert all(all(k < j for k in pred) for j, (_, _, pred) in enumerate(foot))
  assert PLAYERS["commons_harvest__open"] * 9 > 64
  for name in NO_ZAPPER:
    assert not E.has_zapper(R.pack(name)) and M.footprint(R.pack(name)) is None


# ---- the host twin -------------------------------------------------------------------------------
def _sampled(pack, rows, want_v, want_z):
  """players= with repeats, which= with repeats, and more rows than the bank has."""
  P = want_v.shape[1]
  rng = np.random.default_rng(5)
  which = rng.integers(0, len(rows), size=3 * len(rows)).astype(np.int32)
  players = rng.integers(0, P, size=which.size).astype(np.int32)
  which[1], players[1] = which[0], players[0]
  gv, gz = E.avatar_ids_host(pack, rows, players, which=which, zap=want_z is not None)
  assert gv.shape == (which.size, P) and np.array_equal(gv, want_v[which, players])
  assert want_z is None or np.array_equal(gz, want_z[which, players])
  gv, gz = E.avatar_ids_host(pack, rows, which=which, zap=want_z is not None)
  assert gv.shape == (which.size, P, P) and np.array_equal(gv, want_v[which])
  assert want_z is None or np.array_equal(gz, want_z[which])


@pytest.mark.parametrize("name", LEVELS)
def test_the_host_twin_equals_the_model_on_real_rows(name):
  pack, rows = R.pack(name), real_rows(name)
  P = PLAYERS[name]
  want_v, want_z = M.of_rows(pack, rows)
  got_v, got_z = E.avatar_ids_host(pack, rows)
  assert got_v.dtype == got_z.dtype == np.int32 and got_v.shape == got_z.shape == (len(rows), P, P)
  assert np.array_equal(got_v, want_v) and np.array_equal(got_z, want_z)
  assert set(np.unique(got_v).tolist()) == {0, 1} and set(np.unique(got_z).tolist()) <= {0, 1}
  f = M.fields_of(pack, rows)
  alive = f.alive.numpy().astype(bool)
  # a living viewer sees itself and never zaps itself; a dead one sees and reaches nobody
  assert np.array_equal(got_v[:, np.arange(P), np.arange(P)].astype(bool), alive)
  assert not got_z[:, np.arange(P), np.arange(P)].any()
  assert not got_v[~alive].any() and not got_z[~alive].any()
  assert not got_v.transpose(0, 2, 1)[~alive].any() and not got_z.transpose(0, 2, 1)[~alive].any()
  if name in R.DEAD_AVATARS:
    assert (~alive).any()
  if name != "territory__rooms":   # (its nine avatars live in nine rooms)
    assert got_z.any()
  # one of the two alone
  only_v, none = E.avatar_ids_host(pack, rows, zap=False)
  assert none is None and np.array_equal(only_v, want_v)
  none, only_z = E.avatar_ids_host(pack, rows, view=False)
  assert none is None and np.array_equal(only_z, want_z)
  _sampled(pack, rows, want_v, want_z)


@pytest.mark.parametrize("name", LEVELS)
def test_in_view_is_where_ego_layer_shows_the_avatar(name):
  """IN_VIEW[p][q] == 1 exactly when one of q's avatar sprites shows on the avatar layer of p's
  EGO_LAYER (viewer p sees its own avatar as "Self")."""
  pack = R.pack(name)
  rows = np.concatenate([real_rows(name), HR.hand_rows(name)[0]])
  P = PLAYERS[name]
  got_v, _ = E.avatar_ids_host(pack, rows, zap=False)
  ego = E.ego_layer_host(pack, rows)[..., M.avatar_layer(pack)]   # [R, P, VH, VW]
  t = pack_lib.loads(pack)
  ssprite = np.asarray(t["state_sprite"]).reshape(-1)
  nsprites = len(bytes(t["sprite_names"]).split(b"\0")) - 1
  vmap = np.asarray(t["view_sprite_map"]).reshape(-1, nsprites)
  names = E.layer_id_names_host(pack)
  states = sorted((s, o) for s, o in M.avatar_states(pack, P).items())
  assert [o for _, o in states] == list(range(P))   # (one avatar state a player in these packs)
  for p in range(P):
    shown = [1 + int(vmap[p, ssprite[s]]) for s, _ in states]
    # every player's avatar has an id of its own in viewer p's table, named after a sprite
    assert len(set(shown)) == P and all(names[i] for i in shown), (p, [names[i] for i in shown])
    for q in range(P):
      assert np.array_equal((ego[:, p] == shown[q]).any(axis=(1, 2)).astype(np.int32), got_v[:, p, q]), (name, p, q)


@pytest.mark.parametrize("name", LEVELS)
def test_hand_placed_rows(name):
  pack = R.pack(name)
  rows, what, tags = HR.hand_rows(name)
  want_v, want_z = M.of_rows(pack, rows)
  got_v, got_z = E.avatar_ids_host(pack, rows)
  for r in range(len(rows)):
    assert np.array_equal(got_v[r], want_v[r]) and np.array_equal(got_z[r], want_z[r]), what[r]
  # the cases, bit by bit: player 0 views, players 1 and 2 are the targets
  assert len(tags["edge_in"]) == len(tags["edge_out"]) == len(tags["corner_in"]) == 16
  for r in tags["edge_in"] + tags["corner_in"]:
    assert got_v[r, 0, 1] == 1, what[r]
  for r in tags["edge_out"]:
    assert got_v[r, 0, 1] == 0 and got_v[r, 0, 0] == 1, what[r]
  assert len(tags["footprint"]) == 4 * len(M.footprint(pack))
  for r in tags["footprint"]:
    assert got_z[r, 0].tolist() == [0, 1] + [0] * (got_z.shape[1] - 2), what[r]
  for r in tags["wall"] + tags["side_wall"]:
    assert not got_z[r, 0].any() and got_v[r, 0, 1] == 1, what[r]
  for r in tags["shadow"]:
    assert got_z[r, 0, 1] == 1 and got_z[r, 0, 2] == 0 and got_z[r, 0].sum() == 1, what[r]
    assert got_z[r, 1, 2] == 1 or got_z[r, 1, 0] == 1   # (the nearer one faces one of its neighbours: o = 3 of 0..3)
  for r in tags["map_corner"]:
    assert got_z[r, 0].tolist() == [0, 1] + [0] * (got_z.shape[1] - 2), what[r]
  for r in tags["dead_viewer"]:
    assert not got_v[r, 0].any() and not got_z[r, 0].any() and not got_v[r, :, 0].any(), what[r]
  for r in tags["dead_target"]:
    assert got_v[r, 0, 1] == 0 and got_z[r, 0, 1] == 0 and got_v[r, 0, 0] == 1, what[r]
  for r in tags["all_dead"]:
    assert not got_v[r].any() and not got_z[r].any()
  _sampled(pack, rows, want_v, want_z)


# ---- refusals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NO_ZAPPER)
def test_a_level_without_a_zapper_refuses_in_range_and_draws_in_view(name):
  pack, rows = R.pack(name), HR.golden_rows(name)
  with pytest.raises(ValueError, match=rf"MpAvatarIds: {name.split('__')[0]} has no Zapper"):
    E.avatar_ids_host(pack, rows)
  with pytest.raises(ValueError, match="has no Zapper"):
    E.avatar_ids_host(pack, rows, view=False)
  want_v, _ = M.of_rows(pack, rows, zap=False)
  got_v, none = E.avatar_ids_host(pack, rows, zap=False)
  assert none is None and np.array_equal(got_v, want_v) and got_v.any()
  _sampled(pack, rows, want_v, None)


def test_an_index_out_of_range_stops_the_host_twin_there():
  pack, rows = R.pack("clean_up"), HR.golden_rows("clean_up")
  want_v, want_z = M.of_rows(pack, rows)
  P, FILL = want_v.shape[1], 0x5A5A5A5A

  def call(which, players):
    lead = (len(which),) + (() if players is None else ())
    out_v = np.full(lead + ((P, P) if players is None else (P,)), FILL, np.int32)
    out_z = out_v.copy()
    keep = E._host_config(pack)
    which = np.asarray(which, np.int32)
    ply = None if players is None else np.asarray(players, np.int32)
    with pytest.raises(ValueError) as err:
      E.avatar_ids_request(E.load_library(), None, E.MP_AVATARIDS_HOST, fingerprint=E.state_layout(pack).fingerprint,
                           pack=ctypes.addressof(keep[0]), pack_len=len(pack),
                           cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p), bank=rows.ctypes.data,
                           bank_rows=len(rows), rows=which.ctypes.data, players=None if ply is None else ply.ctypes.data,
                           count=len(which), dst=out_v.ctypes.data, dst_bytes=out_v.nbytes, dst_zap=out_z.ctypes.data,
                           dst_zap_bytes=out_z.nbytes)
    return str(err.value), out_v, out_z

  text, out_v, out_z = call([1, 0, len(rows), 2], None)
  assert re.search(rf"MpAvatarIds: rows\[2\] = {len(rows)} is not a row of the bank; the elements from 2 on", text)
  assert np.array_equal(out_v[:2], want_v[[1, 0]]) and np.array_equal(out_z[:2], want_z[[1, 0]])
  assert (out_v[2:] == FILL).all() and (out_z[2:] == FILL).all()
  text, out_v, out_z = call([3, 3, 4], [6, P, 0])
  assert re.search(rf"MpAvatarIds: players\[1\] = {P} is not a player of this pack; the elements from 1 on", text)
  assert np.array_equal(out_v[0], want_v[3, 6]) and np.array_equal(out_z[0], want_z[3, 6])
  assert (out_v[1:] == FILL).all() and (out_z[1:] == FILL).all()
  text, _, _ = call([0, -1], None)
  assert "rows[1] = -1" in text
  with pytest.raises(ValueError, match="neither view nor zap"):
    E.avatar_ids_host(pack, rows, view=False, zap=False)
  with pytest.raises(ValueError, match="fingerprint"):
    E.avatar_ids_host(pack, rows, fingerprint=1)
  with pytest.raises(ValueError, match="which has 2 entries, players 3"):
    E.avatar_ids_host(pack, rows, [0, 1, 2], which=[0, 1])


def test_the_specs_name_the_leaves():
  cfg = substrate.get_config("clean_up")
  ind, _, spec = substrate.select_observations(cfg, R.pack("clean_up"), ("RGB",) + substrate.AVATAR_IDS_NAMES, ())
  assert ind[-2:] == list(substrate.AVATAR_IDS_NAMES)
  for n in substrate.AVATAR_IDS_NAMES:
    assert spec[n].shape == (7,) and spec[n].dtype == np.int32 and spec[n].name == n
    assert n not in cfg.individual_observation_names   # (no default observation list names them)
