"""WORLD.LAYER and the world planes (the world ops of MpEgoLayer and MpEgoPlanes) without a GPU: the
library's host twins held to the numpy model (tests/world_view_model.py) on records written from
the CPU oracle, the tie between WORLD.LAYER and every viewer's EGO_LAYER, the refusals of the host
form — the new ones and the ones that stay — and the op constants as a compiler sees them.  Every
comparison is exact equality."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import ego_layer_model as EM
import view_hash_model as VM
import world_view_model as WM
from meltingpot_amd import substrate
from meltingpot_amd import engine as E

KITCHEN = "collaborative_cooking__cramped"
MATRIX = "prisoners_dilemma_in_the_matrix__repeated"
COMMONS = "commons_harvest__open"
LEVELS = ("clean_up", COMMONS, KITCHEN, MATRIX)
# (chosen with the CPU oracle: all four facings among the LIVING avatars of every level, a dead
# avatar on clean_up, and every plane of `occurring`'s table lit somewhere and dark somewhere)
STEPS, KEEP, SEED = 48, (8, 16, 24, 32, 40, 48), 1
C = 4


@functools.lru_cache(maxsize=None)
def case(name):
  """(pack, rows uint8 [6, S]) of a level: one oracle world after 8, 16, ... 48 random steps with
  beams (the rows of tests/test_view_hash_cpu.py)."""
  pack = E.load_pack(name)
  rows, _, _ = VM.oracle_rows(pack, len(substrate.get_config(name).action_set), SEED, STEPS, KEEP)
  return pack, rows


def occurring(pack, rows, classes=C):
  """A table from the MODEL's view of the rows: the ids that occur on some cell but not on every
  cell of every row, dealt to `classes` classes in turn; id 0 and every other id belong to none."""
  wl = WM.layer_of_rows(pack, rows)
  ids = [i for i in np.unique(wl) if i > 0 and not (wl == i).any(-1).all()]
  assert len(ids) >= classes
  table = np.full(E.num_world_layer_ids_host(pack), -1, np.int32)
  table[ids] = np.arange(len(ids)) % classes
  return table


# ---- 1. the host twins against the model ---------------------------------------------------------
@pytest.mark.parametrize("name", LEVELS)
def test_the_host_twins_equal_the_model(name):
  pack, rows = case(name)
  lay = E.state_layout(pack)
  H, W, L = WM.geometry(pack)
  P = lay.P
  assert P == {"clean_up": 7, COMMONS: 16}.get(name, 2)
  if name == KITCHEN:
    assert H * W < 64 and (H * W) % 2 == 1   # (a map smaller than a wave, odd blocks)
  fields, _ = WM.fields_of(pack, rows)
  alive = fields.alive.numpy()[:, :P].astype(bool)
  assert set(fields.orientation.numpy()[:, :P][alive].tolist()) == {0, 1, 2, 3}
  if name == "clean_up":
    assert (~alive).any()
  # WORLD.LAYER
  assert E.num_world_layer_ids_host(pack) == WM.num_ids(pack, P)
  want = WM.layer_of_rows(pack, rows)
  got = E.world_layer_host(pack, rows)
  assert got.dtype == np.int32 and got.shape == want.shape == (len(rows), H, W, L)
  assert np.array_equal(got, want)
  assert got.min() == 0 and got.max() < E.num_world_layer_ids_host(pack)
  which = np.array([3, 3, 0, 5, 1, 1, 2, 4, 0], np.int32)   # repeats, more elements than rows
  assert np.array_equal(E.world_layer_host(pack, rows, which=which), want[which])
  if name == MATRIX:
    # the world's sprite map is not the identity here, and no viewer's: Wt is a table of its own
    wt = WM.table(pack, P)
    viewers = EM.lut(pack, P)
    assert all(not np.array_equal(wt, viewers[p, :256]) for p in range(P))
    assert not np.array_equal(WM.sprite_maps(pack)[P], np.arange(WM.sprite_maps(pack).shape[1]))
  # the planes
  classes = occurring(pack, rows)
  assert classes.min() == -1 and classes.max() == C - 1
  for facing in (False, True):
    want = WM.planes_of_rows(pack, rows, classes, C, facing=facing)
    got = E.world_planes_host(pack, rows, classes, facing=facing)
    assert got.dtype == np.uint8 and got.shape == want.shape == (len(rows), C + 4 * facing, H, W)
    assert np.array_equal(got, want)
    assert set(np.unique(got).tolist()) == {0, 1}
    # every class plane and every facing plane is 1 somewhere and 0 somewhere
    assert got.any(axis=(0, 2, 3)).all() and (got == 0).any(axis=(0, 2, 3)).all()
    assert np.array_equal(E.world_planes_host(pack, rows, classes, which=which, facing=facing), want[which])
    for layers in ([0], [L - 1, 0], list(range(0, L, 2))):
      got = E.world_planes_host(pack, rows, classes, layers=layers, facing=facing)
      assert np.array_equal(got, WM.planes_of_rows(pack, rows, classes, C, layers=layers, facing=facing)), layers
  # the facing planes say where the living stand: one cell a living avatar, none for a dead one
  got = E.world_planes_host(pack, rows, classes, facing=True)
  assert np.array_equal(got[:, C:].sum(axis=(1, 2, 3)), alive.sum(1))
  # with the identity table, plane c is (WORLD.LAYER == c).any(-1); C = 64 uses every bit of a mask
  n = E.num_world_layer_ids_host(pack)
  if n <= 64:
    wl = E.world_layer_host(pack, rows)
    got = E.world_planes_host(pack, rows, np.arange(n, dtype=np.int32))
    assert got.shape[1] == n
    for c in range(n):
      assert np.array_equal(got[:, c].astype(bool), (wl == c).any(-1)), c
  t64 = np.random.default_rng(3).integers(-1, 64, size=n).astype(np.int32)
  got = E.world_planes_host(pack, rows, t64, facing=True, num_classes=64)
  assert got.shape[1] == 68 and np.array_equal(got, WM.planes_of_rows(pack, rows, t64, 64, facing=True))


def test_world_layer_id_names():
  pack, _ = case("clean_up")
  names = E.world_layer_id_names_host(pack)
  assert len(names) == E.num_world_layer_ids_host(pack) and names[0] == "" and names[1] == "OutOfBounds"
  # both number the pack's sprites: the names are "LAYER"'s as far as the world's ids go
  assert names == E.layer_id_names_host(pack)[:len(names)]


# ---- 2. the tie to every viewer's EGO_LAYER ------------------------------------------------------
@pytest.mark.parametrize("name", [COMMONS, KITCHEN, "externality_mushrooms__dense"])
def test_every_viewer_sees_the_world_through_its_own_sprite_map(name):
  """On a level whose world map is the identity, for every living viewer p and every window cell on
  the map, EGO_LAYER_p = 1 + view_sprite_map[p][WORLD.LAYER - 1], and 0 where WORLD.LAYER is 0."""
  pack, rows = case(name)
  H, W, L, (vl, vr, vf, vb), torus = EM.geometry(pack)
  maps = WM.sprite_maps(pack)
  fields, P = WM.fields_of(pack, rows)
  assert np.array_equal(maps[P], np.arange(maps.shape[1])) and not torus
  wl = E.world_layer_host(pack, rows)     # [R, H, W, L]
  ego = E.ego_layer_host(pack, rows)      # [R, P, VH, VW, L]
  ax, ay = fields.avatar_x.numpy()[:, :P].astype(int), fields.avatar_y.numpy()[:, :P].astype(int)
  ori, alive = fields.orientation.numpy()[:, :P].astype(int), fields.alive.numpy()[:, :P].astype(bool)
  seen = 0
  for r in range(len(rows)):
    for p in range(P):
      if not alive[r, p]:
        continue
      for vy in range(vf + vb + 1):
        for vx in range(vl + vr + 1):
          dx, dy = vx - vl, vy - vf
          tx, ty = [(dx, dy), (-dy, dx), (-dx, -dy), (dy, -dx)][ori[r, p]]
          x, y = ax[r, p] + tx, ay[r, p] + ty
          if not (0 <= x < W and 0 <= y < H):
            continue
          w = wl[r, y, x]
          assert np.array_equal(ego[r, p, vy, vx], np.where(w > 0, 1 + maps[p][np.maximum(w, 1) - 1], 0)), (r, p, vy, vx)
          seen += 1
  assert seen > 100


# ---- 3. refusals ---------------------------------------------------------------------------------
def _host_request(struct="planes", **over):
  """A well-formed host request of a world op on two clean_up rows, with some fields replaced."""
  pack, rows = case("clean_up")
  rows = np.ascontiguousarray(rows[:2])
  keep = E._host_config(pack)
  H, W, L = WM.geometry(pack)
  n = E.num_world_layer_ids_host(pack)
  classes = (np.arange(n, dtype=np.int32) % 4) - 1   # entries in [-1, 3)
  players = np.zeros(2, np.int32)
  if struct == "planes":
    out = np.zeros(2 * 7 * H * W + 1, np.uint8)
    req = dict(op=E.MP_EGOPLANES_WORLD_HOST, dst_bytes=2 * 7 * H * W, classes=classes.ctypes.data, classes_len=n,
               num_classes=3, facing=1)
  else:
    out = np.zeros(2 * H * W * L, np.int32)
    req = dict(op=E.MP_EGO_WORLD_HOST, dst_bytes=out.nbytes)
  req.update(fingerprint=E.state_layout(pack).fingerprint, pack=ctypes.addressof(keep[0]), pack_len=len(pack),
             cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p), bank=rows.ctypes.data, bank_rows=2, count=2,
             dst=out.ctypes.data)
  req.update(over)
  if req.get("players") == "set":
    req["players"] = players.ctypes.data
  if "dst_offset" in req:
    req["dst"] = out.ctypes.data + req.pop("dst_offset")
  if "class_entry" in req:
    classes[5] = req.pop("class_entry")
  op = req.pop("op")
  send = {"planes": E.ego_planes_request, "layer": E.ego_layer_request, "hash": E.view_hash_request,
          "ids": E.avatar_ids_request}[struct]
  try:
    return send(E.load_library(), None, op, **req)
  finally:
    del keep, rows, classes, players


def test_host_requests_are_refused_with_their_message():
  pack, rows = case("clean_up")
  n = E.num_world_layer_ids_host(pack)
  assert _host_request().num_ids == n   # (the well-formed one passes, and says how long a table is)
  assert _host_request(dst_offset=1).num_ids == n   # (a destination on an odd byte)
  assert _host_request(count=0, dst=None, bank=None, classes=None, classes_len=0).num_ids == n   # (the question alone)
  _host_request("layer")
  # the new refusals
  for struct, who in (("planes", "MpEgoPlanes"), ("layer", "MpEgoLayer")):
    with pytest.raises(ValueError, match=who + ": the world ops take no players"):
      _host_request(struct, players="set")
  with pytest.raises(ValueError, match=r"classes_len %d: a class table of the world has one entry per id of the "
                     r"world's sprite map, %d" % (n - 1, n)):
    _host_request(classes_len=n - 1)
  with pytest.raises(ValueError, match=r"classes_len %d" % (n + 1)):
    _host_request(classes_len=n + 1)
  with pytest.raises(ValueError, match=r"classes\[5\] = 3 is outside \[-1, num_classes = 3\)"):
    _host_request(class_entry=3)
  with pytest.raises(ValueError, match=r"classes\[5\] = -2 is outside"):
    _host_request(class_entry=-2)
  with pytest.raises(ValueError, match="layer_mask .* names no layer"):
    _host_request(layer_mask=1 << 9)
  with pytest.raises(ValueError, match="MpEgoLayer: dst .* is not 4-byte aligned"):
    _host_request("layer", dst_offset=2)
  with pytest.raises(ValueError, match=r"MpEgoLayer: MP_EGO_WORLD_HOST takes no engine|MpEgoLayer: NULL engine"):
    _host_request("layer", op=E.MP_EGO_WORLD_DRAW)
  with pytest.raises(ValueError, match="MpEgoPlanes: NULL engine"):
    _host_request(op=E.MP_EGOPLANES_WORLD_REGISTER)
  with pytest.raises(ValueError, match=r"rows\[1\] = 6 is not a row of the bank"):
    E.world_layer_host(pack, rows, which=[0, 6])
  with pytest.raises(ValueError, match=r"rows\[0\] = -1 is not a row of the bank"):
    E.world_planes_host(pack, rows, np.zeros(n, np.int32), which=[-1, 0])
  with pytest.raises(ValueError, match="classes must be %d integers" % n):
    E.world_planes_host(pack, rows, np.zeros(n + 1, np.int32))
  # the refusals that stay
  for struct in ("planes", "layer"):
    with pytest.raises(ValueError, match="reserved words"):
      _host_request(struct, reserved=1)
    with pytest.raises(ValueError, match="unknown op 9"):
      _host_request(struct, op=9)
    with pytest.raises(ValueError, match="unknown op 0"):
      _host_request(struct, op=0)
    with pytest.raises(ValueError, match="unknown op 7"):
      _host_request(struct, op=7)
  keep = E._host_config(pack)
  for send, who in ((E.view_hash_request, "MpViewHash"), (E.avatar_ids_request, "MpAvatarIds")):
    for op in (4, 5, 6):
      with pytest.raises(ValueError, match=f"{who}: unknown op {op}"):
        send(E.load_library(), None, op, pack=ctypes.addressof(keep[0]), pack_len=len(pack),
             cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p))


def test_the_op_constants_as_a_compiler_sees_them(tmp_path):
  include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))), "include")
  src = tmp_path / "ops.c"
  src.write_text('#include <stdio.h>\n#include "mp_engine.h"\nint main(void) {\n'
                 '  printf("%d %d %d %d %d %d %d %d\\n", MP_EGO_WORLD_DRAW, MP_EGO_WORLD_REGISTER, MP_EGO_WORLD_HOST,\n'
                 '         MP_EGOPLANES_WORLD_DRAW, MP_EGOPLANES_WORLD_REGISTER, MP_EGOPLANES_WORLD_HOST,\n'
                 '         (int)sizeof(MpEgoLayer), (int)sizeof(MpEgoPlanes));\n  return 0;\n}\n')
  exe = tmp_path / "ops"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", include, "-o", str(exe), str(src)], check=True)
  out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
  assert [int(v) for v in out] == [4, 5, 6, 4, 5, 6, ctypes.sizeof(E.MpEgoLayer), ctypes.sizeof(E.MpEgoPlanes)]
  assert (E.MP_EGO_WORLD_DRAW, E.MP_EGO_WORLD_REGISTER, E.MP_EGO_WORLD_HOST) == (4, 5, 6)
  assert (E.MP_EGOPLANES_WORLD_DRAW, E.MP_EGOPLANES_WORLD_REGISTER, E.MP_EGOPLANES_WORLD_HOST) == (4, 5, 6)


# ---- the Python surface that needs no device -----------------------------------------------------
def test_specs_and_refusals_that_need_no_device():
  cfg = substrate.get_config("clean_up")
  cfg.global_observation_names = ["WORLD.RGB", "WORLD.LAYER"]
  pack = E.load_pack("clean_up")
  spec = substrate.observation_spec_of(cfg, pack)
  assert spec["WORLD.LAYER"].shape == WM.geometry(pack) and spec["WORLD.LAYER"].dtype == np.int32
  keys = list(spec)
  assert keys.index("WORLD.LAYER") == keys.index("WORLD.RGB") + 1
  assert "WORLD.LAYER" not in substrate.observation_spec_of(substrate.get_config("clean_up"), pack)   # (no default names it)
  _, glob, chosen = substrate.select_observations(substrate.get_config("clean_up"), pack, ["RGB"], ["WORLD.LAYER"])
  assert glob == ["WORLD.LAYER"] and chosen["WORLD.LAYER"].shape == WM.geometry(pack)
  # a one-world substrate refuses the leaf before it creates an engine
  with pytest.raises(ValueError, match=r"WORLD\.LAYER.*needs a batched substrate"):
    substrate.build_from_config(cfg, roles=cfg.default_player_roles)
  # a mixture whose members' maps differ names the leaf
  with pytest.raises(ValueError, match=r"leaf 'WORLD\.LAYER' differs: territory__rooms \(21, 21, 11\) int32, "
                     r"territory__open \(23, 39, 11\) int32"):
    substrate.build_mixture(["territory__rooms", "territory__open"], num_worlds=[2, 2], env_seed=1,
                            individual_observations=["READY_TO_SHOOT"], global_observations=["WORLD.LAYER"])
