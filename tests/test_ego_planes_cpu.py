"""Class-indicator feature planes of each player's view (the MpEgoPlanes request) without a GPU
(its struct, wrappers and kernels: tests/test_request_abi_cpu.py): the
library's host twin held to the numpy model (tests/ego_planes_model.py: EGO_LAYER from
tests/ego_layer_model.py through the class table, the facing planes from positions and
orientations) on records written from the CPU oracle.  Every comparison is exact byte equality.
The names (`layer_id_names`, `layer_classes`) and the Python refusals run on the CPU oracle behind
the engine interface."""
import ctypes
import functools
import os

import numpy as np
import pytest

import ego_layer_model as EM
import ego_planes_model as PM
import view_hash_model as VM
from meltingpot_amd import substrate
from meltingpot_amd import engine as E
from oracle_engine import OracleBatchEngine

KITCHEN = "collaborative_cooking__cramped"
MATRIX = "prisoners_dilemma_in_the_matrix__repeated"
LEVELS = ("clean_up", KITCHEN, MATRIX)
STEPS, KEEP, SEED = 48, (8, 16, 24, 32, 40, 48), 1


@functools.lru_cache(maxsize=None)
def case(name):
  """(pack, rows uint8 [6, S], facings, dead viewers) of a level: one oracle world after 8, 16, ...
  48 random steps with beams (the rows of tests/test_view_hash_cpu.py)."""
  pack = E.load_pack(name)
  rows, facings, dead = VM.oracle_rows(pack, len(substrate.get_config(name).action_set), SEED, STEPS, KEEP)
  return pack, rows, facings, dead


def table_of(pack, C, seed=3):
  """A random table with every class of [-1, C) in it where the ids suffice."""
  n = E.num_layer_ids_host(pack)
  t = np.random.default_rng(seed).integers(-1, C, size=n).astype(np.int32)
  t[:min(n, C + 1)] = np.arange(-1, min(n, C + 1) - 1)
  return t


# ---- the host twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("facing", [False, True])
@pytest.mark.parametrize("name", LEVELS)
def test_the_host_twin_equals_the_model(name, facing):
  pack, rows, facings, dead = case(name)
  # the chosen seed shows every facing, and (clean_up: the level with a beam that removes) a dead viewer
  assert facings == {0, 1, 2, 3}, facings
  if name == "clean_up":
    assert dead >= 1
  lay = E.state_layout(pack)
  C = 6
  classes = table_of(pack, C)
  assert set(classes.tolist()) == set(range(-1, C))   # (a table with -1 entries)
  want = PM.of_rows(pack, rows, classes, C, facing=facing)
  got = E.ego_planes_host(pack, rows, classes, facing=facing)
  _, _, _, (vl, vr, vf, vb), _ = EM.geometry(pack)
  assert got.dtype == np.uint8 and got.shape == want.shape == (len(rows), lay.P, C + 4 * facing, vf + vb + 1, vl + vr + 1)
  assert np.array_equal(got, want)
  assert set(np.unique(got).tolist()) == {0, 1}
  if facing:
    # a living viewer sees itself at (vf, vl), facing as it faces; a dead viewer's facing planes are 0
    import torch
    from meltingpot_amd import pack as pack_lib
    fields = substrate.StateFields(torch.from_numpy(rows.copy()), substrate.SubstrateStateLayout(lay, pack_lib.loads(pack)))
    alive = fields.alive.numpy()[:, :lay.P].astype(bool)
    assert np.array_equal(got[:, :, C, vf, vl].astype(bool), alive)
    assert not got[:, :, C:][~alive].any()
  # sampled (row, player) views, rows repeated and out of order, more views than rows
  rng = np.random.default_rng(5)
  which = rng.integers(0, len(rows), size=3 * len(rows)).astype(np.int32)
  players = rng.integers(0, lay.P, size=which.size).astype(np.int32)
  which[1], players[1] = which[0], players[0]
  got = E.ego_planes_host(pack, rows, classes, players, which=which, facing=facing)
  assert got.shape == (which.size,) + want.shape[2:] and np.array_equal(got, want[which, players])
  assert np.array_equal(E.ego_planes_host(pack, rows, classes, which=which[:4], facing=facing), want[which[:4]])
  # a choice of layers
  L = lay.L
  for layers in ([0], [L - 1, 0], list(range(0, L, 2))):
    got = E.ego_planes_host(pack, rows, classes, layers=layers, facing=facing)
    assert np.array_equal(got, PM.of_rows(pack, rows, classes, C, layers=layers, facing=facing)), layers
  assert np.array_equal(E.ego_planes_host(pack, rows, classes, layers=range(L), facing=facing), want)


@pytest.mark.parametrize("name", LEVELS)
def test_one_class_and_sixty_four(name):
  pack, rows, _, _ = case(name)
  n = E.num_layer_ids_host(pack)
  # C = 1: "something of the table is here"; the default num_classes is 1 + the largest entry
  one = np.where(np.arange(n) % 3 == 1, 0, -1).astype(np.int32)
  got = E.ego_planes_host(pack, rows, one, facing=True)
  assert got.shape[2] == 5 and np.array_equal(got, PM.of_rows(pack, rows, one, 1, facing=True))
  assert got[:, :, 0].any() and not got[:, :, 0].all()
  # C = 64: every bit of a cell's mask, with more classes than ids occur
  t64 = table_of(pack, 64)
  got = E.ego_planes_host(pack, rows, t64, facing=True, num_classes=64)
  assert got.shape[2] == 68 and np.array_equal(got, PM.of_rows(pack, rows, t64, 64, facing=True))
  high = np.full(n, -1, np.int32)
  high[1] = 63   # OutOfBounds alone, in the last plane
  got = E.ego_planes_host(pack, rows, high)
  assert got.shape[2] == 64 and not got[:, :, :63].any()
  assert np.array_equal(got, PM.of_rows(pack, rows, high, 64))


def test_identities_that_need_no_model():
  # with the identity table, plane c is (EGO_LAYER == c).any(-1)
  for name in (MATRIX, "clean_up"):
    pack, rows, _, _ = case(name)
    n = E.num_layer_ids_host(pack)
    assert n <= 64
    ego = E.ego_layer_host(pack, rows)   # [R, P, VH, VW, L]
    got = E.ego_planes_host(pack, rows, np.arange(n, dtype=np.int32))
    assert got.shape[2] == n
    for c in range(n):
      assert np.array_equal(got[:, :, c].astype(bool), (ego == c).any(-1)), (name, c)
  # for a viewer that faces north the class planes are those of "LAYER" (the window not turned)
  pack, rows, _, _ = case("clean_up")
  import torch
  from meltingpot_amd import pack as pack_lib
  lay = E.state_layout(pack)
  fields = substrate.StateFields(torch.from_numpy(rows.copy()), substrate.SubstrateStateLayout(lay, pack_lib.loads(pack)))
  classes = table_of(pack, 6)
  got = E.ego_planes_host(pack, rows, classes)
  north = PM.class_planes(EM.of_rows(pack, rows, north=True), classes, 6)
  faces_north = fields.orientation.numpy()[:, :lay.P] == 0
  assert faces_north.any() and not faces_north.all()
  assert np.array_equal(got[faces_north], north[faces_north])
  turned = fields.alive.numpy()[:, :lay.P].astype(bool) & ~faces_north
  assert (got[turned] != north[turned]).any()


# ---- refusals ------------------------------------------------------------------------------------
def _host_request(**over):
  """A well-formed MP_EGOPLANES_HOST request on two clean_up rows, with some fields replaced."""
  pack, rows, _, _ = case("clean_up")
  rows = np.ascontiguousarray(rows[:2])
  keep = E._host_config(pack)
  P = E.state_layout(pack).P
  n = E.num_layer_ids_host(pack)
  classes = (np.arange(n, dtype=np.int32) % 4) - 1   # entries in [-1, 3)
  out = np.zeros(2 * P * 7 * 121 + 1, np.uint8)
  req = dict(op=E.MP_EGOPLANES_HOST, fingerprint=E.state_layout(pack).fingerprint, pack=ctypes.addressof(keep[0]),
             pack_len=len(pack), cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p), bank=rows.ctypes.data,
             bank_rows=2, count=2, dst=out.ctypes.data, dst_bytes=2 * P * 7 * 121, classes=classes.ctypes.data,
             classes_len=n, num_classes=3, facing=1)
  req.update(over)
  if "dst_offset" in req:
    req["dst"] = out.ctypes.data + req.pop("dst_offset")
  if "class_entry" in req:
    classes[5] = req.pop("class_entry")
  op = req.pop("op")
  try:
    return E.ego_planes_request(E.load_library(), None, op, **req)
  finally:
    del keep, rows, classes


def test_requests_are_refused_with_their_message():
  n = E.num_layer_ids_host(case("clean_up")[0])
  assert _host_request().num_ids == n   # (the well-formed one passes, and says how long a table is)
  assert _host_request(dst_offset=1).num_ids == n   # (a destination on an odd byte)
  assert _host_request(count=0, dst=None, bank=None, classes=None, classes_len=0).num_ids == n   # (the question alone)
  with pytest.raises(ValueError, match="MpEgoPlanes: NULL engine"):
    _host_request(op=E.MP_EGOPLANES_DRAW)
  with pytest.raises(ValueError, match="MpEgoPlanes: NULL engine"):
    _host_request(op=E.MP_EGOPLANES_REGISTER)
  with pytest.raises(ValueError, match="needs the pack"):
    _host_request(pack=None)
  with pytest.raises(ValueError, match=r"2 elements of 5929 bytes need 11858 bytes, dst has 16"):
    _host_request(dst_bytes=16)
  with pytest.raises(ValueError, match="fingerprint 0000000000000001 is not this pack's"):
    _host_request(fingerprint=1)
  with pytest.raises(ValueError, match="unknown op 9"):
    _host_request(op=9)
  with pytest.raises(ValueError, match="reserved words"):
    _host_request(reserved=1)
  with pytest.raises(ValueError, match="NULL classes"):
    _host_request(classes=None)
  with pytest.raises(ValueError, match=r"classes_len %d: a class table has one entry per id, %d" % (n - 1, n)):
    _host_request(classes_len=n - 1)
  with pytest.raises(ValueError, match=r"classes_len %d" % (n + 1)):
    _host_request(classes_len=n + 1)
  for C in (0, 65, -1):
    with pytest.raises(ValueError, match=r"num_classes %d is outside \[1, 64\]" % C):
      _host_request(num_classes=C)
  with pytest.raises(ValueError, match=r"classes\[5\] = 3 is outside \[-1, num_classes = 3\)"):
    _host_request(class_entry=3)
  with pytest.raises(ValueError, match=r"classes\[5\] = -2 is outside"):
    _host_request(class_entry=-2)
  with pytest.raises(ValueError, match="facing 2"):
    _host_request(facing=2)
  with pytest.raises(ValueError, match="layer_mask .* names no layer"):
    _host_request(layer_mask=1 << 9)
  pack, rows, _, _ = case("clean_up")
  classes = table_of(pack, 3)
  with pytest.raises(ValueError, match=r"rows\[1\] = 6 is not a row of the bank"):
    E.ego_planes_host(pack, rows, classes, which=[0, 6])
  with pytest.raises(ValueError, match=r"players\[0\] = 7 is not a player"):
    E.ego_planes_host(pack, rows, classes, [7, 0], which=[0, 1])
  with pytest.raises(ValueError, match="classes must be %d integers" % n):
    E.ego_planes_host(pack, rows, classes[:-1])
  with pytest.raises(ValueError, match=r"num_classes 0 is outside \[1, 64\]"):
    E.ego_planes_host(pack, rows, classes, num_classes=0)
  with pytest.raises(ValueError, match=r"num_classes 65 is outside \[1, 64\]"):
    E.ego_planes_host(pack, rows, classes, num_classes=65)
  with pytest.raises(ValueError, match=r"num_classes 0 is outside .* 1 \+ the largest entry"):
    E.ego_planes_host(pack, rows, np.full(n, -1))
  with pytest.raises(ValueError, match=r"classes\[\d+\] = 2 is outside \[-1, num_classes = 2\)"):
    E.ego_planes_host(pack, rows, classes, num_classes=2)
  with pytest.raises(ValueError, match="9 is no layer of the view"):
    E.ego_planes_host(pack, rows, classes, layers=[0, 9])
  with pytest.raises(ValueError, match="includes no layer"):
    E.ego_planes_host(pack, rows, classes, layers=[])
  with pytest.raises(ValueError, match="rows of 100 bytes"):
    E.ego_planes_host(pack, rows[:, :100], classes)


# ---- names -----------------------------------------------------------------------------------------
def test_layer_id_names_of_every_committed_pack():
  from meltingpot_amd import pack as pack_lib
  import glob
  seen = 0
  for path in sorted(glob.glob(os.path.join(os.path.dirname(E.__file__), "assets", "*.mpk"))):
    name = os.path.basename(path)[:-len(".mpk")]
    pack = E.load_pack(name)
    names = E.layer_id_names_host(pack)
    assert len(names) == E.num_layer_ids_host(pack)
    assert names[0] == "" and names[1] == "OutOfBounds", (name, names[:3])
    sprites = bytes(pack_lib.loads(pack)["sprite_names"]).split(b"\0")[:-1]
    assert all(names[i] == sprites[i - 1].decode() for i in range(1, len(names)))
    seen += 1
  assert seen >= 5
  names = E.layer_id_names_host(E.load_pack("clean_up"))
  assert names[:7] == ("", "OutOfBounds", "OutOfView", "Avatar1", "Self", "BeamZap", "BeamClean")


class NamesBatchEngine(OracleBatchEngine):
  """OracleBatchEngine with what Substrate asks of an engine for the names (it draws nothing)."""

  def state_layout(self):
    return E.state_layout(self.pack_bytes)

  @property
  def num_layer_ids(self):
    return E.num_layer_ids_host(self.pack_bytes)

  @property
  def layer_id_names(self):
    return E.layer_id_names_host(self.pack_bytes)


def test_layer_classes_and_python_refusals(monkeypatch):
  monkeypatch.setattr(substrate.engine_lib, "Engine", NamesBatchEngine)
  cfg = substrate.get_config("clean_up")
  roles = cfg.default_player_roles
  one = substrate.build_from_config(cfg, roles=roles)
  try:
    with pytest.raises(ValueError, match="observe_ego_planes needs a batched substrate"):
      one.observe_ego_planes(np.zeros(34, np.int32))
    with pytest.raises(ValueError, match="set_ego_planes needs a batched substrate"):
      one.set_ego_planes(np.zeros(34, np.int32))
  finally:
    one.close()
  env = substrate.build_from_config(cfg, roles=roles, num_worlds=2)
  try:
    names = env.layer_id_names
    assert len(names) == env.num_layer_ids == 34 and names[1] == "OutOfBounds"
    assert env.state_layout().sprite_names[:3] == ("OutOfBounds", "OutOfView", "Avatar1")
    groups = ["Self", "Avatar*", "Beam*", "Wall*", "OutOfBounds"]
    table = env.layer_classes(groups)
    assert table.dtype == np.int32 and table.shape == (34,)
    # round trip: an id's class names it, and every id no group names is -1
    import fnmatch
    for i, n in enumerate(names):
      hits = [c for c, g in enumerate(groups) if n and fnmatch.fnmatchcase(n, g)]
      assert table[i] == (hits[0] if hits else -1), (i, n)
    assert table[names.index("Self")] == 0 and table[names.index("Avatar7")] == 1 and table[names.index("BeamClean")] == 2
    assert table[0] == -1 and table[names.index("Apple")] == -1
    # a class of several names and patterns; a name twice in ONE class is no conflict
    nested = env.layer_classes([("Apple", "Grass*", "Apple"), ["water_?"], "Dirt"])
    assert nested[names.index("Apple")] == 0 == nested[names.index("GrassEdge")] and nested[names.index("water_3")] == 1
    assert nested[names.index("Dirt")] == 2 and (nested >= 0).sum() == 3 + 4 + 1
    # the table is what ego_planes_host and hash_views_host take
    pack, rows, _, _ = case("clean_up")
    planes = E.ego_planes_host(pack, rows, table, facing=True)
    assert planes.shape[2] == len(groups) + 4 and np.array_equal(planes, PM.of_rows(pack, rows, table, facing=True))
    assert np.array_equal(E.hash_views_host(pack, rows, classes=table), VM.of_rows(pack, rows, classes=table))
    with pytest.raises(ValueError, match="'Banana\\*' matches no id of this level"):
      env.layer_classes(["Self", "Banana*"])
    with pytest.raises(ValueError, match=r"id \d+ \('Self'\) is matched by class 0 and by class 1"):
      env.layer_classes(["Self", "S*"])
    with pytest.raises(ValueError, match="'no_such_layer' is no layer of this level"):
      env.observe_ego_planes(table, layers=["no_such_layer"])
    with pytest.raises(ValueError, match="observe_ego_planes takes the WorldStates"):
      env.observe_ego_planes(table, states=np.zeros((1, 8), np.uint8))
  finally:
    env.close()
