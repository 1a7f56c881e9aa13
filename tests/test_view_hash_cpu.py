"""The hash of each player's view (the MpViewHash request) without a GPU (its struct, wrappers and
kernels: tests/test_request_abi_cpu.py): the library's host twin
held to the numpy model (tests/view_hash_model.py: EGO_LAYER from tests/ego_layer_model.py, plain
uint64 arithmetic) on records written from the CPU oracle.  Every comparison is exact integer
equality.  The Python refusals run on the CPU oracle behind the engine interface."""
import ctypes
import functools

import numpy as np
import pytest

import ego_layer_model as EM
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
  48 random steps with beams."""
  pack = E.load_pack(name)
  rows, facings, dead = VM.oracle_rows(pack, len(substrate.get_config(name).action_set), SEED, STEPS, KEEP)
  return pack, rows, facings, dead


def fields_of(pack, rows):
  import torch

  from meltingpot_amd import pack as pack_lib
  layout = substrate.SubstrateStateLayout(E.state_layout(pack), pack_lib.loads(pack))
  return substrate.StateFields(torch.from_numpy(rows), layout)


# ---- structure ---------------------------------------------------------------------------------
def test_the_models_fmix64_is_the_published_one():
  M64 = (1 << 64) - 1

  def exact(h):
    h ^= h >> 33; h = h * 0xff51afd7ed558ccd & M64
    h ^= h >> 33; h = h * 0xc4ceb9fe1a85ec53 & M64
    return h ^ h >> 33
  vals = [1, M64, 0, 0x0123456789abcdef, 5 << 32 | 0xffffffff]
  assert [int(v) for v in VM.fmix64(np.array(vals, np.uint64))] == [exact(v) for v in vals]


# ---- the host twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LEVELS)
def test_the_host_twin_equals_the_model(name):
  pack, rows, facings, dead = case(name)
  # the chosen seed shows every facing, and (clean_up: the level with a beam that removes) a dead viewer
  assert facings == {0, 1, 2, 3}, facings
  if name == "clean_up":
    assert dead >= 1
  want = VM.of_rows(pack, rows)
  got = E.hash_views_host(pack, rows)
  assert got.dtype == np.int64 and got.shape == want.shape == (len(rows), E.state_layout(pack).P)
  assert np.array_equal(got, want)
  assert len(np.unique(got)) > 1
  # sampled (row, player) views, rows repeated and out of order, more views than rows
  rng = np.random.default_rng(5)
  which = rng.integers(0, len(rows), size=3 * len(rows)).astype(np.int32)
  players = rng.integers(0, want.shape[1], size=which.size).astype(np.int32)
  got = E.hash_views_host(pack, rows, players, which=which)
  assert got.shape == (which.size,) and np.array_equal(got, want[which, players])
  assert np.array_equal(E.hash_views_host(pack, rows, which=which[:4]), want[which[:4]])


def test_the_levels_are_the_ones_the_views_differ_on():
  """clean_up: 7 players, 11 x 11 x 9 views; the kitchen's map (5 rows of 9) is no taller than the
  5 x 5 window and three cells lie ahead of the avatar, so its views reach off the map: some of
  these have OutOfBounds cells next to cells of the map."""
  pack, rows, _, _ = case("clean_up")
  assert EM.of_rows(pack, rows).shape[1:] == (7, 11, 11, 9)
  pack, rows, _, _ = case(KITCHEN)
  H, W, _, (vl, vr, vf, vb), _ = EM.geometry(pack)
  assert H <= vf + vb + 1 and (H, W) == (5, 9)
  ego = EM.of_rows(pack, rows)
  assert ego.shape[1:] == (2, 5, 5, 9)
  oob = (ego == EM.lut(pack, ego.shape[1])[:, EM.OOB][None, :, None, None, None]).all(axis=-1)   # [R, P, VH, VW]
  share = oob.mean(axis=(2, 3))
  assert ((share > 0) & (share < 1)).any() and (share == 0).any()


def test_a_dead_viewer_hashes_an_all_out_of_bounds_view():
  pack, rows, _, _ = case("clean_up")
  f = fields_of(pack, rows.copy())
  got = E.hash_views_host(pack, rows)
  table = EM.lut(pack, got.shape[1])
  seen = 0
  for r, p in zip(*np.nonzero(f.alive.numpy()[:, :got.shape[1]] == 0)):
    blank = np.full((11, 11, 9), table[p, EM.OOB], np.int32)
    assert got[r, p] == VM.view_hash(blank)
    seen += 1
  assert seen >= 1


@pytest.mark.parametrize("name", LEVELS)
def test_layer_subsets_and_a_class_table_equal_the_model(name):
  pack, rows, _, _ = case(name)
  L = E.state_layout(pack).L
  P = E.state_layout(pack).P
  for layers in ([0], [L - 1], list(range(0, L, 2)), list(range(L))):
    got = E.hash_views_host(pack, rows, layers=layers)
    assert np.array_equal(got, VM.of_rows(pack, rows, layers=layers)), layers
  assert np.array_equal(E.hash_views_host(pack, rows, layers=range(L)), E.hash_views_host(pack, rows))
  # a table that merges two ids that occur in these views
  n = E.num_layer_ids_host(pack)
  assert n == VM.num_ids(pack, P)
  ego = EM.of_rows(pack, rows)
  ids = np.unique(ego)
  ids = ids[ids > 0]
  assert ids.size >= 2 and ids.max() < n
  classes = np.arange(n, dtype=np.int32)
  classes[ids[1]] = classes[ids[0]]
  got = E.hash_views_host(pack, rows, classes=classes)
  assert np.array_equal(got, VM.of_rows(pack, rows, classes=classes))
  assert (got != E.hash_views_host(pack, rows)).any()
  # two ids of one class are indistinguishable: exchanging them in a view changes nothing
  swapped = np.where(ego == ids[0], ids[1], np.where(ego == ids[1], ids[0], ego))
  assert np.array_equal(VM.view_hash(swapped, classes=classes), got)
  # classes and layers together, on sampled views
  got = E.hash_views_host(pack, rows, [P - 1, 0], which=[2, 5], layers=[L - 1, 0], classes=classes)
  assert np.array_equal(got, VM.of_rows(pack, rows, layers=[0, L - 1], classes=classes)[[2, 5], [P - 1, 0]])


def test_one_byte_changes_the_hashes_of_the_viewers_that_see_it_and_no_others():
  pack, rows, _, _ = case("clean_up")
  lay = E.state_layout(pack)
  H, W, L, (vl, vr, vf, vb), _ = EM.geometry(pack)
  reach = max(vl, vr, vf, vb)
  f = fields_of(pack, rows.copy())
  ax, ay, alive = (v.numpy()[:, :lay.P].astype(int) for v in (f.avatar_x, f.avatar_y, f.alive))
  table = EM.lut(pack, lay.P)
  before = E.hash_views_host(pack, rows)
  checked = 0
  for r in range(len(rows)):
    for p in range(lay.P):
      far = [q for q in range(lay.P) if max(abs(ax[r, q] - ax[r, p]), abs(ay[r, q] - ay[r, p])) > reach]
      if not alive[r, p] or not far:
        continue
      # the byte of layer 0 under viewer p's own cell (inside p's window whatever it faces) becomes
      # a state whose id differs for p
      edited = rows.copy()
      off = lay.cell_offset(0, ax[r, p], ay[r, p])
      old = int(edited[r, off])
      new = next(s for s in range(1, 256) if table[p, s] != table[p, old])
      edited[r, off] = new
      after = E.hash_views_host(pack, edited)
      assert np.array_equal(after, VM.of_rows(pack, edited))
      assert after[r, p] != before[r, p]
      for q in far:   # a viewer whose window does not hold the cell
        assert after[r, q] == before[r, q]
      others = np.ones(len(rows), bool)
      others[r] = False
      assert np.array_equal(after[others], before[others])
      # the model says exactly who sees it
      changed = (EM.of_rows(pack, edited)[r] != EM.of_rows(pack, rows)[r]).any(axis=(1, 2, 3))
      assert np.array_equal(after[r] != before[r], changed)
      # on an excluded layer the edit changes nothing
      rest = list(range(1, L))
      assert np.array_equal(E.hash_views_host(pack, edited, layers=rest), E.hash_views_host(pack, rows, layers=rest))
      assert (E.hash_views_host(pack, edited, layers=[0]) != E.hash_views_host(pack, rows, layers=[0])).any()
      checked += 1
      break
  assert checked >= 3


# ---- refusals ------------------------------------------------------------------------------------
def _host_request(**over):
  """A well-formed MP_VIEWHASH_HOST request on two clean_up rows, with some fields replaced."""
  pack, rows, _, _ = case("clean_up")
  rows = np.ascontiguousarray(rows[:2])
  keep = E._host_config(pack)
  P = E.state_layout(pack).P
  out = np.zeros(2 * P + 1, np.int64)
  classes = np.arange(E.num_layer_ids_host(pack), dtype=np.int32)
  req = dict(op=E.MP_VIEWHASH_HOST, fingerprint=E.state_layout(pack).fingerprint, pack=ctypes.addressof(keep[0]),
             pack_len=len(pack), cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p), bank=rows.ctypes.data,
             bank_rows=2, count=2, dst=out.ctypes.data, dst_bytes=2 * P * 8)
  req.update(over)
  if "dst_offset" in req:
    req["dst"] = out.ctypes.data + req.pop("dst_offset")
  if req.pop("with_classes", False):
    req["classes"] = classes.ctypes.data
  op = req.pop("op")
  try:
    return E.view_hash_request(E.load_library(), None, op, **req)
  finally:
    del keep, rows, classes


def test_requests_are_refused_with_their_message():
  n = E.num_layer_ids_host(case("clean_up")[0])
  assert _host_request().num_ids == n   # (the well-formed one passes, and says how long a table is)
  assert _host_request(with_classes=True, classes_len=n).num_ids == n
  assert _host_request(count=0, dst=None, bank=None).num_ids == n   # (the question alone)
  with pytest.raises(ValueError, match="MpViewHash: NULL engine"):
    _host_request(op=E.MP_VIEWHASH_DRAW)
  with pytest.raises(ValueError, match="MpViewHash: NULL engine"):
    _host_request(op=E.MP_VIEWHASH_REGISTER)
  with pytest.raises(ValueError, match="needs the pack"):
    _host_request(pack=None)
  with pytest.raises(ValueError, match=r"2 elements of 56 bytes need 112 bytes, dst has 16"):
    _host_request(dst_bytes=16)
  with pytest.raises(ValueError, match="not 8-byte aligned"):
    _host_request(dst_offset=4)
  with pytest.raises(ValueError, match="fingerprint 0000000000000001 is not this pack's"):
    _host_request(fingerprint=1)
  with pytest.raises(ValueError, match="unknown op 9"):
    _host_request(op=9)
  with pytest.raises(ValueError, match="reserved words"):
    _host_request(reserved=1)
  with pytest.raises(ValueError, match=r"classes_len %d: a class table has one entry per id, %d" % (n - 1, n)):
    _host_request(with_classes=True, classes_len=n - 1)
  with pytest.raises(ValueError, match=r"classes_len %d" % (n + 1)):
    _host_request(with_classes=True, classes_len=n + 1)
  with pytest.raises(ValueError, match=r"classes_len %d" % n):
    _host_request(classes_len=n)   # (a length without a table)
  with pytest.raises(ValueError, match="layer_mask .* names no layer"):
    _host_request(layer_mask=1 << 9)
  pack, rows, _, _ = case("clean_up")
  with pytest.raises(ValueError, match=r"rows\[1\] = 6 is not a row of the bank"):
    E.hash_views_host(pack, rows, which=[0, 6])
  with pytest.raises(ValueError, match=r"players\[0\] = 7 is not a player"):
    E.hash_views_host(pack, rows, [7, 0], which=[0, 1])
  with pytest.raises(ValueError, match="classes must be %d integers" % n):
    E.hash_views_host(pack, rows, classes=np.arange(n - 1))
  with pytest.raises(ValueError, match="9 is no layer of the view"):
    E.hash_views_host(pack, rows, layers=[0, 9])
  with pytest.raises(ValueError, match="includes no layer"):
    E.hash_views_host(pack, rows, layers=[])


class HashBatchEngine(OracleBatchEngine):
  """OracleBatchEngine with what Substrate asks of an engine before it hashes (it hashes nothing)."""

  def state_layout(self):
    return E.state_layout(self.pack_bytes)


def test_python_refusals(monkeypatch):
  monkeypatch.setattr(substrate.engine_lib, "Engine", HashBatchEngine)
  cfg = substrate.get_config("clean_up")
  roles = cfg.default_player_roles
  one = substrate.build_from_config(cfg, roles=roles)
  try:
    with pytest.raises(ValueError, match="hash_views needs a batched substrate"):
      one.hash_views()
    with pytest.raises(ValueError, match="set_view_hashes needs a batched substrate"):
      one.set_view_hashes()
  finally:
    one.close()
  env = substrate.build_from_config(cfg, roles=roles, num_worlds=2)
  try:
    names = env.state_layout().layer_names
    assert len(names) == 9
    assert env._view_layers([names[3], 0]) == [3, 0] and env._view_layers(None) is None
    assert env._view_layers(names[1]) == [1]
    with pytest.raises(ValueError, match="'no_such_layer' is no layer of this level"):
      env.hash_views(layers=["no_such_layer"])
    with pytest.raises(ValueError, match="'no_such_layer' is no layer of this level"):
      env.set_view_hashes(layers=[names[0], "no_such_layer"])
    with pytest.raises(ValueError, match="hash_views takes the WorldStates"):
      env.hash_views(states=np.zeros((1, 8), np.uint8))
  finally:
    env.close()
