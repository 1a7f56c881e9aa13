"""EGO_LAYER (the MpEgoLayer request) without a GPU (its struct, wrappers and kernels:
tests/test_request_abi_cpu.py): the library's host twin held to the numpy
model (tests/ego_layer_model.py) and — for every viewer that faces north — to the oracle's layer
view, on the real rows of tests/golden/state_rows.npz (saved on a GPU by the recipe of
tests/states_recipe.py).  The Python refusals run on the CPU oracle behind the engine interface."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ego_layer_model as M
import states_recipe as R
import util
from meltingpot_amd import substrate
from meltingpot_amd import engine as E
from oracle_engine import OracleBatchEngine

HERE = os.path.dirname(os.path.abspath(__file__))
PACKS = ("clean_up", "commons_harvest__open", "coins", "collaborative_cooking__cramped",
         "prisoners_dilemma_in_the_matrix__repeated")


def golden_rows(name):
  return dict(np.load(os.path.join(HERE, "golden", "state_rows.npz")))[name + "/rows"]


def fields_of(name, rows):
  from meltingpot_amd import pack as pack_lib
  layout = substrate.SubstrateStateLayout(E.state_layout(R.pack(name)), pack_lib.loads(R.pack(name)))
  return substrate.StateFields(torch.from_numpy(np.ascontiguousarray(rows)), layout)


# ---- the host twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PACKS)
def test_the_host_twin_equals_the_model(name):
  rows = golden_rows(name)
  want = M.of_rows(R.pack(name), rows)
  got = E.ego_layer_host(R.pack(name), rows)
  assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
  # sampled (row, player) views, rows repeated and out of order, more views than rows
  rng = np.random.default_rng(5)
  which = rng.integers(0, len(rows), size=3 * len(rows)).astype(np.int32)
  players = rng.integers(0, want.shape[1], size=which.size).astype(np.int32)
  got = E.ego_layer_host(R.pack(name), rows, players, which=which)
  assert got.shape == (which.size,) + want.shape[2:] and np.array_equal(got, want[which, players])
  assert np.array_equal(E.ego_layer_host(R.pack(name), rows, which=which[:4]), want[which[:4]])


@pytest.mark.parametrize("name", ["clean_up", "commons_harvest__open"])
def test_a_viewer_that_faces_north_sees_the_oracle_s_layer_view(name):
  """Rows 0 .. 5 of the fixture are worlds 0 and 4 after steps 1, 16 and 17 of the recipe."""
  rows = golden_rows(name)[:6]
  f = fields_of(name, rows)
  got = E.ego_layer_host(R.pack(name), rows)
  north = M.of_rows(R.pack(name), rows, north=True)
  A = R.actions(got.shape[1], len(substrate.get_config(name).action_set))
  seen = {"north": 0, "turned": 0}
  for i, (w, steps) in enumerate([(0, 1), (4, 1), (0, 16), (4, 16), (0, 17), (4, 17)]):
    o = util.make_oracles(R.pack(name), 1, offset=w)[0]
    o.reset()
    for k in range(steps):
      if o.done:
        o.reset()
      else:
        o.step(A[k, w])
    for p in range(o.P):
      assert np.array_equal(north[i, p], o.layer_view(p)), (name, i, p)   # (the model's north crop)
      if int(f.orientation[i, p]) == 0:
        assert np.array_equal(got[i, p], o.layer_view(p)), (name, i, p)
        seen["north"] += 1
      elif int(f.alive[i, p]):
        seen["turned"] += not np.array_equal(got[i, p], o.layer_view(p))
    o.close()
  assert seen["north"] > 0 and seen["turned"] > 0, seen


@pytest.mark.parametrize("name", R.DEAD_AVATARS)
def test_a_dead_viewer_is_all_out_of_bounds(name):
  rows = golden_rows(name)[6:7]
  f = fields_of(name, rows)
  dead = np.flatnonzero(f.alive[0].numpy() == 0)
  assert dead.size > 0
  got = E.ego_layer_host(R.pack(name), rows)
  table = M.lut(R.pack(name), got.shape[1])
  for p in dead:
    assert (got[0, p] == table[p, M.OOB]).all()
  alive = np.flatnonzero(f.alive[0].numpy() != 0)
  assert any((got[0, p] != table[p, M.OOB]).any() for p in alive)


# ---- refusals ------------------------------------------------------------------------------------
def _host_request(**over):
  """A well-formed MP_EGO_HOST request on two clean_up rows, with some fields replaced."""
  pack = R.pack("clean_up")
  rows = np.ascontiguousarray(golden_rows("clean_up")[:2])
  keep = E._host_config(pack)
  out = np.zeros(E.ego_layer_host(pack, rows).size + 1, np.int32)
  req = dict(op=E.MP_EGO_HOST, fingerprint=E.state_layout(pack).fingerprint, pack=ctypes.addressof(keep[0]),
             pack_len=len(pack), cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p), bank=rows.ctypes.data,
             bank_rows=2, count=2, dst=out.ctypes.data, dst_bytes=(out.size - 1) * 4)
  req.update(over)
  if "dst_offset" in req:
    req["dst"] = out.ctypes.data + req.pop("dst_offset")
  op = req.pop("op")
  try:
    E.ego_layer_request(E.load_library(), None, op, **req)
  finally:
    del keep, rows
  return out


def test_requests_are_refused_with_their_message():
  _host_request()   # (the well-formed one passes)
  with pytest.raises(ValueError, match="MpEgoLayer: NULL engine"):
    _host_request(op=E.MP_EGO_DRAW)
  with pytest.raises(ValueError, match="MpEgoLayer: NULL engine"):
    _host_request(op=E.MP_EGO_REGISTER)
  with pytest.raises(ValueError, match="needs the pack"):
    _host_request(pack=None)
  with pytest.raises(ValueError, match=r"2 elements of \d+ bytes need \d+ bytes, dst has 16"):
    _host_request(dst_bytes=16)
  with pytest.raises(ValueError, match="not 4-byte aligned"):
    _host_request(dst_offset=2)
  with pytest.raises(ValueError, match="fingerprint 0000000000000001 is not this pack's"):
    _host_request(fingerprint=1)
  with pytest.raises(ValueError, match="unknown op 9"):
    _host_request(op=9)
  with pytest.raises(ValueError, match="reserved words"):
    _host_request(reserved=1)
  with pytest.raises(ValueError, match=r"rows\[1\] = 2 is not a row of the bank"):
    E.ego_layer_host(R.pack("clean_up"), golden_rows("clean_up")[:2], which=[0, 2])
  with pytest.raises(ValueError, match=r"players\[0\] = 7 is not a player"):
    E.ego_layer_host(R.pack("clean_up"), golden_rows("clean_up")[:2], [7, 0])


class EgoBatchEngine(OracleBatchEngine):
  """OracleBatchEngine with what Substrate asks of an engine for the leaf (the leaf stays zero)."""

  @property
  def ego_layer_shape(self):
    vh, vw, L = substrate.layer_spec(self.pack_bytes).shape
    return (self.N, self.P, vh, vw, L)

  def bind_ego_layer(self, out):
    return out

  def bind_ego_layer_ring(self, tensor=None, slots=None):
    return torch.zeros((int(slots),) + self.ego_layer_shape, dtype=torch.int32) if tensor is None else tensor


def _config_with_the_leaf(name="clean_up"):
  cfg = substrate.get_config(name)
  cfg.individual_observation_names = list(cfg.individual_observation_names) + ["EGO_LAYER"]
  return cfg


def test_python_refusals_and_the_spec(monkeypatch):
  monkeypatch.setattr(substrate.engine_lib, "Engine", EgoBatchEngine)
  for name in substrate.SUBSTRATES:   # no default observation list names the leaf
    assert "EGO_LAYER" not in substrate.get_config(name).individual_observation_names
  cfg = _config_with_the_leaf()
  roles = cfg.default_player_roles
  with pytest.raises(ValueError, match='"EGO_LAYER" needs a batched substrate'):
    substrate.build_from_config(cfg, roles=roles)
  with pytest.raises(ValueError, match='"EGO_LAYER" needs a batched substrate'):
    substrate.get_factory_from_config(cfg).build(roles)
  env = substrate.build_from_config(cfg, roles=roles, num_worlds=2)
  try:
    spec = env.observation_spec()[0]["EGO_LAYER"]
    want = substrate.layer_spec(E.load_pack("clean_up"))
    assert spec.shape == want.shape and spec.dtype == np.int32 and spec.name == "EGO_LAYER"
    ts = env.reset()
    assert tuple(ts.observation["EGO_LAYER"].shape) == (2, len(roles)) + want.shape
    assert ts.observation["EGO_LAYER"].dtype == torch.int32
    assert "EGO_LAYER" not in env.step_leaves()
    a = np.zeros((3, 2, len(roles)), np.int32)
    with pytest.raises(ValueError, match=r"states=True.*observe_states"):
      env.step_many(a, observations=("EGO_LAYER",))
    with pytest.raises(ValueError, match=r"states=True.*observe_states"):
      env.step_many(a, observations=("READY_TO_SHOOT", "EGO_LAYER"))
  finally:
    env.close()
  # a ring slot per submission, named like every other leaf
  env = substrate.build_from_config(cfg, roles=roles, num_worlds=2, rollout_length=3)
  try:
    assert tuple(env.rollout["observation"]["EGO_LAYER"].shape) == (3, 2, len(roles)) + want.shape
    assert tuple(env.reset().observation["EGO_LAYER"].shape) == (2, len(roles)) + want.shape
  finally:
    env.close()
  # an unknown name is still refused, and the leaf is no global observation
  cfg = substrate.get_config("clean_up")
  cfg.global_observation_names = list(cfg.global_observation_names) + ["EGO_LAYER"]
  with pytest.raises(ValueError, match="EGO_LAYER"):
    substrate.build_from_config(cfg, roles=roles, num_worlds=2)
