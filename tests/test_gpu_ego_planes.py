"""Class-indicator feature planes of each player's view on the GPU (MpEgoPlanes;
Engine.observe_ego_planes / bind_ego_planes, Substrate.observe_ego_planes / set_ego_planes,
MixtureSubstrate's): both kernels against the numpy model of tests/ego_planes_model.py (EGO_LAYER
from tests/ego_layer_model.py through the class table; the facing planes from the positions and
orientations) and against the library's host twin, edited windows and tori, sampled views and
destinations that start on any byte, indices and class entries out of range, the registered tensor
behind every kind of submission with and without a rollout ring, and the mixture's shared tensor.
Every comparison is exact byte equality."""
import numpy as np
import pytest
import torch

import ego_layer_model as EM
import ego_planes_model as PM
import geometry
import util
from meltingpot_amd import engine, substrate
from meltingpot_amd import pack as pack_lib

pytestmark = pytest.mark.gpu

E = engine
N = 6
SEED = 5   # (chosen with the CPU oracle: all four facings and dead viewers within 25 random steps of clean_up)
KITCHEN = "collaborative_cooking__cramped"
MATRIX = "prisoners_dilemma_in_the_matrix__repeated"
# clean_up's table by name: 10 classes, "OutOfView" and id 0 belong to none (checked with the CPU
# oracle's rows and the model: every plane of it, and each of the four facing planes, is 1 somewhere
# in the 25 x 6 rows of test 1, and 0 somewhere; no apple grows in them, so "Apple" shares a class)
CLEAN_UP_GROUPS = ["Self", "Avatar*", "Beam*", "Wall", "water_*", "Dirt", "Sand", ("Shadow*", "GrassEdge"),
                   ("Apple", "Grass"), "OutOfBounds"]
# the mixture's table by name: the two kitchens number two of their sprites differently, so the
# mixture takes one table a member
KITCHEN_GROUPS = ["Self", "Avatar*", "OutOfBounds", "*tomato*", "*dish*"]
FILL = 0xA5


def _same(got, want, what):
  got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
  want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
  assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape)
  assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def _fields(eng, bank):
  layout = substrate.SubstrateStateLayout(eng.state_layout(), pack_lib.loads(eng.pack_bytes))
  return substrate.StateFields(bank, layout)


def _model(eng, bank, classes, C=None, layers=None, facing=False):
  classes = classes.cpu().numpy() if isinstance(classes, torch.Tensor) else classes
  return PM.of_fields(eng.pack_bytes, _fields(eng, bank), classes, C, layers, facing)


def _occurring(eng, bank, C):
  """A table from the MODEL's view of the rows: the ids that occur, dealt to C classes in turn
  (every class plane is then 1 somewhere); id 0 and every other id belong to no class."""
  ids = np.unique(EM.of_fields(eng.pack_bytes, _fields(eng, bank)))
  ids = ids[ids > 0]
  assert ids.size >= C
  table = np.full(eng.num_layer_ids, -1, np.int32)
  table[ids] = np.arange(ids.size) % C
  return table


PLAYERS = {"commons_harvest__open": 16}   # (the others: the level's default roles)


def _build(name, **kw):
  cfg = substrate.get_config(name)
  roles = ("default",) * PLAYERS[name] if name in PLAYERS else cfg.default_player_roles
  return substrate.build_from_config(cfg, roles=roles, num_worlds=N, env_seed=SEED, **kw)


def _actions(rng, eng, *shape):
  a = util.random_actions(rng, 1, int(np.prod(shape)), eng.P, eng.num_actions)
  return torch.from_numpy(a.reshape(shape + (eng.P,))).to(eng.device)


def _all_pairs(R, P, device):
  rows = torch.arange(R, dtype=torch.int32, device=device).repeat_interleave(P)
  players = torch.arange(P, dtype=torch.int32, device=device).repeat(R)
  return rows, players


def _both_kernels(eng, bank, want, classes, what, **kw):
  """k_ego_planes_rows over every row and k_ego_planes_views over every (row, player) of `bank`."""
  R, P = want.shape[:2]
  _same(eng.observe_ego_planes(classes, bank, **kw), want, (what, "rows"))
  rows, players = _all_pairs(R, P, eng.device)
  _same(eng.observe_ego_planes(classes, bank, rows=rows, players=players, **kw),
        want.reshape((R * P,) + want.shape[2:]), (what, "views"))


# ---- 1. live worlds, saved rows, the model and the host twin ---------------------------------------
@pytest.mark.parametrize("name", ["clean_up", "commons_harvest__open", KITCHEN, MATRIX])
def test_live_worlds_saved_rows_the_model_and_the_host_twin_agree(name):
  env = _build(name)
  eng = env.engine
  P = env.num_players
  assert P == {"clean_up": 7, "commons_harvest__open": 16}.get(name, 2)
  env.reset()
  rng = np.random.default_rng(SEED)
  res = env.step_many(_actions(rng, eng, 25, N), states=True)
  bank = res.states.data
  f = _fields(eng, bank)
  # the condition: every facing, and (clean_up: the level with a beam that removes) a dead viewer
  assert set(np.unique(f.orientation.cpu().numpy()[:, :P]).tolist()) == {0, 1, 2, 3}
  if name == "clean_up":
    assert bool((f.alive.cpu().numpy()[:, :P] == 0).any())
  if name == "clean_up":
    classes = env.layer_classes(CLEAN_UP_GROUPS)
    C = len(CLEAN_UP_GROUPS)
    assert classes[0] == -1 and classes[env.layer_id_names.index("OutOfView")] == -1
  else:
    C = 5
    classes = _occurring(eng, bank, C)
  assert classes.min() == -1 and classes.max() == C - 1
  want = _model(eng, bank, classes, facing=True)
  VH, VW = eng.ego_layer_shape[2:4]
  assert want.shape == (25 * N, P, C + 4, VH, VW)
  # every class plane and each of the four facing planes is 1 somewhere in the bank, and some byte is 0
  # (the matrix game's two players meet in these rows only face to face or back to back — the CPU
  # oracle's rows say so — so there the two sideways planes stay 0)
  lit = want.any(axis=(0, 1, 3, 4))
  assert lit[:C + 1].all() and (name == MATRIX or lit.all()), lit
  assert (want == 0).any() and set(np.unique(want).tolist()) == {0, 1}
  live = env.observe_ego_planes(classes, facing=True)
  assert live.dtype == torch.uint8 and tuple(live.shape) == (N, P, C + 4, VH, VW)
  _same(live, want[-N:], (name, "live worlds against the model"))
  _same(env.observe_ego_planes(classes, env.save_state(), facing=True), live, (name, "save_state"))
  _same(env.observe_ego_planes(classes, res.states, facing=True), want, (name, "every row, through the Substrate"))
  _both_kernels(eng, bank, want, classes, (name, "facing"), facing=True)
  host = E.ego_planes_host(eng.pack_bytes, bank.cpu().numpy(), classes, facing=True, fingerprint=eng.state_fingerprint)
  _same(host, want, (name, "the host twin"))
  # without facing: the class planes alone
  _both_kernels(eng, bank, np.ascontiguousarray(want[:, :, :C]), classes, (name, "no facing"))
  # layers by name and index, with a device table
  names = env.state_layout().layer_names
  L = len(names)
  dev_classes = torch.from_numpy(classes).to(eng.device)
  _same(env.observe_ego_planes(dev_classes, layers=[names[L - 1], 0], facing=True, num_classes=C),
        _model(eng, bank[-N:], classes, C, layers=[0, L - 1], facing=True), (name, "layers"))
  worlds, viewers = [5, 0, 0, 3, 2, 2, 1, 4], [0, 1, 1, 0, 1, P - 1, 0, 1]
  _same(env.observe_ego_planes(dev_classes, res.states, rows=worlds, players=viewers, layers=[0], num_classes=C),
        _model(eng, bank, classes, C, layers=[0])[worlds, viewers], (name, "layers, views"))
  # 64 classes: every bit of a cell's mask
  table64 = np.random.default_rng(SEED).integers(-1, 64, size=eng.num_layer_ids).astype(np.int32)
  _both_kernels(eng, bank[-2 * N:], _model(eng, bank[-2 * N:], table64, 64, facing=True), table64, (name, "C = 64"),
                facing=True, num_classes=64)
  eng.sync()
  util.no_faults(eng)
  env.close()


# ---- 2. geometry -----------------------------------------------------------------------------------
GEOMETRIES = [dict(name="clean_up", view=(0, 0, 0, 0)),
              dict(name="clean_up", view=(0, 7, 3, 0)),
              dict(name="coins", view=(3, 18, 1, 0)),
              dict(name="clean_up", topology="TORUS", open_edges=True, view=(5, 5, 21, 1)),
              dict(name="commons_harvest__open", topology="TORUS", open_edges=True)]


@pytest.mark.parametrize("variant", GEOMETRIES, ids=geometry.variant_id)
def test_edited_windows_and_tori(variant):
  assert variant in geometry.ACCEPTED
  eng = E.Engine(geometry.variant_pack(variant), N, device=0)
  eng.reset()
  A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 25, N, eng.P, eng.num_actions)).to(eng.device)
  banks = []
  for k in range(25):
    eng.step(A[k])
    if k % 6 == 0 or k == 24:
      banks.append(eng.save_worlds().clone())
  bank = torch.cat(banks)
  f = _fields(eng, bank)
  assert set(np.unique(f.orientation.cpu().numpy()).tolist()) == {0, 1, 2, 3}
  C = 3
  classes = _occurring(eng, bank, C)
  want = _model(eng, bank, classes, facing=True)
  H, W, _, view, torus = EM.geometry(eng.pack_bytes)
  VH, VW = view[2] + view[3] + 1, view[0] + view[1] + 1
  assert want.shape[2:] == (C + 4, VH, VW)
  if variant.get("view") == (0, 0, 0, 0):
    # a one-cell view: a block of C' bytes, every byte another plane; a living viewer sees itself
    assert (VH, VW) == (1, 1)
    alive = f.alive.cpu().numpy()[:, :eng.P].astype(bool)
    assert np.array_equal(want[:, :, C, 0, 0].astype(bool), alive)
  if variant.get("view") == (5, 5, 21, 1):
    # a window taller than the torus: a viewer that faces north or south sees ITSELF twice
    assert torus and VH > H
    ori, alive = f.orientation.cpu().numpy()[:, :eng.P], f.alive.cpu().numpy()[:, :eng.P].astype(bool)
    twice = alive & (ori % 2 == 0)
    assert twice.any()
    assert (want[:, :, C, view[2], view[0]][twice] == 1).all() and (want[:, :, C, view[2] - H, view[0]][twice] == 1).all()
  _both_kernels(eng, bank, want, classes, geometry.variant_id(variant), facing=True)
  _same(eng.observe_ego_planes(classes, facing=True), want[-N:], "live worlds")
  host = E.ego_planes_host(eng.pack_bytes, bank.cpu().numpy(), classes, facing=True, fingerprint=eng.state_fingerprint)
  _same(host, want, "the host twin")
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 3. destinations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", "commons_harvest__open"])
def test_repeated_rows_sampled_views_and_destinations_on_any_byte(name):
  env = _build(name)
  eng = env.engine
  P = env.num_players
  env.reset()
  rng = np.random.default_rng(SEED)
  for k in range(4):
    env.step(_actions(rng, eng, N))
  bank = env.save_state().data
  C = 3
  classes = _occurring(eng, bank, C)
  want = _model(eng, bank, classes, facing=True)
  view = int(np.prod(want.shape[2:]))
  assert view % 2 == 1   # (an odd view block: every second one starts, and ends, off a 16-byte line)
  count = 3 * N + 1   # R > N
  r = rng.integers(0, N, size=count).astype(np.int32)
  r[1] = r[0]
  p = rng.integers(0, P, size=count).astype(np.int32)
  p[1] = p[0]
  for src in (bank, None):   # rows of a bank; world indices of the live worlds
    every = eng.observe_ego_planes(classes, src, rows=r, facing=True)
    assert tuple(every.shape) == (count,) + want.shape[1:]
    _same(every, want[r], (name, "repeated rows"))
    views = eng.observe_ego_planes(classes, src, rows=r, players=p, facing=True)
    assert tuple(views.shape) == (count,) + want.shape[2:]
    _same(views, want[r, p], (name, "players= against the model"))
  for shift in (1, 3, 8, 16):
    n = count * P * view
    base = torch.full((n + shift + 37,), FILL, dtype=torch.uint8, device=eng.device)
    out = base[shift:shift + n].view((count,) + want.shape[1:])
    assert out.data_ptr() % 16 == (base.data_ptr() + shift) % 16
    assert eng.observe_ego_planes(classes, bank, rows=r, facing=True, out=out) is out
    _same(out, want[r], (name, "out", shift))
    got = base.cpu().numpy()
    assert (got[:shift] == FILL).all() and (got[shift + n:] == FILL).all()
    n = count * view
    base = torch.full((n + shift + 37,), FILL, dtype=torch.uint8, device=eng.device)
    out = base[shift:shift + n].view((count,) + want.shape[2:])
    eng.observe_ego_planes(classes, bank, rows=r, players=p, facing=True, out=out)
    _same(out, want[r, p], (name, "views out", shift))
    got = base.cpu().numpy()
    assert (got[:shift] == FILL).all() and (got[shift + n:] == FILL).all()
  eng.sync()
  util.no_faults(eng)
  env.close()


# ---- 4. bad indices ---------------------------------------------------------------------------------
def test_an_index_or_class_out_of_range_is_skipped_and_reported():
  eng = E.Engine(E.load_pack("clean_up"), N, device=0)
  eng.reset()
  bank = eng.save_worlds()
  C = 4
  classes = _occurring(eng, bank, C)
  want = _model(eng, bank, classes, facing=True)
  P = eng.P
  shape = want.shape[2:]
  out = torch.full((5, P) + shape, FILL, dtype=torch.uint8, device=eng.device)
  eng.observe_ego_planes(classes, bank, rows=[1, N, 0, -1, N + 40], facing=True, out=out)
  with pytest.raises(ValueError, match=r"MpEgoPlanes: rows\[(1\] = 6|3\] = -1|4\] = 46) is not a row"):
    eng.sync()
  got = out.cpu().numpy()
  assert np.array_equal(got[0], want[1]) and np.array_equal(got[2], want[0])
  assert (got[[1, 3, 4]] == FILL).all()
  out = torch.full((4,) + shape, FILL, dtype=torch.uint8, device=eng.device)
  eng.observe_ego_planes(classes, bank, rows=[2, 2, 5, 1], players=[0, P, 6, -1], facing=True, out=out)
  with pytest.raises(ValueError, match=rf"MpEgoPlanes: players\[(1\] = {P}|3\] = -1) is not a player"):
    eng.sync()
  got = out.cpu().numpy()
  assert np.array_equal(got[0], want[2, 0]) and np.array_equal(got[2], want[5, 6]) and (got[[1, 3]] == FILL).all()
  # the live worlds: a world index out of range
  out = torch.full((2, P) + shape, FILL, dtype=torch.uint8, device=eng.device)
  eng.observe_ego_planes(classes, None, rows=[N + 3, 4], facing=True, out=out)
  with pytest.raises(ValueError, match=r"MpEgoPlanes: rows\[0\] = 9"):
    eng.sync()
  got = out.cpu().numpy()
  assert (got[0] == FILL).all() and np.array_equal(got[1], want[4])
  # a DEVICE table with an entry >= C: the entry counts as -1, and is reported
  oob = int(np.flatnonzero(np.array(eng.layer_id_names) == "OutOfBounds")[0])
  assert oob == 1 and classes[oob] >= 0
  bad = classes.copy()
  bad[oob] = C
  got = eng.observe_ego_planes(torch.from_numpy(bad).to(eng.device), bank, facing=True, num_classes=C)
  with pytest.raises(ValueError, match=rf"MpEgoPlanes: classes\[1\] = {C} is outside \[-1, num_classes\)"):
    eng.sync()
  as_none = classes.copy()
  as_none[oob] = -1
  _same(got, _model(eng, bank, as_none, C, facing=True), "the entry counted as -1")
  # host-side refusals launch nothing, and the engine stays usable
  with pytest.raises(ValueError, match=rf"classes\[1\] = {C} is outside"):
    eng.observe_ego_planes(bad, bank, num_classes=C)
  with pytest.raises(ValueError, match="classes must be %d integers" % eng.num_layer_ids):
    eng.observe_ego_planes(classes[:-1], bank)
  for C_bad in (0, 65):
    with pytest.raises(ValueError, match=rf"num_classes {C_bad} is outside \[1, 64\]"):
      eng.observe_ego_planes(np.full(eng.num_layer_ids, -1, np.int32), bank, num_classes=C_bad)
  dev = torch.from_numpy(classes).to(eng.device)
  req = dict(fingerprint=eng.state_fingerprint, count=N, dst=got.data_ptr(), dst_bytes=got.numel(),
             classes=dev.data_ptr(), classes_len=eng.num_layer_ids, num_classes=C, facing=1)
  with pytest.raises(ValueError, match="NULL classes"):
    E.ego_planes_request(eng._L, eng._h, E.MP_EGOPLANES_DRAW, **dict(req, classes=None))
  with pytest.raises(ValueError, match=r"classes_len %d" % (eng.num_layer_ids - 1)):
    E.ego_planes_request(eng._L, eng._h, E.MP_EGOPLANES_DRAW, **dict(req, classes_len=eng.num_layer_ids - 1))
  with pytest.raises(ValueError, match=r"num_classes 65 is outside \[1, 64\]"):
    E.ego_planes_request(eng._L, eng._h, E.MP_EGOPLANES_DRAW, **dict(req, num_classes=65))
  with pytest.raises(ValueError, match=r"need %d bytes, dst has %d" % (got.numel(), got.numel() - 1)):
    E.ego_planes_request(eng._L, eng._h, E.MP_EGOPLANES_DRAW, **dict(req, dst_bytes=got.numel() - 1))
  with pytest.raises(ValueError, match="fingerprint"):
    eng.observe_ego_planes(classes, bank, fingerprint=1)
  with pytest.raises(ValueError, match="without a row list"):
    eng.observe_ego_planes(classes, bank[:2], players=[0, 0, 0])
  with pytest.raises(ValueError, match="device"):
    E.ego_planes_request(eng._L, eng._h, E.MP_EGOPLANES_REGISTER, **dict(req, dst=got.cpu().numpy().ctypes.data))
  with pytest.raises(ValueError, match="includes no layer"):
    eng.observe_ego_planes(classes, bank, layers=[])
  fresh = E.Engine(E.load_pack("clean_up"), 2, device=0)
  with pytest.raises(ValueError, match="never been reset"):
    fresh.observe_ego_planes(classes)
  fresh.close()
  eng.step(torch.zeros((N, P), dtype=torch.int32, device=eng.device))
  _same(eng.observe_ego_planes(classes, facing=True), _model(eng, eng.save_worlds(), classes, C, facing=True),
        "after the reports")
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 5. the registered tensor ------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 4])
def test_the_registered_tensor_follows_every_submission(T):
  kw = dict(rollout_length=T) if T else {}
  env, twin = _build("clean_up", **kw), _build("clean_up", **kw)
  eng = env.engine
  P = env.num_players
  names = env.state_layout().layer_names
  classes = env.layer_classes(CLEAN_UP_GROUPS)
  C = len(CLEAN_UP_GROUPS)
  fused = eng.fused
  reg = env.set_ego_planes(classes, facing=True)
  VH, VW = eng.ego_layer_shape[2:4]
  assert reg.dtype == torch.uint8 and tuple(reg.shape) == ((T,) if T else ()) + (N, P, C + 4, VH, VW)
  rng = np.random.default_rng(SEED)
  history = {}   # ring slot -> what it was given

  def check(what):
    want = _model(eng, env.save_state().data, classes, C, facing=True)
    _same(env.observe_ego_planes(classes, facing=True), want, (what, "observe_ego_planes"))
    if not T:
      _same(reg, want, (what, "registered"))
      return
    _same(reg[env.slot], want, (what, "the submission's slot"))
    history[env.slot] = want
    for s, kept in history.items():   # slots written earlier keep what they held
      _same(reg[s], kept, (what, "slot", s))

  env.reset(); twin.reset()
  check("reset")
  a = _actions(rng, eng, N)
  env.step(a); twin.step(a)
  check("step")
  if not T:
    a, mask = _actions(rng, eng, N), torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=eng.device)
    env.step(a, active=mask); twin.step(a, active=mask)
    check("masked step")
  a = _actions(rng, eng, 5, N)
  env.step_many(a); twin.step_many(a)
  check("step_many")
  if not T:
    stopped = [torch.zeros(N, dtype=torch.uint8, device=eng.device) for _ in range(2)]
    env.step_many(a, until=("last", "reward"), stopped=stopped[0])
    twin.step_many(a, until=("last", "reward"), stopped=stopped[1])
    check("step_many(until=)")
    worlds = [4, 0, 3]
    a = _actions(rng, eng, 3, len(worlds))
    env.step_many(a, worlds=worlds); twin.step_many(a, worlds=worlds)
    check("step_many(worlds=)")
  saved = env.save_state()
  a = _actions(rng, eng, N)
  env.step(a); twin.step(a)
  check("step")
  src = [2, -1, 0, 0, -1, 5]
  env.load_state(saved, src); twin.load_state(substrate.WorldStates(saved.data, twin.engine.state_fingerprint), src)
  check("load_state")
  # the twin without the registration ends on identical records and identical leaves
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  ours, theirs = env.observation(), twin.observation()
  assert set(ours) == set(theirs)
  for n in theirs:
    assert torch.equal(ours[n], theirs[n]), n
  # another table, without facing, replaces the registration
  if not T:
    other = torch.full((env.num_layer_ids,), -1, dtype=torch.int32, device=eng.device)
    other[1:] = 1
    reg2 = env.set_ego_planes(other, layers=[names[0], 2], num_classes=3)
    assert tuple(reg2.shape) == (N, P, 3, VH, VW)
    before = reg.clone()
    a = _actions(rng, eng, N)
    env.step(a); twin.step(a)
    _same(reg2, _model(eng, env.save_state().data, other, 3, layers=[0, 2]), "another table")
    assert not reg2[:, :, 0].any() and not reg2[:, :, 2].any() and reg2[:, :, 1].any()
    assert torch.equal(reg, before)   # (the first tensor is written no more)
    reg = reg2
  # clearing the registration: the tensor is written no more, the engine's launches are its own
  frozen = reg.clone()
  assert env.set_ego_planes(None) is None
  assert eng.fused == fused == twin.engine.fused
  a = _actions(rng, eng, N)
  env.step(a); twin.step(a)
  assert torch.equal(reg, frozen)
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  for e in (eng, twin.engine):
    e.sync()
    util.no_faults(e)
  env.close()
  twin.close()


def test_tune_does_not_write_the_registered_tensor():
  eng = E.Engine(E.load_pack("clean_up"), N, device=0)
  eng.bind(E.OBS_WORLD_RGB)
  classes = np.arange(eng.num_layer_ids, dtype=np.int32) % 7
  shape = eng.ego_planes_shape(7, True)
  # (a registered tensor that starts on an odd byte)
  base = torch.full((int(np.prod(shape)) + 1,), FILL, dtype=torch.uint8, device=eng.device)
  reg = eng.bind_ego_planes(base[1:].view(shape), classes, facing=True)
  eng.tune()
  assert bool((base == FILL).all())
  eng.reset()
  _same(reg, _model(eng, eng.save_worlds(), classes, 7, facing=True), "after the reset")
  assert int(base[0]) == FILL
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 6. mixture --------------------------------------------------------------------------------------
def test_a_mixture_of_two_kitchens_shares_one_tensor():
  names = [KITCHEN, "collaborative_cooking__ring"]
  for T in (0, 2):
    kw = dict(rollout_length=T) if T else {}
    mix = substrate.build_mixture(names, num_worlds=[3, 4], env_seed=SEED, **kw)
    P = mix.num_players
    first = mix._members[0]
    dev = first.engine.device
    classes = mix.layer_classes(KITCHEN_GROUPS)
    C = len(KITCHEN_GROUPS)
    assert len(classes) == 2 and not np.array_equal(classes[0], classes[1])
    VH, VW = first.engine.ego_layer_shape[2:4]
    reg = mix.set_ego_planes(classes, facing=True)
    assert tuple(reg.shape) == ((T,) if T else ()) + (7, P, C + 4, VH, VW) and reg.dtype == torch.uint8
    mix.reset()
    A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 5, 7, P, mix.action_spec()[0].num_values)).to(dev)
    for k in range(5):
      mix.step(A[k])
    whole = mix.observe_ego_planes(classes, facing=True)
    assert tuple(whole.shape) == (7, P, C + 4, VH, VW)
    now = reg[mix.slot] if T else reg
    _same(now, whole, (T, "registered"))
    for i, m in enumerate(mix._members):
      sl = mix.member_slice(i)
      own = m.observe_ego_planes(classes[i], facing=True)
      _same(whole[sl], own, (T, i, "the member's own call"))
      _same(own, _model(m.engine, m.save_state().data, classes[i], C, facing=True), (T, i, "model"))
      m.engine.sync()
      util.no_faults(m.engine)
    # one table for every member is taken as it is
    shared = mix.observe_ego_planes(classes[0], num_classes=C)
    _same(shared[mix.member_slice(1)], mix._members[1].observe_ego_planes(classes[0], num_classes=C), (T, "one table"))
    assert mix.set_ego_planes(None) is None
    mix.close()
