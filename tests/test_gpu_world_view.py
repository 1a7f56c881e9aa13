"""WORLD.LAYER and the world planes on the GPU (the world ops of MpEgoLayer and MpEgoPlanes;
Engine.observe_world_layer / observe_world_planes / bind_*, Substrate's leaf "WORLD.LAYER",
observe_world_layer, observe_world_planes, set_world_planes): both kernels against the numpy model
of tests/world_view_model.py and the library's host twins, WORLD.LAYER against the pixels of
"WORLD.RGB", edited map geometries, destinations that start on any byte, indices out of range, the
leaf and the registered planes behind every kind of submission with and without a rollout ring,
saved states and mixtures.  Every comparison is exact equality."""
import numpy as np
import pytest
import torch

import geometry
import util
import world_view_model as WM
from meltingpot_amd import engine, substrate
from meltingpot_amd import pack as pack_lib

pytestmark = pytest.mark.gpu

E = engine
N = 6
SEED = 5
KITCHEN = "collaborative_cooking__cramped"
MATRIX = "prisoners_dilemma_in_the_matrix__repeated"
COMMONS = "commons_harvest__open"
PLAYERS = {COMMONS: 16}   # (the others: the level's default roles)
FILL = 0xA5
C = 4


def _same(got, want, what):
  got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
  want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
  assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def _fields(eng, bank):
  layout = substrate.SubstrateStateLayout(eng.state_layout(), pack_lib.loads(eng.pack_bytes))
  return substrate.StateFields(bank, layout)


def _layer(eng, bank):
  return WM.layer_of_fields(eng.pack_bytes, _fields(eng, bank), eng.P)


def _planes(eng, bank, classes, num_classes=None, layers=None, facing=False):
  classes = classes.cpu().numpy() if isinstance(classes, torch.Tensor) else classes
  return WM.planes_of_fields(eng.pack_bytes, _fields(eng, bank), eng.P, classes, num_classes, layers, facing)


def _occurring(eng, bank, classes=C):
  """A table from the MODEL's view of the rows: the ids that occur on some cell but not on every
  cell of every row, dealt to `classes` classes in turn; id 0 and every other id belong to none."""
  wl = _layer(eng, bank)
  ids = [i for i in np.unique(wl) if i > 0 and not (wl == i).any(-1).all()]
  assert len(ids) >= classes
  table = np.full(eng.num_world_layer_ids, -1, np.int32)
  table[ids] = np.arange(len(ids)) % classes
  return table


def _config(name, world_rgb=True):
  cfg = substrate.get_config(name)
  cfg.global_observation_names = (["WORLD.RGB"] if world_rgb else []) + ["WORLD.LAYER"]
  return cfg


def _build(name, leaf=False, **kw):
  cfg = _config(name) if leaf else substrate.get_config(name)
  roles = ("default",) * PLAYERS[name] if name in PLAYERS else cfg.default_player_roles
  return substrate.build_from_config(cfg, roles=roles, num_worlds=N, env_seed=SEED, **kw)


def _actions(rng, eng, *shape):
  a = util.random_actions(rng, 1, int(np.prod(shape)), eng.P, eng.num_actions)
  return torch.from_numpy(a.reshape(shape + (eng.P,))).to(eng.device)


# ---- 4. live worlds, saved rows, the model and the host twins ------------------------------------
@pytest.mark.parametrize("name", ["clean_up", COMMONS, KITCHEN, MATRIX])
def test_live_worlds_saved_rows_the_model_and_the_host_twins_agree(name):
  env = _build(name)
  eng = env.engine
  P = env.num_players
  assert P == {"clean_up": 7, COMMONS: 16}.get(name, 2)
  env.reset()
  res = env.step_many(_actions(np.random.default_rng(SEED), eng, 25, N), states=True)
  bank = res.states.data
  H, W, L = WM.geometry(eng.pack_bytes)
  assert eng.num_world_layer_ids == WM.num_ids(eng.pack_bytes, P) == env.num_world_layer_ids
  assert len(env.world_layer_id_names) == env.num_world_layer_ids and env.world_layer_id_names[1] == "OutOfBounds"
  # WORLD.LAYER
  want = _layer(eng, bank)
  assert want.shape == (25 * N, H, W, L)
  live = env.observe_world_layer()
  assert live.dtype == torch.int32 and tuple(live.shape) == (N, H, W, L)
  _same(live, want[-N:], (name, "live worlds against the model"))
  _same(env.observe_world_layer(env.save_state()), live, (name, "save_state"))
  _same(env.observe_world_layer(res.states), want, (name, "every row"))
  _same(E.world_layer_host(eng.pack_bytes, bank.cpu().numpy(), fingerprint=eng.state_fingerprint), want,
        (name, "the host twin"))
  rows = [5, 0, 0, 3, 149, 2, 2, 1]
  _same(env.observe_world_layer(res.states, rows=rows), want[rows], (name, "rows"))
  # the planes, with and without facing, with a choice of layers
  classes = _occurring(eng, bank)
  assert classes.min() == -1 and classes.max() == C - 1
  full = _planes(eng, bank, classes, facing=True)
  assert full.shape == (25 * N, C + 4, H, W) and set(np.unique(full).tolist()) == {0, 1}
  assert full[:, :C].any(axis=(0, 2, 3)).all() and (full == 0).any(axis=(0, 2, 3)).all()
  lit = env.observe_world_planes(classes, facing=True)
  assert lit.dtype == torch.uint8 and tuple(lit.shape) == (N, C + 4, H, W)
  _same(lit, full[-N:], (name, "live planes against the model"))
  _same(env.observe_world_planes(classes, res.states, facing=True), full, (name, "planes, every row"))
  _same(env.observe_world_planes(classes, res.states), np.ascontiguousarray(full[:, :C]), (name, "no facing"))
  _same(E.world_planes_host(eng.pack_bytes, bank.cpu().numpy(), classes, facing=True,
                            fingerprint=eng.state_fingerprint), full, (name, "the planes' host twin"))
  names = env.state_layout().layer_names
  dev_classes = torch.from_numpy(classes).to(eng.device)
  _same(env.observe_world_planes(dev_classes, res.states, rows=rows, layers=[names[L - 1], 0], facing=True, num_classes=C),
        _planes(eng, bank, classes, C, layers=[0, L - 1], facing=True)[rows], (name, "layers"))
  table64 = np.random.default_rng(SEED).integers(-1, 64, size=eng.num_world_layer_ids).astype(np.int32)
  _same(env.observe_world_planes(table64, res.states, facing=True, num_classes=64),
        _planes(eng, bank, table64, 64, facing=True), (name, "C = 64"))
  # 32 classes are the last that fit a u32 mask, 33 the first that take the u64 kernel
  for Cn in (32, 33):
    table = np.random.default_rng(Cn).integers(-1, Cn, size=eng.num_world_layer_ids).astype(np.int32)
    table[1:3] = (Cn - 1, Cn - 2)   # (the highest bits are in use)
    _same(env.observe_world_planes(table, res.states, rows=rows, facing=True, num_classes=Cn),
          _planes(eng, bank, table, Cn, facing=True)[rows], (name, "C =", Cn))
  eng.sync()
  util.no_faults(eng)
  env.close()


# ---- 5. pixels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean_up", MATRIX])
def test_equal_cells_of_world_layer_are_equal_blocks_of_world_rgb(name):
  env = _build(name, leaf=True)
  eng = env.engine
  P = env.num_players
  H, W, L = WM.geometry(eng.pack_bytes)
  ts = env.reset()
  S = ts.observation["WORLD.RGB"].shape[1] // H
  assert tuple(ts.observation["WORLD.RGB"].shape) == (N, H * S, W * S, 3)
  rng = np.random.default_rng(SEED)
  repeated = set()
  for k in range(10):
    ts = env.step(_actions(rng, eng, N))
    layer = ts.observation["WORLD.LAYER"].cpu().numpy()
    rgb = ts.observation["WORLD.RGB"].cpu().numpy()
    f = _fields(eng, env.save_state().data)
    ax, ay = f.avatar_x.cpu().numpy()[:, :P], f.avatar_y.cpu().numpy()[:, :P]
    ori, alive = f.orientation.cpu().numpy()[:, :P], f.alive.cpu().numpy()[:, :P]
    for w in range(N):
      facing = np.full((H, W), -1, np.int64)
      for p in range(P):
        if alive[w, p]:
          facing[ay[w, p], ax[w, p]] = ori[w, p]
      blocks = rgb[w].reshape(H, S, W, S, 3).transpose(0, 2, 1, 3, 4).reshape(H * W, -1)
      keys = np.concatenate([layer[w].reshape(H * W, L), facing.reshape(H * W, 1)], axis=1)
      seen = {}
      for cell in range(H * W):
        key = tuple(keys[cell].tolist())
        if key in seen:
          assert np.array_equal(blocks[cell], blocks[seen[key]]), (k, w, cell, seen[key], key)
          repeated.add(key)
        else:
          seen[key] = cell
  assert len(repeated) >= 2
  eng.sync()
  util.no_faults(eng)
  env.close()


# ---- 6. edited geometries ----------------------------------------------------------------------------
GEOMETRIES = [dict(name=KITCHEN, width=17),              # 85 cells: H * W and L * H * W no multiples of 16
              dict(name="clean_up", width=63),           # 1323 cells: more than one run of 1024, neither a multiple of 16
              dict(name="territory__rooms", width=33),   # 11 layers
              dict(name="clean_up", width=64, height=64)]   # 4096 cells: two waves a workgroup


@pytest.mark.parametrize("variant", GEOMETRIES, ids=geometry.variant_id)
def test_edited_maps_destinations_on_any_byte_and_bad_rows(variant):
  assert variant in geometry.ACCEPTED
  eng = E.Engine(geometry.variant_pack(variant), N, device=0)
  eng.reset()
  A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 8, N, eng.P, eng.num_actions)).to(eng.device)
  for k in range(8):
    eng.step(A[k])
  bank = eng.save_worlds().clone()
  H, W, L = WM.geometry(eng.pack_bytes)
  if "height" not in variant:
    assert (H * W) % 16 and (L * H * W) % 16
  else:
    assert H * W > 1024
  classes = _occurring(eng, bank, 3)
  want_layer = _layer(eng, bank)
  want = _planes(eng, bank, classes, facing=True)
  count = 2 * N + 1   # count > N, rows with repeats
  r = np.random.default_rng(SEED).integers(0, N, size=count).astype(np.int32)
  r[1] = r[0]
  for src in (bank, None):   # rows of a bank; world indices of the live worlds
    _same(eng.observe_world_layer(src, rows=r), want_layer[r], ("layer", src is None))
    _same(eng.observe_world_planes(classes, src, rows=r, facing=True), want[r], ("planes", src is None))
  # WORLD.LAYER into elements that start 4, 8 and 12 bytes off a 16-byte line
  for shift in (1, 2, 3):
    n = count * H * W * L
    base = torch.full((n + shift + 9,), -7, dtype=torch.int32, device=eng.device)
    out = base[shift:shift + n].view(count, H, W, L)
    assert eng.observe_world_layer(bank, rows=r, out=out) is out
    _same(out, want_layer[r], ("layer out", shift))
    got = base.cpu().numpy()
    assert (got[:shift] == -7).all() and (got[shift + n:] == -7).all()
  # the planes on an odd byte: no byte outside the blocks is touched
  view = int(np.prod(want.shape[1:]))
  for shift in (1, 3, 8, 15):
    n = count * view
    base = torch.full((n + shift + 37,), FILL, dtype=torch.uint8, device=eng.device)
    out = base[shift:shift + n].view((count,) + want.shape[1:])
    assert eng.observe_world_planes(classes, bank, rows=r, facing=True, out=out) is out
    _same(out, want[r], ("planes out", shift))
    got = base.cpu().numpy()
    assert (got[:shift] == FILL).all() and (got[shift + n:] == FILL).all()
  _same(E.world_planes_host(eng.pack_bytes, bank.cpu().numpy(), classes, facing=True, fingerprint=eng.state_fingerprint),
        want, "the host twin")
  eng.sync()
  util.no_faults(eng)
  # a row index out of range: its element stays as it was, the next synchronising call names it
  out = torch.full((4,) + want.shape[1:], FILL, dtype=torch.uint8, device=eng.device)
  eng.observe_world_planes(classes, bank, rows=[1, N, 0, -1], facing=True, out=out)
  with pytest.raises(ValueError, match=r"MpEgoPlanes \(MP_EGOPLANES_WORLD_DRAW\): rows\[(1\] = 6|3\] = -1) is not a row"):
    eng.sync()
  got = out.cpu().numpy()
  assert np.array_equal(got[0], want[1]) and np.array_equal(got[2], want[0]) and (got[[1, 3]] == FILL).all()
  out = torch.full((3, H, W, L), -7, dtype=torch.int32, device=eng.device)
  eng.observe_world_layer(None, rows=[N + 3, 4, 2], out=out)
  with pytest.raises(ValueError, match=r"MpEgoLayer \(MP_EGO_WORLD_DRAW\): rows\[0\] = 9 is not a row"):
    eng.sync()
  got = out.cpu().numpy()
  assert (got[0] == -7).all() and np.array_equal(got[1:], want_layer[[4, 2]])
  # a DEVICE table with an entry >= C counts as -1 and is reported
  used = int(np.flatnonzero(classes >= 0)[0])
  bad = classes.copy()
  bad[used] = 3
  got = eng.observe_world_planes(torch.from_numpy(bad).to(eng.device), bank, facing=True, num_classes=3)
  with pytest.raises(ValueError, match=rf"MP_EGOPLANES_WORLD_DRAW\): classes\[{used}\] = 3 is outside \[-1, num_classes\)"):
    eng.sync()
  as_none = classes.copy()
  as_none[used] = -1
  _same(got, _planes(eng, bank, as_none, 3, facing=True), "the entry counted as -1")
  # refusals before a launch, and the engine works afterwards
  with pytest.raises(ValueError, match="the world ops take no players"):
    E.ego_layer_request(eng._L, eng._h, E.MP_EGO_WORLD_DRAW, fingerprint=eng.state_fingerprint, count=N,
                        players=torch.zeros(N, dtype=torch.int32, device=eng.device).data_ptr(),
                        dst=out.data_ptr(), dst_bytes=out.numel() * 4)
  with pytest.raises(ValueError, match="classes must be %d integers" % eng.num_world_layer_ids):
    eng.observe_world_planes(classes[:-1], bank)
  eng.step(A[0])
  _same(eng.observe_world_layer(), _layer(eng, eng.save_worlds()), "after the reports")
  _same(eng.observe_world_planes(classes, facing=True), _planes(eng, eng.save_worlds(), classes, 3, facing=True),
        "after the reports")
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 7. the leaf and the registered planes -----------------------------------------------------------
@pytest.mark.parametrize("T", [0, 3])
def test_the_leaf_and_the_registered_planes_follow_every_submission(T):
  kw = dict(rollout_length=T) if T else {}
  env, twin = _build("clean_up", leaf=True, **kw), _build("clean_up", **kw)
  eng = env.engine
  P = env.num_players
  H, W, L = WM.geometry(eng.pack_bytes)
  spec = env.observation_spec()[0]["WORLD.LAYER"]
  assert spec.shape == (H, W, L) and spec.dtype == np.int32
  assert "WORLD.LAYER" in env.state_leaves() and "WORLD.LAYER" not in twin.state_leaves()
  # the leaf sits where "WORLD.RGB" sits: behind it among the global leaves, in the spec and in a timestep
  for keys in (list(env.observation_spec()[0]), list(env.observation())):
    assert keys.index("WORLD.LAYER") == keys.index("WORLD.RGB") + 1 == keys.index("COLLECTIVE_REWARD") - 1, keys
  groups = ["Avatar*", "Beam*", "Wall", "water_*", ("Apple", "Grass"), "Dirt"]
  classes = env.world_layer_classes(groups)
  Cg = len(groups)
  assert classes.shape == (env.num_world_layer_ids,) and classes[0] == -1 and classes.max() == Cg - 1
  fused = eng.fused
  reg = env.set_world_planes(classes, facing=True)
  assert reg.dtype == torch.uint8 and tuple(reg.shape) == ((T,) if T else ()) + (N, Cg + 4, H, W)
  rng = np.random.default_rng(SEED)
  history = {}   # ring slot -> (the leaf, the planes) it was given

  def check(ts, what):
    leaf = ts.observation["WORLD.LAYER"]
    assert tuple(leaf.shape) == (N, H, W, L) and leaf.dtype == torch.int32
    bank = env.save_state().data
    want, planes = _layer(eng, bank), _planes(eng, bank, classes, Cg, facing=True)
    _same(leaf, want, (what, "the leaf against the model"))
    _same(leaf, env.observe_world_layer(), (what, "observe_world_layer"))
    _same(env.observe_world_planes(classes, facing=True), planes, (what, "observe_world_planes"))
    if not T:
      _same(reg, planes, (what, "registered"))
      return
    assert ts.slot == env.slot
    _same(env.rollout["observation"]["WORLD.LAYER"][ts.slot], want, (what, "ring slot"))
    _same(reg[ts.slot], planes, (what, "the planes' slot"))
    history[ts.slot] = (want, planes)
    for s, (l, p) in history.items():   # slots written earlier keep what they held
      _same(env.rollout["observation"]["WORLD.LAYER"][s], l, (what, "slot", s))
      _same(reg[s], p, (what, "planes slot", s))

  check(env.reset(), "reset"); twin.reset()
  a = _actions(rng, eng, N)
  check(env.step(a), "step"); twin.step(a)
  # (a masked step cannot write a rollout ring — a slot row of a skipped world has no defined
  # content — and the substrate refuses it: the leaf and the planes follow one where it is legal)
  if T:
    with pytest.raises(ValueError, match="a masked step cannot write a rollout ring"):
      env.step(_actions(np.random.default_rng(0), eng, N), active=torch.ones(N, dtype=torch.uint8, device=eng.device))
  if not T:
    a, mask = _actions(rng, eng, N), torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=eng.device)
    check(env.step(a, active=mask), "masked step"); twin.step(a, active=mask)
  a = _actions(rng, eng, 5, N)
  check(env.step_many(a).timestep, "step_many"); twin.step_many(a)
  saved = env.save_state()
  a = _actions(rng, eng, N)
  check(env.step(a), "step"); twin.step(a)
  src = [2, -1, 0, 0, -1, 5]
  check(env.load_state(saved, src), "load_state")
  twin.load_state(substrate.WorldStates(saved.data, twin.engine.state_fingerprint), src)
  with pytest.raises(ValueError, match=r"WORLD\.LAYER.*states=True.*observe_states"):
    env.step_many(_actions(rng, eng, 2, N), observations=("WORLD.LAYER",))
  # the twin without the leaf and the planes ends on identical records and identical other leaves
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  ours, theirs = env.observation(), twin.observation()
  assert set(ours) == set(theirs) | {"WORLD.LAYER"}
  for n in theirs:
    assert torch.equal(ours[n], theirs[n]), n
  # clearing the registrations: neither is written any more, the engine's launches are its own
  leaf = env.rollout["observation"]["WORLD.LAYER"] if T else env.observation()["WORLD.LAYER"]
  frozen = (leaf.clone(), reg.clone())
  assert env.set_world_planes(None) is None
  eng.bind_world_layer(None)
  assert eng.fused == fused == twin.engine.fused
  a = _actions(rng, eng, N)
  env.step(a); twin.step(a)
  assert torch.equal(leaf, frozen[0]) and torch.equal(reg, frozen[1])
  assert torch.equal(eng.save_worlds(), twin.engine.save_worlds())
  for e in (eng, twin.engine):
    e.sync()
    util.no_faults(e)
  env.close()
  twin.close()


def test_tune_writes_neither_the_leaf_nor_the_planes():
  eng = E.Engine(E.load_pack("clean_up"), N, device=0)
  eng.bind(E.OBS_WORLD_RGB)
  leaf = eng.bind_world_layer(torch.full(eng.world_layer_shape, -7, dtype=torch.int32, device=eng.device))
  classes = np.arange(eng.num_world_layer_ids, dtype=np.int32) % 7
  shape = eng.world_planes_shape(7, True)
  base = torch.full((int(np.prod(shape)) + 1,), FILL, dtype=torch.uint8, device=eng.device)   # (on an odd byte)
  reg = eng.bind_world_planes(base[1:].view(shape), classes, facing=True)
  eng.tune()
  assert bool((leaf == -7).all()) and bool((base == FILL).all())
  eng.reset()
  _same(leaf, _layer(eng, eng.save_worlds()), "the leaf after the reset")
  _same(reg, _planes(eng, eng.save_worlds(), classes, 7, facing=True), "the planes after the reset")
  assert int(base[0]) == FILL
  eng.sync()
  util.no_faults(eng)
  eng.close()


# ---- 8. saved states and mixtures --------------------------------------------------------------------
def test_saved_states_and_refusals():
  env = _build("clean_up", leaf=True)
  env.reset()
  res = env.step_many(_actions(np.random.default_rng(SEED), env.engine, 4, N), states=True)
  rows = [7, 7, 0, 23, 5]
  drawn = env.observe_states(res.states, ("WORLD.LAYER",), rows=rows)
  assert set(drawn) == {"WORLD.LAYER"}
  _same(drawn["WORLD.LAYER"], env.observe_world_layer(res.states, rows=rows), "observe_states")
  _same(env.observe_states(res.states, ("WORLD.LAYER",))["WORLD.LAYER"], _layer(env.engine, res.states.data), "every row")
  assert "WORLD.LAYER" in env.observe_states(res.states)   # (a leaf of this substrate: in the default set)
  with pytest.raises(ValueError, match=r"WORLD\.LAYER.*not per player"):
    env.observe_states(res.states, ("WORLD.LAYER",), rows=rows, players=[0] * len(rows))
  with pytest.raises(ValueError, match="observe_world_layer takes the WorldStates"):
    env.observe_world_layer(res.states.data)
  env.engine.sync()
  util.no_faults(env.engine)
  env.close()
  # build_substrate names it among the global observations
  cfg = substrate.get_config("clean_up")
  env = substrate.build_substrate(lab2d_settings=geometry.settings("clean_up"), individual_observations=["RGB"],
                                  global_observations=["WORLD.RGB", "WORLD.LAYER"], action_table=cfg.action_set,
                                  num_worlds=N, env_seed=SEED)
  ts = env.reset()
  _same(ts.observation["WORLD.LAYER"], _layer(env.engine, env.save_state().data), "build_substrate")
  env.close()
  # a one-world substrate refuses all of it
  with pytest.raises(ValueError, match=r"WORLD\.LAYER.*needs a batched substrate"):
    substrate.build_from_config(_config("clean_up"), roles=cfg.default_player_roles)
  one = substrate.build_from_config(cfg, roles=cfg.default_player_roles)
  try:
    for call in (lambda: one.observe_world_layer(), lambda: one.observe_world_planes(np.zeros(3, np.int32)),
                 lambda: one.set_world_planes(np.zeros(3, np.int32))):
      with pytest.raises(ValueError, match="needs a batched substrate"):
        call()
  finally:
    one.close()


def test_mixtures_share_the_leaf_or_are_refused():
  names = [KITCHEN, "collaborative_cooking__ring"]
  for T in (0, 2):
    kw = dict(rollout_length=T) if T else {}
    mix = substrate.build_mixture(names, num_worlds=[3, 4], env_seed=SEED, global_observations=["WORLD.LAYER"], **kw)
    P = mix.num_players
    dev = mix._members[0].engine.device
    ts = mix.reset()
    A = torch.from_numpy(util.random_actions(np.random.default_rng(SEED), 5, 7, P, mix.action_spec()[0].num_values)).to(dev)
    for k in range(5):
      ts = mix.step(A[k])
    leaf = ts.observation["WORLD.LAYER"]
    H, W, L = WM.geometry(mix._members[0].engine.pack_bytes)
    assert tuple(leaf.shape) == (7, H, W, L) and leaf.dtype == torch.int32
    if T:
      _same(mix.rollout["observation"]["WORLD.LAYER"][mix.slot], leaf, (T, "the ring's slot"))
    for i, m in enumerate(mix._members):
      _same(leaf[mix.member_slice(i)], _layer(m.engine, m.save_state().data), (T, i, "model"))
      _same(leaf[mix.member_slice(i)], m.observe_world_layer(), (T, i, "the member's own call"))
      m.engine.sync()
      util.no_faults(m.engine)
    mix.close()
  # members whose maps differ: (21, 21, 11) and (23, 39, 11)
  with pytest.raises(ValueError, match=r"leaf 'WORLD\.LAYER' differs: territory__rooms \(21, 21, 11\) int32, "
                     r"territory__open \(23, 39, 11\) int32"):
    substrate.build_mixture(["territory__rooms", "territory__open"], num_worlds=[2, 2], env_seed=SEED,
                            individual_observations=["READY_TO_SHOOT"], global_observations=["WORLD.LAYER"])
