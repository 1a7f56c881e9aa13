"""Sampled (state, player) views of saved world states (MpStatesView, Engine.observe_views,
Substrate.observe_states(players=...)): element i is ONE player's view of ONE row of a bank.  Every
result is compared byte for byte — with what the step launches that wrote the rows left in the bound
leaves, with `pool_rgb` of the full views, with MpStatesObserve of the same rows and with the CPU
oracle on edited geometries — for samples with repeats, ragged last workgroups, views that start on
odd bytes, rows with dead avatars.  The engine that draws is left exactly as it was, every refusal
happens on the host, and an index that is no row or no player leaves its element alone."""
import ctypes

import numpy as np
import pytest
import torch

import geometry
import states_recipe as recipe
import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

E = engine
N = recipe.N
R_ALL = N * len(recipe.SAVE_AT)   # 25 rows


def _same(got, want, what):
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
  assert torch.equal(got, want), (what, (got != want).nonzero()[:4].tolist())


def _same_leaf(kind, got, want, what):
  if kind != E.OBS_EVENTS:
    return _same(got, want, what)
  for a, b in zip(got.cpu().numpy(), want.cpu().numpy()):
    n = int(a[0, 0])
    assert tuple(a[0]) == tuple(b[0]) and sorted(map(tuple, a[1:1 + n].tolist())) == sorted(map(tuple, b[1:1 + n].tolist())), what


def _player_kinds(road):
  return tuple(k for k in road["kinds"] if k != E.OBS_WORLD_RGB)


def _dead_pairs(name, road):
  """(row, player) of every dead avatar of the 25 rows, read from the rows' own bytes."""
  lay = E.state_layout(recipe.pack(name))
  off = lay.grid_pad + lay.fields["aalive"][0]
  alive = road["all"][:, off:off + lay.P].cpu().numpy()
  return [(int(r), int(p)) for r, p in zip(*np.nonzero(alive == 0))]


def _samples(name, road, P):
  """count -> (rows, players), seeded, with repeats; where the level has rows with a dead avatar,
  one sample of the larger counts is such a (row, player)."""
  rng = np.random.default_rng(23)
  dead = _dead_pairs(name, road) if name in recipe.DEAD_AVATARS else []
  out = {}
  for count in (1, 5, 37):
    rows, players = rng.integers(0, R_ALL, size=count), rng.integers(0, P, size=count)
    if dead and count > 1:
      rows[count // 2], players[count // 2] = dead[int(rng.integers(0, len(dead)))]
    out[count] = (rows.astype(np.int64), players.astype(np.int64))
  return out, dead


# 1. against the launches that wrote the rows
@pytest.mark.parametrize("name", recipe.PACKS)
def test_sampled_views_are_what_the_step_launches_drew(name):
  road = recipe.road(name)
  e = engine.Engine(recipe.pack(name), N, device=0)   # never reset: the rows are another engine's
  assert e.state_fingerprint == road["fingerprint"]
  P = e.P
  samples, dead = _samples(name, road, P)
  if name in recipe.DEAD_AVATARS:
    assert dead and any((int(r), int(p)) in dead for c in (5, 37) for r, p in zip(*samples[c]))
  for kind in _player_kinds(road):
    full = road["all_views"][kind]
    for count, (rows, players) in samples.items():
      got = e.observe_views(road["all"], kind, players, rows)
      assert got.shape[0] == count
      _same(got, full[torch.from_numpy(rows).to(e.device), torch.from_numpy(players).to(e.device)],
            (name, kind, count))
    # every player of one row in one call: the row's full leaf
    _same(e.observe_views(road["all"], kind, list(range(P)), [13] * P), full[13], (name, kind, "one row"))
    # rows=None: rows 0 .. count - 1
    players = samples[5][1]
    _same(e.observe_views(road["all"], kind, players), full[torch.arange(5), torch.from_numpy(players)],
          (name, kind, "rows=None"))
    _same(e.observe_views(road["all"], kind, [P - 1] * R_ALL), full[:, P - 1], (name, kind, "rows=None, 25"))
  e.sync()
  util.no_faults(e)
  e.close()


# 2. the pooled kinds, and views that start on odd bytes
@pytest.mark.parametrize("name", ["clean_up", "collaborative_cooking__cramped"])
def test_pooled_views_equal_pool_rgb_of_the_full_views(name):
  road = recipe.road(name)
  e = engine.Engine(recipe.pack(name), N, device=0)
  full = road["all_views"][E.OBS_RGB].cpu().numpy()
  samples, _ = _samples(name, road, e.P)
  for k, kind in E.OBS_RGB_POOL.items():
    for count, (rows, players) in samples.items():
      want = engine.pool_rgb(full[rows, players], k)
      got = e.observe_views(road["all"], kind, players, rows)
      assert np.array_equal(got.cpu().numpy(), want), (name, k, count)
      for at in (1, 13):
        buf = torch.full((want.size + 32,), 0xAB, dtype=torch.uint8, device=e.device)
        out = buf[at:at + want.size].view(want.shape)
        assert e.observe_views(road["all"], kind, players, rows, out=out) is out
        host = buf.cpu().numpy()
        assert np.array_equal(host[at:at + want.size].reshape(want.shape), want), (name, k, count, at)
        assert (host[:at] == 0xAB).all() and (host[at + want.size:] == 0xAB).all(), (name, k, count, at)
  # the full view on odd bytes as well
  rows, players = samples[5]
  want = full[rows, players]
  for at in (1, 13):
    buf = torch.full((want.size + 32,), 0xAB, dtype=torch.uint8, device=e.device)
    e.observe_views(road["all"], E.OBS_RGB, players, rows, out=buf[at:at + want.size].view(want.shape))
    host = buf.cpu().numpy()
    assert np.array_equal(host[at:at + want.size].reshape(want.shape), want), (name, at)
    assert (host[:at] == 0xAB).all() and (host[at + want.size:] == 0xAB).all(), (name, at)
  e.sync()
  util.no_faults(e)
  e.close()


# 3. edited geometries: against MpStatesObserve of the same rows and straight against the oracle
GEOMETRIES = [
    dict(name="clean_up", view=(0, 0, 0, 0)),
    dict(name="clean_up", view=(3, 0, 0, 4)),
    dict(name="collaborative_cooking__cramped", view=(0, 63, 0, 0)),
    dict(name="clean_up", view=(31, 32, 32, 31)),
    dict(name="clean_up", width=64, height=64),
    dict(name="clean_up", topology="TORUS", open_edges=True, height=30, view=(30, 0, 9, 1)),
    dict(name="coins", topology="TORUS", open_edges=True, view=(5, 17, 9, 1)),
]


@pytest.mark.parametrize("v", GEOMETRIES, ids=[geometry.variant_id(v) for v in GEOMETRIES])
def test_geometries_against_observe_states_and_the_oracle(v):
  assert v in geometry.ACCEPTED
  blob = geometry.variant_pack(v)
  n, steps = 3, 6
  e = engine.Engine(blob, n, device=0)
  P = e.P
  rng = np.random.default_rng(5)
  acts = util.random_actions(rng, steps, n, P, e.num_actions)
  e.reset()
  for s in range(steps):
    e.step(torch.from_numpy(acts[s]).to(e.device))
  bank = e.save_worlds()
  big = v.get("view") == (31, 32, 32, 31)
  count = 3 if big else 11
  rows = rng.integers(0, n, size=count)
  players = rng.integers(0, P, size=count)
  rows[:2], players[:2] = (0, 1), (0, P - 1)   # (both oracle worlds are among the samples)
  got = {}
  for kind in (E.OBS_RGB, E.OBS_RGB_POOL8, E.OBS_LAYER):
    whole = e.observe_states(bank, kind, rows=rows)
    got[kind] = e.observe_views(bank, kind, players, rows)
    _same(got[kind], whole[torch.arange(count), torch.from_numpy(players)], (v, kind))
  e.sync()
  util.no_faults(e)
  oracles = util.make_oracles(blob, 2)
  try:
    for w, o in enumerate(oracles):
      o.reset()
      for s in range(steps):
        o.step(acts[s, w])
    for i in range(count):
      if rows[i] >= 2:
        continue
      o, p = oracles[rows[i]], int(players[i])
      rgb = o.render_agent(p)
      assert np.array_equal(got[E.OBS_RGB][i].cpu().numpy(), rgb), (v, i)
      assert np.array_equal(got[E.OBS_RGB_POOL8][i].cpu().numpy(), engine.pool_rgb(rgb, 8)), (v, i)
      assert np.array_equal(got[E.OBS_LAYER][i].cpu().numpy(), o.layer_view(p)), (v, i)
  finally:
    for o in oracles:
      o.close()
    e.close()


# 4. the engine is left as it was
def _draw_views(e, road):
  P = e.P
  for kind in _player_kinds(road) + (E.OBS_RGB_POOL4,):
    e.observe_views(road["banks"][8], kind, [p % P for p in range(N)])
    e.observe_views(road["all"], kind, [0, P - 1, 2, 2, 1, 0, 3], rows=[7, 7, 21, 0, 13, 2, 19])


def test_the_engine_is_left_as_it_was():
  name = "clean_up"
  road = recipe.road(name)
  A = torch.from_numpy(road["actions"]).to("cuda:0")
  ring = (E.OBS_RGB, E.OBS_LAYER, E.OBS_REWARD)
  plain = (E.OBS_WORLD_RGB, E.OBS_READY_TO_SHOOT, E.OBS_POSITION, E.OBS_ORIENTATION, E.OBS_STEP_TYPE,
           E.OBS_EVENTS)

  def build():
    eng = engine.Engine(recipe.pack(name), N, device=0)
    bufs = {k: eng.bind_ring(k, slots=3) for k in ring}
    bufs.update({k: eng.bind(k) for k in plain})
    eng.reset()
    for s in range(5):
      eng.step(A[s])
    return eng, bufs

  e, bufs = build()
  twin, twin_bufs = build()
  before = (e.snapshot(), e.counters(), e.ring, {k: v.clone() for k, v in bufs.items()}, e.plan)
  _draw_views(e, road)
  _draw_views(e, road)
  after = (e.snapshot(), e.counters(), e.ring, bufs, e.plan)
  assert np.array_equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2]
  assert before[4] == after[4]
  for k in bufs:
    _same_leaf(k, after[3][k], before[3][k], ("bound buffer", k))
  for s in range(5, 13):   # the next 8 steps: as on the twin that never drew a view
    e.step(A[s])
    twin.step(A[s])
    if s % 3 == 0:
      _draw_views(e, road)
    for k in bufs:
      _same_leaf(k, bufs[k], twin_bufs[k], ("step", s, k))
  assert np.array_equal(e.snapshot(), twin.snapshot()) and e.counters() == twin.counters()
  assert e.ring == twin.ring
  util.no_faults(e)
  e.close(); twin.close()


def test_rows_of_another_engine_are_drawn_and_rows_of_another_level_refused():
  name = "clean_up"
  other = engine.Engine(recipe.pack(name), 3, device=0, world_offset=11)
  kinds = tuple(k for k in recipe.record_kinds(other) if k != E.OBS_WORLD_RGB)
  bufs = {k: other.bind(k) for k in kinds}
  A = torch.from_numpy(recipe.actions(other.P, other.num_actions, n=3)).to(other.device)
  other.reset()
  for s in range(8):
    other.step(A[s])
  bank = other.save_worlds()
  e = engine.Engine(recipe.pack(name), N, device=0)   # never reset
  rows, players = [2, 0, 1, 2], [0, other.P - 1, 3, 0]
  for kind in kinds:
    _same(e.observe_views(bank, kind, players, rows, fingerprint=other.state_fingerprint),
          bufs[kind][rows, players], ("travel", kind))
  e.sync()
  util.no_faults(e)
  foreign = engine.Engine(recipe.pack("coins"), 2, device=0)
  foreign.reset()
  frows = foreign.save_worlds()
  padded = torch.zeros((2, e.info.world_state_bytes), dtype=torch.uint8, device=e.device)
  with pytest.raises(ValueError, match="fingerprint"):
    e.observe_views(padded, E.OBS_RGB, [0, 1], fingerprint=foreign.state_fingerprint)
  with pytest.raises(ValueError, match="bank must be"):
    e.observe_views(frows, E.OBS_RGB, [0, 1], fingerprint=foreign.state_fingerprint)
  with pytest.raises(ValueError, match="rows has 3 entries, players 2"):
    e.observe_views(bank, E.OBS_RGB, [0, 1], rows=[0, 1, 2])
  with pytest.raises(ValueError, match="not a per-player kind"):
    e.observe_views(bank, E.OBS_WORLD_RGB, [0, 1])
  for eng in (other, e, foreign):
    eng.close()


# 5. refusals, through the raw request
def _rc(e, **fields):
  req = E.MpStatesView(ctypes.sizeof(E.MpStatesView))
  for k, v in fields.items():
    setattr(req, k, v)
  return e._L.mp_snapshot(e._h, ctypes.addressof(req), ctypes.sizeof(req))


def test_refusals_happen_on_the_host_and_leave_everything_alone():
  name = "clean_up"
  road = recipe.road(name)
  e = engine.Engine(recipe.pack(name), N, device=0)
  e.reset()
  L = e._L
  S = e.info.world_state_bytes
  bank, fp = road["banks"][8], e.state_fingerprint
  rows = torch.tensor([1, 0], dtype=torch.int32, device=e.device)
  players = torch.zeros(N, dtype=torch.int32, device=e.device)
  per = {k: int(np.prod(e.shapes[k][0][2:])) * torch.empty((), dtype=e.shapes[k][1]).element_size()
         for k in e.shapes}
  dst = torch.full((N * per[E.OBS_RGB] + 64,), 0xAB, dtype=torch.uint8, device=e.device)
  snap = e.snapshot()
  ok = dict(kind=E.OBS_POSITION, fingerprint=fp, bank=bank.data_ptr(), bank_rows=N, count=N,
            players=players.data_ptr(), dst=dst.data_ptr(), dst_bytes=dst.numel())
  assert _rc(e, **ok) == 0   # (the request the refusals below are one edit away from)
  e.sync()
  dst.fill_(0xAB)

  def refused(what, code=E.MP_ERR_INVALID, **kw):
    assert _rc(e, **dict(ok, **kw)) == code, (what, L.mp_last_error())
    assert b"MpStatesView" in L.mp_last_error(), what
    return L.mp_last_error()

  refused("NULL bank", bank=None)
  refused("NULL dst", dst=None)
  assert b"players" in refused("NULL players", players=None)
  refused("count", count=0)
  refused("count", count=-3)
  refused("bank_rows", bank_rows=0)
  refused("struct_size", struct_size=64)
  assert b"fingerprint" in refused("fingerprint", fingerprint=fp ^ 1)
  refused("dst_bytes", dst_bytes=N * per[E.OBS_POSITION] - 1)
  refused("dst_bytes of a pixel kind", kind=E.OBS_RGB, dst_bytes=N * per[E.OBS_RGB] - 1)
  refused("more rows than the bank has", count=N + 1)
  refused("element alignment", kind=E.OBS_POSITION, dst=dst.data_ptr() + 2)
  refused("element alignment", kind=E.OBS_READY_TO_SHOOT, dst=dst.data_ptr() + 4)
  refused("element alignment", kind=E.OBS_LAYER, dst=dst.data_ptr() + 1)
  host = torch.zeros((N, S), dtype=torch.uint8)
  pinned = torch.zeros((N, S), dtype=torch.uint8).pin_memory()
  for b in (host, pinned):
    refused("a bank in host memory", bank=b.data_ptr())
  refused("rows in host memory", rows=torch.zeros(N, dtype=torch.int32).data_ptr())
  refused("players in host memory", players=torch.zeros(N, dtype=torch.int32).data_ptr())
  refused("dst in host memory", dst=host.data_ptr(), dst_bytes=host.numel())
  assert b"allocation" in refused("bank past its allocation", bank_rows=1 << 30, rows=rows.data_ptr(), count=2)
  refused("rows past their allocation", rows=rows.data_ptr(), count=1 << 28, dst_bytes=1 << 40)
  for kind in (-1, 24, 99):
    refused("kind out of range", kind=kind)
  assert b"not a per-player kind" in refused("WORLD.RGB", kind=E.OBS_WORLD_RGB)
  for kind in (E.OBS_REWARD, E.OBS_AUX0, E.OBS_STEP_TYPE, E.OBS_DISCOUNT, E.OBS_COLLECTIVE_REWARD, E.OBS_EVENTS,
               E.OBS_AUX1, E.OBS_ZAP_MATRIX, E.OBS_INTERACTION_INVENTORIES, E.OBS_MATRIX_CUMULANTS,
               E.OBS_INTERACTION_REWARDS):
    assert b"not a function of the record" in refused("transition kind", kind=kind), kind
  refused("a kind the level does not have", code=-5, kind=E.OBS_INVENTORY)   # MP_ERR_UNSUPPORTED
  for word in (0, 1):
    req = E.MpStatesView(ctypes.sizeof(E.MpStatesView))
    for k, val in ok.items():
      setattr(req, k, val)
    req.reserved[word] = 1
    assert L.mp_snapshot(e._h, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
    assert b"reserved" in L.mp_last_error()
  # nothing was launched: dst and the engine are as they were
  e.sync()
  assert bool((dst == 0xAB).all()) and np.array_equal(e.snapshot(), snap)
  util.no_faults(e)
  e.close()


# 6. an index that is no row or no player is never used as one
def test_bad_indices_leave_their_elements_alone_and_are_reported_once():
  name = "clean_up"
  road = recipe.road(name)
  e = engine.Engine(recipe.pack(name), N, device=0)
  e.reset()
  snap = e.snapshot()
  bank, P = road["banks"][8], e.P
  kinds = (E.OBS_POSITION, E.OBS_READY_TO_SHOOT, E.OBS_LAYER, E.OBS_RGB, E.OBS_RGB_POOL8)
  cases = [([3, 99, 1, -1, 3], [0, 1, 2, 3, 4], [1, 3], r"rows\[[13]\] = (99|-1) "),
           ([0, 1, 2, 3, 4], [0, P, 2, -1, 1], [1, 3], rf"players\[[13]\] = ({P}|-1) ")]
  # twelve bad pairs in one request (more than the eight MpStatesObserve keeps), three good ones
  twelve_rows = [3, 99, -1, 4, -7, 1 << 20, 1, 25, 2, 0, N, -1 << 30, 2, 4, 0]
  twelve_players = [0, 1, 2, P, 4, 5, 6, 0, -2, P + 3, 1, 2, -1, 1 << 20, 3]
  cases.append((twelve_rows, twelve_players, [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13], r"(rows|players)\[\d+\] = "))
  assert len(cases[2][2]) == 12
  for rows, players, bad, message in cases:
    good = [i for i in range(len(rows)) if i not in bad]
    for kind in kinds:
      shape, dtype = e.shapes[kind]
      out = torch.full((len(rows),) + tuple(shape[2:]), 7, dtype=dtype, device=e.device)
      e.observe_views(bank, kind, players, rows, out=out)
      with pytest.raises(ValueError, match=r"MpStatesView: " + message):
        e.sync()
      e.sync()   # reported once
      util.no_faults(e)
      for i in bad:   # EVERY such element, however many
        assert bool((out[i] == 7).all()), (kind, i)
      want = e.observe_views(bank, kind, [players[i] for i in good], [rows[i] for i in good])
      _same(out[good], want, ("the elements whose indices are a row and a player", kind))
  e.sync()
  assert np.array_equal(e.snapshot(), snap)
  util.no_faults(e)
  e.close()


# 7. the substrate
@pytest.mark.parametrize("rgb_pool", [1, 8])
def test_substrate_draws_sampled_players(rgb_pool):
  name = "clean_up"
  cfg = substrate.get_config(name)
  n = 4
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=17, rgb_pool=rgb_pool)
  P, nact = env.num_players, env.action_spec()[0].num_values
  A = util.random_actions(np.random.default_rng(9), 6, n, P, nact)
  env.reset()
  res = env.step_many(A, states=True)
  states = res.states   # 24 rows
  rng = np.random.default_rng(3)
  r, p = rng.integers(0, len(states), size=9), rng.integers(0, P, size=9)
  names = ("RGB", "LAYER", "POSITION")
  before = env.observe_states(states, names, rows=r)
  got = env.observe_states(states, names, rows=r, players=p)
  H, W = (int(d) for d in before["RGB"].shape[2:4])
  lshape = before["LAYER"].shape[2:]
  assert tuple(got) == names
  assert got["RGB"].shape == (9, H, W, 3) and got["LAYER"].shape == (9,) + tuple(lshape) and got["POSITION"].shape == (9, 2)
  if rgb_pool == 8:
    assert (H, W) == (11, 11)
  idx = torch.arange(9)
  for leaf in names:
    _same(got[leaf], before[leaf][idx, torch.from_numpy(p)], (leaf, rgb_pool))
  with pytest.raises(ValueError, match="WORLD.RGB.*not per player"):
    env.observe_states(states, ("RGB", "WORLD.RGB"), rows=r, players=p)
  default = env.observe_states(states, rows=r, players=p)
  assert "WORLD.RGB" not in default and "RGB" in default and "READY_TO_SHOOT" in default
  for leaf, value in default.items():
    _same(value, env.observe_states(states, (leaf,), rows=r)[leaf][idx, torch.from_numpy(p)], (leaf, "default"))
  # players=None: what it returned before
  again = env.observe_states(states, names, rows=r)
  assert tuple(again) == names and all(torch.equal(again[k], before[k]) for k in names)
  assert before["RGB"].shape == (9, P, H, W, 3)
  torch.cuda.synchronize()
  env.close()
