"""The state hash on the GPU (MpStatesHash: k_hash_rows hashes rows where they lie).  The device's
values are the host loop's and the numpy restatement's on the same bytes; a state keeps its hash
through everything that legitimately differs between two records of it (the destination engine's
counters, the orders cache, padding, the bytes of avatars that do not play) and loses it with any
byte that counts; an index outside the bank is reported, not read; refusals launch nothing; and a
request moves nothing of the engine's."""
import ctypes

import numpy as np
import pytest
import torch

import states_recipe as R
import test_state_hash_cpu as C
import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

E = engine
N = R.N
SENTINEL = -0x0123456789ABCDEF


def _stepped(name, n=N, steps=20, seed=7, **kw):
  """An engine on the recipe's pack after `steps` seeded random steps (one launch; the recipe's
  episodes end at step 16, so the worlds are four steps into their second episode)."""
  e = engine.Engine(R.pack(name), n, device=0, **kw)
  e.reset()
  e.step_many(util.random_actions(np.random.default_rng(seed), steps, n, e.P, e.num_actions))
  return e


def _env(name, n=N, seed=51, steps=20):
  cfg = substrate.get_config(name)
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=n, env_seed=seed)
  env.reset()
  if steps:
    env.step_many(util.random_actions(np.random.default_rng(seed), steps, n, env.num_players,
                                      env.action_spec()[0].num_values))
  return env


# ---- device equals host equals numpy ---------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_device_hashes_are_the_host_forms(name):
  e = _stepped(name)
  lay = e.state_layout()
  bank = e.save_worlds()
  h = e.hash_states(bank)
  assert h.dtype == torch.int64 and tuple(h.shape) == (N,)
  rows = bank.cpu().numpy()
  host = E.hash_states_host(R.pack(name), rows)
  assert np.array_equal(h.cpu().numpy(), host), name
  assert np.array_equal(host, C.numpy_hash(rows, C.numpy_mask(lay)))
  assert torch.equal(e.hash_worlds(), h)
  assert len(set(host.tolist())) == N   # five worlds, five seeds, five states
  # row lists: repeats, more rows than worlds, a world list
  pick = [4, 0, 0, 3, 1, 2, 4, 4, 1]
  assert torch.equal(e.hash_states(bank, rows=pick), h[pick])
  assert torch.equal(e.hash_worlds(worlds=[3, 3, 0]), h[[3, 3, 0]])
  out = torch.zeros(N, dtype=torch.int64, device=e.device)
  assert e.hash_states(bank, out=out).data_ptr() == out.data_ptr() and torch.equal(out, h)
  # a bank of one row
  one = bank[2:3].clone()
  assert e.hash_states(one).tolist() == [int(host[2])]
  # the mask the engine hashes with (MP_HASH_MASK with an engine) is the pack's
  mask = np.zeros(lay.world_stride, np.uint8)
  req = E.MpStatesHash(ctypes.sizeof(E.MpStatesHash), E.MP_HASH_MASK)
  req.out, req.out_bytes = mask.ctypes.data, mask.nbytes
  assert e._L.mp_snapshot(e._h, ctypes.addressof(req), ctypes.sizeof(req)) == 0
  assert np.array_equal(mask, E.state_hash_mask(R.pack(name))) and np.array_equal(mask, C.numpy_mask(lay))
  req.plane_mask, req.flags = 1 << (lay.grid_planes - 1), E.MP_HASH_CUSTOM
  assert e._L.mp_snapshot(e._h, ctypes.addressof(req), ctypes.sizeof(req)) == 0
  assert np.array_equal(mask, C.numpy_mask(lay, planes=(lay.grid_planes - 1,)))
  e.sync()
  util.no_faults(e)
  e.close()


def test_the_arena_with_three_of_its_players():
  name = C.MATRIX_ARENA
  e = engine.Engine(E.load_pack(name), N, device=0, num_players=3)
  e.reset()
  e.step_many(util.random_actions(np.random.default_rng(3), 12, N, e.P, e.num_actions))
  lay = e.state_layout()
  assert lay.P == 3 and lay.player_block == 6000
  rows = e.save_worlds().cpu().numpy()
  h = e.hash_worlds().cpu().numpy()
  assert np.array_equal(h, C.numpy_hash(rows, C.numpy_mask(lay)))
  assert np.array_equal(h, E.hash_states_host(E.load_pack(name), rows, num_players=3))
  spec = dict(planes=(lay.avatar_layer,), fields=("player_block", "ax"))
  assert np.array_equal(e.hash_worlds(**spec).cpu().numpy(), C.numpy_hash(rows, C.numpy_mask(lay, **spec)))
  e.sync()
  util.no_faults(e)
  e.close()


# ---- what a state keeps its hash through, and what it loses it with --------------------------------
def test_invariances_of_the_default_spec():
  name = "clean_up"
  env, twin = _env(name), _env(name, seed=52, steps=7)   # another seed, another number of steps
  eng, lay = env._eng, env.state_layout()
  original = env.save_state()
  h = env.hash_states(original)
  assert tuple(h.shape) == (N,) and torch.equal(h, env.hash_worlds())
  # loaded into a substrate with another history and saved again: other bytes, the same states
  twin.load_state(original, list(range(N)))
  again = twin.save_state()
  assert not torch.equal(again.data, original.data)   # (ctr[] and reward_fx are the destination's)
  assert torch.equal(twin.hash_states(again), h) and torch.equal(twin.hash_worlds(), h)

  def edited(edit):
    s = substrate.WorldStates(original.data.clone(), original.fingerprint)
    edit(env.state_fields(s), s.data)
    assert not torch.equal(s.data, original.data)
    return env.hash_states(s)

  def bookkeeping(f, data):
    f.ctr[:] = 12345
    f.reward_fx[:] = -5
  assert torch.equal(edited(bookkeeping), h)

  def junk(f, data):
    data[:, lay.grid_bytes:lay.grid_pad] = 0xAB                      # the padding
    data[:, lay.grid_pad + lay.tail_bytes:] = 0xCD                   # behind the tail
    for fname, (off, elem, count) in lay.fields.items():             # the avatars that do not play
      if count == 16:
        data[:, lay.grid_pad + off + elem * lay.P:lay.grid_pad + off + elem * 16] = 0xEF
  assert lay.grid_pad > lay.grid_bytes and lay.P < 16
  assert torch.equal(edited(junk), h)

  def no_orders(f, data):
    assert bool((f.orders_step != 0).all())   # (the cache is there after a step)
    f.orders_step[:] = 0
  assert torch.equal(edited(no_orders), h)

  # (one apple removed: test_a_custom_spec_is_a_cell, on a level whose map starts with apples)
  def later(f, data):
    f.step[3] += 1
  got = edited(later)
  assert got[3] != h[3] and torch.equal(got[[0, 1, 2, 4]], h[[0, 1, 2, 4]])
  eng.sync(); twin._eng.sync()
  util.no_faults(eng); util.no_faults(twin._eng)
  env.close(); twin.close()


def test_distinct_hashes_count_distinct_masked_rows():
  name = "commons_harvest__open"
  n = 64
  e = _stepped(name, n=n, steps=5)
  src = np.random.default_rng(8).integers(0, 20, n).astype(np.int32)
  e.load_worlds(e.save_worlds(), src)   # 64 worlds, at most 20 states, each world with its own counters
  e.step_many(np.zeros((e.N, e.P), np.int32) + 3, repeat=3)   # the same actions everywhere: duplicates stay duplicates
  bank = e.save_worlds()
  h = e.hash_worlds().cpu().numpy()
  # (and every row with a counter byte of its own: 64 different records)
  bank[:, e.state_layout().field_offset("ctr", 7)] = torch.arange(n, dtype=torch.uint8, device=e.device)
  rows = bank.cpu().numpy()
  mask = E.state_hash_mask(R.pack(name))
  distinct = len(np.unique(rows & mask, axis=0))
  assert distinct == len(set(src.tolist())) and len(np.unique(rows, axis=0)) == n
  uniq, inverse = torch.unique(e.hash_states(bank), return_inverse=True)
  assert len(uniq) == len(set(h.tolist())) == distinct
  same = inverse.cpu().numpy()
  assert all((same[i] == same[j]) == (src[i] == src[j]) for i in range(n) for j in range(0, n, 7))
  e.sync()
  util.no_faults(e)
  e.close()


def test_a_custom_spec_is_a_cell():
  """The avatar plane plus the avatars' positions: eating an apple stays in the cell, a move leaves it."""
  name = "commons_harvest__open"
  env = _env(name, n=2, steps=4)
  lay = env.state_layout()
  original = env.save_state()
  spec = dict(planes=(lay.avatar_layer,), fields=("avatar_x", "avatar_y"))
  cell = env.hash_states(original, **spec)
  rows = original.data.cpu().numpy()
  want = C.numpy_hash(rows, C.numpy_mask(env._eng.state_layout(), planes=(lay.avatar_layer,), fields=("ax", "ay")))
  assert np.array_equal(cell.cpu().numpy(), want)
  assert torch.equal(env.hash_worlds(**spec), cell) and not torch.equal(cell, env.hash_states(original))
  s = substrate.WorldStates(original.data.clone(), original.fingerprint)
  f = env.state_fields(s)
  apple = lay.state_id("apple.apple")
  al = lay.state_layers[apple]
  ys, xs = (f.grid[0, al] == apple).nonzero(as_tuple=True)
  assert len(ys) > 0
  wait = lay.state_id("apple.appleWait")   # (the eaten apple waits on its own layer)
  f.grid[0, al, ys[0], xs[0]] = 0
  f.grid[0, lay.state_layers[wait], ys[0], xs[0]] = wait
  assert torch.equal(env.hash_states(s, **spec), cell)
  full = env.hash_states(s)   # one apple removed: another state
  assert full[0] != env.hash_states(original)[0] and full[1] == env.hash_states(original)[1]
  # a move: the avatar's byte to a free cell, and its position with it (a well-formed row)
  AL = lay.avatar_layer
  x0, y0 = int(f.avatar_x[0, 0]), int(f.avatar_y[0, 0])
  g = f.grid[0].cpu().numpy()
  free = [(x, y) for y in range(1, lay.H - 1) for x in range(1, lay.W - 1)
          if not g[[l for l in range(lay.L) if lay.layer_names[l] not in ("logic", "alternateLogic", "background")], y, x].any()]
  x1, y1 = free[0]
  f.grid[0, AL, y1, x1] = f.grid[0, AL, y0, x0]
  f.grid[0, AL, y0, x0] = 0
  f.avatar_x[0, 0], f.avatar_y[0, 0] = x1, y1
  assert not env.check_states(s).cpu().numpy().any()
  moved = env.hash_states(s, **spec)
  assert moved[0] != cell[0] and moved[1] == cell[1]
  assert np.array_equal(moved.cpu().numpy(), C.numpy_hash(s.data.cpu().numpy(), C.numpy_mask(env._eng.state_layout(), planes=(AL,), fields=("ax", "ay"))))
  # the spec before this one again, and the default in between: the engine keeps one custom mask
  only_x = env.hash_states(s, fields=("avatar_x",))
  assert torch.equal(env.hash_states(s, **spec), moved) and not torch.equal(only_x, moved)
  with pytest.raises(ValueError, match="apples"):
    env.hash_states(s, fields=("apples",))
  with pytest.raises(ValueError, match="player block"):
    env.hash_worlds(fields=("player_block",))
  with pytest.raises(ValueError, match="no grid plane"):
    env.hash_worlds(planes=(lay.grid_planes,))
  env._eng.sync()
  util.no_faults(env._eng)
  env.close()


# ---- a bad index is reported, not read --------------------------------------------------------------
def test_a_row_index_outside_the_bank_keeps_its_element():
  e = _stepped("coins", steps=3)
  bank = e.save_worlds()
  h = e.hash_states(bank)
  for bad in (N, -1, 1 << 30):
    out = torch.full((3,), SENTINEL, dtype=torch.int64, device=e.device)
    e.hash_states(bank, rows=[0, bad, 2], out=out)
    with pytest.raises(ValueError, match=r"MpStatesHash: rows\[1\] = %d" % bad):
      e.sync()
    assert out.tolist() == [int(h[0]), SENTINEL, int(h[2])]
    e.sync()   # reported once
  out = torch.full((2,), SENTINEL, dtype=torch.int64, device=e.device)
  e.hash_worlds(worlds=[N, 1], out=out)
  with pytest.raises(ValueError, match=r"MpStatesHash: rows\[0\] = %d" % N):
    e.sync()
  assert out.tolist() == [SENTINEL, int(h[1])]
  # the engine is as usable as before
  e.step(np.zeros((N, e.P), np.int32))
  assert torch.equal(e.hash_worlds(), e.hash_states(e.save_worlds()))
  e.sync()
  util.no_faults(e)
  e.close()


# ---- refusals ----------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
  e = _stepped("clean_up", steps=4)
  L = e._L
  S = e.info.world_state_bytes
  bank = e.save_worlds()
  out = torch.full((N + 1,), SENTINEL, dtype=torch.int64, device=e.device)
  rows = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32, device=e.device)
  state, ctr, fp = bank.clone(), e.counters(), e.state_fingerprint
  lay = e.state_layout()
  ok = dict(fingerprint=fp, bank=bank.data_ptr(), bank_rows=N, count=N, out=out.data_ptr(), out_bytes=N * 8)

  def request(op=E.MP_HASH_ROWS, **fields):
    req = E.MpStatesHash(ctypes.sizeof(E.MpStatesHash), op)
    for k, v in dict(ok, **fields).items():
      setattr(req, k, v)
    return L.mp_snapshot(e._h, ctypes.addressof(req), ctypes.sizeof(req)), L.mp_last_error().decode()

  def refused(word, **fields):
    rc, msg = request(**fields)
    assert rc == E.MP_ERR_INVALID and word in msg, (word, rc, msg)

  hip = ctypes.CDLL("libamdhip64.so")
  base, size = ctypes.c_void_p(), ctypes.c_size_t()
  assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(bank.data_ptr())) == 0
  host = np.zeros((N, S), np.uint8)
  refused("NULL bank", bank=None)
  refused("NULL out", out=None)
  refused("at least 1", count=0)
  refused("at least 1", bank_rows=0)
  refused("without a row list", count=N + 1, out_bytes=(N + 1) * 8)
  refused("16-byte aligned", bank=bank.data_ptr() + 8, bank_rows=N - 1, count=1)
  refused("8-byte aligned", out=out.data_ptr() + 4)
  refused("4-byte aligned", rows=rows.data_ptr() + 2, count=2)
  refused("need", out_bytes=N * 8 - 1)
  refused("fingerprint", fingerprint=fp ^ 1)
  refused("MpStatesHash (bank)", bank=host.ctypes.data)
  refused("allocation", bank=(base.value + size.value - S) & ~15, bank_rows=2, count=1)
  refused("unknown op", op=7)
  refused("goes without an engine", op=E.MP_HASH_HOST)
  refused("names no plane", flags=E.MP_HASH_CUSTOM, plane_mask=1 << lay.grid_planes)
  refused("names no field", flags=E.MP_HASH_CUSTOM, field_mask=1 << len(lay.fields))
  refused("no player block", flags=E.MP_HASH_CUSTOM | E.MP_HASH_PLAYER_BLOCK, plane_mask=1)
  refused("default spec", plane_mask=1)
  refused("every world is hashed", op=E.MP_HASH_WORLDS, count=N - 1)
  refused("struct_size", struct_size=96)
  fresh = engine.Engine(R.pack("clean_up"), N, device=0)   # never reset
  req = E.MpStatesHash(ctypes.sizeof(E.MpStatesHash), E.MP_HASH_WORLDS)
  req.count, req.out, req.out_bytes = N, out.data_ptr(), N * 8
  assert L.mp_snapshot(fresh._h, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"never been reset" in L.mp_last_error()
  fresh.close()
  e.sync()
  assert bool((out == SENTINEL).all())
  assert torch.equal(e.save_worlds(), state) and e.counters() == ctr
  # the same request, well-formed, runs
  assert request()[0] == 0
  assert torch.equal(out[:N], e.hash_worlds()) and int(out[N]) == SENTINEL
  with pytest.raises(ValueError, match="bank must be"):
    e.hash_states(bank[:, :-16])
  with pytest.raises(ValueError, match="out must be"):
    e.hash_states(bank, out=out)
  e.sync()
  util.no_faults(e)
  e.close()


# ---- nothing else moved ------------------------------------------------------------------------------
def test_a_hash_changes_nothing_of_the_engine():
  name = "clean_up"
  e = engine.Engine(R.pack(name), N, device=0)
  ring = {k: e.bind_ring(k, slots=3) for k in (E.OBS_RGB, E.OBS_REWARD)}
  plain = {k: e.bind(k) for k in (E.OBS_WORLD_RGB, E.OBS_POSITION, E.OBS_STEP_TYPE, E.OBS_EVENTS)}
  A = torch.from_numpy(R.actions(e.P, e.num_actions)).to(e.device)
  e.reset()
  for s in range(4):
    e.step(A[s])
  bank = e.save_worlds()
  before = (e.snapshot(), e.counters(), e.ring, {k: v.clone() for k, v in {**ring, **plain}.items()}, e.plan)
  e.hash_states(bank)
  e.hash_states(bank, rows=[4, 0], planes=(0, 3), fields=("ctr",))
  e.hash_worlds()
  e.hash_worlds(worlds=[1], fields=("step",))
  after = (e.snapshot(), e.counters(), e.ring, {**ring, **plain}, e.plan)
  assert (before[0] == after[0]).all() and before[1] == after[1] and before[2] == after[2] and before[4] == after[4]
  for k, v in before[3].items():
    assert torch.equal(v, after[3][k]), k
  e.sync()
  util.no_faults(e)
  e.close()
