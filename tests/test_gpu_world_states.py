"""World states as device data: mp_save_worlds copies chosen worlds' records into rows of a
device tensor, mp_load_worlds starts any worlds from such rows in one launch shaped like a masked
reset.  A loaded world IS the world it was saved from: under the same actions every later output
is byte-identical to the source's continuation (auto-resets included), and the oracle replaying
the SOURCE's seed and action history agrees — on every pack, plan and view, through rings and
`Substrate`.  The load launch writes the record's observations (A) as the source's last launch
did and the transition kinds (B) as a reset does; counters stay the engine's own; every refusal
happens on the host, and an index out of range is reported, never followed."""
import os

import numpy as np
import pytest
import torch

import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(engine.__file__), "assets")
PACKS = sorted(f[:-4] for f in os.listdir(ASSETS) if f.endswith(".mpk"))
E = engine
SCALARS = (E.OBS_REWARD, E.OBS_READY_TO_SHOOT, E.OBS_AUX0, E.OBS_STEP_TYPE, E.OBS_DISCOUNT,
           E.OBS_COLLECTIVE_REWARD, E.OBS_POSITION, E.OBS_ORIENTATION, E.OBS_EVENTS)
GROUP_A = (E.OBS_READY_TO_SHOOT, E.OBS_POSITION, E.OBS_ORIENTATION)
GROUP_B = (E.OBS_REWARD, E.OBS_AUX0, E.OBS_STEP_TYPE, E.OBS_DISCOUNT, E.OBS_COLLECTIVE_REWARD)
LATEST_INTERACTION = (E.OBS_INTERACTION_INVENTORIES, E.OBS_INTERACTION_REWARDS)


def _engine(pack, n, kinds=SCALARS, **kw):
  e = engine.Engine(pack, n, device=0, **kw)
  bufs = {k: e.bind(k) for k in kinds}
  return e, bufs


def _snap(bufs):
  return {k: v.clone() for k, v in bufs.items()}


def _events(ev, w):
  """World w's event rows, sorted (rows of one step come in no particular order)."""
  rows = np.asarray(ev[w])
  n = int(rows[0, 0])
  return int(rows[0, 1]), sorted(map(tuple, rows[1:1 + n].tolist()))


def _same(a, b, worlds_a, worlds_b, what=""):
  """Outputs `a` of worlds_a equal outputs `b` of worlds_b, kind by kind (events sorted)."""
  wa = torch.as_tensor(np.asarray(worlds_a), device=next(iter(a.values())).device)
  wb = torch.as_tensor(np.asarray(worlds_b), device=wa.device)
  for k in a:
    if k == E.OBS_EVENTS:
      ea, eb = a[k].cpu().numpy(), b[k].cpu().numpy()
      for i, j in zip(np.asarray(worlds_a).tolist(), np.asarray(worlds_b).tolist()):
        assert _events(ea, i) == _events(eb, j), (what, "events", i, j)
    else:
      x, y = a[k].index_select(0, wa), b[k].index_select(0, wb)
      assert torch.equal(x, y), (what, k, (x != y).nonzero()[:4].tolist())


def _request(e, op, **fields):
  """The return code of one MpWorldStates request (mp_snapshot / mp_restore) on engine e."""
  import ctypes
  req = engine.MpWorldStates(ctypes.sizeof(engine.MpWorldStates), op)
  for k, v in fields.items():
    setattr(req, k, v)
  call = e._L.mp_restore if op == engine.MP_STATES_LOAD else e._L.mp_snapshot
  return call(e._h, ctypes.addressof(req), ctypes.sizeof(req))


def _load_rc(e, bank, rows, src, fp):
  return _request(e, engine.MP_STATES_LOAD, bank=bank, bank_rows=rows, src=src, fingerprint=fp)


def _save_rc(e, count, dst, dst_bytes, worlds=None):
  return _request(e, engine.MP_STATES_SAVE, worlds=worlds, count=count, bank=dst, bank_bytes=dst_bytes)


def _bank_rows(e, worlds=None):
  return e.save_worlds(worlds).clone()


def _no_counters(rows, locate=None):
  """`rows` without the bytes of WorldTail::ctr[] and reward_fx (the 36 bytes behind the seed;
  row 0 of `locate`, default `rows`, must be world 0's record: its seed locates the tail) — what
  a load keeps from the destination."""
  seed = np.frombuffer(np.uint64(util.world_seed(0)).tobytes(), np.uint8)
  row = (rows if locate is None else locate)[0].cpu().numpy()
  at = [i for i in range(0, row.size - 8, 8) if (row[i:i + 8] == seed).all()]
  assert len(at) == 1, at
  keep = torch.ones(row.size, dtype=torch.bool, device=rows.device)
  keep[at[0] + 8:at[0] + 8 + 36] = False
  return rows[:, keep]


def test_fork_equals_continuation_in_this_engine_and_another():
  pack = engine.load_pack("clean_up")
  n = 64
  kinds = SCALARS + (E.OBS_RGB, E.OBS_WORLD_RGB)
  e, bufs = _engine(pack, n, kinds)
  e2, bufs2 = _engine(pack, n, kinds)
  assert e.state_fingerprint == e2.state_fingerprint != 0
  P, nact = e.P, e.num_actions
  rng = np.random.default_rng(1)
  A = torch.from_numpy(util.random_actions(rng, 40, n, P, nact)).to(e.device)
  B = torch.from_numpy(util.random_actions(rng, 25, n, P, nact)).to(e.device)
  e.reset()
  for s in range(40):
    e.step(A[s])
  bank = e.save_worlds()
  assert bank.shape == (n, e.info.world_state_bytes) and bank.dtype == torch.uint8
  ref = []
  for s in range(25):
    e.step(B[s])
    ref.append(_snap(bufs))
  ref_state = e.save_worlds().clone()
  src = torch.arange(n, dtype=torch.int32, device=e.device)
  for eng, out in ((e, bufs), (e2, bufs2)):
    eng.load_worlds(bank, src)
    for s in range(25):
      eng.step(B[s])
      _same(out, ref[s], range(n), range(n), ("step", s))
    assert torch.equal(_no_counters(eng.save_worlds()), _no_counters(ref_state))
    util.no_faults(eng)
  e.close(); e2.close()


def test_permuted_and_duplicated_loads_match_the_oracle_of_the_source():
  pack = engine.load_pack("clean_up")
  n, k, steps = 16, 30, 100
  kinds = (E.OBS_REWARD, E.OBS_WORLD_RGB, E.OBS_RGB)
  e, bufs = _engine(pack, n, kinds)
  P, nact = e.P, e.num_actions
  rng = np.random.default_rng(2)
  A = util.random_actions(rng, k, n, P, nact)
  B = util.random_actions(rng, steps, n, P, nact)
  dA, dB = torch.from_numpy(A).to(e.device), torch.from_numpy(B).to(e.device)
  e.reset()
  for s in range(k):
    e.step(dA[s])
  bank = _bank_rows(e)
  e.step(dA[0])   # (the engine moves on before the load)
  src = rng.permutation(n).astype(np.int32)
  src[3] = src[5] = src[11]   # several worlds take one row
  e.load_worlds(bank, src)
  for s in range(steps):
    e.step(dB[s])
  grid, avat, glob = e.dump()
  rew = bufs[E.OBS_REWARD].cpu().numpy()
  wrgb = bufs[E.OBS_WORLD_RGB].cpu().numpy()
  rgb = bufs[E.OBS_RGB].cpu().numpy()
  from oracle import oracle as orc
  for w in range(n):
    o = orc.Oracle(pack, util.world_seed(int(src[w])))   # the SOURCE's seed and whole history
    o.reset()
    for s in range(k):
      o.step(A[s, src[w]])
    for s in range(steps):
      o.step(B[s, w])
    og, oa, ogl = o.dump()
    assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), w
    assert np.array_equal(glob[w], ogl), w
    assert np.array_equal(rew[w], o.rewards()), w
    assert np.array_equal(wrgb[w], o.render_world()), w
    for p in range(P):
      assert np.array_equal(rgb[w, p], o.render_agent(p)), (w, p)
    o.close()
  util.no_faults(e)
  e.close()


def _reset_values(pack, n, history, mask, kinds, **kw):
  """What a masked reset writes after `history` (actions [k, n, P]) on a twin engine."""
  t, tb = _engine(pack, n, kinds, **kw)
  t.reset()
  for a in history:
    t.step(a)
  t.reset(mask=mask)
  out = _snap(tb)
  t.close()
  return out


def test_what_the_load_launch_writes():
  pack = engine.load_pack("clean_up")
  n, k = 16, 30
  kinds = SCALARS + (E.OBS_AUX1, E.OBS_AUX2, E.OBS_AUX3, E.OBS_AUX4, E.OBS_ZAP_MATRIX, E.OBS_LAYER,
                     E.OBS_RGB)
  e, bufs = _engine(pack, n, kinds, debug_observations=True)
  P, nact = e.P, e.num_actions
  rng = np.random.default_rng(3)
  A = torch.from_numpy(util.random_actions(rng, k + 7, n, P, nact)).to(e.device)
  e.reset()
  for s in range(k):
    e.step(A[s])
  bank = _bank_rows(e)
  at_save = _snap(bufs)
  for s in range(k, k + 7):
    e.step(A[s])
  before = _bank_rows(e)
  src = np.full(n, -1, np.int32)
  loaded = np.arange(0, n, 2)
  src[loaded] = rng.permutation(n)[:len(loaded)]
  left = np.setdiff1d(np.arange(n), loaded)
  e.load_worlds(bank, src)
  got = _snap(bufs)
  after = _bank_rows(e)
  mask = np.zeros(n, np.uint8)
  mask[loaded] = 1
  reset = _reset_values(pack, n, A[:k + 7], mask, kinds, debug_observations=True)
  # (A) the source's, as its last launch wrote them
  for kind in GROUP_A + (E.OBS_LAYER, E.OBS_RGB):
    _same({kind: got[kind]}, {kind: at_save[kind]}, loaded, src[loaded], ("A", kind))
  # (B) as a masked reset writes them
  for kind in GROUP_B + (E.OBS_EVENTS, E.OBS_AUX1, E.OBS_AUX2, E.OBS_AUX3, E.OBS_AUX4, E.OBS_ZAP_MATRIX):
    _same({kind: got[kind]}, {kind: reset[kind]}, loaded, loaded, ("B", kind))
  assert (got[E.OBS_STEP_TYPE][loaded] == 0).all()
  # worlds left alone: their record, and what a masked reset leaves
  assert torch.equal(after[left], before[left])
  # loaded records are their rows of the bank, but for the counters the destination keeps
  assert torch.equal(_no_counters(after, bank)[loaded], _no_counters(bank)[src[loaded].astype(np.int64)])
  for kind in kinds:
    _same({kind: got[kind]}, {kind: reset[kind]}, left, left, ("left", kind))
  util.no_faults(e)
  e.close()


def _continuation(name, n, k, cont, kinds, pack=None, seed=0, load_src=None, **kw):
  """Steps n worlds k steps, saves, steps `cont` more recording every bound output, loads a
  permutation of the rows and replays the same actions: loaded world w must reproduce world
  src[w]'s record of outputs.  Returns (engine, bufs, src, at_save, at_load)."""
  pack = pack or engine.load_pack(name)
  e, bufs = _engine(pack, n, kinds, **kw)
  P, nact = e.P, e.num_actions
  rng = np.random.default_rng(seed)
  A = torch.from_numpy(util.random_actions(rng, k, n, P, nact)).to(e.device)
  B = torch.from_numpy(util.random_actions(rng, cont, n, P, nact)).to(e.device)
  e.reset()
  for s in range(k):
    e.step(A[s])
  bank = _bank_rows(e)
  at_save = _snap(bufs)
  ref = []
  for s in range(cont):
    e.step(B[s])
    ref.append(_snap(bufs))
  src = rng.permutation(n).astype(np.int32) if load_src is None else load_src
  e.load_worlds(bank, src)
  at_load = _snap(bufs)
  # (the matrix's latest-interaction kinds are outputs no record holds: written by an
  # interaction, zeroed / left by a reset or a load — not compared along the continuation)
  keep = {k: v for k, v in bufs.items() if k not in LATEST_INTERACTION}
  for s in range(cont):
    e.step(B[s][torch.as_tensor(src.astype(np.int64), device=e.device)])
    _same(keep, ref[s], range(n), src, (name, "step", s))
  util.no_faults(e)
  return e, bufs, src, at_save, at_load


@pytest.mark.parametrize("name", PACKS)
def test_every_pack_continues_from_a_permuted_load(name):
  pack = engine.load_pack(name)
  probe = engine.Engine(pack, 1, device=0, debug_observations=True)
  optional = (E.OBS_ZAP_MATRIX, E.OBS_AUX1, E.OBS_INVENTORY, E.OBS_INTERACTION_INVENTORIES,
              E.OBS_MATRIX_CUMULANTS, E.OBS_INTERACTION_REWARDS)
  extra = tuple(k for k in optional if probe._L.mp_obs_bytes(probe._h, k) > 0)
  probe.close()
  n = 4
  e, bufs, src, at_save, at_load = _continuation(name, n, 12, 8, SCALARS + (E.OBS_RGB,) + extra,
                                                 pack=pack, debug_observations=True)
  for kind in GROUP_A + (E.OBS_RGB,) + tuple(k for k in extra if k == E.OBS_INVENTORY):
    _same({kind: at_load[kind]}, {kind: at_save[kind]}, range(n), src, (name, "A", kind))
  before = _snap(bufs)
  # (B): what a reset of every world writes now (the records are the engine's own)
  e.reset(mask=np.ones(n, np.uint8))
  reset = _snap(bufs)
  for kind in GROUP_B + (E.OBS_EVENTS,) + tuple(k for k in extra if k != E.OBS_INVENTORY):
    if kind == E.OBS_INTERACTION_REWARDS:   # (a reset leaves it as it was: so does a load)
      assert torch.equal(reset[kind], before[kind])
      continue
    _same({kind: at_load[kind]}, {kind: reset[kind]}, range(n), range(n), (name, "B", kind))
  e.close()


PLANS = [
    dict(kinds=(E.OBS_RGB,)),
    dict(kinds=(E.OBS_RGB_POOL2,)),
    dict(kinds=(E.OBS_RGB_POOL4, E.OBS_WORLD_RGB)),
    dict(kinds=(E.OBS_RGB_POOL8,)),
    dict(kinds=(E.OBS_LAYER, E.OBS_WORLD_RGB)),
    dict(kinds=(E.OBS_WORLD_RGB,), world_pool=2),
    dict(kinds=(E.OBS_RGB, E.OBS_WORLD_RGB), world_pool=4),
    dict(kinds=(E.OBS_WORLD_RGB, E.OBS_LAYER), world_pool=8),
    dict(kinds=(E.OBS_RGB, E.OBS_WORLD_RGB), dev={"batch_worlds": 2, "max_groups": 2}),
    dict(kinds=(E.OBS_RGB, E.OBS_WORLD_RGB, E.OBS_LAYER), unfused=True),
    dict(kinds=()),
]


@pytest.mark.parametrize("plan", range(len(PLANS)))
def test_every_plan_and_view_continues_from_a_load(plan):
  cfg = dict(PLANS[plan])
  kinds = SCALARS + tuple(cfg.pop("kinds"))
  n = 24
  e, bufs, src, at_save, at_load = _continuation("clean_up", n, 10, 6, kinds, seed=plan, **cfg)
  for kind in kinds:
    if kind in GROUP_A or kind not in SCALARS:   # (A): the pixels, LAYER, the record's scalars
      _same({kind: at_load[kind]}, {kind: at_save[kind]}, range(n), src, ("A", plan, kind))
  e.close()


def test_a_load_writes_the_ring_slot_a_masked_reset_writes():
  pack = engine.load_pack("clean_up")
  n, T = 8, 3
  e = engine.Engine(pack, n, device=0)
  ring = {k: e.bind_ring(k, slots=T) for k in (E.OBS_STEP_TYPE, E.OBS_POSITION, E.OBS_RGB)}
  twin = engine.Engine(pack, n, device=0)
  tring = {k: twin.bind_ring(k, slots=T) for k in (E.OBS_STEP_TYPE, E.OBS_POSITION, E.OBS_RGB)}
  P, nact = e.P, e.num_actions
  A = torch.from_numpy(util.random_actions(np.random.default_rng(4), 4, n, P, nact)).to(e.device)
  for eng in (e, twin):
    eng.reset()
    for s in range(4):
      eng.step(A[s])
  bank = e.save_worlds()
  before = dict(e.ring)
  src = np.full(n, -1, np.int32)
  src[::2] = [1, 0, 3, 2]
  e.load_worlds(bank, src)
  mask = (src >= 0).astype(np.uint8)
  twin.reset(mask=mask)
  assert e.ring == twin.ring and e.ring["next"] == (before["next"] + 1) % T
  slot = e.ring["last"]
  st, tst = ring[E.OBS_STEP_TYPE][slot].cpu().numpy(), tring[E.OBS_STEP_TYPE][slot].cpu().numpy()
  assert np.array_equal(st, tst) and (st[mask == 1] == 0).all()
  # the loaded worlds' pixels are their sources' (the twin's masked-out worlds are unchanged)
  rgb, trgb = ring[E.OBS_RGB][slot], tring[E.OBS_RGB][slot]
  prev = (slot + T - 1) % T
  for w in range(n):
    if src[w] >= 0:
      assert torch.equal(rgb[w], ring[E.OBS_RGB][prev][src[w]]), w
    else:
      assert torch.equal(rgb[w], trgb[w]), w
  util.no_faults(e)
  e.close(); twin.close()


def test_finished_rows_load_finished_and_auto_reset_like_their_source():
  pack = util.patch_pack(engine.load_pack("clean_up"), MAXFRAMES=9)
  n = 6
  for auto in (True, False):
    e, bufs = _engine(pack, n, SCALARS + (E.OBS_RGB,), auto_reset=auto)
    P, nact = e.P, e.num_actions
    A = torch.from_numpy(util.random_actions(np.random.default_rng(5), 14, n, P, nact)).to(e.device)
    e.reset()
    for s in range(9):
      e.step(A[s])
    assert (bufs[E.OBS_STEP_TYPE] == 2).all()
    bank = _bank_rows(e)
    ref = []
    for s in range(9, 12):
      e.step(A[s])
      ref.append(_snap(bufs))
    src = np.array([5, 4, 3, 2, 1, 0], np.int32)
    e.load_worlds(bank, src)
    assert (bufs[E.OBS_STEP_TYPE] == 2).all()
    assert (bufs[E.OBS_DISCOUNT] == 0).all() and (bufs[E.OBS_REWARD] == 0).all()
    assert (bufs[E.OBS_EVENTS][:, 0, :2] == 0).all()
    for i, s in enumerate(range(9, 12)):
      e.step(A[s][torch.as_tensor(src.astype(np.int64), device=e.device)])
      _same(bufs, ref[i], range(n), src, (auto, s))
    if auto:
      assert (ref[0][E.OBS_STEP_TYPE] == 0).all()
    util.no_faults(e)
    e.close()


def test_counters_are_the_work_this_engine_did():
  pack = engine.load_pack("clean_up")
  n = 8
  e = engine.Engine(pack, n, device=0)
  other = engine.Engine(pack, n, device=0)
  P, nact = e.P, e.num_actions
  A = torch.from_numpy(util.random_actions(np.random.default_rng(6), 30, n, P, nact)).to(e.device)
  other.reset()
  for s in range(30):
    other.step(A[s])
  bank = other.save_worlds()   # rows with 30 steps of someone else's work in their counters
  e.reset()
  for s in range(5):
    e.step(A[s])
  rows = e.save_worlds()
  e.load_worlds(bank, np.arange(n, dtype=np.int32))
  for s in range(7):
    e.step(A[s])
  e.load_worlds(rows, np.arange(n, dtype=np.int32)[::-1].copy())
  e.load_worlds(bank, np.full(n, -1, np.int32))
  for s in range(4):
    e.step(A[s])
  c = e.counters()
  assert c["world_steps"] == n * 16, c
  assert c["agent_steps"] == n * P * 16, c
  assert c["episodes"] == n, c
  util.no_faults(e)
  e.close(); other.close()


def test_refusals_and_out_of_range_indices():
  pack = engine.load_pack("clean_up")
  n = 8
  e, bufs = _engine(pack, n, SCALARS + (E.OBS_WORLD_RGB,))
  L = e._L
  S = e.info.world_state_bytes
  with pytest.raises(ValueError, match="never been reset"):
    e.save_worlds()
  P, nact = e.P, e.num_actions
  A = torch.from_numpy(util.random_actions(np.random.default_rng(7), 12, n, P, nact)).to(e.device)
  e.reset()
  for s in range(3):
    e.step(A[s])
  bank = e.save_worlds()
  src = torch.arange(n, dtype=torch.int32, device=e.device)
  with pytest.raises(ValueError, match="fingerprint"):
    e.load_worlds(bank, src, fingerprint=e.state_fingerprint ^ 1)
  other = engine.Engine(engine.load_pack("commons_harvest__open"), n, device=0)
  assert other.state_fingerprint != e.state_fingerprint
  pads = engine.Engine(pack, n, device=0, dev={"record_pad": 1})
  assert pads.state_fingerprint != e.state_fingerprint
  fewer = engine.Engine(pack, n, device=0, num_players=3)
  assert fewer.state_fingerprint != e.state_fingerprint
  assert engine.Engine(pack, 3, device=0, world_offset=100).state_fingerprint == e.state_fingerprint
  for eng in (other, pads, fewer):
    eng.close()
  fp = e.state_fingerprint
  # a bank that is not device memory: plain host, pinned host
  host = torch.zeros((n, S), dtype=torch.uint8)
  pinned = torch.zeros((n, S), dtype=torch.uint8).pin_memory()
  for b in (host, pinned):
    assert _load_rc(e, b.data_ptr(), n, src.data_ptr(), fp) == engine.MP_ERR_INVALID
    assert _save_rc(e, n, b.data_ptr(), b.numel()) == engine.MP_ERR_INVALID
  # a bank whose rows run past the end of its allocation; a buffer too small for the rows
  assert _load_rc(e, bank.data_ptr(), 1 << 30, src.data_ptr(), fp) == engine.MP_ERR_INVALID
  assert b"allocation" in L.mp_last_error()
  assert _save_rc(e, n, bank.data_ptr(), bank.numel() - 1) == engine.MP_ERR_INVALID
  assert _load_rc(e, bank.data_ptr(), n, host[0].data_ptr(), fp) == engine.MP_ERR_INVALID
  # a request that names the wrong entry point, a wrong struct_size, an unknown op
  assert _request(e, engine.MP_STATES_SAVE, struct_size=8) == engine.MP_ERR_INVALID
  assert _request(e, 9) == engine.MP_ERR_INVALID
  assert e._L.mp_restore(e._h, None, 0) == engine.MP_ERR_INVALID
  # out-of-range indices: never followed, the world / row left alone, reported at the next sync
  before = e.save_worlds().clone()
  bad = np.arange(n, dtype=np.int32)[::-1].copy()
  bad[2], bad[5] = n + 3, -7
  e.load_worlds(bank, bad)
  with pytest.raises(ValueError, match="src"):
    e.sync()
  e.sync()   # (reported once)
  after = e.save_worlds()
  assert torch.equal(after[2], before[2]) and torch.equal(after[5], before[5])
  out = torch.full((3, S), 0xAB, dtype=torch.uint8, device=e.device)
  e.save_worlds(torch.tensor([1, n, 0], dtype=torch.int32), out=out)
  with pytest.raises(ValueError, match="worlds"):
    e.sync()
  assert (out[1] == 0xAB).all() and torch.equal(out[0], after[1]) and torch.equal(out[2], after[0])
  # the engine goes on stepping correctly: the same as a twin that took the same loads
  twin, tb = _engine(pack, n, SCALARS + (E.OBS_WORLD_RGB,))
  twin.reset()
  for s in range(3):
    twin.step(A[s])
  fixed = bad.copy()
  fixed[2], fixed[5] = -1, -1
  twin.load_worlds(bank, fixed)
  for s in range(3, 12):
    e.step(A[s]); twin.step(A[s])
  _same(bufs, tb, range(n), range(n), "after refusals")
  assert torch.equal(e.save_worlds(), twin.save_worlds())
  util.no_faults(e)
  e.close(); twin.close()


def test_at_size_every_world_matches_the_oracle_of_its_source():
  pack = engine.load_pack("clean_up")
  n, k, steps = 4096, 8, 32
  e, bufs = _engine(pack, n, (E.OBS_REWARD, E.OBS_WORLD_RGB))
  assert e.fused
  P, nact = e.P, e.num_actions
  rng = np.random.default_rng(8)
  A = util.random_actions(rng, k, n, P, nact)
  B = util.random_actions(rng, steps, n, P, nact)
  e.reset()
  dA = torch.from_numpy(A).to(e.device)
  for s in range(k):
    e.step(dA[s])
  bank = e.save_worlds()[torch.from_numpy(rng.permutation(n)).to(e.device)]   # a shuffled bank
  order = e.save_worlds()   # (which source each bank row is: its seed word)
  S = e.info.world_state_bytes
  src = rng.permutation(n).astype(np.int32)
  e.load_worlds(bank, src)
  dB = torch.from_numpy(B).to(e.device)
  for s in range(steps):
    e.step(dB[s])
  grid, avat, glob = e.dump()
  rew = bufs[E.OBS_REWARD].cpu().numpy()
  wrgb = bufs[E.OBS_WORLD_RGB].cpu().numpy()
  # the source world of bank row r, found by its record (unique per world: its seed)
  rows = bank.cpu().numpy()
  worlds = order.cpu().numpy()
  key = {worlds[w].tobytes(): w for w in range(n)}
  source_of_row = np.array([key[rows[r].tobytes()] for r in range(n)])
  source = source_of_row[src]            # world w continues world source[w]
  dest_of_source = np.empty(n, np.int64)
  dest_of_source[source] = np.arange(n)
  acts = np.concatenate([A, B[:, dest_of_source]], axis=0)   # source s's whole history
  sample = set(range(0, n, 257))
  for s, og, oa, ogl, orew, _, views in util.replay_parallel(pack, acts, looks=(k + steps,),
                                                             sample=sample, world_view=True):
    w = int(dest_of_source[s])
    assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), (w, s)
    assert np.array_equal(glob[w], ogl), (w, s)
    assert np.array_equal(rew[w], orew), (w, s)
    if s in sample:
      assert np.array_equal(wrgb[w], views[k + steps]), (w, s)
  util.no_faults(e)
  e.close()


@pytest.mark.parametrize("mode", ["batched", "ring", "one"])
def test_substrate_save_state_and_load_state(mode):
  n = 1 if mode == "one" else 6
  kw = {"rollout_length": 3} if mode == "ring" else {}
  roles = substrate.get_config("clean_up").default_player_roles
  env = substrate.build("clean_up", roles=roles, num_worlds=n, **kw)
  other = substrate.build("clean_up", roles=roles, num_worlds=n, **kw)
  P = env.num_players
  rng = np.random.default_rng(9)
  acts = rng.integers(0, env.action_spec()[0].num_values, size=(12, n, P))
  def act(e, a):
    return e.step(a[0] if mode == "one" else torch.from_numpy(a).to(e.engine.device))
  env.reset()
  for s in range(5):
    act(env, acts[s])
  states = env.save_state()
  assert isinstance(states, substrate.WorldStates) and len(states) == n
  assert states.fingerprint == env.engine.state_fingerprint == other.engine.state_fingerprint
  def flat(ts):
    if mode == "one":
      return [np.asarray(ts.step_type)] + [np.asarray(r) for r in ts.reward] + [
          np.asarray(v) for d in ts.observation for v in d.values()]
    return [ts.step_type.cpu().numpy(), ts.reward.cpu().numpy()] + [
        v.cpu().numpy() for v in ts.observation.values()]
  snaps = [flat(act(env, acts[s])) for s in range(5, 12)]   # (ring leaves: copied at once)
  for target in (env, other):
    if target is other:
      other.reset()
    ts = target.load_state(states, 0 if mode == "one" else list(range(n)))
    assert ts.first()  if mode == "one" else bool((ts.step_type == 0).all())
    if mode == "ring":
      assert ts.slot == target.slot
    for i, s in enumerate(range(5, 12)):
      got = flat(act(target, acts[s]))
      for x, y in zip(got, snaps[i]):
        assert np.array_equal(x, y), (mode, target is other, s)
  # one row selected, loaded into every world
  picked = states[0] if mode == "one" else states[[2]]
  ts = other.load_state(picked, 0 if mode == "one" else [0] * n)
  with pytest.raises(ValueError):
    other.load_state(substrate.WorldStates(states.data, states.fingerprint ^ 1),
                     0 if mode == "one" else list(range(n)))
  env.close(); other.close()
