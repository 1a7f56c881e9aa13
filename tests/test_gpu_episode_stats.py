"""Episode statistics on the device (MpEpisodeStats; Engine.set_episode_stats, Engine.tally_events and
their Substrate forms): a registered engine folds every submission into per-world statistics by one
launch of k_episode_stats behind it.  The identity: engine A, driven by a seeded program of resets,
masked resets, steps, masked and listed steps, loads, registered episode starts and step_many in all
four families, holds after every call what its twin B holds, which runs the equivalent loop of single
masked steps — and both hold what the numpy model (tests/episode_stats_model.py) computes from B's
leaves.  Episodes are 12 frames long, so the K = 65 and K = 129 calls cross several episode ends in
the middle of a launch.

Results of the checks that set bounds: none — every comparison here is for equal bits."""
import numpy as np
import pytest
import torch

from meltingpot_amd import engine, substrate
from tests import episode_stats_model as model
from tests import util
from tests.test_episode_stats_cpu import CLEAN_SLOTS, crafted_rows

pytestmark = pytest.mark.gpu

E = engine
MAXFRAMES = 12
COMMONS = "commons_harvest__open"
KITCHENS = ("collaborative_cooking__cramped", "collaborative_cooking__asymmetric")
COLUMNS = {
    "clean_up": (("zap.source", "zap.target", "edible_consumed.player_index", "player_cleaned.player_index"),
                 ("zap.source>target",)),
    COMMONS: (("zap.source", "zap.target", "edible_consumed.player_index"), ("zap.source>target", "zap.target>source")),
}


def _pack(name):
  return util.patch_pack(E.load_pack(name), MAXFRAMES=MAXFRAMES)


def _actions(rng, name, shape, device):
  slots = CLEAN_SLOTS if name == "clean_up" else util.ZAP_HEAVY_SLOTS
  return torch.from_numpy(slots[rng.integers(0, 16, size=shape)].astype(np.int32)).to(device)


class Twin:
  """Engine B and the numpy model: every operation of the program as single (masked) steps of B,
  the model fed B's leaves and the mask of the worlds that ran."""

  def __init__(self, name, n, auto_reset, columns, pairs):
    self.e = E.Engine(_pack(name), n, device=0, auto_reset=auto_reset)
    self.stats = self.e.set_episode_stats(columns, pairs)
    self.model = model.Model(n, self.e.P, columns, pairs)
    self.started = np.zeros(n, bool)
    self.n = n

  def fold(self, ran):
    e = self.e
    self.model.step(e.observe_host(E.OBS_STEP_TYPE), e.observe_host(E.OBS_REWARD), e.observe_host(E.OBS_EVENTS),
                    np.asarray(ran, bool))

  def reset(self, mask=None):
    self.e.reset(mask=mask)
    ran = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
    self.started |= ran
    self.fold(ran)

  def load(self, bank, src):
    self.e.load_worlds(bank, torch.from_numpy(src).to(self.e.device))
    ran = src >= 0
    self.started |= ran
    self.fold(ran)

  def step(self, actions, mask=None):
    """One step of the worlds `mask` selects (None: all); returns the worlds that ran."""
    if mask is None:
      self.e.step(actions)
      ran = self.started.copy()
    else:
      self.e.step(actions, active=torch.from_numpy(mask.astype(np.uint8)).to(self.e.device))
      ran = mask.astype(bool) & self.started
    self.fold(ran)
    return ran

  def many(self, A, active=None, stop=0, stopped=None):
    """The loop of single masked steps a K-step request equals; `stopped` (host uint8 [n]) is
    updated in place as the request updates its tensor."""
    K = A.shape[0]
    for k in range(K):
      m = np.ones(self.n, bool) if active is None else active[k] != 0
      if stopped is not None:
        m = m & (stopped == 0)
      ran = self.step(A[k], None if m.all() else m)
      if stop:
        st = self.e.observe_host(E.OBS_STEP_TYPE)
        paid = (self.e.observe_host(E.OBS_REWARD) != 0).any(axis=1)
        reason = ((st == 2) * (stop & E.MP_STOP_LAST)) | (paid * (stop & E.MP_STOP_REWARD))
        stopped[ran & (reason != 0)] = reason[ran & (reason != 0)]


def _same(a_stats, twin, what):
  model.assert_equal(a_stats.arrays, twin.stats.arrays, (what, "A against B"))
  model.assert_equal(twin.stats.arrays, twin.model.arrays(), (what, "B against the model"))


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("name, n", [("clean_up", 5), (COMMONS, 9)])
def test_the_identity(name, n, auto_reset):
  columns, pairs = COLUMNS[name]
  rng = np.random.default_rng(1000 * n + auto_reset)
  a = E.Engine(_pack(name), n, device=0, auto_reset=auto_reset)
  stats = a.set_episode_stats(columns, pairs)
  b = Twin(name, n, auto_reset, columns, pairs)
  dev, P = a.device, a.P
  assert stats.columns == columns and stats.index(columns[1]) == 1 and stats.index(pairs[0]) == 0
  assert tuple(stats.total["pairs"].shape) == (n, len(pairs), P, P) and stats.total["counts"].dtype == torch.int64

  def both_reset(mask=None):
    a.reset(mask=mask)
    b.reset(mask)

  def both_step(mask=None):
    A = _actions(rng, name, (n, P), dev)
    if mask is None:
      a.step(A)
    else:
      a.step(A, active=torch.from_numpy(mask).to(dev))
    b.step(A, mask)

  def listed(K, worlds, until=None):
    """worlds=: entry i of the list steps world worlds[i]; a repeated entry and one that is no
    world run nothing (and are reported once by the next synchronising call)."""
    M = len(worlds)
    A = _actions(rng, name, (K, M, P), dev)
    owner = {}
    for i, w in enumerate(worlds):
      if 0 <= w < n and w not in owner:
        owner[w] = i
    full = torch.zeros((K, n, P), dtype=torch.int32, device=dev)
    mask = np.zeros((K, n), np.uint8)
    for w, i in owner.items():
      full[:, w] = A[:, i]
      mask[:, w] = 1
    bad = len(owner) < M
    if K == 1 and until is None:
      a.step(A[0], worlds=worlds)
      b.many(full, mask)
    elif until is None:
      a.step_many(A, worlds=torch.tensor(worlds, dtype=torch.int32, device=dev))
      b.many(full, mask)
    else:
      stopped_a = torch.zeros(n, dtype=torch.uint8, device=dev)
      stopped_b = np.zeros(n, np.uint8)
      a.step_many(A, worlds=worlds, until=until, stopped=stopped_a)
      b.many(full, mask, stop=E.MP_STOP_LAST | E.MP_STOP_REWARD, stopped=stopped_b)
      assert stopped_a.cpu().numpy().tolist() == stopped_b.tolist()
    if bad:
      with pytest.raises(ValueError, match="MpStepListed"):
        a.sync()

  # some worlds are never reset for a while: they run nothing
  first = np.zeros(n, np.uint8)
  first[1::2] = 1
  both_reset(first)
  _same(stats, b, "masked reset")
  both_step()
  _same(stats, b, "step with unstarted worlds")
  both_reset()
  _same(stats, b, "reset")
  for _ in range(3):
    both_step()
  bank = a.save_worlds().clone()           # rows of running episodes, step 3
  _same(stats, b, "steps")
  both_step(np.array([w % 3 != 0 for w in range(n)], np.uint8))
  _same(stats, b, "step(active=)")
  listed(1, [2, 2, n + 4])
  _same(stats, b, "step(worlds=)")
  stopped_a = torch.zeros(n, dtype=torch.uint8, device=dev)
  stopped_b = np.zeros(n, np.uint8)
  for K in (1, 3, 65, 129):
    A = _actions(rng, name, (K, n, P), dev)
    a.step_many(A, keep=())               # (the statistics' rows travel without being asked for)
    b.many(A)
    _same(stats, b, ("step_many", K))
    active = (rng.random((K, n)) < 0.6).astype(np.uint8)
    active[:, 0] = np.arange(K) < K // 2   # lengths=
    A = _actions(rng, name, (K, n, P), dev)
    r = a.step_many(A, active=torch.from_numpy(active).to(dev), events=True)
    b.many(A, active)
    _same(stats, b, ("step_many(active=)", K))
    assert set(r) == {"reward", "collective_reward", "step_type", "discount", "events"}
    A = _actions(rng, name, (K, n, P), dev)
    r = a.step_many(A, active=torch.from_numpy(active).to(dev), until=("last", "reward"), stopped=stopped_a,
                    keep=("reward",))
    b.many(A, active, stop=E.MP_STOP_LAST | E.MP_STOP_REWARD, stopped=stopped_b)
    assert stopped_a.cpu().numpy().tolist() == stopped_b.tolist(), K
    assert set(r) == {"reward", "stopped", "ran"}
    _same(stats, b, ("step_many(until=)", K))
    stopped_a.zero_()
    stopped_b[:] = 0
    listed(K, [n - 1, n + 2, n - 1])      # M = 3: entry 1 is no world, entry 2 repeats entry 0's
    _same(stats, b, ("step_many(worlds=)", K))
    listed(K, [3, 0, 4], until=("last", "reward"))
    _same(stats, b, ("step_many(worlds=, until=)", K))
    if K == 3:
      # a load cuts running episodes short (dropped, not counted); -1 leaves a world alone
      src = rng.integers(-1, n, size=n).astype(np.int32)
      src[0], src[1] = -1, 2
      a.load_worlds(bank, torch.from_numpy(src).to(dev))
      b.load(bank, src)
      _same(stats, b, "load_worlds")
      if auto_reset:
        rows = torch.from_numpy(rng.integers(-1, n, size=n).astype(np.int32)).to(dev)
        a.set_episode_starts(bank, rows)
        b.e.set_episode_starts(bank, rows.clone())
    if K == 65:
      both_reset(np.array([w % 2 == 0 for w in range(n)], np.uint8))
      _same(stats, b, "masked reset in the middle of episodes")
  # the program really finished episodes in every world, counted events, and dropped none
  got = model.flatten(stats.arrays)
  assert got["episodes"].min() >= (3 if auto_reset else 1), got["episodes"]
  assert got["total.counts"].sum() > 0 and got["total.pairs"].sum() > 0
  assert (got["dropped"] == 0).all()
  util.no_faults(a, sync=True)
  util.no_faults(b.e, sync=True)
  a.close()
  b.e.close()


def test_columns_empty_needs_no_events_row_and_a_request_without_its_rows_is_refused():
  import ctypes
  n = 5
  a = E.Engine(_pack("clean_up"), n, device=0)
  b = E.Engine(_pack("clean_up"), n, device=0)
  sa = a.set_episode_stats(())
  sb = b.set_episode_stats("default")
  assert sb.columns == a.event_columns() == E.level_event_columns(1)
  rng = np.random.default_rng(5)
  A = _actions(rng, "clean_up", (30, n, a.P), a.device)
  for e in (a, b):
    e.reset()
    e.step_many(A, keep=())
  assert "events" not in a._stats_scratch and "events" in b._stats_scratch
  fa, fb = model.flatten(sa.arrays), model.flatten(sb.arrays)
  for key in ("episodes", "open", "running.returns", "last.returns", "total.returns", "total.length"):
    assert fa[key].tobytes() == fb[key].tobytes(), key
  assert fa["episodes"].min() >= 2 and fa["total.counts"].shape == (n, 0, a.P)
  # the C ABI: a K-step request of a registered engine names its rows, and `ran`
  req = E.MpStepTrajectory(ctypes.sizeof(E.MpStepTrajectory), 2, 0, 0)
  req.actions, req.actions_step_bytes = A.data_ptr(), n * a.P * 4
  before = model.flatten(sb.arrays)
  assert b._L.mp_restore(b._h, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert b"REWARD and STEP_TYPE" in b._L.mp_last_error()
  until = E.MpStepUntil(ctypes.sizeof(E.MpStepUntil), 2, 0, 0)
  until.actions, until.actions_step_bytes, until.gamma = A.data_ptr(), n * a.P * 4, 1.0
  assert b._L.mp_restore(b._h, ctypes.addressof(until), ctypes.sizeof(until)) == E.MP_ERR_INVALID
  assert b"MpStepUntil" in b._L.mp_last_error()
  # ... with its rows but without `ran`: which steps ran could not be read
  kinds = (E.OBS_REWARD, E.OBS_STEP_TYPE, E.OBS_EVENTS)
  bufs = [torch.zeros((2,) + shape, dtype=dtype, device=b.device) for shape, dtype in (b.shapes[k] for k in kinds)]
  rows = (E.MpStepRow * 3)()
  for i, (kind, buf) in enumerate(zip(kinds, bufs)):
    rows[i].kind, rows[i].rows, rows[i].step_bytes = kind, buf.data_ptr(), buf[0].numel() * buf.element_size()
  until.num_rows, until.rows = 3, ctypes.cast(rows, ctypes.POINTER(E.MpStepRow))
  assert b._L.mp_restore(b._h, ctypes.addressof(until), ctypes.sizeof(until)) == E.MP_ERR_INVALID
  assert b"must name ran" in b._L.mp_last_error()
  after = model.flatten(sb.arrays)
  assert all(before[k].tobytes() == after[k].tobytes() for k in before)
  # tensors that are not the engine's device's, and too many columns
  with pytest.raises(ValueError):
    b.set_episode_stats(("zap.source",) * 33)
  with pytest.raises(ValueError, match="pair"):
    b.set_episode_stats(("zap.source>target",))
  host = E.EpisodeStats((), (), E.episode_stats_arrays(n, a.P, 0, 0, lambda shape, dtype: torch.zeros(
      shape, dtype=getattr(torch, dtype))))
  with pytest.raises(ValueError):
    b.set_episode_stats((), out=host)
  util.no_faults(a, sync=True)
  util.no_faults(b, sync=True)
  a.close()
  b.close()


def test_the_fused_frame_launch_and_a_ring_give_the_same_statistics():
  n, name = 5, "clean_up"
  columns, pairs = COLUMNS[name]
  plain, fused, ring, never = (E.Engine(_pack(name), n, device=0) for _ in range(4))
  fused.bind(E.OBS_WORLD_RGB)
  never.bind(E.OBS_WORLD_RGB)              # the twin that is never registered
  for kind in (E.OBS_REWARD, E.OBS_STEP_TYPE, E.OBS_EVENTS):
    ring.bind_ring(kind, slots=3)
  engines = (plain, fused, ring)
  was_fused = fused.fused
  assert was_fused and never.fused
  stats = [e.set_episode_stats(columns, pairs) for e in engines]
  assert fused.fused                       # (the frame launch stays fused; the statistics launch follows it)
  rng = np.random.default_rng(9)

  def run(engines, steps):
    for _ in range(steps):
      A = _actions(rng, name, (n, plain.P), plain.device)
      for e in engines:
        e.step(A)
    A = _actions(rng, name, (7, n, plain.P), plain.device)
    for e in engines:
      e.step_many(A, keep=())

  for e in engines + (never,):
    e.reset()
  run(engines + (never,), 30)
  assert model.flatten(stats[0].arrays)["episodes"].min() >= 2
  model.assert_equal(stats[1].arrays, stats[0].arrays, "WORLD.RGB bound (fused)")
  model.assert_equal(stats[2].arrays, stats[0].arrays, "a ring of 3 slots")

  def same_as_never(what):
    assert torch.equal(fused.hash_worlds(), never.hash_worlds()), what
    for kind in (E.OBS_REWARD, E.OBS_STEP_TYPE, E.OBS_WORLD_RGB):
      assert np.array_equal(fused.observe_host(kind), never.observe_host(kind)), (what, kind)
    # (event rows beyond a header's count are not written: the decoded events are what compares)
    assert fused.events_all() == never.events_all(), what

  same_as_never("registered")
  # clearing the registration: the launches and the results of an engine never registered
  fused.set_episode_stats(None)
  assert fused.episode_stats is None and fused.fused == was_fused
  frozen = model.flatten(stats[1].arrays)
  run((fused, never), 5)
  same_as_never("cleared")
  now = model.flatten(stats[1].arrays)
  assert all(frozen[k].tobytes() == now[k].tobytes() for k in frozen), "a cleared registration is not written"
  for e in engines + (never,):
    util.no_faults(e, sync=True)
    e.close()


def test_a_substrate_with_a_rollout_ring_and_a_one_world_substrate():
  cfg = substrate.get_config("clean_up")
  kw = dict(roles=cfg.default_player_roles, num_worlds=5, env_seed=21)
  ring = substrate.build("clean_up", rollout_length=3, **kw)
  plain = substrate.build("clean_up", **kw)
  stats = [env.set_episode_stats(pairs=("zap.source>target",)) for env in (ring, plain)]
  assert stats[0].columns == ring.event_columns()
  rng = np.random.default_rng(2)
  A = _actions(rng, "clean_up", (12, 5, ring.num_players), ring.engine.device)
  for env in (ring, plain):
    env.reset()
    for k in range(8):
      env.step(A[k])
    env.step_many(A)
  model.assert_equal(stats[0].arrays, stats[1].arrays, "rollout_length=3")
  got = model.flatten(stats[1].arrays)
  assert (got["running.length"] == 20).all() and got["open"].all() and got["running.counts"].sum() > 0
  r = plain.step_many(A, events=True)
  counts = plain.tally_events(r)
  assert tuple(counts.shape) == (5, len(stats[1].columns), plain.num_players)
  plain.set_episode_stats(None)
  assert plain.engine.episode_stats is None
  for env in (ring, plain):
    util.no_faults(env.engine, sync=True)
    env.close()
  single = substrate.build("clean_up", roles=cfg.default_player_roles)
  with pytest.raises(ValueError, match="num_worlds"):
    single.set_episode_stats()
  single.close()


def test_tally_events_on_crafted_rows_and_on_a_real_result():
  P, name = 7, "clean_up"
  e = E.Engine(_pack(name), 6, device=0)
  assert e.P == P
  columns, pairs = ("zap.source", "zap.target", "edible_consumed.player_index"), ("zap.source>target",)
  rows = crafted_rows(P)                                     # counts 0, 1, 63, 64, 65, 127
  ev = np.stack([rows, rows[::-1], rows])
  active = np.array([[1] * 6, [1, 0, 1, 0, 1, 1], [1, 1, 1, 1, 0, 1]], np.uint8)
  ran = np.array([3, 3, 1, 0, 2, 2], np.int32)
  for mask, limit in ((None, None), (active, None), (active, ran), (None, ran)):
    got, got_pairs = e.tally_events(ev, columns, active=mask, ran=limit, pairs=pairs)
    want = np.zeros((6, len(columns), P), np.int64)
    want_pairs = np.zeros((6, 1, P, P), np.int64)
    for w in range(6):
      done = 0
      for k in range(3):
        if (mask is not None and not mask[k, w]) or (limit is not None and done >= limit[w]):
          continue
        done += 1
        c, p = model.tally(ev[k, w], columns, pairs, P)
        want[w] += c
        want_pairs[w] += p
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (mask, limit)
    assert np.array_equal(got_pairs.cpu().numpy(), want_pairs), (mask, limit)
  assert want.sum() > 0 and want_pairs.sum() > 0
  # a real result against the host decode of the same rows
  rng = np.random.default_rng(4)
  e.reset()
  A = _actions(rng, name, (40, 6, P), e.device)
  r = e.step_many(A, events=True)
  out = torch.full((6, 4, P), -1, dtype=torch.int32, device=e.device)
  got = e.tally_events(r["events"], out=out)
  assert got is out and e.event_columns() == COLUMNS[name][0]
  host = r["events"].cpu().numpy()
  want = np.zeros((6, 4, P), np.int64)
  names = {"zap": ((0, "source"), (1, "target")), "edible_consumed": ((2, "player_index"),),
           "player_cleaned": ((3, "player_index"),)}
  for k in range(40):
    for w in range(6):
      for event, payload in E.Engine._decode_events(host[k, w], w):
        for column, key in names.get(event, ()):
          if 1 <= int(payload[key]) <= P:
            want[w, column, int(payload[key]) - 1] += 1
  assert np.array_equal(got.cpu().numpy(), want) and want[:, :2].sum() > 0 and want[:, 2:].sum() > 0
  with pytest.raises(ValueError):
    e.tally_events(r["events"][:, :, :5])
  with pytest.raises(ValueError):
    e.tally_events(r["events"], ("nothing.player",))
  util.no_faults(e, sync=True)
  e.close()


def test_a_mixture_registers_each_member_its_slice():
  kw = dict(num_worlds=[3, 2], env_seed=3, individual_observations=("POSITION",), global_observations=())
  mix = substrate.build_mixture(KITCHENS, **kw)
  alone = substrate.build_mixture(KITCHENS, **kw)
  stats = mix.set_episode_stats()
  assert tuple(stats.running["counts"].shape) == (5, len(stats.columns), mix.num_players)
  parts = [m.set_episode_stats() for m in alone._members]
  rng = np.random.default_rng(6)
  dev = mix.engines[0].device
  nact = mix.action_spec()[0].num_values
  A = torch.from_numpy(rng.integers(0, nact, size=(24, 5, mix.num_players)).astype(np.int32)).to(dev)
  mask = torch.from_numpy(rng.random((24, 5)) < 0.7).to(dev)
  for env in (mix, alone):
    env.reset()
    for k in range(4):
      env.step(A[k])
    env.step(A[4], active=mask[4])
    env.step_many(A)
    env.step_many(A, active=mask)
  for i, part in enumerate(parts):
    sl = mix.member_slice(i)
    model.assert_equal(stats.slice(sl.start, sl.stop).arrays, part.arrays, ("member", i))
  got = model.flatten(stats.arrays)
  assert got["open"].all() and (got["running.length"] > 24).all()
  mix.set_episode_stats(None)
  assert all(e.episode_stats is None for e in mix.engines)
  for e in mix.engines + alone.engines:
    util.no_faults(e, sync=True)
  mix.close()
  alone.close()
