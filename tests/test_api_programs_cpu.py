"""The program tests without a GPU: the generator's promises, the coverage of the committed set, the
model against an independent restatement of itself, and the runner against deliberately wrong
models — each must be reported at the first op where it can show.  For the STATE programs also:
the first set's programs are op for op what they were (CRCs), every adjacency with a new class is
held, and the model's own runs contain the crossings the programs are there for (printed under
`pytest -s`; profiles/r24_state_programs.md).  For the UNIT programs the same again: the state set is
pinned by CRCs too, every adjacency with a unit class is held, each level's two programs contain the
crossings of listed steps, statistics and view units (exemptions listed by name), and eight more
wrong models are reported at their first op (profiles/r31_unit_programs.md)."""
import collections
import functools
import zlib

import numpy as np
import pytest

import api_programs as ap
import states_recipe
from engine_model import ModelEngine
from meltingpot_amd import engine as E


def _profile(name):
  return next((s, p) for s, p in ap.COMMITTED if p["name"] == name)


def _same_op(a, b):
  return a.keys() == b.keys() and all(
      np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def test_the_committed_set_is_the_one_the_issue_names():
  names = [p["name"] for _, p in ap.COMMITTED]
  assert len(set(names)) == len(names) == 3 * len(ap.LEVEL_PACKS) + 2
  for pack in ap.LEVEL_PACKS:
    three = [p for _, p in ap.COMMITTED if p["pack"] == pack and not p["stock"]]
    assert sorted(p["n"] for p in three) == [5, 13, 37]
    assert sum(1 for p in three if p["ring"] == ap.RING_SLOTS) == 1
    assert sum(1 for p in three if p["world_pool"] == 8) == 1
  from meltingpot_amd import pack as pack_lib
  assert len({int(pack_lib.loads(E.load_pack(p))["hdr"][1]) for p in ap.LEVEL_PACKS}) == 9   # nine levels
  stock = [p for _, p in ap.COMMITTED if p["stock"]]
  assert len(stock) == 2 and all(p["pack"] == "clean_up" and not p["num_players"] for p in stock)
  assert {p["auto_reset"] for _, p in ap.COMMITTED} == {True, False}
  assert {p["unfused"] for _, p in ap.COMMITTED} == {None, True}
  assert any(p["num_players"] for _, p in ap.COMMITTED)


@pytest.mark.parametrize("seed,profile", ap.COMMITTED, ids=[p["name"] for _, p in ap.COMMITTED])
def test_programs_are_deterministic_and_within_bounds(seed, profile):
  prog, again = ap.make_program(seed, profile), ap.make_program(seed, profile)
  assert len(prog) == len(again) and all(_same_op(a, b) for a, b in zip(prog, again))
  assert not all(_same_op(a, b) for a, b in zip(prog, ap.make_program(seed + 1, profile)))
  assert prog[0]["op"] == "reset_all"
  assert {op["op"] for op in prog} == set(ap.OP_CLASSES)
  assert ap.MIN_OPS <= len(prog) <= ap.MAX_OPS
  assert ap.world_steps(prog) <= ap.MAX_WORLD_STEPS
  assert ap.longest_host_run(prog) >= ap.HOST_RUN
  g = ap._geometry(profile)
  N, P, A, nact = g["N"], g["P"], g["A"], g["nact"]
  banks, have_snap, bound = [], False, set(profile["views"])
  agent = (E.OBS_RGB,) + tuple(E.OBS_RGB_POOL.values())
  bad = total = 0
  for op in prog:
    c = op["op"]
    if c in ("masked_reset", "masked_reseed"):
      assert op["mask"].shape == (N,) and op["mask"].dtype == np.uint8 and op["mask"].any()
      if c == "masked_reseed":
        assert op["seeds"].shape == (N,) and op["seeds"].dtype == np.uint64
    elif c == "step_host":     # a refused call is no part of a program
      assert op["actions"].shape == (N, P) and (op["actions"] >= 0).all() and (op["actions"] < nact).all()
    elif c == "step_dev":
      assert op["actions"].shape == (N, P) and op["actions"].dtype == np.int32
      bad += int(((op["actions"] < 0) | (op["actions"] >= nact)).sum()); total += op["actions"].size
    elif c == "step_fields":
      assert op["fields"].shape == (N, P, A)
      assert (op["fields"] >= g["lo"]).all() and (op["fields"] <= g["hi"]).all()
    elif c in ("step_many", "step_many_rows"):
      assert op["K"] in ap.MANY_K
      wide = N + 3 if op["form"] == "slice" else N
      lead = () if op["form"] == "repeat" else (op["K"],)
      assert op["actions"].shape == lead + (wide, P) + ((A,) if op["fields"] else ())
      assert 0 <= op["lo"] and op["lo"] + N <= wide
      if op["fields"]:
        assert (op["actions"] >= g["lo"]).all() and (op["actions"] <= g["hi"]).all()
      # (the engine's own shape rules take what the runner will pass)
      E.check_step_many(lead + (N, P) + ((A,) if op["fields"] else ()), op["actions"].dtype, N, P,
                        repeat=op["K"] if op["form"] == "repeat" else None, num_fields=A if op["fields"] else None)
      if c == "step_many_rows":
        assert op["observations"] and set(op["observations"]) <= set(g["row_kinds"])
        E.check_step_rows(op["observations"], taken=[E.OBS_EVENTS])
    elif c == "save":
      w = op["worlds"]
      assert 1 <= len(w) <= N and len(set(w.tolist())) == len(w) and w.min() >= 0 and w.max() < N
      banks.append(len(w))
    elif c == "load":
      assert 0 <= op["bank"] < len(banks)
      src = op["src"]
      assert src.shape == (N,) and src.min() >= -1 and src.max() < banks[op["bank"]]
      assert (src == -1).any() and (src >= 0).any()
    elif c == "snapshot":
      have_snap = True
    elif c == "restore":
      assert have_snap
    elif c == "rebind":
      if op["bind"]:
        assert op["kind"] not in bound
        assert op["kind"] not in agent or not bound & set(agent), "one per-agent view at a time"
        bound.add(op["kind"])
      else:
        assert op["kind"] in bound
        bound.discard(op["kind"])
  assert bad <= max(3, 0.05 * total)


def test_every_ordered_pair_of_op_classes_is_adjacent_somewhere():
  programs = [ap.make_program(s, p) for s, p in ap.COMMITTED]
  table = ap.pair_counts(programs)
  print(ap.format_pair_table(table))
  print("ops", sum(len(p) for p in programs), "world-steps", sum(ap.world_steps(p) for p in programs))
  off = ~np.eye(len(ap.OP_CLASSES), dtype=bool)
  missing = [(ap.OP_CLASSES[i], ap.OP_CLASSES[j]) for i, j in np.argwhere((table == 0) & off)]
  assert not missing, missing
  assert any(0 < ap.world_steps(p) for p in programs)
  # out-of-range ids do occur in the set
  nbad = sum(int(((op["actions"] < 0) | (op["actions"] >= ap._geometry(p.profile)["nact"])).sum())
             for p in programs for op in p if op["op"] == "step_dev")
  assert nbad > 0


# ---------------------------------------------------------------- the model against itself

class ScratchModel(ModelEngine):
  """The model restated: a world is copied not from its log but from its HISTORY — the program-
  level calls it has seen (re-seeds, resets, every step's raw actions, steps on a finished world
  included), run again from scratch through a fresh one-world model — and step_many is the
  unrolled loop of public single steps (so: no ring)."""

  def __init__(self, *a, **kw):
    super().__init__(*a, **kw)
    self._kw = kw
    self._hist = [[("origin", w)] for w in range(self.N)]

  def reset(self, seeds=None, mask=None):
    for w in range(self.N):
      if mask is None or mask[w]:
        self._hist[w].append(("reset", None if seeds is None else int(seeds[w])))
    super().reset(seeds, mask)

  def step(self, actions, active=None, worlds=None):
    a = np.asarray(actions, np.int32)
    if worlds is not None:
      self.step_many(a[None], keep=(), active=active, worlds=worlds)
      return
    for w in range(self.N):
      if active is None or active[w]:
        self._hist[w].append(("step", a[w].copy()))
    super().step(a, active)

  def step_fields(self, fields, active=None):
    f = np.asarray(fields, np.int32)
    for w in range(self.N):
      if active is None or active[w]:
        self._hist[w].append(("fields", f[w].copy()))
    super().step_fields(f, active)

  def step_many(self, actions, *, repeat=None, fields=False, events=False, observations=(),
                keep=("reward", "collective_reward", "step_type", "discount"), active=None, until=None,
                stopped=None, returns=False, gamma=1.0, states=False, hashes=False, worlds=None, out=None):
    """The defining identity, unrolled: the loop of step(A[k], active=M[k] & (stopped == 0)) with
    `stopped` updated on the "host" from what each step left.  A list (worlds=) is the identity of
    MpStepListed, restated: the world's owner is its first entry; the full request gets the caller's
    `stopped` itself (an unlisted world is masked out, so its byte stays), and every other per-call
    tensor is gathered by entry on top of what `out` held."""
    assert not self._slots
    a = np.asarray(actions, np.int32)
    if worlds is not None:
      names = [int(w) for w in worlds]
      M = len(names)
      owner = {}
      for i in reversed(range(M)):
        if 0 <= names[i] < self.N:
          owner[names[i]] = i
      K = int(repeat) if repeat is not None else a.shape[0]
      blocks = [a if repeat is not None else a[k] for k in range(K)]
      full = np.zeros((K, self.N) + blocks[0].shape[1:], np.int32)
      mask = np.zeros((K, self.N), np.uint8)
      for w, i in owner.items():
        for k in range(K):
          full[k, w] = blocks[k][i]
          mask[k, w] = 1 if active is None else (np.asarray(active)[k, i] if np.ndim(active) == 2 else np.asarray(active)[i]) != 0
      res = self.step_many(full, fields=fields, events=events, observations=observations, keep=keep, active=mask,
                           until=until, stopped=stopped, returns=returns, gamma=gamma)
      got = {}
      for key, value in res.items():
        if key == "stopped":
          got[key] = value
          continue
        axis = 0 if key in ("ran", "returns") else 1
        shape = value.shape[:axis] + (M,) + value.shape[axis + 1:]
        g = np.array(out[key]) if out and key in out else np.zeros(shape, value.dtype)
        for w, i in owner.items():
          g[(slice(None),) * axis + (i,)] = value[(slice(None),) * axis + (w,)]
        got[key] = g
      return got
    K = int(repeat) if repeat is not None else a.shape[0]
    keys = list(keep) + (["events"] if events else []) + [int(k) for k in observations]
    rows = {key: [] for key in keys}
    stopping = until is not None or stopped is not None or returns is not False
    stop = sum(E.STOP_NAMES[n] for n in ((until,) if isinstance(until, str) else until or ()))
    stopped = np.zeros(self.N, np.uint8) if stopped is None else stopped
    ran, ret, g = np.zeros(self.N, np.int32), np.zeros((self.N, self.P)), np.ones(self.N)
    out_states, out_hashes = [], []
    for k in range(K):
      block = a if repeat is not None else a[k]
      m = np.ones(self.N, bool) if active is None else np.asarray(active)[k] != 0 if np.ndim(active) == 2 else np.asarray(active) != 0
      if stopping:
        m = m & (stopped == 0)
      (self.step_fields if fields else self.step)(block, active=None if m.all() else m)
      reward, kind = self.observe_host(E.OBS_REWARD), self.observe_host(E.OBS_STEP_TYPE)
      for w in np.nonzero(m)[0]:
        ran[w] += 1
        ret[w] = ret[w] + g[w] * reward[w]
        g[w] = g[w] * np.float64(gamma)
        reason = (1 if stop & 1 and kind[w] == 2 else 0) | (2 if stop & 2 and (reward[w] != 0).any() else 0)
        if reason and stopping:
          stopped[w] = reason
      for key in keys:
        rows[key].append(self.observe_host(E.STEP_MANY_NAMES.get(key, key)))
      if states:
        out_states.append(self.save_worlds())
      if hashes:
        out_hashes.append(self.hash_worlds())
    out = {key: np.stack(v) for key, v in rows.items()}
    if states:
      out["states"] = out_states
    if hashes:
      out["hashes"] = np.array(out_hashes, np.int64)
    if stopping:
      out.update(stopped=stopped, ran=ran)
      if returns is not False:
        out["returns"] = ret
    return out

  def _row(self, w):
    return dict(super()._row(w), hist=list(self._hist[w]))

  def _become(self, w, row):
    hist = row["hist"]
    one = ModelEngine(self.pack_bytes, 1, **dict(self._kw, world_offset=hist[0][1]))
    for entry in hist[1:]:
      if entry[0] == "reset":
        one.reset(None if entry[1] is None else np.array([entry[1]], np.uint64), np.array([1], np.uint8))
      elif entry[0] == "step":
        one.step(entry[1][None])
      else:
        one.step_fields(entry[1][None])
    assert one._o[0].done == row["finished"]
    self._o[w].close()
    self._o[w], self._seed[w], self._log[w] = one._o[0], one._seed[0], one._log[0]
    one._o = []
    self._started[w] = row["started"]
    self.exact[w] = row.get("exact", True)
    self._paused[w] = False
    self._hist[w] = list(hist)


@pytest.mark.parametrize("name", ["coins-n5", "territory__inside_out-n5", "gift_refinements-n13",
                                  "prisoners_dilemma_in_the_matrix__repeated-n13"])
def test_the_model_equals_its_restatement(name):
  seed, profile = _profile(name)
  assert not profile["ring"]
  prog = ap.make_program(seed, profile)
  a, b = ap.make_model(profile), ap.make_model(profile, ScratchModel)
  assert ap.run_program(prog, a, b) == len(prog)
  assert ap.run_program(prog, ap.make_model(profile, ScratchModel), ap.make_model(profile), stop_after=7) == 7
  a.close(); b.close()


def test_a_ring_program_runs_model_against_model():
  seed, profile = _profile("clean_up-n5")
  assert profile["ring"] == ap.RING_SLOTS
  prog = ap.make_program(seed, profile)
  a, b = ap.make_model(profile), ap.make_model(profile)
  assert ap.run_program(prog, a, b) == len(prog)
  assert a.ring["slots"] == ap.RING_SLOTS and a._cursor > len(prog) // 3
  a.close(); b.close()


# ---------------------------------------------------------------- the comparer is sensitive

class LoadIgnoresMinusOne(ModelEngine):
  def _source_row(self, rows, src, w):
    return rows[max(int(src[w]), 0)]


class LoadTakesTheNextRow(ModelEngine):
  def _source_row(self, rows, src, w):
    return rows[(int(src[w]) + 1) % len(rows)] if src[w] >= 0 else None


class ManyDoesNotAutoReset(ModelEngine):
  def _many_auto_reset(self):
    return False


class ReseedKeepsTheEpisodeCount(ModelEngine):
  def _reseed(self, w, seed):
    episodes = sum(1 for e in self._log[w] if e[0] == "reset")
    super()._reseed(w, seed)
    for _ in range(episodes):
      self._o[w].reset()
      self._log[w].append(("reset",))


class FrozenRepeatsTheLastReward(ModelEngine):
  def _frozen_rewards(self, w):
    return self._o[w].rewards()


def _trace(program, model):
  """What the runner looks at, after every op, of a model run alone."""
  side = ap._Side(model)
  out = []
  for op in program:
    side.apply(op, program.profile["ring"])
    out.append((model.dump(), [model.observe_host(k) for k in model.scalar_kinds], side.rows,
                model.counters(), {k: np.array(v) for k, v in model._bound.items()}))
  return out


def _equal(a, b):
  if isinstance(a, dict):
    return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
  if isinstance(a, (tuple, list)):
    return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
  if a is None or b is None:
    return a is b
  a, b = np.asarray(a), np.asarray(b)
  if a.ndim >= 2 and a.shape[-2:] == (E.EVENT_ROWS, 4):
    return ap.canonical_events(a) == ap.canonical_events(b)
  return np.array_equal(a, b)


# (wrong model, op classes at which it can first show, a profile and the seed of a program that
# shows it; None: the committed one.  A frozen world repeats a reward only if the episode's last
# step paid one, which 17 frames of random play rarely do: that program's seed was searched for)
WRONG_MODELS = [
    (LoadIgnoresMinusOne, ("load",), "coins-n5", None),
    (LoadTakesTheNextRow, ("load",), "coins-n5", None),
    (ManyDoesNotAutoReset, ("step_many", "step_many_rows"), "coop_mining-n5", None),
    (ReseedKeepsTheEpisodeCount, ("masked_reseed",), "coins-n5", None),
    (FrozenRepeatsTheLastReward, ap.STEP_CLASSES, "coins-n5", 14),
]


@pytest.mark.parametrize("wrong,classes,name,seed", WRONG_MODELS, ids=[w[0].__name__ for w in WRONG_MODELS])
def test_the_runner_reports_a_wrong_model_at_its_first_op(wrong, classes, name, seed):
  committed, profile = _profile(name)
  seed = committed if seed is None else seed
  prog = ap.make_program(seed, profile)
  right, bad = _trace(prog, ap.make_model(profile)), _trace(prog, ap.make_model(profile, wrong))
  first = next((i for i, (x, y) in enumerate(zip(right, bad)) if not _equal(x, y)), None)
  assert first is not None, "this program never shows the wrong model: choose another"
  assert prog[first]["op"] in classes, (first, prog[first]["op"])
  with pytest.raises(ap.Mismatch) as err:
    ap.run_program(prog, ap.make_model(profile, wrong), ap.make_model(profile))
  text = str(err.value)
  assert f"program seed {seed}, profile {name}, op {first}: {prog[first]['op']}" in text, text
  assert "world" in text or "bad_actions" in text
  # a prefix that stops short of the op passes
  assert ap.run_program(prog, ap.make_model(profile, wrong), ap.make_model(profile), stop_after=first) == first


# ================================================================== the state programs
# CRC-32 of "\n".join(short_form(op)) of each committed program of the first set, as the generator
# wrote it before the state classes were added: those 29 programs stay op for op what they were
FIRST_SET_CRCS = [
    4229355257, 2548632098, 3766868341, 402132235, 2269418939, 74637082, 1292735000, 2397877344,
    3355606509, 3136088153, 946387555, 139620854, 3277654155, 1143666235, 3869652750, 3137392074,
    3630345819, 2909569933, 2884176625, 1941212377, 3781382393, 3925682546, 1392560469, 2038339635,
    2426985218, 1545311275, 2224218350, 3564122540, 677060799]
# ... and of every argument's bytes (short_form abbreviates a large array to its shape)
FIRST_SET_BYTES_CRCS = [
    2218820954, 1087914836, 693833364, 2217402031, 640452086, 658944506, 3774009416, 2608778444,
    2177914804, 1057346918, 715140307, 1940672399, 1462608127, 192815018, 1923028878, 1441881605,
    3443458307, 1188046538, 3366471218, 3842153393, 2954082966, 2612787414, 3963182066, 77860825,
    1191621424, 3415859352, 2449972944, 2053290610, 3506065503]


def _bytes_crc(prog):
  c = 0
  for op in prog:
    for k, v in op.items():
      c = zlib.crc32(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode(),
                     zlib.crc32(k.encode(), c))
  return c


def test_the_first_set_is_op_for_op_what_it_was():
  programs = [ap.make_program(s, p) for s, p in ap.COMMITTED]
  assert all(p["classes"] == ap.OP_CLASSES for _, p in ap.COMMITTED)
  assert [zlib.crc32("\n".join(ap.short_form(op) for op in prog).encode()) for prog in programs] == FIRST_SET_CRCS
  assert [_bytes_crc(prog) for prog in programs] == FIRST_SET_BYTES_CRCS


STATE_IDS = [p["name"] for _, p in ap.STATE_COMMITTED]


@functools.lru_cache(maxsize=None)
def _state_program(name):
  seed, profile = next((s, p) for s, p in ap.STATE_COMMITTED if p["name"] == name)
  return ap.make_program(seed, profile)


@functools.lru_cache(maxsize=None)
def _state_cover(name):
  """What the model's run of a state program contains (computed once, shared, read-only)."""
  return ap.program_cover(_state_program(name))


def test_the_state_set_is_the_one_the_issue_names():
  profiles = [p for _, p in ap.STATE_COMMITTED]
  assert len(set(STATE_IDS)) == len(profiles) == 2 * len(ap.LEVEL_PACKS) + 1
  assert all(p["auto_reset"] and not p["ring"] and p["classes"] == ap.STATE_CLASSES for p in profiles)
  for pack in ap.LEVEL_PACKS:
    two = [p for p in profiles if p["pack"] == pack and not p["stock"]]
    assert sorted(p["n"] for p in two) == [6, 23] and [n % 4 for n in (6, 23)] == [2, 3]
    assert all(p["frames"] == (33 if pack in ("coins", "territory__inside_out") else 17) for p in two)
    pooled = [p for p in two if p["world_pool"] == 8]
    assert len(pooled) == 1 and set(pooled[0]["views"]) == {E.OBS_WORLD_RGB, E.OBS_LAYER}
    other = [p for p in two if p["world_pool"] == 1]
    assert len(other) == 1 and other[0]["views"] == (E.OBS_RGB,)
    assert sorted(p["unfused"] is True for p in two) == [False, True]
    if "in_the_matrix" not in pack and pack != "coins":
      assert sum(1 for p in two if p["num_players"]) == 1
    # the pack is the level's variant that pays often, where the parity tests have one
    raw = E.load_pack(pack)
    rich = pack in ("clean_up", "collaborative_cooking__cramped", "coop_mining", "gift_refinements",
                    "externality_mushrooms__dense", "prisoners_dilemma_in_the_matrix__repeated")
    assert (ap.rich_pack(pack, raw) != raw) == rich, pack
  stock = [p for p in profiles if p["stock"]]
  assert len(stock) == 1 and stock[0]["pack"] == "clean_up" and stock[0]["n"] == 23
  assert ap.profile_pack(stock[0]) == E.load_pack("clean_up")
  # both kinds of registration, the all-zeros mask, K = 65 and a read wider than the worlds occur
  ops = [op for name in STATE_IDS for op in _state_program(name)]
  assert {op["fresh"] for op in ops if op["op"] == "starts_set"} == {False, True}
  assert any(op.get("mask_form") == "zeros" for op in ops)
  assert any(op.get("K") == 65 and op.get("mask") is not None for op in ops)
  assert {op["mask_dtype"] for op in ops if op["op"] == "step_active"} == {"uint8", "bool", "list"}
  assert {op["until"] for op in ops if op["op"] == "many_until"} == set(ap.UNTILS)
  assert {op["gamma"] for op in ops if op["op"] == "many_until" and op["returns"]} == set(ap.GAMMAS)


@pytest.mark.parametrize("name", STATE_IDS)
def test_state_programs_are_deterministic_and_within_bounds(name):
  seed, profile = next((s, p) for s, p in ap.STATE_COMMITTED if p["name"] == name)
  prog, again = _state_program(name), ap.make_program(seed, profile)
  assert len(prog) == len(again) and all(_same_op(a, b) for a, b in zip(prog, again))
  assert prog[0]["op"] == "reset_all"
  assert {op["op"] for op in prog} == set(profile["classes"]) == set(ap.STATE_CLASSES)
  assert ap.STATE_MIN_OPS <= len(prog) <= ap.STATE_MAX_OPS
  assert ap.world_steps(prog) <= ap.STATE_MAX_WORLD_STEPS
  assert ap.longest_host_run(prog) >= ap.HOST_RUN
  adjacent = {(a["op"], b["op"]) for a, b in zip(prog[:-1], prog[1:])}
  assert set(ap.assigned_pairs(profile)) <= adjacent
  g = ap._geometry(profile)
  N, P, A = g["N"], g["P"], g["A"]
  banks, registered, wide = [], None, 0
  for op in prog:
    c = op["op"]
    if c in ("many_active", "many_until", "step_many_states"):
      K = op["K"]
      assert K in (ap.STATES_K if c == "step_many_states" else ap.STATE_K)
      lead = () if op["form"] == "repeat" else (K,)
      E.check_step_many(lead + (N, P) + ((A,) if op["fields"] else ()), op["actions"].dtype, N, P,
                        repeat=K if op["form"] == "repeat" else None, num_fields=A if op["fields"] else None)
      m = ap.op_mask(op, N)
      assert (m is None) == (op["mask_form"] == "none") and (m is None or m.shape == (K, N))
      assert c != "many_active" or m is not None
      if op["mask_form"] == "slice":
        assert op["mask"].shape == (K, N + 3) and 0 <= op["mlo"] <= 3
      if c == "many_until":
        E.check_step_until(N, P, until=op["until"], returns=op["returns"], gamma=op["gamma"])
        assert op["returns"] or op["gamma"] == 1.0
    if c == "step_active":
      assert op["actions"].shape == (N, P) and op["mask"].shape == (N,)
    if c in ("save", "step_many_states"):
      banks.append(len(op["worlds"]) if c == "save" else op["K"] * N)
    if c in ("load", "observe_rows", "observe_views", "check", "starts_set") or (c == "hash" and op["bank"] >= 0):
      assert 0 <= op["bank"] < len(banks)
    if c in ("starts_set", "starts_rows"):
      registered = banks[op["bank"]] if c == "starts_set" else registered
      rows = op["rows"]
      assert rows.shape == (N,) and rows.dtype == np.int32 and rows.min() == -1 and rows.max() < registered
      valid = rows[rows >= 0]
      assert len(valid) > len(set(valid.tolist())), "several worlds share one row"
    if c in ("observe_rows", "observe_views") or (c == "hash" and op["rows"] is not None):
      assert op["rows"].min() >= 0 and op["rows"].max() < banks[op["bank"]]
    if c == "observe_rows":
      wide += len(op["rows"]) > N
    if c == "observe_views":
      assert len(op["players"]) == len(op["rows"]) and op["players"].max() < P and 0 <= op["offset"] <= 15
      assert op["kind"] != E.OBS_WORLD_RGB
    if c == "check":
      assert 0 <= op["row"] < banks[op["bank"]]
  assert wide == 1, "one read of a program has more rows than worlds"


def test_every_pair_with_a_state_class_is_adjacent_somewhere():
  programs = [ap.make_program(s, p) for s, p in ap.COMMITTED] + [_state_program(n) for n in STATE_IDS]
  table = ap.pair_counts(programs, ap.STATE_CLASSES)
  print(ap.format_pair_table(table, ap.STATE_CLASSES))
  states = programs[len(ap.COMMITTED):]
  print("state programs: ops", sum(len(p) for p in states), "world-steps", sum(ap.world_steps(p) for p in states))
  idx = {c: i for i, c in enumerate(ap.STATE_CLASSES)}
  missing = [(a, b) for a in ap.MUTATING for b in ap.MUTATING if a != b and table[idx[a], idx[b]] == 0]
  assert not missing, missing
  missing = [(a, r) for a in ap.NEW_MUTATING for r in ap.READ_ONLY if table[idx[a], idx[r]] == 0]
  assert not missing, missing


def _level_cover(pack):
  total = collections.Counter()
  for n in ap.STATE_WORLD_COUNTS:
    total.update(_state_cover(f"{pack}-states-n{n}"))
  return total


def test_the_models_runs_hold_the_crossings_on_every_level():
  """Conditions on the inputs, by the model alone: what a level's two programs contain."""
  conditions = ap.COVER_CONDITIONS + (ap.DEAD_AVATAR_CONDITION,)
  print("| level | " + " | ".join(conditions) + " | inexact worlds at the end |")
  print("|---|" + "---|" * (len(conditions) + 1))
  covers = {pack: _level_cover(pack) for pack in ap.LEVEL_PACKS}
  for pack, cover in covers.items():
    print(f"| {pack} | " + " | ".join(str(cover[k]) for k in conditions) + f" | {cover['inexact worlds at the end']} of 29 |")
  for pack, cover in covers.items():
    for k in ap.COVER_CONDITIONS:
      assert cover[k] > 0, (pack, k)
    if pack in states_recipe.DEAD_AVATARS:
      assert cover[ap.DEAD_AVATAR_CONDITION] > 0, pack
    assert cover["inexact worlds at the end"] < 29, pack   # (the model still speaks for some world)


# the levels whose two programs hold the reward conditions (the search found seeds for all nine)
REWARD_LEVELS = ap.LEVEL_PACKS


def test_the_models_runs_pay_rewards_where_it_matters():
  print("| level | " + " | ".join(ap.REWARD_CONDITIONS) + " |")
  print("|---|" + "---|" * len(ap.REWARD_CONDITIONS))
  for pack in ap.LEVEL_PACKS:
    cover = _level_cover(pack)
    print(f"| {pack} | " + " | ".join(str(cover[k]) for k in ap.REWARD_CONDITIONS) + " |")
  assert len(REWARD_LEVELS) >= 6
  for pack in REWARD_LEVELS:
    cover = _level_cover(pack)
    for k in ap.REWARD_CONDITIONS:
      assert cover[k] > 0, (pack, k)


@pytest.mark.parametrize("name", ["coins-states-n6", "commons_harvest__open-states-n6",
                                  "prisoners_dilemma_in_the_matrix__repeated-states-n6"])
def test_the_model_equals_its_restatement_on_state_programs(name):
  prog = _state_program(name)
  profile = prog.profile
  a, b = ap.make_model(profile), ap.make_model(profile, ScratchModel)
  assert ap.run_program(prog, a, b) == len(prog)
  a.close(); b.close()


# ---- the runner against wrong models of the state classes
class SkippedWritesItsLeaves(ModelEngine):
  def _skipped(self, w, by_mask=True):
    super()._skipped(w, by_mask)
    if self._started[w]:
      self._write_transition(w, int(self._target(E.OBS_STEP_TYPE)[w]), np.zeros(self.P), [])


class StoppedRunsOneMoreStep(ModelEngine):
  _late = None

  def _stops(self, w, stop):
    self._late = {} if self._late is None else self._late
    now, before = super()._stops(w, stop), self._late.pop(w, 0)
    if now and not before:
      self._late[w] = now
    return before


class GammaCountsTheCallsSteps(ModelEngine):
  def _discount(self, g, gamma, k, w):
    out = np.float64(1.0)
    for _ in range(k + 1):
      out = out * np.float64(gamma)
    return out


class RowsAreReadAtRegistration(ModelEngine):
  def set_episode_starts(self, bank, rows, fresh=False):
    super().set_episode_starts(bank, np.array(rows), fresh)


class PausedOnLastNeverRestarts(ModelEngine):
  def _restart(self, w):
    if self._paused[w]:
      self._wrote_frozen(w)
    else:
      super()._restart(w)


class RestoreRewindsStopped(ModelEngine):
  _seen = _kept = None

  def step_many(self, actions, **kw):
    if kw.get("stopped") is not None:
      self._seen = kw["stopped"]
    return super().step_many(actions, **kw)

  def snapshot(self):
    self._kept = None if self._seen is None else self._seen.copy()
    return super().snapshot()

  def restore(self, snap):
    super().restore(snap)
    if self._seen is not None:
      self._seen[:] = 0 if self._kept is None else self._kept


class ObserveRowsLoadsWorldZero(ModelEngine):
  def observe_states(self, bank, kind, rows=None):
    first = bank[0] if rows is None else bank[int(np.asarray(rows)[0])]
    self._become(0, first)
    return super().observe_states(bank, kind, rows)


MASKED = ("step_active", "many_active", "many_until", "step_many_states")
# (wrong model, op classes at which it can first show, the state program that shows it)
WRONG_STATE_MODELS = [
    (SkippedWritesItsLeaves, MASKED, "clean_up-states-n6"),
    (StoppedRunsOneMoreStep, ("many_until",), "clean_up-states-n6"),
    (GammaCountsTheCallsSteps, ("many_until",), "externality_mushrooms__dense-states-n6"),
    (RowsAreReadAtRegistration, ap.ALL_STEP_CLASSES, "commons_harvest__open-states-n6"),
    (PausedOnLastNeverRestarts, ap.ALL_STEP_CLASSES, "clean_up-states-n6"),
    (RestoreRewindsStopped, ("restore",), "clean_up-states-n6"),
    (ObserveRowsLoadsWorldZero, ("observe_rows",), "clean_up-states-n6"),
]


def _state_trace(program, model):
  """What the runner looks at, after every op, of a model run alone (it does not know which worlds
  the model speaks for: a program in which a wrong model first shows in a world that took a
  fresh=True start is not one to choose)."""
  side = ap._Side(model)
  side.profile, side.states_banks = program.profile, {}
  out = []
  for op in program:
    op = ap.resolve(op, side)
    side.apply(op, 0)
    out.append((model.dump(), [model.observe_host(k) for k in model.scalar_kinds], side.rows, side.read,
                side.stopped.copy(), model.counters(), {k: np.array(v) for k, v in model._bound.items()}))
  return out


@pytest.mark.parametrize("wrong,classes,name", WRONG_STATE_MODELS, ids=[w[0].__name__ for w in WRONG_STATE_MODELS])
def test_the_runner_reports_a_wrong_state_model_at_its_first_op(wrong, classes, name):
  prog = _state_program(name)
  profile = prog.profile
  right, bad = _state_trace(prog, ap.make_model(profile)), _state_trace(prog, ap.make_model(profile, wrong))
  first = next((i for i, (x, y) in enumerate(zip(right, bad)) if not _equal(x, y)), None)
  assert first is not None, "this program never shows the wrong model: choose another"
  assert prog[first]["op"] in classes, (first, prog[first]["op"])
  with pytest.raises(ap.Mismatch) as err:
    ap.run_program(prog, ap.make_model(profile, wrong), ap.make_model(profile))
  text = str(err.value)
  assert f"program seed {prog.seed}, profile {name}, op {first}: {prog[first]['op']}" in text, text
  print(wrong.__name__, "->", text[:300])
  # a prefix that stops short of the op passes
  assert ap.run_program(prog, ap.make_model(profile, wrong), ap.make_model(profile), stop_after=first) == first


# ================================================================== the unit programs
# the state set pinned like the first: CRC-32 of every program's short forms and of its arguments' bytes
STATE_SET_CRCS = [
    3816710759, 4143868851, 217564662, 3440129169, 3437300365, 698209822, 2511290929, 4040866472, 596609386,
    3793023513, 1785998425, 3175777831, 696836456, 1997367625, 3823030810, 3758347594, 4222190984, 3078957703,
    2818926858]
STATE_SET_BYTES_CRCS = [
    691786250, 2652828220, 2620479898, 1658825342, 4229507520, 797941129, 171602092, 3414761698, 623677607,
    1590449189, 2444314014, 2489661867, 2185322165, 4027376909, 2679954219, 721275784, 537908407, 2502742082,
    3080636833]


def test_the_state_set_is_op_for_op_what_it_was():
  programs = [_state_program(n) for n in STATE_IDS]
  assert [zlib.crc32("\n".join(ap.short_form(op) for op in prog).encode()) for prog in programs] == STATE_SET_CRCS
  assert [_bytes_crc(prog) for prog in programs] == STATE_SET_BYTES_CRCS


UNIT_IDS = [p["name"] for _, p in ap.UNIT_COMMITTED]
# the bounds of a unit program: the state set's, but 80 ops at least — with 70 the search did not find
# totals that hold finished episodes at the end on coins and territory (their episodes are 33 frames), so
# the last stats_set of a program is followed by UNIT_STATS_TAIL ops
assert (ap.UNIT_MIN_OPS, ap.UNIT_MAX_OPS, ap.UNIT_MAX_WORLD_STEPS) == (80, 110, 260)
assert ap.UNIT_LAST_STATS_CLEAR < ap.UNIT_LAST_STATS_SET == ap.UNIT_MIN_OPS - ap.UNIT_STATS_TAIL


@functools.lru_cache(maxsize=None)
def _unit_program(name):
  seed, profile = next((s, p) for s, p in ap.UNIT_COMMITTED if p["name"] == name)
  return ap.make_program(seed, profile)


@functools.lru_cache(maxsize=None)
def _unit_cover(name):
  return ap.program_cover(_unit_program(name))


def test_the_unit_set_is_the_one_the_issue_names():
  profiles = [p for _, p in ap.UNIT_COMMITTED]
  assert len(set(UNIT_IDS)) == len(profiles) == 2 * len(ap.LEVEL_PACKS) + 1 == 19
  assert not set(UNIT_IDS) & (set(STATE_IDS) | {p["name"] for _, p in ap.COMMITTED})
  rings = 0
  for li, pack in enumerate(ap.LEVEL_PACKS):
    small, large = (next(p for p in profiles if p["name"] == f"{pack}-units-n{n}") for n in (6, 23))
    assert small["n"] == 6 and not small["ring"] and small["classes"] == ap.UNIT_CLASSES
    assert all(p["rich"] and p["auto_reset"] and p["frames"] == ap.LONG_EPISODES.get(pack, ap.EPISODE_FRAMES)
               for p in (small, large))
    assert bool(small["num_players"]) == ("in_the_matrix" not in pack and pack != "coins")
    if small["num_players"]:
      assert small["num_players"] == ap._geometry(large)["P"] - 1
    assert large["n"] == 23
    if large["ring"]:
      rings += 1
      assert large["ring"] == ap.RING_SLOTS and not set(large["classes"]) & set(ap.RING_REFUSED)
      assert set(large["classes"]) | set(ap.RING_REFUSED) == set(ap.UNIT_CLASSES)
      first = _unit_program(large["name"])[1]
      assert first["op"] == "step_listed" and first["refused"]
    else:
      assert large["world_pool"] == 8 and set(large["views"]) == {E.OBS_WORLD_RGB, E.OBS_LAYER}
      assert large["classes"] == ap.UNIT_CLASSES
    assert bool(large["ring"]) == bool(li % 2)   # the two forms alternate by level
  assert rings == 4
  stock = [p for p in profiles if p["stock"]]
  assert len(stock) == 1 and ap.profile_pack(stock[0]) == E.load_pack("clean_up") and stock[0]["classes"] == ap.UNIT_CLASSES
  ops = [op for name in UNIT_IDS for op in _unit_program(name)]
  listed = [op for op in ops if op["op"] in ap.LISTED_CLASSES and not op.get("refused")]
  share = sum(op["bad"] for op in listed) / len(listed)
  assert 0.1 < share < 0.4, share   # about one in four carries bad entries
  many = [op for op in listed if op["op"] == "many_listed"]
  assert {op["form"] for op in many} == {"plain", "repeat", "slice"} and {op["fields"] for op in many} == {False, True}
  assert {None if op["active"] is None else op["active"].ndim for op in many} == {None, 1, 2}
  assert {op["until"] for op in many} == set(ap.UNTILS) | {None}
  assert any(op["observations"] for op in many) and any(op["returns"] and op["gamma"] != 1.0 for op in many)
  sets = [op for op in ops if op["op"] == "stats_set"]
  assert {"default", ()} <= {op["columns"] for op in sets} and any("[" in "".join(op["columns"]) for op in sets)
  units = [op for op in ops if op["op"] == "units_set"]
  assert {n for op in units for n in op["units"]} == set(ap.UNIT_NAMES)
  assert {op["hash"]["classes"] is None for op in units if "hash" in op["units"]} == {False, True}
  planes = [op["planes"] for op in units if "planes" in op["units"]]
  assert {p["facing"] for p in planes} == {False, True} and {p["num_classes"] is None for p in planes} == {False, True}
  assert all((p["classes"] == -1).any() for p in planes) and len({p["offset"] for p in planes}) > 4
  reads = [op for op in ops if op["op"] == "unit_rows"]
  assert {op["unit"] for op in reads} == set(ap.UNIT_NAMES) and {op["bank"] < 0 for op in reads} == {False, True}
  assert {op["players"] is None for op in reads} == {False, True}


@pytest.mark.parametrize("name", UNIT_IDS)
def test_unit_programs_are_deterministic_and_within_bounds(name):
  seed, profile = next((s, p) for s, p in ap.UNIT_COMMITTED if p["name"] == name)
  prog, again = _unit_program(name), ap.make_program(seed, profile)
  assert len(prog) == len(again) and all(_equal(a, b) for a, b in zip(prog, again))   # (an op may nest a dict)
  assert prog[0]["op"] == "reset_all"
  assert {op["op"] for op in prog if not op.get("refused")} == set(profile["classes"])
  assert ap.UNIT_MIN_OPS <= len(prog) <= ap.UNIT_MAX_OPS
  assert ap.world_steps(prog) <= ap.UNIT_MAX_WORLD_STEPS
  assert ap.longest_host_run(prog) >= ap.HOST_RUN
  adjacent = {(a["op"], b["op"]) for a, b in zip(prog[:-1], prog[1:])}
  assert set(ap.assigned_pairs(profile)) <= adjacent
  g = ap._geometry(profile)
  N, P, A = g["N"], g["P"], g["A"]
  banks, wide, live = [], 0, set()
  for op in prog:
    c = op["op"]
    if c in ("save", "step_many_states"):
      banks.append(len(op["worlds"]) if c == "save" else op["K"] * N)
    if c in ap.LISTED_CLASSES:
      w = op["worlds"]
      M = len(w)
      assert w.dtype == np.int32 and 1 <= M <= N
      inside = w[(w >= 0) & (w < N)]
      assert op["bad"] == (len(inside) < M) == (len(set(inside.tolist())) < len(inside))   # both kinds, or neither
      E.check_step_listed(w, N, P)
      if c == "step_listed":
        assert op["actions"].shape == (M, P)
      else:
        K = op["K"]
        assert K in ap.STATE_K
        lead = () if op["form"] == "repeat" else (K,)
        E.check_step_listed(w, N, P, actions=np.zeros(lead + (M, P) + ((A,) if op["fields"] else ()), np.int32),
                            repeat=K if op["form"] == "repeat" else None, num_fields=A if op["fields"] else None,
                            active=op["active"])
        assert op["actions"].shape == lead + (M + 3 if op["form"] == "slice" else M, P) + ((A,) if op["fields"] else ())
        if op["until"] is not None:
          E.check_step_until(N, P, until=op["until"], gamma=op["gamma"])
        assert op["returns"] or op["gamma"] == 1.0
    if c == "stats_set":
      cols = g["columns"][0] if op["columns"] == "default" else op["columns"]
      for name_ in tuple(cols) + tuple(op["pairs"]):
        E.parse_event_column(name_)
      assert len(op["pairs"]) == (0 if profile["pack"] in ap.NO_BEAM else 1)
    if c == "units_set":
      assert op["units"] and set(op["units"]) <= set(ap.UNIT_NAMES)
      live |= set(op["units"])
      if "planes" in op["units"]:
        p = op["planes"]
        C = int(p["classes"].max()) + 1 if p["num_classes"] is None else p["num_classes"]
        assert p["classes"].shape == (g["ids"],) and p["classes"].min() == -1 and p["classes"].max() < C <= 64
        assert 0 <= p["offset"] <= 15
      if "hash" in op["units"]:
        h = op["hash"]
        assert (h["layers"] is None and h["classes"] is None) or h["classes"].shape == (g["ids"],)
    if c == "units_clear":
      assert op["unit"] in live
      live.discard(op["unit"])
    if c == "unit_rows":
      there = N if op["bank"] < 0 else banks[op["bank"]]
      assert op["rows"].min() >= 0 and op["rows"].max() < there
      assert op["players"] is None or (len(op["players"]) == len(op["rows"]) and op["players"].max() < P)
      wide += len(op["rows"]) > N
  assert wide == 1, "one unit read of a program has more rows than worlds"


def test_every_pair_with_a_unit_class_is_adjacent_somewhere():
  programs = [_unit_program(n) for n in UNIT_IDS]
  table = ap.pair_counts(programs, ap.UNIT_CLASSES)
  print(ap.format_pair_table(table, ap.UNIT_CLASSES))
  print("unit programs: ops", sum(len(p) for p in programs), "world-steps", sum(ap.world_steps(p) for p in programs))
  idx = {c: i for i, c in enumerate(ap.UNIT_CLASSES)}
  missing = [(a, b) for a, b in ap.required_unit_pairs() if table[idx[a], idx[b]] == 0]
  assert not missing, missing
  assert len(ap.required_unit_pairs()) == 27 * 26 - 21 * 20 + 6


# what a level cannot hold by its rules (at most two a level; none of the listed-step conditions, nor
# the restore-then-skip one)
UNIT_EXEMPT = {pack: [] for pack in ap.LEVEL_PACKS}
for _pack in ap.LEVEL_PACKS:
  if _pack not in states_recipe.DEAD_AVATARS + ("territory__inside_out",):
    UNIT_EXEMPT[_pack].append((ap.UNIT_DEAD_VIEWER, "no rule of the level takes an avatar off the map"))
  if _pack in ap.NO_BEAM:
    UNIT_EXEMPT[_pack].append(("non-zero total.pairs at the end", "the level has no two-player event: no pair column"))
# (an interaction takes two players who have both collected a resource and then meet and fire: six
# worlds of the programs' weighted random play held none in 300 steps with no episode end at all, more
# than the 260 world-steps of a whole program — no MAXFRAMES and no bound near the set's reaches one)
UNIT_EXEMPT["prisoners_dilemma_in_the_matrix__repeated"].append(
    ("non-zero total.pairs at the end", "random play does not reach an interaction within a program's world-steps"))
NEVER_EXEMPT = tuple(k for k in ap.UNIT_COVER_CONDITIONS if "listed" in k or "skipped that world" in k)


def _unit_level_cover(pack):
  total = collections.Counter()
  for n in (6, 23):
    total.update(_unit_cover(f"{pack}-units-n{n}"))
  return total


def test_the_models_runs_hold_the_unit_crossings_on_every_level():
  import ego_layer_model
  conditions = ap.UNIT_COVER_CONDITIONS + (ap.UNIT_DEAD_VIEWER, ap.UNIT_OFF_THE_MAP)
  print("| level | " + " | ".join(conditions) + " |")
  print("|---|" + "---|" * len(conditions))
  covers = {pack: _unit_level_cover(pack) for pack in ap.LEVEL_PACKS}
  for pack, cover in covers.items():
    print(f"| {pack} | " + " | ".join(str(cover[k]) for k in conditions) + " |")
  assert len(NEVER_EXEMPT) == 5
  for pack, cover in covers.items():
    exempt = [k for k, _ in UNIT_EXEMPT[pack]]
    assert len(exempt) <= 2 and not set(exempt) & set(NEVER_EXEMPT)
    torus = ego_layer_model.geometry(E.load_pack(pack))[4]
    for k in conditions:
      if k in exempt or (k == ap.UNIT_OFF_THE_MAP and torus):
        continue
      assert cover[k] > 0, (pack, k)


def test_the_model_equals_its_restatement_on_a_unit_program():
  prog = _unit_program("clean_up-units-n6")
  profile = prog.profile
  a, b = ap.make_model(profile), ap.make_model(profile, ScratchModel)
  assert ap.run_program(prog, a, b) == len(prog)
  a.close(); b.close()


def test_a_ring_unit_program_runs_model_against_model():
  prog = _unit_program("coins-units-n23")
  profile = prog.profile
  assert profile["ring"] == ap.RING_SLOTS
  a, b = ap.make_model(profile), ap.make_model(profile)
  assert ap.run_program(prog, a, b) == len(prog)
  assert a.ring["slots"] == ap.RING_SLOTS and a.units
  a.close(); b.close()


# ---- the runner against wrong models of the unit classes
class SkippedWorldsViewIsLeftAlone(ModelEngine):
  """(as a bound LAYER's element is)"""
  def _unit_worlds(self):
    return range(self.N) if self._touched is None else sorted(self._touched)


class RestoreRedrawsTheUnits(ModelEngine):
  def restore(self, snap):
    super().restore(snap)
    self._draw_units()


class RepeatedEntryStepsItsWorldTwice(ModelEngine):
  def _listed(self, a, worlds, out, kw):
    res = super()._listed(a, worlds, out, dict(kw))
    worlds = np.asarray(worlds)
    owned = {i for i, _ in self._owners(worlds)}
    again = [i for i, w in enumerate(worlds.tolist()) if 0 <= w < self.N and i not in owned]
    if again:
      act = kw.get("active")
      super()._listed(a[again] if kw.get("repeat") is not None else a[:, again], worlds[again], None,
                      dict(kw, active=None if act is None else np.asarray(act)[..., again], stopped=None, until=None,
                           returns=False, keep=(), events=False, observations=()))
    return res


class StoppedIsIndexedByEntry(ModelEngine):
  def _stopped_at(self, i, w):
    return i


class BadEntrysRanIsZero(ModelEngine):
  def _bad_ran(self, before):
    return 0


class LoadCutCountsIntoTotal(ModelEngine):
  def _cut(self, v, how):
    super()._cut(v, how)
    if how == "load":
      st = self.stats
      for key in st.running:
        st.total[key][v] = st.total[key][v] + st.running[key][v]

  def _finished_after_cut(self, v, own):   # (the right model asserts here that the cut sums are nowhere)
    pass


class StatisticsFoldASkippedStep(ModelEngine):
  def _skipped(self, w, by_mask=True):
    super()._skipped(w, by_mask)
    if self._started[w]:
      self._fold(w)


class ListedStatisticsGoToTheEntry(ModelEngine):
  def _stats_world(self, w):
    return w if self._credit is None else self._credit[w]


SKIPPING = ("step_active", "many_active", "many_until", "step_many_states") + ap.LISTED_CLASSES
# (wrong model, op classes at which it can first show, the unit program that shows it)
WRONG_UNIT_MODELS = [
    (SkippedWorldsViewIsLeftAlone, SKIPPING, "clean_up-units-n6"),
    (RestoreRedrawsTheUnits, ("restore",), "clean_up-units-n6"),
    (RepeatedEntryStepsItsWorldTwice, ap.LISTED_CLASSES, "clean_up-units-n6"),
    (StoppedIsIndexedByEntry, ("many_listed",), "clean_up-units-n6"),
    (BadEntrysRanIsZero, ("many_listed",), "commons_harvest__open-units-n6"),
    (LoadCutCountsIntoTotal, ("load",), "clean_up-units-n6"),
    (StatisticsFoldASkippedStep, SKIPPING, "clean_up-units-n6"),
    (ListedStatisticsGoToTheEntry, ap.LISTED_CLASSES, "clean_up-units-n6"),
]


def _unit_trace(program, model):
  """What the runner looks at, after every op, of a model run alone: the state trace's, the
  statistics and the registered tensors."""
  import episode_stats_model
  side = ap._Side(model)
  side.profile, side.states_banks = program.profile, {}
  out = []
  for op in program:
    op = ap.resolve(op, side)
    side.apply(op, program.profile["ring"])
    stats = None if model.stats is None else {k: np.array(ap._bits(v)) for k, v in
                                              episode_stats_model.flatten(model.stats.arrays()).items()}
    out.append((model.dump(), [model.observe_host(k) for k in model.scalar_kinds], side.rows, side.read,
                side.stopped.copy(), model.counters(), {k: np.array(v) for k, v in model._bound.items()},
                stats, {n: np.array(u["out"]) for n, u in side.units.items()}))
  return out


@pytest.mark.parametrize("wrong,classes,name", WRONG_UNIT_MODELS, ids=[w[0].__name__ for w in WRONG_UNIT_MODELS])
def test_the_runner_reports_a_wrong_unit_model_at_its_first_op(wrong, classes, name):
  prog = _unit_program(name)
  profile = prog.profile
  right, bad = _unit_trace(prog, ap.make_model(profile)), _unit_trace(prog, ap.make_model(profile, wrong))
  first = next((i for i, (x, y) in enumerate(zip(right, bad)) if not _equal(x, y)), None)
  assert first is not None, "this program never shows the wrong model: choose another"
  assert prog[first]["op"] in classes, (first, prog[first]["op"])
  with pytest.raises(ap.Mismatch) as err:
    ap.run_program(prog, ap.make_model(profile, wrong), ap.make_model(profile))
  text = str(err.value)
  assert f"program seed {prog.seed}, profile {name}, op {first}: {prog[first]['op']}" in text, text
  print(wrong.__name__, "->", text[:300])
  # a prefix that stops short of the op passes
  assert ap.run_program(prog, ap.make_model(profile, wrong), ap.make_model(profile), stop_after=first) == first
