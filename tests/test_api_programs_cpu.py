"""The program tests without a GPU: the generator's promises, the coverage of the committed set, the
model against an independent restatement of itself, and the runner against deliberately wrong
models — each must be reported at the first op where it can show."""
import numpy as np
import pytest

import api_programs as ap
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

  def step(self, actions):
    a = np.asarray(actions, np.int32)
    for w in range(self.N):
      self._hist[w].append(("step", a[w].copy()))
    super().step(a)

  def step_fields(self, fields):
    f = np.asarray(fields, np.int32)
    for w in range(self.N):
      self._hist[w].append(("fields", f[w].copy()))
    super().step_fields(f)

  def step_many(self, actions, *, repeat=None, fields=False, events=False, observations=(),
                keep=("reward", "collective_reward", "step_type", "discount")):
    assert not self._slots
    a = np.asarray(actions, np.int32)
    K = int(repeat) if repeat is not None else a.shape[0]
    keys = list(keep) + (["events"] if events else []) + [int(k) for k in observations]
    rows = {key: [] for key in keys}
    for k in range(K):
      (self.step_fields if fields else self.step)(a if repeat is not None else a[k])
      for key in keys:
        rows[key].append(self.observe_host(E.STEP_MANY_NAMES.get(key, key)))
    return {key: np.stack(v) for key, v in rows.items()}

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
