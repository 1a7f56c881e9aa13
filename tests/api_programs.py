"""Test infrastructure: seeded random PROGRAMS of engine API calls, and the runner that executes one
on an `engine.Engine` and on the oracle-backed model of tests/engine_model.py (and on a twin
engine with another launch form), comparing after every call.

`make_program(seed, profile)` writes the program: a list of ops (dicts with concrete numpy
arguments), deterministic, no GPU code.  `run_program(program, engine, model, twin)` applies each op
to all of them; "engine" is only an interface here (reset / step / step_fields / step_many /
save_worlds / load_worlds / snapshot / restore / bind / bind_ring / unbind / observe_host / dump /
counters / fault_words / ring / _bound), which the model satisfies too — so the CPU suite runs the
runner model against model, and against deliberately wrong models."""
import zlib

import numpy as np

from meltingpot_amd import engine as E
from meltingpot_amd import pack as pack_lib
import engine_model
import util

OP_CLASSES = ("reset_all", "masked_reset", "masked_reseed", "step_dev", "step_host", "step_fields",
              "step_many", "step_many_rows", "save", "load", "snapshot", "restore", "rebind")
STEP_CLASSES = ("step_dev", "step_host", "step_fields", "step_many", "step_many_rows")
MIN_OPS, MAX_OPS, MAX_WORLD_STEPS = 40, 60, 150
MANY_K = (1, 2, 7, 33)
HOST_RUN = 5            # host steps in a row: the ring of four pinned action buffers wraps
EPISODE_FRAMES = 17     # MAXFRAMES of the patched packs: episodes end inside every program
RING_SLOTS = 3

# one pack per level
LEVEL_PACKS = ("clean_up", "coins", "collaborative_cooking__cramped", "commons_harvest__open",
               "coop_mining", "externality_mushrooms__dense", "gift_refinements",
               "territory__inside_out", "prisoners_dilemma_in_the_matrix__repeated")
WORLD_COUNTS = (5, 13, 37)
INITIAL_VIEWS = ((), (E.OBS_RGB,), (E.OBS_WORLD_RGB, E.OBS_LAYER))


def _profiles():
  out = []
  for li, pack in enumerate(LEVEL_PACKS):
    hdr = pack_lib.loads(E.load_pack(pack))["hdr"]
    default_p = int(hdr[20]) or int(hdr[7])
    fewer = "in_the_matrix" not in pack and pack != "coins"   # (levels that allow fewer players)
    for j, n in enumerate(WORLD_COUNTS):
      out.append(dict(
          name=f"{pack}-n{n}", pack=pack, stock=False, n=n,
          ring=RING_SLOTS if j == li % 3 else 0,
          world_pool=8 if j == (li + 1) % 3 else 1,
          auto_reset=(li + j) % 2 == 0,
          unfused=True if (li + j) % 3 == 1 else None,
          num_players=max(1, default_p - 1) if fewer and j == (li + 2) % 3 else 0,
          views=INITIAL_VIEWS[(li + j) % 3]))
  # the committed clean_up pack, unpatched: the kernels with its constants compiled in
  out.append(dict(name="stock_clean_up-n13", pack="clean_up", stock=True, n=13, ring=0, world_pool=1,
                  auto_reset=True, unfused=None, num_players=0, views=(E.OBS_WORLD_RGB,)))
  out.append(dict(name="stock_clean_up-n37", pack="clean_up", stock=True, n=37, ring=RING_SLOTS,
                  world_pool=1, auto_reset=True, unfused=None, num_players=0, views=(E.OBS_RGB,)))
  return out


PROFILES = _profiles()
# the committed set: (program seed, profile), chosen so that every ordered pair of distinct op
# classes is adjacent somewhere in it (tests/test_api_programs_cpu.py prints the table)
COMMITTED = [(1000 + i, p) for i, p in enumerate(PROFILES)]


def profile_pack(profile):
  raw = E.load_pack(profile["pack"])
  return raw if profile["stock"] else util.patch_pack(raw, MAXFRAMES=EPISODE_FRAMES)


def bound_scalars(profile):
  """The scalar kinds a program's engines bind before the first reset (in place, or as ring kinds
  in a ring profile): two kinds every path of a started world writes, and one a frozen world does
  not — in a ring its slot then keeps the bytes it had, the carry rule per slot."""
  return (E.OBS_STEP_TYPE, E.OBS_REWARD, E.OBS_POSITION)


class Program(list):
  """The ops of one program, with the (seed, profile) it was made from."""
  seed = None
  profile = None


def _geometry(profile):
  t = pack_lib.loads(E.load_pack(profile["pack"]))
  hdr = t["hdr"]
  P = profile["num_players"] or int(hdr[20]) or int(hdr[7])
  A = int(hdr[21])
  spec = np.asarray(t["action_spec"]).reshape(-1, 3)[:A]
  R = ((len(t["mx_states"]) - 8) // 2 if "mx_states" in t else int(t["gr_i32"][7]) if "gr_i32" in t else 0)
  kinds = [E.OBS_LAYER, E.OBS_POSITION, E.OBS_ORIENTATION, E.OBS_READY_TO_SHOOT] + ([E.OBS_INVENTORY] if R else [])
  return dict(N=profile["n"], P=P, A=A, nact=len(np.asarray(t["action_table"]).reshape(-1, 4)),
              lo=spec[:, 0].astype(np.int32), hi=spec[:, 1].astype(np.int32), row_kinds=kinds)


def _ids(rng, g, shape, bad=0.0):
  a = rng.integers(0, g["nact"], size=shape, dtype=np.int32)
  if bad:
    out = rng.choice(np.array([-1, g["nact"], g["nact"] + 3, -5, 100], np.int32), size=shape)
    a = np.where(rng.random(shape) < bad, out, a).astype(np.int32)
  return a


def _fields(rng, g, shape):
  return rng.integers(g["lo"], g["hi"] + 1, size=tuple(shape) + (g["A"],), dtype=np.int32)


def _attempt(rng, profile, g):
  N, P = g["N"], g["P"]
  length = int(rng.integers(MIN_OPS, MAX_OPS + 1))
  ops = [dict(op="reset_all")]
  budget, banks, have_snap, host_run_done = MAX_WORLD_STEPS, [], False, False
  bound = set(profile["views"])
  pooled = int(rng.choice(list(E.OBS_RGB_POOL.values())))
  agent_kinds = (E.OBS_RGB, pooled)
  while len(ops) < length:
    allowed = [c for c in OP_CLASSES if c != ops[-1]["op"] and
               not (c == "load" and not banks) and not (c == "restore" and not have_snap) and
               not (c in STEP_CLASSES and budget < 1) and
               not (c == "step_host" and not host_run_done and (budget < HOST_RUN or len(ops) + HOST_RUN > length))]
    c = str(rng.choice(allowed))
    if c == "reset_all":
      ops.append(dict(op=c))
    elif c in ("masked_reset", "masked_reseed"):
      mask = (rng.random(N) < 0.4).astype(np.uint8)
      mask[rng.integers(N)] = 1
      op = dict(op=c, mask=mask)
      if c == "masked_reseed":
        op["seeds"] = rng.integers(1, 1 << 62, size=N, dtype=np.uint64)
      ops.append(op)
    elif c == "step_dev":
      ops.append(dict(op=c, actions=_ids(rng, g, (N, P), bad=0.01)))
      budget -= 1
    elif c == "step_host":
      run = 1 if host_run_done else HOST_RUN + int(rng.integers(0, 2))
      run = min(run, budget, length - len(ops))
      for _ in range(run):
        ops.append(dict(op=c, actions=_ids(rng, g, (N, P))))
      budget -= run
      host_run_done = host_run_done or run >= HOST_RUN
    elif c == "step_fields":
      ops.append(dict(op=c, fields=_fields(rng, g, (N, P)), host=bool(rng.integers(2))))
      budget -= 1
    elif c in ("step_many", "step_many_rows"):
      ks = [k for k in MANY_K if k <= budget]
      K = int(rng.choice(ks, p=np.array([3, 3, 3, 1][:len(ks)]) / sum([3, 3, 3, 1][:len(ks)])))
      form = str(rng.choice(["plain", "repeat", "slice"], p=[0.5, 0.25, 0.25]))
      fields = bool(rng.random() < 0.25)
      lead = () if form == "repeat" else (K,)
      wide = N + 3 if form == "slice" else N
      acts = _fields(rng, g, lead + (wide, P)) if fields else _ids(rng, g, lead + (wide, P), bad=0.01)
      op = dict(op=c, K=K, form=form, fields=fields, actions=acts, lo=int(rng.integers(0, 4)) if form == "slice" else 0)
      if c == "step_many_rows":
        pick = rng.random(len(g["row_kinds"])) < 0.5
        pick[rng.integers(len(pick))] = True
        op["observations"] = tuple(int(k) for k, p in zip(g["row_kinds"], pick) if p)
      ops.append(op)
      budget -= K
    elif c == "save":
      m = int(rng.integers(1, N + 1))
      ops.append(dict(op=c, worlds=rng.choice(N, size=m, replace=False).astype(np.int32)))
      banks.append(m)
    elif c == "load":
      b = int(rng.integers(len(banks)))
      src = rng.integers(0, banks[b], size=N).astype(np.int32)   # (with duplicates)
      src[rng.random(N) < 0.3] = -1
      i, j = rng.choice(N, size=2, replace=False)
      src[i], src[j] = -1, int(rng.integers(banks[b]))
      ops.append(dict(op=c, bank=b, src=src))
    elif c == "snapshot":
      ops.append(dict(op=c))
      have_snap = True
    elif c == "restore":
      ops.append(dict(op=c))
    elif c == "rebind":
      kind = int(rng.choice([E.OBS_RGB, pooled, E.OBS_WORLD_RGB, E.OBS_LAYER]))
      other = [k for k in agent_kinds if k != kind and k in bound]
      if kind in bound:
        bind = False
      elif kind in agent_kinds and other:   # one per-agent view at a time: the other one leaves
        kind, bind = other[0], False
      else:
        bind = True
      (bound.add if bind else bound.discard)(kind)
      ops.append(dict(op=c, kind=kind, bind=bind))
  return ops


def world_steps(program):
  return sum(op.get("K", 1) for op in program if op["op"] in STEP_CLASSES)


def longest_host_run(program):
  best = run = 0
  for op in program:
    run = run + 1 if op["op"] == "step_host" else 0
    best = max(best, run)
  return best


def make_program(seed, profile):
  """The program of (seed, profile): deterministic; the first draw that holds every op class."""
  g = _geometry(profile)
  for attempt in range(1000):
    rng = np.random.default_rng([int(seed), zlib.crc32(profile["name"].encode()), attempt])
    ops = _attempt(rng, profile, g)
    if {op["op"] for op in ops} == set(OP_CLASSES) and longest_host_run(ops) >= HOST_RUN:
      prog = Program(ops)
      prog.seed, prog.profile = int(seed), profile
      return prog
  raise AssertionError(f"no program for seed {seed}, profile {profile['name']}")


def pair_counts(programs):
  """[from, to] counts of adjacent op classes over `programs`."""
  idx = {c: i for i, c in enumerate(OP_CLASSES)}
  table = np.zeros((len(OP_CLASSES),) * 2, np.int64)
  for prog in programs:
    for a, b in zip(prog[:-1], prog[1:]):
      table[idx[a["op"]], idx[b["op"]]] += 1
  return table


def format_pair_table(table):
  short = [c.replace("step_", "s_").replace("masked_", "m_") for c in OP_CLASSES]
  lines = ["| from \\ to | " + " | ".join(short) + " |", "|---|" + "---|" * len(short)]
  for i, c in enumerate(short):
    lines.append(f"| {c} | " + " | ".join("." if i == j else str(int(v)) for j, v in enumerate(table[i])) + " |")
  return "\n".join(lines)


# ------------------------------------------------------------------------------------ the runner

def short_form(op):
  """An op's class and arguments, short enough for an assertion message."""
  parts = [op["op"]]
  for k, v in op.items():
    if k == "op":
      continue
    if isinstance(v, np.ndarray):
      parts.append(f"{k}={v.tolist()}" if v.size <= 40 else f"{k}=<{v.dtype}{list(v.shape)}>")
    else:
      parts.append(f"{k}={v}")
  return " ".join(parts)


class Mismatch(AssertionError):
  pass


class FaultStop(AssertionError):
  """A fault word is set: the run stops, nothing more is launched."""


def _host(x):
  return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _zero(x):
  x.zero_() if hasattr(x, "zero_") else x.fill(0)
  return x


def bind_view(eng, kind, ring):
  """Binds `kind` to a zeroed buffer (a ring of `ring` slots, or in place)."""
  return _zero(eng.bind_ring(kind, slots=ring, tune=False) if ring else eng.bind(kind))


def canonical_events(rows):
  """EVENTS blocks [..., EVENT_ROWS, 4] -> per block (count, dropped, sorted counted rows)."""
  rows = np.asarray(rows).reshape(-1, E.EVENT_ROWS, 4)
  return [(int(r[0, 0]), int(r[0, 1]), sorted(map(tuple, r[1:1 + int(r[0, 0])].tolist()))) for r in rows]


def first_difference(kind, got, want, leading=("world",)):
  """None, or where `got` and `want` first differ, as text."""
  got, want = np.asarray(got), np.asarray(want)
  if kind in (E.OBS_EVENTS, "events"):
    a, b = canonical_events(got), canonical_events(want)
    per = int(np.prod(got.shape[:-2])) // got.shape[0] if got.ndim > 3 else 1
    for i, (x, y) in enumerate(zip(a, b)):
      if x != y:
        where = f"step {i // per} world {i % per}" if got.ndim > 3 else f"world {i}"
        return f"{where}: (count, dropped, rows) {x} != {y}"
    return None
  if got.shape != want.shape:
    return f"shape {got.shape} != {want.shape}"
  if np.array_equal(got, want):
    return None
  at = np.argwhere(got != want)[0]
  names = list(leading) + ["index"] * (len(at) - len(leading))
  head = ", ".join(f"{n} {int(v)}" for n, v in zip(names[:len(leading)], at[:len(leading)]))
  return f"{head}, index {at[len(leading):].tolist()}: {got[tuple(at)]!r} != {want[tuple(at)]!r}"


class _Side:
  """One engine of a run and what the program keeps for it."""

  def __init__(self, eng):
    self.eng = eng
    self.banks = []
    self.snap = None
    self.rows = None     # what the last step_many returned

  def dev(self, a):
    if hasattr(self.eng, "to_device"):
      return self.eng.to_device(a)
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)

  def apply(self, op, ring, views=True):
    eng, c = self.eng, op["op"]
    self.rows = None
    if c == "reset_all":
      eng.reset()
    elif c == "masked_reset":
      eng.reset(None, op["mask"])
    elif c == "masked_reseed":
      eng.reset(op["seeds"], op["mask"])
    elif c == "step_dev":
      eng.step(self.dev(op["actions"]))
    elif c == "step_host":
      eng.step(op["actions"])
    elif c == "step_fields":
      eng.step_fields(op["fields"] if op["host"] else self.dev(op["fields"]))
    elif c in ("step_many", "step_many_rows"):
      acts = self.dev(op["actions"])
      if op["form"] == "slice":   # a column slice of a wider tensor: non-contiguous along K only
        acts = acts[:, op["lo"]:op["lo"] + eng.N]
      kw = dict(fields=op["fields"], repeat=op["K"] if op["form"] == "repeat" else None)
      if c == "step_many_rows":
        kw.update(events=True, observations=op["observations"])
      self.rows = {k: _host(v) for k, v in eng.step_many(acts, **kw).items()}
    elif c == "save":
      self.banks.append(eng.save_worlds(op["worlds"]))
    elif c == "load":
      eng.load_worlds(self.banks[op["bank"]], op["src"])
    elif c == "snapshot":
      self.snap = eng.snapshot()
    elif c == "restore":
      eng.restore(self.snap)
    elif c == "rebind":
      if views:
        bind_view(eng, op["kind"], ring) if op["bind"] else eng.unbind(op["kind"])
    else:
      raise ValueError(c)


def _check_faults(eng, where):
  words = np.asarray(eng.fault_words()[:6])
  if words.any():
    raise FaultStop(f"{where}: fault words {words.tolist()}; nothing more is launched")


def compare_with_model(eng, model, rows, model_rows, fail):
  """Everything the model speaks about, engine against model; `fail(kind, text)` raises."""
  for name, got, want in zip(("record grid", "record avatars", "record globals"), eng.dump(), model.dump()):
    d = first_difference(name, got, want)
    if d:
      fail(name, d)
  for kind in model.scalar_kinds:
    d = first_difference(kind, eng.observe_host(kind), model.observe_host(kind))
    if d:
      fail(f"kind {kind}", d)
  if (rows is None) != (model_rows is None) or (rows is not None and set(rows) != set(model_rows)):
    fail("step_many rows", f"keys {rows and sorted(map(str, rows))} != {model_rows and sorted(map(str, model_rows))}")
  for key in rows or ():
    d = first_difference(key, rows[key], model_rows[key], leading=("step", "world"))
    if d:
      fail(f"step_many row {key}", d)
  got, want = eng.counters()["bad_actions"], model.counters()["bad_actions"]
  if got != want:
    fail("bad_actions", f"{got} != {want}")
  if dict(eng.ring) != dict(model.ring):
    fail("ring position", f"{dict(eng.ring)} != {dict(model.ring)}")
  for kind, want in model._bound.items():
    # (a ring kind: every slot — the one written last holds the model's, the others did not change)
    ring_kind = np.asarray(want).ndim == len(model.shapes[kind][0]) + 1
    d = first_difference(kind, _host(eng._bound[kind]), want, leading=("slot", "world") if ring_kind else ("world",))
    if d:
      fail(f"{'ring' if ring_kind else 'bound'} kind {kind} (last slot {eng.ring['last']})", d)


def compare_views_with_model(eng, model, fail, kinds=engine_model.VIEW_KINDS):
  """Every view kind drawn by mp_observe from the records, against the model's."""
  for kind in kinds:
    d = first_difference(kind, eng.observe_host(kind), model.view_value(kind))
    if d:
      fail(f"observed kind {kind}", d)


def produced_kinds(eng):
  return [k for k in range(E.OBS_RGB_POOL8 + 1) if eng._L.mp_obs_bytes(eng._h, k) > 0]


def compare_with_twin(eng, twin, locate, fail):
  """EVERY output kind the level produces, and the saved records without the counters' bytes,
  byte-identical between two engines of different launch forms (the carry-rule kinds included)."""
  import torch
  from test_gpu_world_states import _no_counters
  for kind in produced_kinds(eng):
    a, b = eng.observe(kind), twin.observe(kind)
    if kind == E.OBS_EVENTS:
      d = first_difference(kind, _host(a), _host(b))
    else:
      d = None if torch.equal(a, b) else first_difference(kind, _host(a), _host(b))
    if d:
      fail(f"twin: kind {kind}", d)
  a, b = _no_counters(eng.save_worlds(), locate), _no_counters(twin.save_worlds(), locate)
  if not torch.equal(a, b):
    fail("twin: save_worlds", first_difference("rows", _host(a), _host(b), leading=("world",)))


def run_program(program, engine, model, twin=None, stop_after=None):
  """Applies each op of `program` (its first `stop_after`, if given) to `engine`, `model` and
  `twin`, comparing after every op; raises Mismatch / FaultStop naming seed, profile, op and kind.
  Returns the number of ops run."""
  profile = program.profile
  ring = profile["ring"]
  sides = [_Side(engine), _Side(model)] + ([_Side(twin)] if twin is not None else [])
  locate = None
  ran = 0
  for i, op in enumerate(program[:stop_after]):
    where = f"program seed {program.seed}, profile {profile['name']}, op {i}: {short_form(op)}"

    def fail(kind, text):
      raise Mismatch(f"{where}: {kind}: {text}")

    for k, side in enumerate(sides):
      side.apply(op, ring, views=k < 2)   # (the twin binds no view)
    # (dump synchronises; a fault word ends the run before anything else is launched)
    engine.dump()
    _check_faults(engine, where)
    if twin is not None:
      twin.dump()
      _check_faults(twin, where + " (twin)")
    compare_with_model(engine, model, sides[0].rows, sides[1].rows, fail)
    if op["op"] in ("load", "restore"):   # (mp_observe draws from the records: a restore is no launch)
      compare_views_with_model(engine, model, fail)
    if twin is not None:
      if locate is None:   # (world 0 still has its first seed: it locates the counters' bytes)
        locate = engine.save_worlds().clone()
      compare_with_twin(engine, twin, locate, fail)
    ran += 1
  if ran:
    compare_views_with_model(engine, model, fail)
    _check_faults(engine, "end of program")
  return ran


# ------------------------------------------------------------------------- engines of a profile

def make_model(profile, cls=engine_model.ModelEngine):
  model = cls(profile_pack(profile), profile["n"], auto_reset=profile["auto_reset"],
              num_players=profile["num_players"], world_pool=profile["world_pool"])
  for kind in bound_scalars(profile) + tuple(profile["views"]):
    bind_view(model, kind, profile["ring"])
  return model


def make_engines(profile):
  """(engine, twin) of a profile on the GPU: the twin has the same pack, seeds and scalar
  bindings but the other launch form — unfused, the generic kernels, no view bound."""
  kw = dict(device=0, auto_reset=profile["auto_reset"], num_players=profile["num_players"],
            world_pool=profile["world_pool"], debug_observations=True)
  pack = profile_pack(profile)
  eng = E.Engine(pack, profile["n"], unfused=profile["unfused"], **kw)
  twin = E.Engine(pack, profile["n"], unfused=True, dev={"generic_kernel": 1}, **kw)
  for kind in bound_scalars(profile):
    bind_view(eng, kind, profile["ring"])
    bind_view(twin, kind, profile["ring"])
  for kind in profile["views"]:
    bind_view(eng, kind, profile["ring"])
  return eng, twin
