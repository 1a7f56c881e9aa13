"""Test infrastructure: seeded random PROGRAMS of engine API calls, and the runner that executes one
on an `engine.Engine` and on the oracle-backed model of tests/engine_model.py (and on a twin
engine with another launch form), comparing after every call.

`make_program(seed, profile)` writes the program: a list of ops (dicts with concrete numpy
arguments), deterministic, no GPU code.  `run_program(program, engine, model, twin)` applies each op
to all of them; "engine" is only an interface here (reset / step / step_fields / step_many /
save_worlds / load_worlds / snapshot / restore / bind / bind_ring / unbind / observe_host / dump /
counters / fault_words / ring / _bound), which the model satisfies too — so the CPU suite runs the
runner model against model, and against deliberately wrong models.

A profile names the op `classes` its programs draw from.  The first set (COMMITTED) draws from the
thirteen OP_CLASSES.  The STATE programs (STATE_COMMITTED) add masked steps, masked and stopping
K-step calls with a persistent `stopped`, per-step state rows that become banks, registered episode
starts whose `rows` are rewritten in place, and four read-only classes that draw, hash and check
saved states; there the twin runs the other form of every new K-step call (see `_Side`).  The
model does not state fresh=True starts: it says which worlds it speaks for (`ModelEngine.exact`),
and the runner compares those.  The UNIT programs (UNIT_COMMITTED) add listed steps (worlds=, with
entries that are no world or repeat one), episode statistics registered and cleared, the three view
units (EGO_LAYER, the view hashes, the planes) registered and cleared, and reads of them; the twin
registers nothing, folds the statistics on the host from what its single steps left, and runs a
list as the masked request over all worlds."""
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
for _p in PROFILES:
  _p["classes"] = OP_CLASSES   # the op classes a profile's programs draw from
# the committed set: (program seed, profile), chosen so that every ordered pair of distinct op
# classes is adjacent somewhere in it (tests/test_api_programs_cpu.py prints the table)
COMMITTED = [(1000 + i, p) for i, p in enumerate(PROFILES)]

# ---- the state programs: masks, stops, episode starts and reads of saved states
# mutating classes (unstop and starts_rows are no engine call: they rewrite the caller's tensors)
NEW_MUTATING = ("step_active", "many_active", "many_until", "unstop", "step_many_states",
                "starts_set", "starts_rows", "starts_clear")
# read-only classes: the runner compares everything after every op, so "nothing of the engine's is
# written" is checked by running them
READ_ONLY = ("observe_rows", "observe_views", "hash", "check")
MUTATING = OP_CLASSES + NEW_MUTATING
STATE_CLASSES = MUTATING + READ_ONLY
NEW_STEP_CLASSES = ("step_active", "many_active", "many_until", "step_many_states")
ALL_STEP_CLASSES = STEP_CLASSES + NEW_STEP_CLASSES
STATE_MIN_OPS, STATE_MAX_OPS, STATE_MAX_WORLD_STEPS = 70, 110, 260
STATE_K = MANY_K + (65,)   # 65: the mask column of a lane crosses a 64-bit word
STATES_K = (1, 2, 7)       # step_many_states: its K x N rows become a bank
GAMMAS = (1.0, 0.97, 0.5)
UNTILS = (("last",), ("reward",), ("last", "reward"))
HASH_SPECS = (None, dict(planes=(0,)), dict(fields=("ax", "ay", "aori", "aalive")),
              dict(planes=(0,), fields=("step", "done")))
STATE_WORLD_COUNTS = (6, 23)   # remainders 2 and 3 of a workgroup of four worlds
LONG_EPISODES = {"coins": 33, "territory__inside_out": 33}   # MAXFRAMES where rewards are rare
# action weights over each level's ACTION_SET (1: forward; 7: zap / interact / mine; 8: clean / consume)
ACTION_WEIGHTS = {
    "clean_up": [1, 4, 1, 1, 1, 2, 2, 2, 4],
    "coins": [1, 4, 1, 1, 1, 1, 1],
    "collaborative_cooking__cramped": [1, 3, 1, 1, 1, 3, 3, 6],   # INTERACT_HEAVY
    "commons_harvest__open": [1, 4, 1, 1, 1, 2, 2, 4],
    "coop_mining": [1, 3, 1, 1, 1, 2, 2, 5],                      # MINE_HEAVY
    "externality_mushrooms__dense": [1, 4, 1, 1, 1, 2, 2, 5],     # ZAP_HEAVY
    "gift_refinements": [1, 4, 1, 1, 1, 2, 2, 5, 2],              # GIFT_HEAVY
    "territory__inside_out": None,                                # (weight 4 on forward)
    "prisoners_dilemma_in_the_matrix__repeated": [1, 4, 1, 1, 1, 2, 2, 4],
}


def _state_profiles():
  out = []
  for li, pack in enumerate(LEVEL_PACKS):
    hdr = pack_lib.loads(E.load_pack(pack))["hdr"]
    default_p = int(hdr[20]) or int(hdr[7])
    fewer = "in_the_matrix" not in pack and pack != "coins"
    for j, n in enumerate(STATE_WORLD_COUNTS):
      pooled = j == li % 2
      out.append(dict(
          name=f"{pack}-states-n{n}", pack=pack, stock=False, rich=True, n=n, ring=0,
          world_pool=8 if pooled else 1, auto_reset=True,
          unfused=True if j == (li // 2) % 2 else None,
          num_players=max(1, default_p - 1) if fewer and j == (li // 4) % 2 else 0,
          views=(E.OBS_WORLD_RGB, E.OBS_LAYER) if pooled else (E.OBS_RGB,),
          frames=LONG_EPISODES.get(pack, EPISODE_FRAMES), classes=STATE_CLASSES))
  out.append(dict(name="stock_clean_up-states-n23", pack="clean_up", stock=True, rich=False, n=23, ring=0,
                  world_pool=1, auto_reset=True, unfused=None, num_players=0, views=(E.OBS_WORLD_RGB,),
                  frames=0, classes=STATE_CLASSES))
  return out


STATE_PROFILES = _state_profiles()
# (program seed, profile): seeds searched on the model alone so that the conditions of
# tests/test_api_programs_cpu.py hold (the search is tests/tools/search_state_programs.py)
STATE_SEEDS = [2001, 2005, 2001, 2007, 2005, 2003, 2000, 2002, 2001, 2003, 2000, 2011, 2001, 2003, 2029, 2019,
               2003, 2000, 2000]
STATE_COMMITTED = list(zip(STATE_SEEDS, STATE_PROFILES))


# ---- the unit programs: listed steps, episode statistics and the three registered view units
UNIT_MUTATING = ("step_listed", "many_listed", "stats_set", "stats_clear", "units_set", "units_clear")
UNIT_READ_ONLY = ("unit_rows",)
UNIT_ALL_MUTATING = MUTATING + UNIT_MUTATING
UNIT_CLASSES = STATE_CLASSES + UNIT_MUTATING + UNIT_READ_ONLY
LISTED_CLASSES = ("step_listed", "many_listed")
UNIT_STEP_CLASSES = ALL_STEP_CLASSES + LISTED_CLASSES
# what a rollout ring refuses (masks, stops, lists), and the registered starts, whose twin is a host
# loop of single steps that would turn the twin's ring K times where the engine's turns once
RING_REFUSED = ("step_active", "many_active", "many_until", "unstop", "step_many_states", "starts_set",
                "starts_rows", "starts_clear") + LISTED_CLASSES
UNIT_RING_CLASSES = tuple(c for c in UNIT_CLASSES if c not in RING_REFUSED)
# (80, where the state set has 70: the statistics' totals must hold finished episodes at the end of a
# program, so its last registration is followed by UNIT_STATS_TAIL ops at least)
UNIT_MIN_OPS, UNIT_MAX_OPS, UNIT_MAX_WORLD_STEPS = 80, 110, 260
UNIT_STATS_TAIL = 18                                     # ops behind the last stats_set
UNIT_LAST_STATS_SET = UNIT_MIN_OPS - UNIT_STATS_TAIL     # no stats_set is drawn behind this op
UNIT_LAST_STATS_CLEAR = UNIT_LAST_STATS_SET - 7          # ... and no stats_clear behind this one
UNIT_STATS_LIFE, UNIT_STARTS_LIFE = 6, 8                 # ops a registration lives at least
UNIT_NAMES = ("ego", "hash", "planes")
PAIR_COLUMNS = ("interaction.row_player_idx>col_player_idx", "gift.gifter_index>receipient_index",
                "extraction_pair.player_a>player_b", "sanctioning.source>target", "zap.source>target")
NO_BEAM = ("coins", "collaborative_cooking__cramped")
FILL = 0xA5   # the byte the runner fills a listed call's tensors with before the call


def _unit_profiles():
  out = []
  for li, pack in enumerate(LEVEL_PACKS):
    hdr = pack_lib.loads(E.load_pack(pack))["hdr"]
    default_p = int(hdr[20]) or int(hdr[7])
    fewer = "in_the_matrix" not in pack and pack != "coins"
    base = dict(pack=pack, stock=False, rich=True, auto_reset=True, frames=LONG_EPISODES.get(pack, EPISODE_FRAMES))
    out.append(dict(base, name=f"{pack}-units-n6", n=6, ring=0, world_pool=1, unfused=True if li % 2 else None,
                    num_players=max(1, default_p - 1) if fewer else 0, views=(E.OBS_RGB,), classes=UNIT_CLASSES))
    if li % 2 == 0:   # form 1: no ring, WORLD.RGB pooled by 8 and LAYER bound
      out.append(dict(base, name=f"{pack}-units-n23", n=23, ring=0, world_pool=8, unfused=None, num_players=0,
                      views=(E.OBS_WORLD_RGB, E.OBS_LAYER), classes=UNIT_CLASSES))
    else:             # form 2: a ring, which refuses a list: the first op behind the reset asks for one
      out.append(dict(base, name=f"{pack}-units-n23", n=23, ring=RING_SLOTS, world_pool=1, unfused=None,
                      num_players=0, views=(E.OBS_RGB,), classes=UNIT_RING_CLASSES))
  out.append(dict(name="stock_clean_up-units-n23", pack="clean_up", stock=True, rich=False, n=23, ring=0,
                  world_pool=1, auto_reset=True, unfused=None, num_players=0, views=(E.OBS_WORLD_RGB,),
                  frames=0, classes=UNIT_CLASSES))
  return out


UNIT_PROFILES = _unit_profiles()
# (program seed, profile): searched on the model alone (tests/tools/search_unit_programs.py)
UNIT_SEEDS = [3002, 3000, 3018, 3012, 3000, 3008, 3015, 3014, 3003, 3001, 3050, 3000, 3003, 3000, 3009, 3018, 3002,
              3003, 3000]
UNIT_COMMITTED = list(zip(UNIT_SEEDS, UNIT_PROFILES))


def is_unit_profile(profile):
  return "-units-" in profile["name"]


def level_columns(profile):
  """(the level's default columns, {column: [filters "key=value" it can take]}, its pair column)."""
  import episode_stats_model
  hdr = pack_lib.loads(E.load_pack(profile["pack"]))["hdr"]
  columns = E.level_event_columns(int(hdr[1]))
  filters = {}
  for name in columns:
    event, key = name.split(".")
    known = episode_stats_model.EVENTS.get(event, (0, {}))[1]
    keys = [k for k in known if k not in E.EVENT_PLAYER_KEYS and k in E.EVENT_FIELDS[event]]
    filters[name] = [f"{k}={v}" for k in keys for v in range(0, min(3, known[k][2] + 1))]
  # (every level's rules list the zap, but two of them have no beam: no two-player event there)
  events = {n.split(".")[0] for n in columns} - ({"zap"} if profile["pack"] in NO_BEAM else set())
  pair = next((p for p in PAIR_COLUMNS if p.split(".")[0] in events), None)
  return columns, filters, pair


def rich_pack(name, raw):
  """The level's variant that pays often, where the parity tests have one; else the pack itself."""
  if name == "clean_up":
    return util.fertile_clean_up(raw)
  if name == "collaborative_cooking__cramped":
    from test_oracle_cook_cpu import stocked
    return stocked(raw)
  if name == "coop_mining":
    from test_oracle_coop_cpu import rich
    return rich(raw)
  if name == "gift_refinements":
    from test_oracle_gift_cpu import rich
    return rich(raw)
  if name == "externality_mushrooms__dense":
    from test_oracle_mushroom_cpu import lush
    return lush(raw)
  if name == "prisoners_dilemma_in_the_matrix__repeated":
    return util.matrix_variant(raw, taste=[(0, 1.0, 0.5)], unready=-1.0)
  return raw


_PACKS = {}


def profile_pack(profile):
  if profile["name"] not in _PACKS:
    raw = E.load_pack(profile["pack"])
    if not profile["stock"]:
      if profile.get("rich"):
        raw = rich_pack(profile["pack"], raw)
      raw = util.patch_pack(raw, MAXFRAMES=profile.get("frames", EPISODE_FRAMES))
    _PACKS[profile["name"]] = raw
  return _PACKS[profile["name"]]


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
  g = dict(N=profile["n"], P=P, A=A, nact=len(np.asarray(t["action_table"]).reshape(-1, 4)),
           lo=spec[:, 0].astype(np.int32), hi=spec[:, 1].astype(np.int32), row_kinds=kinds)
  if is_unit_profile(profile):
    import ego_layer_model
    g.update(ids=E.num_layer_ids_host(profile_pack(profile), num_players=profile["num_players"]),
             L=ego_layer_model.geometry(E.load_pack(profile["pack"]))[2], columns=level_columns(profile))
  return g


def _ids(rng, g, shape, bad=0.0):
  a = rng.integers(0, g["nact"], size=shape, dtype=np.int32)
  if bad:
    out = rng.choice(np.array([-1, g["nact"], g["nact"] + 3, -5, 100], np.int32), size=shape)
    a = np.where(rng.random(shape) < bad, out, a).astype(np.int32)
  return a


def _fields(rng, g, shape):
  return rng.integers(g["lo"], g["hi"] + 1, size=tuple(shape) + (g["A"],), dtype=np.int32)


class _Gen:
  """The state of one draw of a program: the ops so far and what the next op may be."""

  def __init__(self, rng, profile, g, length, budget):
    self.rng, self.profile, self.g, self.length, self.budget = rng, profile, g, length, budget
    self.ops = [dict(op="reset_all")]
    self.banks, self.have_snap, self.host_run_done = [], False, False
    self.bound = set(profile["views"])
    self.pooled = int(rng.choice(list(E.OBS_RGB_POOL.values())))
    self.agent_kinds = (E.OBS_RGB, self.pooled)
    self.registered = None     # the rows of the bank a registration names
    self.rows_of = None        # ... of the last `rows` tensor handed out (it outlives a clear)
    self.wide_reads = 0
    later = "states" in profile["name"] or is_unit_profile(profile)
    w = ACTION_WEIGHTS.get(profile["pack"]) if profile.get("rich") or later else None
    self.wide_unit_reads = 0
    self.set_at = {"stats": -100, "starts": -100}   # the op of the last stats_set / starts_set
    self.stats_live, self.units_live, self.listed_first = False, set(), bool(profile["ring"]) and is_unit_profile(profile)
    if later and w is None:
      w = [1, 4] + [1] * (g["nact"] - 2)
    self.weights = None if w is None else np.asarray(w, np.float64) / sum(w)
    assert self.weights is None or len(self.weights) == g["nact"], profile["name"]

  def blocked(self, c):
    ops, budget, length = self.ops, self.budget, self.length
    return (c == ops[-1]["op"] or (c in ("load", "starts_set", "observe_rows", "observe_views", "check") and not self.banks) or
            (c == "restore" and not self.have_snap) or (c in ALL_STEP_CLASSES and budget < 1) or
            (c == "starts_clear" and self.registered is None) or (c == "starts_rows" and self.rows_of is None) or
            (c == "stats_clear" and not self.stats_live) or (c == "units_clear" and not self.units_live) or
            (c in LISTED_CLASSES and budget < 1) or
            (c == "step_host" and not self.host_run_done and (budget < HOST_RUN or len(ops) + HOST_RUN > length)))

  def ids(self, shape, bad=0.0):
    if self.weights is None:
      return _ids(self.rng, self.g, shape, bad)
    rng, nact = self.rng, self.g["nact"]
    a = rng.choice(nact, size=shape, p=self.weights).astype(np.int32)
    if bad:
      out = rng.choice(np.array([-1, nact, nact + 3, -5, 100], np.int32), size=shape)
      a = np.where(rng.random(shape) < bad, out, a).astype(np.int32)
    return a

  def _many(self, c, ks, weights, cols=None):
    """The action block of a K-step op: K, plain / repeat / slice, ids or raw fields (`cols`: its
    columns, the entries of a list; None: the worlds)."""
    rng, g = self.rng, self.g
    N, P = cols or g["N"], g["P"]
    ks = [k for k in ks if k <= self.budget]
    p = np.array(weights[:len(ks)], np.float64)
    K = int(rng.choice(ks, p=p / p.sum()))
    form = str(rng.choice(["plain", "repeat", "slice"], p=[0.5, 0.25, 0.25]))
    fields = bool(rng.random() < 0.25)
    lead = () if form == "repeat" else (K,)
    wide = N + 3 if form == "slice" else N
    acts = _fields(rng, g, lead + (wide, P)) if fields else self.ids(lead + (wide, P), bad=0.01)
    self.budget -= K
    return dict(op=c, K=K, form=form, fields=fields, actions=acts, lo=int(rng.integers(0, 4)) if form == "slice" else 0)

  def _row_kinds(self):
    rng, kinds = self.rng, self.g["row_kinds"]
    pick = rng.random(len(kinds)) < 0.5
    pick[rng.integers(len(pick))] = True
    return tuple(int(k) for k, p in zip(kinds, pick) if p)

  def _mask(self, op, forms, p):
    """Adds a mask of one of `forms` to the K-step op."""
    rng, N, K = self.rng, self.g["N"], op["K"]
    form = str(rng.choice(forms, p=np.array(p) / sum(p)))
    op.update(mask_form=form, mlo=0, mask_dtype=str(rng.choice(["uint8", "bool"])))
    if form == "kn":
      op["mask"] = (rng.random((K, N)) < 0.6).astype(np.uint8)
    elif form == "n":
      op["mask"] = (rng.random(N) < 0.6).astype(np.uint8)
    elif form == "prefix":
      lengths = rng.integers(0, K + 1, size=N)
      op["mask"] = (np.arange(K)[:, None] < lengths[None]).astype(np.uint8)
    elif form == "slice":
      op["mask"] = (rng.random((K, N + 3)) < 0.6).astype(np.uint8)
      op["mlo"] = int(rng.integers(0, 4))
    elif form == "zeros":
      op["mask"] = np.zeros((K, N), np.uint8)
    else:
      op["mask"] = None

  def _pick_rows(self, count, rows_in_bank):
    """`count` bank rows with repeats, out of at most three distinct ones (each distinct row is
    replayed on an oracle once)."""
    rng = self.rng
    distinct = rng.choice(rows_in_bank, size=min(3, rows_in_bank), replace=False)
    return rng.choice(distinct, size=count).astype(np.int32)

  def draw(self, c):
    rng, g, ops = self.rng, self.g, self.ops
    N, P = g["N"], g["P"]
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
      ops.append(dict(op=c, actions=self.ids((N, P), bad=0.01)))
      self.budget -= 1
    elif c == "step_host":
      run = 1 if self.host_run_done else HOST_RUN + int(rng.integers(0, 2))
      run = min(run, self.budget, self.length - len(ops))
      for _ in range(run):
        ops.append(dict(op=c, actions=self.ids((N, P))))
      self.budget -= run
      self.host_run_done = self.host_run_done or run >= HOST_RUN
    elif c == "step_fields":
      ops.append(dict(op=c, fields=_fields(rng, g, (N, P)), host=bool(rng.integers(2))))
      self.budget -= 1
    elif c in ("step_many", "step_many_rows"):
      op = self._many(c, MANY_K, [3, 3, 3, 1])
      if c == "step_many_rows":
        op["observations"] = self._row_kinds()
      ops.append(op)
    elif c == "save":
      m = int(rng.integers(1, N + 1))
      ops.append(dict(op=c, worlds=rng.choice(N, size=m, replace=False).astype(np.int32)))
      self.banks.append(m)
    elif c == "load":
      b = int(rng.integers(len(self.banks)))
      src = rng.integers(0, self.banks[b], size=N).astype(np.int32)   # (with duplicates)
      src[rng.random(N) < 0.3] = -1
      i, j = rng.choice(N, size=2, replace=False)
      src[i], src[j] = -1, int(rng.integers(self.banks[b]))
      ops.append(dict(op=c, bank=b, src=src))
    elif c == "snapshot":
      ops.append(dict(op=c))
      self.have_snap = True
    elif c == "restore":
      ops.append(dict(op=c))
    elif c == "rebind":
      kind = int(rng.choice([E.OBS_RGB, self.pooled, E.OBS_WORLD_RGB, E.OBS_LAYER]))
      other = [k for k in self.agent_kinds if k != kind and k in self.bound]
      if kind in self.bound:
        bind = False
      elif kind in self.agent_kinds and other:   # one per-agent view at a time: the other one leaves
        kind, bind = other[0], False
      else:
        bind = True
      (self.bound.add if bind else self.bound.discard)(kind)
      ops.append(dict(op=c, kind=kind, bind=bind))
    # ---- the state classes
    elif c == "step_active":
      mask = (rng.random(N) < 0.6).astype(np.uint8)
      host = bool(rng.integers(2))
      ops.append(dict(op=c, actions=self.ids((N, P), bad=0.0 if host else 0.01), host=host, mask=mask,
                      mask_dtype=str(rng.choice(["uint8", "bool", "list"]))))
      self.budget -= 1
    elif c == "many_active":
      op = self._many(c, STATE_K, [3, 3, 3, 2, 1])
      self._mask(op, ["kn", "n", "prefix", "slice", "zeros"], [7, 4, 4, 4, 1])
      op["observations"] = self._row_kinds() if rng.random() < 0.5 else None
      ops.append(op)
    elif c == "many_until":
      op = self._many(c, STATE_K, [1, 2, 3, 3, 1])
      self._mask(op, ["none", "kn", "n", "prefix", "slice"], [4, 3, 1, 2, 2])
      op["observations"] = self._row_kinds() if rng.random() < 0.3 else None
      op["until"] = UNTILS[int(rng.integers(len(UNTILS)))]
      op["returns"] = bool(rng.random() < 0.7)
      op["gamma"] = float(rng.choice(GAMMAS)) if op["returns"] else 1.0
      op["use_stopped"] = bool(rng.random() < 0.6)
      ops.append(op)
    elif c == "unstop":
      mask = (rng.random(N) < 0.5).astype(np.uint8)
      mask[rng.integers(N)] = 1
      ops.append(dict(op=c, mask=mask))
    elif c == "step_many_states":
      op = self._many(c, STATES_K, [2, 3, 3])
      self._mask(op, ["none", "kn", "prefix"], [2, 2, 1])
      ops.append(op)
      self.banks.append(op["K"] * N)
    elif c == "starts_set":
      b = int(rng.integers(len(self.banks)))
      rows = self._start_rows(self.banks[b])
      # finished_world: where the bank holds a row saved from a finished episode, that world takes it
      # (the runner asks the model which rows those are: `resolve`)
      ops.append(dict(op=c, bank=b, rows=rows, fresh=bool(rng.random() < 0.2),
                      finished_world=int(rng.integers(N))))
      self.registered = self.rows_of = self.banks[b]
    elif c == "starts_rows":
      ops.append(dict(op=c, rows=self._start_rows(self.rows_of)))
    elif c == "starts_clear":
      ops.append(dict(op=c))
      self.registered = None
    elif c == "observe_rows":
      b = int(rng.integers(len(self.banks)))
      kinds = list(E.PIXEL_KINDS) + list(g["row_kinds"])
      wide = self.wide_reads == 0   # one read of a program has more rows than worlds
      self.wide_reads += 1
      count = N + 2 if wide else int(rng.integers(1, min(N, 6) + 1))
      ops.append(dict(op=c, bank=b, kind=int(rng.choice(kinds)), rows=self._pick_rows(count, self.banks[b])))
    elif c == "observe_views":
      b = int(rng.integers(len(self.banks)))
      kinds = [k for k in E.PIXEL_KINDS if k != E.OBS_WORLD_RGB] + list(g["row_kinds"])
      count = int(rng.integers(1, min(N, 6) + 1))
      ops.append(dict(op=c, bank=b, kind=int(rng.choice(kinds)), rows=self._pick_rows(count, self.banks[b]),
                      players=rng.integers(0, P, size=count).astype(np.int32), offset=int(rng.integers(0, 16))))
    elif c == "hash":
      b = int(rng.integers(-1, len(self.banks)))   # -1: hash_worlds
      rows = None if b < 0 or rng.random() < 0.3 else self._pick_rows(int(rng.integers(1, 9)), self.banks[b])
      ops.append(dict(op=c, bank=b, rows=rows, spec=int(rng.integers(len(HASH_SPECS)))))
    elif c == "check":
      b = int(rng.integers(len(self.banks)))
      ops.append(dict(op=c, bank=b, row=int(rng.integers(self.banks[b])), player=int(rng.integers(P)),
                      field=str(rng.choice(["orientation", "avatar_x"]))))
    # ---- the unit classes
    elif c == "step_listed":
      worlds, bad = self._list()
      ops.append(dict(op=c, worlds=worlds, bad=bad, actions=self.ids((len(worlds), P), bad=0.01)))
      self.budget -= 1
    elif c == "many_listed":
      worlds, bad = self._list()
      M = len(worlds)
      op = self._many(c, STATE_K, [1, 2, 4, 4, 1], cols=M)
      op.update(worlds=worlds, bad=bad)
      K = op["K"]
      form = str(rng.choice(["none", "km", "m"], p=[0.4, 0.4, 0.2]))
      op["active"] = None if form == "none" else (rng.random((K, M) if form == "km" else (M,)) < 0.7).astype(np.uint8)
      op["observations"] = self._row_kinds() if rng.random() < 0.4 else None
      op["until"] = UNTILS[int(rng.integers(len(UNTILS)))] if rng.random() < 0.6 else None
      op["returns"] = bool(op["until"] is not None and rng.random() < 0.7)
      op["gamma"] = float(rng.choice(GAMMAS)) if op["returns"] else 1.0
      op["use_stopped"] = op["until"] is not None   # (the persistent `stopped` [N], by world)
      ops.append(op)
    elif c == "stats_set":
      columns, filters, pair = g["columns"]
      how = str(rng.choice(["default", "none", "subset"], p=[0.4, 0.15, 0.45])) if columns else "none"
      if how == "subset":
        pick = rng.random(len(columns)) < 0.6
        pick[rng.integers(len(pick))] = True
        chosen = [n for n, p in zip(columns, pick) if p]
        able = [n for n in chosen if filters[n]]
        if able:   # one [key=value] filter where the level has a filterable payload
          n = able[int(rng.integers(len(able)))]
          chosen[chosen.index(n)] = f"{n}[{filters[n][int(rng.integers(len(filters[n])))]}]"
        cols = tuple(chosen)
      else:
        cols = "default" if how == "default" else ()
      ops.append(dict(op=c, columns=cols, pairs=(pair,) if pair else ()))
      self.stats_live = True
    elif c == "stats_clear":
      ops.append(dict(op=c))
      self.stats_live = False
    elif c == "units_set":
      pick = rng.random(3) < 0.6
      pick[rng.integers(3)] = True
      ids, L = g["ids"], g["L"]
      op = dict(op=c, units=tuple(n for n, p in zip(UNIT_NAMES, pick) if p))

      def layers():
        if rng.random() < 0.5:
          return None
        keep = rng.random(L) < 0.6
        keep[rng.integers(L)] = True
        return tuple(int(i) for i in np.nonzero(keep)[0])
      if "hash" in op["units"]:
        both = bool(rng.random() < 0.6)   # drawn layers and a drawn class table, or neither
        op["hash"] = dict(layers=layers() if both else None,
                          classes=rng.integers(0, 4, size=ids).astype(np.int32) if both else None)
      if "planes" in op["units"]:
        C = int(rng.integers(2, 6))
        table = rng.integers(-1, C, size=ids).astype(np.int32)
        table[rng.integers(ids)] = -1
        table[rng.integers(ids)] = C - 1 if rng.random() < 0.5 else 0
        given = bool(rng.random() < 0.5)
        op["planes"] = dict(classes=table, layers=layers(), facing=bool(rng.random() < 0.6),
                            num_classes=C if given else None, offset=int(rng.integers(0, 16)))
      ops.append(op)
      self.units_live |= set(op["units"])
    elif c == "units_clear":
      name = sorted(self.units_live)[int(rng.integers(len(self.units_live)))]
      ops.append(dict(op=c, unit=name))
      self.units_live.discard(name)
    elif c == "unit_rows":
      unit = str(rng.choice(UNIT_NAMES))
      b = int(rng.integers(-1, len(self.banks)))   # -1: the live worlds
      there = N if b < 0 else self.banks[b]
      wide = self.wide_unit_reads == 0   # one read of a program has more rows than worlds
      self.wide_unit_reads += 1
      count = N + 2 if wide else int(rng.integers(1, min(N, 6) + 1))
      rows = self._pick_rows(count, there)
      op = dict(op=c, unit=unit, bank=b, rows=rows,
                players=rng.integers(0, P, size=count).astype(np.int32) if rng.random() < 0.5 else None)
      if unit == "hash":
        op["params"] = dict(layers=None, classes=rng.integers(0, 3, size=g["ids"]).astype(np.int32)
                            if rng.random() < 0.5 else None)
      if unit == "planes":
        C = int(rng.integers(1, 5))
        table = rng.integers(-1, C, size=g["ids"]).astype(np.int32)
        op["params"] = dict(classes=table, layers=None, facing=bool(rng.random() < 0.5), num_classes=C)
        op["offset"] = int(rng.integers(0, 16))
      ops.append(op)
    else:
      raise ValueError(c)

  def _list(self):
    """(worlds int32 [M], bad): the list of a listed op; about one in four carries one entry outside
    [0, N) and one that repeats an earlier entry's world."""
    rng, N = self.rng, self.g["N"]
    M = N if rng.random() < 0.3 else int(rng.integers(1, N + 1))
    worlds = rng.choice(N, size=M, replace=False).astype(np.int32)
    bad = bool(M >= 3 and rng.random() < 0.25)
    if bad:
      three = sorted(rng.choice(M, size=3, replace=False).tolist())
      out = three.pop(int(rng.integers(3)))
      worlds[three[1]] = worlds[three[0]]
      worlds[out] = int(rng.choice([-1, -7, N, N + 5]))
    return worlds, bad

  def _start_rows(self, rows_in_bank):
    """`rows` of a registration: valid indices and -1s, several worlds on one row."""
    rng, N = self.rng, self.g["N"]
    rows = self._pick_rows(N, rows_in_bank)
    rows[rng.random(N) < 0.3] = -1
    i, j, k = rng.choice(N, size=3, replace=False)
    rows[i] = rows[j] = int(rng.integers(rows_in_bank))
    rows[k] = -1
    return rows.astype(np.int32)


def _attempt(rng, profile, g):
  length = int(rng.integers(MIN_OPS, MAX_OPS + 1))
  gen = _Gen(rng, profile, g, length, MAX_WORLD_STEPS)
  while len(gen.ops) < length:
    allowed = [c for c in OP_CLASSES if not gen.blocked(c)]
    gen.draw(str(rng.choice(allowed)))
  return gen.ops


def required_pairs():
  """The adjacencies the state programs owe: every ordered pair of distinct mutating classes with a
  new class in it, and every read-only class behind every new mutating class."""
  pairs = [(a, b) for a in MUTATING for b in MUTATING if a != b and (a in NEW_MUTATING or b in NEW_MUTATING)]
  return pairs + [(a, r) for a in NEW_MUTATING for r in READ_ONLY]


def required_unit_pairs():
  """The adjacencies the unit programs owe: every ordered pair of distinct mutating classes with a
  unit class in it, and unit_rows behind every mutating unit class."""
  pairs = [(a, b) for a in UNIT_ALL_MUTATING for b in UNIT_ALL_MUTATING
           if a != b and (a in UNIT_MUTATING or b in UNIT_MUTATING)]
  return pairs + [(a, r) for a in UNIT_MUTATING for r in UNIT_READ_ONLY]


def assigned_pairs(profile):
  """The share of `required_pairs` that the program of `profile` must hold: the generator steers
  its draws toward them, deterministically."""
  if is_unit_profile(profile):
    # a pair with a class a ring refuses goes round the profiles without one, the others round all
    names = [p["name"] for p in UNIT_PROFILES]
    free = [p["name"] for p in UNIT_PROFILES if not p["ring"]]
    out, at = [], [0, 0]
    for pair in required_unit_pairs():
      refused = any(c in RING_REFUSED for c in pair)
      pool = free if refused else names
      if pool[at[refused] % len(pool)] == profile["name"]:
        out.append(pair)
      at[refused] += 1
    return out
  i = [p["name"] for p in STATE_PROFILES].index(profile["name"])
  return required_pairs()[i::len(STATE_PROFILES)]


def _attempt_states(rng, profile, g, min_ops=STATE_MIN_OPS, max_ops=STATE_MAX_OPS, steps=STATE_MAX_WORLD_STEPS):
  """A program over the profile's classes (STATE_CLASSES, or the unit programs'); None if this draw
  misses a class, a pair or the host run."""
  gen = _Gen(rng, profile, g, max_ops, steps)
  todo = set(assigned_pairs(profile))
  classes = profile["classes"]
  refused = []
  if gen.listed_first:   # a ring refuses a list: one listed call, which must raise and change nothing
    worlds, bad = gen._list()
    refused = [dict(op="step_listed", worlds=worlds, bad=bad, refused=True,
                    actions=gen.ids((len(worlds), g["P"])))]
    gen.ops += refused
  while len(gen.ops) < max_ops:
    seen = {op["op"] for op in gen.ops[len(refused) + 1:]} | {"reset_all"}
    if len(gen.ops) >= min_ops and not todo and seen == set(classes) and gen.host_run_done:
      break
    allowed = [c for c in classes if not gen.blocked(c)]
    prev = gen.ops[-1]["op"]
    unit = is_unit_profile(profile)
    if unit:
      # the statistics stay registered over the last part of a program, so that its totals hold
      # finished episodes at the end; a registration of either kind lives a few ops at least
      at = len(gen.ops)
      allowed = [c for c in allowed if (prev, c) in todo or not (
          (c == "stats_clear" and (at >= UNIT_LAST_STATS_CLEAR or at - gen.set_at["stats"] < UNIT_STATS_LIFE)) or
          (c == "stats_set" and at > UNIT_LAST_STATS_SET) or
          (c == "starts_clear" and at - gen.set_at["starts"] < UNIT_STARTS_LIFE))]
    closing = [c for c in allowed if (prev, c) in todo]      # an owed pair that this draw completes
    opening = [c for c in allowed if any(a == c for a, _ in todo)]
    missing = [c for c in allowed if c not in seen]
    skipping = [c for c in allowed if c in ("step_active", "many_active", "many_until") + LISTED_CLASSES]
    favoured = [c for c in allowed if c in UNIT_MUTATING + UNIT_READ_ONLY]
    if unit and len(gen.ops) >= UNIT_LAST_STATS_SET and not gen.stats_live and prev != "stats_set":
      c = "stats_set"
    elif closing:
      c = str(rng.choice(closing))
    elif unit and prev == "restore" and skipping and gen.units_live and rng.random() < 0.6:
      c = str(rng.choice(skipping))   # (a restore, then a step that skips worlds, a unit registered)
    elif unit and favoured and rng.random() < 0.3:
      c = str(rng.choice(favoured))
    elif opening and rng.random() < 0.6:
      c = str(rng.choice(opening))
    elif missing and rng.random() < 0.5:
      c = str(rng.choice(missing))
    else:
      c = str(rng.choice(allowed))
    before = len(gen.ops)
    gen.draw(c)
    if c in ("stats_set", "starts_set"):
      gen.set_at[c.split("_")[0]] = before
    todo.discard((prev, c))
    for a, b in zip(gen.ops[before:-1], gen.ops[before + 1:]):   # (a run of host steps)
      todo.discard((a["op"], b["op"]))
  seen = {op["op"] for op in gen.ops if not op.get("refused")}
  if todo or seen != set(classes) or not gen.host_run_done:
    return None
  return gen.ops


def world_steps(program):
  return sum(op.get("K", 1) for op in program if op["op"] in UNIT_STEP_CLASSES and not op.get("refused"))


def longest_host_run(program):
  best = run = 0
  for op in program:
    run = run + 1 if op["op"] == "step_host" else 0
    best = max(best, run)
  return best


def make_program(seed, profile):
  """The program of (seed, profile): deterministic; the first draw that holds every op class of
  the profile (and, for a state profile, the adjacencies it owes)."""
  g = _geometry(profile)
  states = set(profile["classes"]) != set(OP_CLASSES)
  for attempt in range(1000):
    rng = np.random.default_rng([int(seed), zlib.crc32(profile["name"].encode()), attempt])
    if is_unit_profile(profile):
      ops = _attempt_states(rng, profile, g, UNIT_MIN_OPS, UNIT_MAX_OPS, UNIT_MAX_WORLD_STEPS)
    else:
      ops = _attempt_states(rng, profile, g) if states else _attempt(rng, profile, g)
    held = set() if ops is None else {op["op"] for op in ops if not op.get("refused")}
    if ops is not None and held == set(profile["classes"]) and longest_host_run(ops) >= HOST_RUN:
      prog = Program(ops)
      prog.seed, prog.profile = int(seed), profile
      return prog
  raise AssertionError(f"no program for seed {seed}, profile {profile['name']}")


def pair_counts(programs, classes=OP_CLASSES):
  """[from, to] counts of adjacent op classes over `programs`."""
  idx = {c: i for i, c in enumerate(classes)}
  table = np.zeros((len(classes),) * 2, np.int64)
  for prog in programs:
    for a, b in zip(prog[:-1], prog[1:]):
      table[idx[a["op"]], idx[b["op"]]] += 1
  return table


def format_pair_table(table, classes=OP_CLASSES):
  short = [c.replace("step_", "s_").replace("masked_", "m_").replace("observe_", "o_").replace("starts_", "st_")
           for c in classes]
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


def stop_bits(until):
  return sum(E.STOP_NAMES[n] for n in (until or ()))


def op_blocks(op, n):
  """The K action blocks [N, P(, A)] of a K-step op, on the host."""
  a = op["actions"]
  if op["form"] == "repeat":
    return [a] * op["K"]
  if op["form"] == "slice":
    a = a[:, op["lo"]:op["lo"] + n]
  return [a[k] for k in range(op["K"])]


def op_mask(op, n):
  """bool [K, N] of a K-step op's mask, or None."""
  m = op.get("mask")
  if m is None:
    return None
  if op["mask_form"] == "slice":
    m = m[:, op["mlo"]:op["mlo"] + n]
  return np.broadcast_to(m != 0, (op["K"], n))


def resolve(op, model_side):
  """The op as every side runs it.  A `starts_set` names a world that takes a row saved from a
  finished episode where the bank has one: which rows those are is the model's to say."""
  if op["op"] != "starts_set":
    return op
  finished = [i for i, row in enumerate(model_side.banks[op["bank"]]) if row["finished"]]
  if not finished:
    return op
  rows = op["rows"].copy()
  rows[op["finished_world"]] = finished[0]
  return dict(op, rows=rows)


class _Side:
  """One engine of a run and what the program keeps for it: its banks, its snapshot, the persistent
  `stopped` bytes and the `rows` of its registration.  The TWIN runs the other form of every
  K-step op of the state classes — the host loop of step(A[k], active=m_k) with `stopped` kept on
  the host — and never registers episode starts: after each of its steps it performs the defining
  identity, load_worlds of the row of each world that was done and ran (for fresh=True the
  gather-and-edit of seed, episode and orders_step)."""

  def __init__(self, eng, twin=False):
    self.eng = eng
    self.twin = twin
    self.real = hasattr(eng, "_L")   # an engine.Engine (device tensors), not a model
    self.banks = []
    self.snap = None
    self.rows = None       # what the last step_many returned
    self.read = None       # what the last read-only op returned
    self.reg = None        # the registration: {"bank", "fresh"}
    self.start_rows = None
    self.stats = None      # the statistics registration: the engine's EpisodeStats (the model's Model)
    self.hstats = None     # the twin's: {"columns", "pairs", "arrays"}, folded on the host
    self.units = {}        # the registered view units: name -> {"out", "wide", "lo", "params"}
    self.raised = None     # what a refused op raised
    n = eng.N
    if self.real and not twin:
      import torch
      self.stopped = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    else:
      self.stopped = np.zeros(n, np.uint8)

  def dev(self, a):
    if hasattr(self.eng, "to_device"):
      return self.eng.to_device(a)
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)

  # ---- the twin's single step, with the identity of a registration
  def _tail(self, name):
    lay = self.eng.state_layout()
    off, elem, count = lay.fields[name]
    raw = self.eng.save_worlds()[:, lay.grid_pad + off:lay.grid_pad + off + elem * count].cpu().numpy()
    return np.ascontiguousarray(raw).view({1: np.uint8, 4: np.int32, 8: np.uint64}[elem])

  def _twin_fold(self, ran=None):
    """The twin registers no statistics: it reads what its submission left on the host and folds it
    through the library's host form (`ran`: bool [N], the worlds that ran; None: all)."""
    if self.hstats is None:
      return
    eng, h = self.eng, self.hstats
    ran = np.ones(eng.N, bool) if ran is None else np.asarray(ran) != 0
    events = eng.observe_host(E.OBS_EVENTS)[None] if h["columns"] or h["pairs"] else None
    E.episode_stats_host(h["arrays"], eng.observe_host(E.OBS_STEP_TYPE)[None], eng.observe_host(E.OBS_REWARD)[None],
                         events, h["columns"], h["pairs"], active=ran[None].astype(np.uint8))

  def _twin_step(self, block, m, fields):
    """One step of the twin: `block` [N, P(, A)] on the host, `m` bool [N] or None."""
    self._twin_one(block, m, fields)
    self._twin_fold(m)

  def _twin_one(self, block, m, fields):
    eng = self.eng
    done = self._tail("done")[:, 0] != 0 if self.reg else None
    if m is None:
      (eng.step_fields if fields else eng.step)(self.dev(block))
    elif fields:
      eng.step_many(self.dev(block[None]), fields=True, keep=(), active=self.dev(m.astype(np.uint8)))
    else:
      eng.step(self.dev(block), active=self.dev(m.astype(np.uint8)))
    if self.reg:
      took = done & (self.start_rows >= 0)
      if m is not None:
        took &= m
      if took.any():
        self._identity(took)

  def _identity(self, took):
    import torch
    eng, bank, rows = self.eng, self.banks[self.reg["bank"]], self.start_rows
    if not self.reg["fresh"]:
      eng.load_worlds(bank, np.where(took, rows, -1).astype(np.int32))
      return
    from meltingpot_amd import substrate
    lay = eng.state_layout()
    own = substrate.StateFields(eng.save_worlds(), lay)   # (the twin's own reset has just set episode + 1)
    gathered = bank[torch.from_numpy(np.where(took, rows, 0)).to(eng.device).long()].clone()
    f = substrate.StateFields(gathered, lay)
    f.seed[:] = own.seed
    f.episode[:] = own.episode
    f.orders_step[:] = 0
    eng.load_worlds(gathered, np.where(took, np.arange(eng.N), -1).astype(np.int32))

  def _twin_loop(self, op):
    """A K-step op as the host loop of single steps; returns ran / stopped / returns / states /
    hashes where the op asks for them."""
    eng, c = self.eng, op["op"]
    n = eng.N
    blocks, M = op_blocks(op, n), op_mask(op, n)
    stopping = c == "many_until"
    stop = stop_bits(op.get("until"))
    states = c == "step_many_states"
    if stopping:
      stopped = self.stopped if op["use_stopped"] else np.zeros(n, np.uint8)
      ran, ret, g = np.zeros(n, np.int32), np.zeros((n, eng.P), np.float64), np.ones(n, np.float64)
    rows = {"states": [], "hashes": []} if states else {}
    for k, block in enumerate(blocks):
      m = None if M is None else M[k].copy()
      if stopping:
        m = (stopped == 0) if m is None else m & (stopped == 0)
      self._twin_step(block, m, op["fields"])
      if stopping:
        reward, kind = eng.observe_host(E.OBS_REWARD), eng.observe_host(E.OBS_STEP_TYPE)
        for w in np.nonzero(m)[0]:
          ran[w] += 1
          ret[w] = ret[w] + g[w] * reward[w]
          g[w] = g[w] * np.float64(op["gamma"])
          reason = ((E.MP_STOP_LAST if (stop & E.MP_STOP_LAST) and kind[w] == 2 else 0) |
                    (E.MP_STOP_REWARD if (stop & E.MP_STOP_REWARD) and (reward[w] != 0).any() else 0))
          if reason:
            stopped[w] = reason
      if states:
        rows["states"].append(eng.save_worlds().clone())
        rows["hashes"].append(_host(eng.hash_worlds()))
    if stopping:
      rows.update(stopped=stopped.copy(), ran=ran)
      if op["returns"]:
        rows["returns"] = ret
    return rows

  # ---- the ops
  def _mask_arg(self, op):
    m = op["mask"]
    if op["mask_dtype"] == "list":
      return (m != 0).tolist()
    d = self.dev(m if op["mask_dtype"] == "uint8" else m != 0)
    if op.get("mask_form") == "slice":
      d = d[:, op["mlo"]:op["mlo"] + self.eng.N]
    return d

  def _many(self, op):
    """A K-step op of any class, as the engine's own K-step call."""
    eng, c = self.eng, op["op"]
    acts = self.dev(op["actions"])
    if op["form"] == "slice":   # a column slice of a wider tensor: non-contiguous along K only
      acts = acts[:, op["lo"]:op["lo"] + eng.N]
    kw = dict(fields=op["fields"], repeat=op["K"] if op["form"] == "repeat" else None)
    if op.get("observations") is not None:
      kw.update(events=True, observations=op["observations"])
    if op.get("mask") is not None:
      kw["active"] = self._mask_arg(op)
    if c == "many_until":
      kw.update(until=op["until"], returns=op["returns"], gamma=op["gamma"])
      if op["use_stopped"]:
        kw["stopped"] = self.stopped
    if c == "step_many_states":
      kw.update(states=True, hashes=True)
    fold = self.twin and self.hstats is not None   # (a ring profile: the K rows, folded on the host)
    if fold:
      kw["events"] = True
    res = dict(eng.step_many(acts, **kw))
    if c == "many_until" and op["use_stopped"] and res["stopped"] is not self.stopped:
      raise Mismatch("step_many did not hand back the caller's `stopped`")
    if fold:
      h = self.hstats
      E.episode_stats_host(h["arrays"], _host(res["step_type"]), _host(res["reward"]),
                           _host(res["events"]) if h["columns"] or h["pairs"] else None, h["columns"], h["pairs"])
      if op.get("observations") is None:
        del res["events"]
    return res

  # ---- the unit classes
  def _filled(self, shape, dtype):
    """A tensor of `shape` whose every byte is FILL."""
    if self.real:
      import torch
      size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
      return torch.full((size,), FILL, dtype=torch.uint8, device=self.eng.device).view(dtype).view(tuple(shape))
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)

  def _listed(self, op):
    """A listed op as the engine's own call, every per-call tensor filled beforehand: a bad entry's
    elements must keep their bytes."""
    eng, many = self.eng, op["op"] == "many_listed"
    M = len(op["worlds"])
    worlds = self.dev(op["worlds"])
    if not many:
      eng.step(self.dev(op["actions"]), worlds=worlds)
      return None
    acts = self.dev(op["actions"])
    if op["form"] == "slice":
      acts = acts[:, op["lo"]:op["lo"] + M]
    K = op["K"]
    kw = dict(fields=op["fields"], repeat=K if op["form"] == "repeat" else None, worlds=worlds)
    keys = ["reward", "collective_reward", "step_type", "discount"]
    if op["observations"] is not None:
      kw.update(events=True, observations=op["observations"])
      keys += ["events"] + list(op["observations"])
    if op["active"] is not None:
      kw["active"] = self.dev(op["active"])
    out = {}
    for key in keys:
      if self.real:
        _, per_world, dtype = E.step_row(eng.shapes, key)
      else:
        shape, dtype = eng.shapes[E.STEP_MANY_NAMES.get(key, key)]
        per_world = tuple(shape[1:])
      out[key] = self._filled((K, M) + tuple(per_world), dtype)
    if op["until"] is not None:
      kw.update(until=op["until"], gamma=op["gamma"], stopped=self.stopped, returns=op["returns"])
      import torch
      out["ran"] = self._filled((M,), torch.int32 if self.real else np.int32)
      if op["returns"]:
        out["returns"] = self._filled((M, eng.P), torch.float64 if self.real else np.float64)
    res = dict(eng.step_many(acts, out=out, **kw))
    if op["until"] is not None and res["stopped"] is not self.stopped:
      raise Mismatch("step_many(worlds=) did not hand back the caller's `stopped`")
    return {k: np.array(_host(v)) for k, v in res.items()}

  def _twin_listed(self, op):
    """The twin's form of a listed op: the masked request over all N worlds of the defining identity,
    as the host loop of masked single steps; ran / returns gathered by entry."""
    n, M = self.eng.N, len(op["worlds"])
    many = op["op"] == "many_listed"
    K = op["K"] if many else 1
    blocks = op_blocks(op, M) if many else [op["actions"]]
    act = None if not many or op["active"] is None else np.broadcast_to(op["active"] != 0, (K, M))
    full = np.zeros((K, n) + blocks[0].shape[1:], np.int32)
    mask = np.zeros((K, n), np.uint8)
    owners, seen = [], set()
    for i, w in enumerate(op["worlds"].tolist()):
      if 0 <= w < n and w not in seen:
        seen.add(w)
        owners.append((i, w))
        full[:, w] = np.stack([b[i] for b in blocks])
        mask[:, w] = 1 if act is None else act[:, i]
    until = op.get("until")
    res = self._twin_loop(dict(op="many_until" if until is not None else "many_active", K=K, form="plain",
                               fields=bool(op.get("fields")), actions=full, lo=0, mask=mask, mask_form="kn", mlo=0,
                               until=until, returns=op.get("returns", False), gamma=op.get("gamma", 1.0),
                               use_stopped=True))
    out = {}
    for key, value in res.items():
      if key == "stopped":
        out[key] = value
        continue
      g = np.full((M,) + value.shape[1:], 0, value.dtype)
      g.view(np.uint8)[...] = FILL
      for i, w in owners:
        g[i] = value[w]
      out[key] = g
    return out

  def _unit_tensor(self, shape, dtype, lo=0):
    """(out, wide): a zeroed destination of a registration that starts `lo` bytes into a wider
    buffer of FILL bytes (uint8 only), on the engine's device; the model's is a numpy array."""
    if not self.real:
      return np.zeros(shape, dtype), None
    import torch
    tdtype = {np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}[dtype]
    if dtype is not np.uint8:
      return torch.zeros(tuple(shape), dtype=tdtype, device=self.eng.device), None
    size = int(np.prod(shape))
    wide = torch.full((size + 48,), FILL, dtype=torch.uint8, device=self.eng.device)
    out = wide[lo:lo + size].view(tuple(shape))
    out.zero_()
    return out, wide

  def _units_set(self, op, ring):
    eng = self.eng
    lead = (ring,) if ring else ()
    for name in op["units"]:
      params = dict(op.get(name, {}))
      lo = params.pop("offset", 0)
      if name == "ego":
        out, wide = self._unit_tensor(lead + tuple(eng.ego_layer_shape), np.int32)
        eng.bind_ego_layer_ring(out) if ring else eng.bind_ego_layer(out)
      elif name == "hash":
        out, wide = self._unit_tensor(lead + (eng.N, eng.P), np.int64)
        eng.bind_view_hash(out, **params)
      else:
        table = params["classes"]
        C = int(table.max()) + 1 if params["num_classes"] is None else params["num_classes"]
        out, wide = self._unit_tensor(lead + tuple(eng.ego_planes_shape(C, params["facing"])), np.uint8, lo)
        eng.bind_ego_planes(out, **params)
      self.units[name] = dict(out=out, wide=wide, lo=lo, params=params)

  def _units_clear(self, name):
    eng = self.eng
    {"ego": eng.bind_ego_layer, "hash": eng.bind_view_hash, "planes": eng.bind_ego_planes}[name](None)
    del self.units[name]

  def unit_value(self, name):
    """The registered tensor of unit `name` on the host; raises if a guard byte around it changed."""
    u = self.units[name]
    if u["wide"] is not None:
      guard = u["wide"].cpu().numpy()
      size = guard.size - 48
      if (guard[:u["lo"]] != FILL).any() or (guard[u["lo"] + size:] != FILL).any():
        raise Mismatch(f"registered {name}: a guard byte around the destination (offset {u['lo']}) was written")
    return np.array(_host(u["out"]))

  def _unit_rows(self, op):
    eng, unit = self.eng, op["unit"]
    bank = None if op["bank"] < 0 else self.banks[op["bank"]]
    kw = dict(bank=bank, rows=self._ints(op["rows"]), players=None if op["players"] is None else self._ints(op["players"]))
    if unit == "ego":
      return np.array(_host(eng.observe_ego_layer(**kw)))
    if unit == "hash":
      return np.array(_host(eng.hash_views(**kw, **op["params"])))
    params = op["params"]
    if not self.real:
      return np.array(eng.observe_ego_planes(params["classes"], **kw, layers=params["layers"], facing=params["facing"],
                                             num_classes=params["num_classes"]))
    # the planes' `out` may start on any byte: inside a wider buffer, with guard bytes around it
    import torch
    shape = eng.ego_planes_shape(params["num_classes"], params["facing"])
    shape = (len(op["rows"]),) + tuple(shape[1:] if op["players"] is None else shape[2:])
    size, lo = int(np.prod(shape)), op["offset"]
    wide = torch.full((size + 48,), FILL, dtype=torch.uint8, device=eng.device)
    eng.observe_ego_planes(params["classes"], **kw, layers=params["layers"], facing=params["facing"],
                           num_classes=params["num_classes"], out=wide[lo:lo + size].view(shape))
    guard = wide.cpu().numpy()
    if (guard[:lo] != FILL).any() or (guard[lo + size:] != FILL).any():
      raise Mismatch(f"observe_ego_planes: a guard byte around `out` (offset {lo}) was written")
    return guard[lo:lo + size].reshape(shape).copy()

  def apply(self, op, ring, views=True):
    """Applies `op`.  A refused op (a list handed to an engine with a ring) must raise, which is kept
    in `raised`; the twin, which would run the masked form, leaves it out."""
    self.raised = None
    if not op.get("refused"):
      return self._apply(op, ring, views)
    self.rows = self.read = None
    if not self.twin:
      try:
        self._apply(op, ring, views)
      except (ValueError, E.EngineError) as e:
        self.raised = e

  def _apply(self, op, ring, views=True):
    eng, c = self.eng, op["op"]
    self.rows = self.read = None
    # (a twin that folds statistics on the host runs single steps, but for a ring, which a K-step
    # call turns once: there it folds the K rows of its own step_many)
    looped = self.twin and (self.reg is not None or c in NEW_STEP_CLASSES or (self.hstats is not None and not ring))
    if c == "reset_all":
      eng.reset()
      if self.twin:
        self._twin_fold()
    elif c == "masked_reset":
      eng.reset(None, op["mask"])
      if self.twin:
        self._twin_fold(op["mask"])
    elif c == "masked_reseed":
      eng.reset(op["seeds"], op["mask"])
      if self.twin:
        self._twin_fold(op["mask"])
    elif c in LISTED_CLASSES:
      self.rows = self._twin_listed(op) if self.twin else self._listed(op)
      if not self.rows:
        self.rows = None
    elif c == "stats_set":
      if self.twin:
        cols = tuple(eng.event_columns()) if isinstance(op["columns"], str) else tuple(op["columns"])
        self.hstats = dict(columns=cols, pairs=tuple(op["pairs"]),
                           arrays=E.numpy_episode_stats(eng.N, eng.P, len(cols), len(op["pairs"])))
      else:
        self.stats = eng.set_episode_stats(op["columns"], op["pairs"])
    elif c == "stats_clear":
      self.stats = self.hstats = None
      if not self.twin:
        eng.clear_episode_stats()
    elif c == "units_set":
      if not self.twin:
        self._units_set(op, ring)
    elif c == "units_clear":
      if not self.twin:
        self._units_clear(op["unit"])
    elif c == "unit_rows":
      self.read = self._unit_rows(op)
    elif c in ("step_dev", "step_host") and looped:
      self._twin_step(op["actions"], None, False)
    elif c == "step_fields" and looped:
      self._twin_step(op["fields"], None, True)
    elif c == "step_dev":
      eng.step(self.dev(op["actions"]))
      if self.twin:
        self._twin_fold()
    elif c == "step_host":
      eng.step(op["actions"])
      if self.twin:
        self._twin_fold()
    elif c == "step_fields":
      eng.step_fields(op["fields"] if op["host"] else self.dev(op["fields"]))
      if self.twin:
        self._twin_fold()
    elif c == "step_active" and looped:
      self._twin_step(op["actions"], op["mask"] != 0, False)
    elif c == "step_active":
      eng.step(op["actions"] if op["host"] else self.dev(op["actions"]), active=self._mask_arg(op))
    elif c in ("step_many", "step_many_rows", "many_active", "many_until", "step_many_states"):
      res = self._twin_loop(op) if looped else self._many(op)
      if c == "step_many_states":
        states = res.pop("states")
        if self.real:
          import torch
          states = (torch.stack(states) if isinstance(states, list) else states).reshape(op["K"] * eng.N, -1)
        else:
          states = [row for step in states for row in step]
        self.banks.append(states)
      self.rows = {k: np.array(_host(v)) for k, v in res.items()}   # (copies: `stopped` is the caller's)
    elif c == "unstop":
      self.stopped *= self.dev(1 - op["mask"]) if self.real and not self.twin else (1 - op["mask"])
    elif c == "starts_set":
      self.reg = dict(bank=op["bank"], fresh=op["fresh"])
      if self.twin:
        self.start_rows = op["rows"].copy()
      else:
        self.start_rows = self.dev(op["rows"].copy())
        eng.set_episode_starts(self.banks[op["bank"]], self.start_rows, fresh=op["fresh"])
    elif c == "starts_rows":   # the caller's tensor, rewritten in place: no engine call
      self.start_rows[:] = op["rows"] if self.twin else self.dev(op["rows"])
    elif c == "starts_clear":
      self.reg = None
      if not self.twin:
        eng.clear_episode_starts()
    elif c == "save":
      self.banks.append(eng.save_worlds(op["worlds"]))
    elif c == "load":
      eng.load_worlds(self.banks[op["bank"]], op["src"])
      if self.twin:
        self._twin_fold(op["src"] >= 0)
    elif c == "snapshot":
      self.snap = eng.snapshot()
    elif c == "restore":
      eng.restore(self.snap)
    elif c == "rebind":
      if views:
        bind_view(eng, op["kind"], ring) if op["bind"] else eng.unbind(op["kind"])
    elif c == "observe_rows":
      self.read = _host(eng.observe_states(self.banks[op["bank"]], op["kind"], rows=self._ints(op["rows"])))
    elif c == "observe_views":
      self.read = self._observe_views(op)
    elif c == "hash":
      spec = HASH_SPECS[op["spec"]] or {}
      if op["bank"] < 0:
        self.read = _host(eng.hash_worlds(**spec))
      else:
        rows = None if op["rows"] is None else self._ints(op["rows"])
        self.read = _host(eng.hash_states(self.banks[op["bank"]], rows, **spec))
    elif c == "check":
      self.read = self._check(op) if self.real and not self.twin else None
    else:
      raise ValueError(c)

  def _ints(self, a):
    return self.dev(np.asarray(a, np.int32))

  def _observe_views(self, op):
    eng = self.eng
    bank, kind = self.banks[op["bank"]], op["kind"]
    if not self.real or kind not in E.PIXEL_KINDS:
      return _host(eng.observe_views(bank, kind, self._ints(op["players"]), rows=self._ints(op["rows"])))
    # a pixel kind's `out` may start on any byte: inside a wider buffer, with guard bytes around it
    import torch
    shape = (len(op["rows"]),) + tuple(int(d) for d in eng.shapes[kind][0][2:])
    size, lo = int(np.prod(shape)), op["offset"]
    wide = torch.full((size + 48,), 0xA5, dtype=torch.uint8, device=eng.device)
    out = wide[lo:lo + size].view(shape)
    eng.observe_views(bank, kind, self._ints(op["players"]), rows=self._ints(op["rows"]), out=out)
    guard = wide.cpu().numpy()
    if (guard[:lo] != 0xA5).any() or (guard[lo + size:] != 0xA5).any():
      raise Mismatch(f"observe_views kind {kind}: a guard byte around `out` (offset {lo}) was written")
    return guard[lo:lo + size].reshape(shape).copy()

  def _check(self, op):
    """(verdicts of the whole bank, device verdict of a broken clone of one row, the host's)."""
    from meltingpot_amd import substrate
    eng = self.eng
    bank = self.banks[op["bank"]]
    verdicts = _host(eng.check_states(bank))
    clone = bank[op["row"]:op["row"] + 1].clone()
    f = substrate.StateFields(clone, eng.state_layout())
    alive = f.alive[0].cpu().numpy() != 0
    if op["field"] == "avatar_x" and alive.any():   # a living avatar off the map
      p = int(np.nonzero(alive)[0][op["player"] % int(alive.sum())])
      f.avatar_x[0, p] = 255
    else:
      f.orientation[0, op["player"]] = 7
    return verdicts, _host(eng.check_states(clone)), clone.cpu().numpy()


LISTED_FAULTS = (9, 10)   # word 11 of a bad entry of a list: not a world / repeats an earlier entry's


def _check_faults(eng, where, listed=False):
  """Stops the run on any fault word (the first 18, and 32..35 of a skipped registered start) before
  anything more is launched.  `listed`: a list with bad entries has been handed over, whose report
  leaves words 9..11 (position + 1, value, what): those alone may be set, with `what` one of
  LISTED_FAULTS."""
  words = np.asarray(eng.fault_words())
  seen = np.concatenate([words[:18], words[32:36]]).astype(np.int64)
  if listed and (words[11] & 255) in LISTED_FAULTS:
    seen[9:12] = 0
  if seen.any():
    raise FaultStop(f"{where}: fault words {words[:18].tolist()} {words[32:36].tolist()}; nothing more is launched")


def _bits(x):
  """float64 arrays compared bit for bit (-0.0 is not 0.0)."""
  x = np.asarray(x)
  return x.view(np.int64) if x.dtype == np.float64 else x


def compare_with_model(eng, model, rows, model_rows, fail, worlds=None, row_worlds=None, record_worlds=None,
                       stopped_worlds=None, listed=False):
  """Everything the model speaks about, engine against model; `fail(kind, text)` raises.
  `worlds`: the worlds the model speaks for (None: all) — the reported world is an index into it;
  `row_worlds`: those it spoke for through the whole call, whose per-step rows compare;
  `record_worlds`: those whose record it states (a restore puts records back, not buffers)."""
  def of(x, axis=0, worlds=worlds):
    return np.asarray(x) if worlds is None else np.take(np.asarray(x), worlds, axis=axis)

  note = "" if worlds is None else f" (of worlds {np.asarray(worlds).tolist()})"
  for name, got, want in zip(("record grid", "record avatars", "record globals"), eng.dump(), model.dump()):
    d = first_difference(name, of(got, 0, record_worlds), of(want, 0, record_worlds))
    if d:
      fail(name, d + ("" if record_worlds is None else f" (of worlds {np.asarray(record_worlds).tolist()})"))
  for kind in model.scalar_kinds:
    d = first_difference(kind, of(eng.observe_host(kind)), of(model.observe_host(kind)))
    if d:
      fail(f"kind {kind}", d + note)
  real = hasattr(eng, "_L")
  skip = {"hashes"} if real else set()   # (a model's hash is a stand-in: run_program checks the engine's)
  if (rows is None) != (model_rows is None) or (rows is not None and set(rows) - skip != set(model_rows) - skip):
    fail("step_many rows", f"keys {rows and sorted(map(str, rows))} != {model_rows and sorted(map(str, model_rows))}")
  for key in rows or ():
    if key in skip:
      continue
    if key in ("stopped", "ran", "returns"):   # [N] or [N, P] (a list: `stopped` by world, the others by entry)
      which = stopped_worlds if listed and key == "stopped" else row_worlds   # (a list: `stopped` is by world)
      d = first_difference(key, _bits(of(rows[key], 0, which)), _bits(of(model_rows[key], 0, which)))
    else:
      d = first_difference(key, of(rows[key], 1, row_worlds), of(model_rows[key], 1, row_worlds), leading=("step", "world"))
    if d:
      fail(f"step_many {'result' if key in ('stopped', 'ran', 'returns') else 'row'} {key}",
           d + ("" if row_worlds is None else f" (of worlds {np.asarray(row_worlds).tolist()})"))
  if worlds is None:   # (the count is the engine's, over all its worlds)
    got, want = eng.counters()["bad_actions"], model.counters()["bad_actions"]
    if got != want:
      fail("bad_actions", f"{got} != {want}")
  if dict(eng.ring) != dict(model.ring):
    fail("ring position", f"{dict(eng.ring)} != {dict(model.ring)}")
  for kind, want in model._bound.items():
    # (a ring kind: every slot — the one written last holds the model's, the others did not change)
    ring_kind = np.asarray(want).ndim == len(model.shapes[kind][0]) + 1
    d = first_difference(kind, of(_host(eng._bound[kind]), int(ring_kind)), of(want, int(ring_kind)),
                         leading=("slot", "world") if ring_kind else ("world",))
    if d:
      fail(f"{'ring' if ring_kind else 'bound'} kind {kind} (last slot {eng.ring['last']})", d + note)


def compare_reads(op, side, model_side, twin_side, fail):
  """A read-only op's result: against the model's `state_value` / `view_of` for the rows the model
  speaks for, against the twin's, and the hash's and the check's own conditions."""
  c, eng, model = op["op"], side.eng, model_side.eng
  if c in ("observe_rows", "observe_views"):
    mrows = [model_side.banks[op["bank"]][int(i)] for i in op["rows"]]
    keep = np.array([r.get("exact", True) for r in mrows])
    d = first_difference(op["kind"], side.read[keep], model_side.read[keep], leading=("row",))
    if d:
      fail(f"{c} kind {op['kind']}", d)
    if twin_side is not None:
      d = first_difference(op["kind"], side.read, twin_side.read, leading=("row",))
      if d:
        fail(f"twin: {c} kind {op['kind']}", d)
  elif c == "hash" and side.real:
    spec = HASH_SPECS[op["spec"]] or {}
    bank = eng.save_worlds() if op["bank"] < 0 else side.banks[op["bank"]]
    which = None if op["bank"] < 0 or op["rows"] is None else op["rows"]
    pack = profile_pack(side.profile)
    host = E.hash_states_host(pack, bank.cpu().numpy(), which=which, num_players=side.profile["num_players"], **spec)
    if not np.array_equal(side.read, host):
      fail("hash", f"device {side.read.tolist()} != hash_states_host {host.tolist()}")
    if twin_side is not None and not np.array_equal(side.read, twin_side.read):
      fail("twin: hash", f"{side.read.tolist()} != {twin_side.read.tolist()}")
    if not spec:   # "the state": equal model rows hash alike, rows whose dumps differ do not
      mbank = model.save_worlds() if op["bank"] < 0 else model_side.banks[op["bank"]]
      mrows = [mbank[int(i)] for i in (range(len(mbank)) if which is None else which)]
      keys = [model.row_key(r) if r.get("exact", True) else None for r in mrows]
      dumps = model.row_dumps(mrows)
      for i in range(len(mrows)):
        for j in range(i):
          if keys[i] is None or keys[j] is None:
            continue
          if keys[i] == keys[j] and side.read[i] != side.read[j]:
            fail("hash", f"elements {j} and {i} are one state (same seed, same log) and hash differently")
          differ = any(not np.array_equal(dumps[i][t], dumps[j][t]) for t in (0, 1))
          if differ and side.read[i] == side.read[j]:
            fail("hash", f"elements {j} and {i} differ in grid or avatars and hash alike")
  elif c == "check" and side.real:
    verdicts, broken, clone = side.read
    if verdicts.any():   # every state reached by play is well formed
      r = int(np.argwhere(verdicts.any(1))[0][0])
      fail("check", f"row {r} of bank {op['bank']}: {eng.state_layout().describe(*verdicts[r])}")
    host = E.check_states_host(profile_pack(side.profile), clone, num_players=side.profile["num_players"])
    if not np.array_equal(broken, host) or not broken.any():
      fail("check", f"a row with {op['field']} broken: device verdict {broken.tolist()}, host {host.tolist()}")


SUBMISSIONS = ("reset_all", "masked_reset", "masked_reseed", "load") + UNIT_STEP_CLASSES


def _stats_bytes(stats):
  """{name: numpy array} of an EpisodeStats, a statistics dict or the model's Model."""
  import episode_stats_model
  arrays = stats.arrays() if callable(getattr(stats, "arrays", None)) else getattr(stats, "arrays", stats)
  return {k: np.array(v) for k, v in episode_stats_model.flatten(arrays).items()}


def compare_stats(op, side, model_side, twin_side, before, fail):
  """The statistics tensors, bit for bit: against the model's for the worlds it has spoken for since
  the registration, against the twin's host fold (`episode_stats_host` of what the twin's steps left)
  for every world, and unchanged by an op that is no submission."""
  if side.stats is None:
    return
  got = _stats_bytes(side.stats)
  model = model_side.eng
  keep = np.nonzero(model.stats_exact)[0]
  want = _stats_bytes(model.stats)
  if got.keys() != want.keys():
    fail("statistics", f"tensors {sorted(got)} != {sorted(want)}")
  for key in want:
    if got[key].dtype != want[key].dtype:
      fail(f"statistics {key}", f"dtype {got[key].dtype} != {want[key].dtype}")
    d = first_difference(key, _bits(got[key][keep]), _bits(want[key][keep]))
    if d:
      fail(f"statistics {key}", d + f" (of worlds {keep.tolist()})")
  if twin_side is not None and twin_side.hstats is not None:
    for key, want in _stats_bytes(twin_side.hstats["arrays"]).items():
      d = first_difference(key, _bits(got[key]), _bits(want))
      if d:
        fail(f"twin: statistics {key} against episode_stats_host of the twin's steps", d)
  if before is not None and (op["op"] not in SUBMISSIONS or op.get("refused")) and op["op"] != "stats_set":
    for key in got:
      if got[key].tobytes() != before[key].tobytes():
        fail(f"statistics {key}", "changed by an op that is no submission")


def _unit_host(side, name, params, rows, players=None, which=None):
  """Unit `name` by the library's host form on host rows (uint8 [R, S])."""
  pack, np_ = profile_pack(side.profile), side.profile["num_players"]
  fp = side.eng.state_fingerprint
  if name == "ego":
    return E.ego_layer_host(pack, rows, players, which=which, num_players=np_, fingerprint=fp)
  if name == "hash":
    return E.hash_views_host(pack, rows, players, which=which, num_players=np_, fingerprint=fp, **params)
  return E.ego_planes_host(pack, rows, params["classes"], players, which=which, layers=params["layers"],
                           facing=params["facing"], num_classes=params["num_classes"], num_players=np_, fingerprint=fp)


def compare_units(op, side, model_side, before, fail):
  """Every registered tensor: after a submission the unit's function of ALL N records as they are
  now, in a ring in the slot the submission wrote with the other slots unchanged — by the model for
  the worlds it speaks for, by the library's host form on the engine's own save_worlds() for all —
  and after any other op unchanged."""
  if not side.units:
    return
  eng, model = side.eng, model_side.eng
  submitted = op["op"] in SUBMISSIONS and not op.get("refused")
  rows = eng.save_worlds().cpu().numpy() if side.real and submitted else None
  for name, u in side.units.items():
    got = side.unit_value(name)
    fresh = op["op"] == "units_set" and name in op["units"]   # (a new tensor, zeroed)
    if name in before and not submitted and not fresh and got.tobytes() != before[name].tobytes():
      fail(f"registered {name}", "changed by an op that is no submission")
    if fresh and got.any():
      fail(f"registered {name}", "written by its registration")
    ring = side.profile["ring"]
    want = model_side.unit_value(name)
    speaks = model.unit_speaks(name) if hasattr(model, "unit_speaks") else np.ones(got.shape[:2 if ring else 1], bool)
    lead = ("slot", "world") if ring else ("world",)
    g, w = got[speaks], want[speaks]
    if not np.array_equal(g, w):
      at = np.argwhere(speaks)[np.argwhere((g != w).reshape(len(g), -1).any(1))[0][0]]
      fail(f"registered {name} (last slot {eng.ring['last']})",
           f"{', '.join(f'{n} {int(v)}' for n, v in zip(lead, at))} differs from the model's")
    if rows is not None:
      host = _unit_host(side, name, u["params"], rows)
      last = got[eng.ring["last"]] if ring else got
      d = first_difference(name, last, host)
      if d:
        fail(f"registered {name} against the host form of save_worlds()", d)
      if ring and name in before and not fresh:
        others = [t for t in range(ring) if t != eng.ring["last"]]
        if got[others].tobytes() != before[name][others].tobytes():
          fail(f"registered {name}", f"a slot other than {eng.ring['last']} was written")


def compare_unit_rows(op, side, model_side, twin_side, fail):
  """A unit_rows read: against the model's for the rows it speaks for, against the library's host
  form of the same rows, and against the twin's."""
  model, name = model_side.eng, op["unit"]
  if op["bank"] < 0:
    keep = np.asarray(model.exact)[op["rows"]] if hasattr(model, "exact") else np.ones(len(op["rows"]), bool)
  else:
    keep = np.array([model_side.banks[op["bank"]][int(i)].get("exact", True) for i in op["rows"]])
  d = first_difference(name, side.read[keep], model_side.read[keep], leading=("row",))
  if d:
    fail(f"unit_rows {name}", d)
  if side.real:
    bank = side.eng.save_worlds() if op["bank"] < 0 else side.banks[op["bank"]]
    host = _unit_host(side, name, op.get("params", {}), bank.cpu().numpy(), op["players"], which=op["rows"])
    d = first_difference(name, side.read, host, leading=("row",))
    if d:
      fail(f"unit_rows {name} against the host form", d)
  if twin_side is not None:
    d = first_difference(name, side.read, twin_side.read, leading=("row",))
    if d:
      fail(f"twin: unit_rows {name}", d)


def compare_views_with_model(eng, model, fail, kinds=engine_model.VIEW_KINDS, worlds=None):
  """Every view kind drawn by mp_observe from the records, against the model's (`worlds`: the
  worlds the model speaks for; None: all)."""
  pick = (lambda x: x) if worlds is None else (lambda x: np.take(x, worlds, axis=0))
  for kind in kinds:
    d = first_difference(kind, pick(eng.observe_host(kind)), pick(model.view_value(kind)))
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


def compare_many_with_twin(op, side, twin_side, locate, fail):
  """A K-step op of the state classes: the engine's one call against the twin's host loop."""
  import torch
  from test_gpu_world_states import _no_counters
  for key in ("ran", "stopped", "returns", "hashes"):
    if key in (twin_side.rows or ()):
      d = first_difference(key, _bits(side.rows[key]), _bits(twin_side.rows[key]),
                           leading=("step", "world") if key == "hashes" else ("world",))
      if d:
        fail(f"twin: step_many result {key}", d)
  if op["op"] == "step_many_states":
    a, b = _no_counters(side.banks[-1], locate), _no_counters(twin_side.banks[-1], locate)
    if not torch.equal(a, b):
      fail("twin: step_many states", first_difference("rows", _host(a), _host(b), leading=("row",)))
    # hashes[k, w] is hash_states of states[k, w]
    again = _host(side.eng.hash_states(side.banks[-1])).reshape(side.rows["hashes"].shape)
    d = first_difference("hashes", side.rows["hashes"], again, leading=("step", "world"))
    if d:
      fail("step_many hashes against hash_states of its states", d)


def _cover(cover, op, model_side, taken_before):
  """What a run contained that only the runner sees (the rest is the model's own `cover`)."""
  c, model = op["op"], model_side.eng
  if c == "restore" and np.asarray(model_side.stopped).any():
    cover["restore while a stopped byte is set"] += 1
  if c == "masked_reseed" and model_side.reg is not None:
    cover["masked_reseed while a registration is set"] += 1
  if c == "starts_rows" and model_side.reg is not None:
    model_side.rewritten = True
  if c == "starts_set":
    model_side.rewritten = False
  if getattr(model_side, "rewritten", False) and model.cover["registered start"] > taken_before:
    cover["starts_rows rewrite between registration and use"] += 1
    model_side.rewritten = False
  if c in ("load", "observe_rows", "observe_views") and model_side.states_banks.get(op["bank"]):
    cover[("load" if c == "load" else "observe_*") + " from a step_many_states bank"] += 1
  if c in ("observe_rows", "observe_views"):
    rows = [model_side.banks[op["bank"]][int(i)] for i in op["rows"]]
    if any((d[1][:, 3] == 0).any() and not r["finished"] for r, d in zip(rows, model.row_dumps(rows))):
      cover["a row with a dead avatar among the drawn rows"] += 1


def _final_cover(cover, model):
  if model.stats is not None:
    cover["non-zero total.counts at the end"] += int(model.stats.total["counts"].any())
    cover["non-zero total.pairs at the end"] += int(model.stats.total["pairs"].any())


def run_program(program, engine, model, twin=None, stop_after=None, cover=None):
  """Applies each op of `program` (its first `stop_after`, if given) to `engine`, `model` and
  `twin`, comparing after every op; raises Mismatch / FaultStop naming seed, profile, op and kind.
  `cover`: a Counter that takes what the run contained.  Returns the number of ops run."""
  import collections
  profile = program.profile
  ring = profile["ring"]
  sides = [_Side(engine), _Side(model)] + ([_Side(twin, twin=True)] if twin is not None else [])
  for side in sides:
    side.profile = profile
  side, model_side, twin_side = sides[0], sides[1], sides[2] if twin is not None else None
  model_side.states_banks = {}
  cover = collections.Counter() if cover is None else cover
  locate = None
  ran = 0
  bad_lists = False
  for i, op in enumerate(program[:stop_after]):
    where = f"program seed {program.seed}, profile {profile['name']}, op {i}: {short_form(op)}"

    def fail(kind, text):
      raise Mismatch(f"{where}: {kind}: {text}")

    op = resolve(op, model_side)
    taken_before = model.cover["registered start"] if hasattr(model, "cover") else 0
    exact_before = model.speaks.copy() if hasattr(model, "speaks") else None
    units_before = {name: side.unit_value(name) for name in side.units}
    stats_before = None if side.stats is None else _stats_bytes(side.stats)
    for k, s in enumerate(sides):
      s.apply(op, ring, views=k < 2)   # (the twin binds no view)
    if op["op"] == "step_many_states":
      model_side.states_banks[len(model_side.banks) - 1] = True
    if op.get("refused"):   # a list handed to an engine with a ring: refused, and nothing changes
      for s in sides[:2]:
        if s.raised is None or "ring" not in str(s.raised):
          fail("a list under a ring", f"not refused ({s.raised!r})")
    if op.get("bad") and not op.get("refused") and side.real:
      # bad entries: the next synchronising call raises ValueError once, naming one of them
      bad_lists = True
      try:
        engine.dump()
      except ValueError as e:
        named = [i for i in range(len(op["worlds"])) if f"worlds[{i}] = {int(op['worlds'][i])} " in str(e)]
        owned = {i for i, _ in engine_model.ModelEngine._owners(engine, op["worlds"])}
        if "MpStepListed" not in str(e) or not named or named[0] in owned:
          fail("bad entries", f"the error names none of them: {e}")
      else:
        fail("bad entries", "the next synchronising call raised nothing")
    # (dump synchronises; a fault word ends the run before anything else is launched)
    engine.dump()
    _check_faults(engine, where, bad_lists)
    if twin is not None:
      twin.dump()
      _check_faults(twin, where + " (twin)")
    exact = getattr(model, "speaks", None)
    worlds = None if exact is None or exact.all() else np.nonzero(exact)[0]
    # (a world the model did not speak for when the call began may be one it speaks for now — it
    # restarted from a row — but its rows of the steps before that are not the model's)
    both = None if exact is None or (exact & exact_before).all() else np.nonzero(exact & exact_before)[0]
    records = None if exact is None or model.exact.all() else np.nonzero(model.exact)[0]
    if op["op"] in LISTED_CLASSES and both is not None:
      # per-call tensors by ENTRY: those whose world the model spoke for, and the bad ones
      entries = np.array([i for i, w in enumerate(op["worlds"].tolist()) if not 0 <= w < engine.N or w in set(both.tolist())],
                         np.int64)
      compare_with_model(engine, model, side.rows, model_side.rows, fail, worlds, entries, records, stopped_worlds=both, listed=True)
    else:
      compare_with_model(engine, model, side.rows, model_side.rows, fail, worlds, both, records)
    if hasattr(model, "stats_exact"):
      model.stats_exact &= model.speaks
    compare_units(op, side, model_side, units_before, fail)
    compare_stats(op, side, model_side, twin_side, stats_before, fail)
    if both is not None:
      # a `stopped` byte decided while the model did not speak for its world is the engine's to say
      # (the twin checks it): the model's side takes it over, so that the world compares again once
      # the model speaks for it
      other = np.setdiff1d(np.arange(engine.N), both)
      model_side.stopped[other] = _host(side.stopped)[other]
    d = first_difference("stopped", _host(side.stopped), _host(model_side.stopped))
    if d:
      fail("the caller's `stopped`", d)
    if op["op"] in ("load", "restore"):   # (mp_observe draws from the records: a restore is no launch)
      compare_views_with_model(engine, model, fail, worlds=records)
    if op["op"] in READ_ONLY:
      compare_reads(op, side, model_side, twin_side, fail)
    if op["op"] == "unit_rows":
      compare_unit_rows(op, side, model_side, twin_side, fail)
    if hasattr(model, "cover"):
      _cover(cover, op, model_side, taken_before)
    if twin is not None:
      if locate is None:   # (world 0 still has its first seed: it locates the counters' bytes)
        locate = engine.save_worlds().clone()
      compare_with_twin(engine, twin, locate, fail)
      if op["op"] in NEW_STEP_CLASSES or op["op"] == "many_listed":
        compare_many_with_twin(op, side, twin_side, locate, fail)
      if not np.array_equal(_host(side.stopped), twin_side.stopped):
        fail("twin: the caller's `stopped`", f"{_host(side.stopped).tolist()} != {twin_side.stopped.tolist()}")
    ran += 1
  if ran:
    compare_views_with_model(engine, model, fail, worlds=records)
    _check_faults(engine, "end of program", bad_lists)
  if hasattr(model, "cover"):
    _final_cover(cover, model)
    cover.update(model.cover)
    cover["inexact worlds at the end"] += int((~model.exact).sum())
  return ran


def program_cover(program):
  """What a run of `program` contains, by the model alone (no engine is looked at): a Counter."""
  import collections
  profile = program.profile
  model = make_model(profile)
  side = _Side(model)
  side.profile, side.states_banks = profile, {}
  cover = collections.Counter()
  try:
    for op in program:
      op = resolve(op, side)
      taken_before = model.cover["registered start"]
      side.apply(op, profile["ring"])
      if op["op"] == "step_many_states":
        side.states_banks[len(side.banks) - 1] = True
      _cover(cover, op, side, taken_before)
    _final_cover(cover, model)
    cover.update(model.cover)
    cover["inexact worlds at the end"] += int((~model.exact).sum())
  finally:
    model.close()
  return cover


# what the model's run of a level's two programs must contain (the reward conditions apart)
COVER_CONDITIONS = (
    "stopped by LAST with steps left to skip",
    "paused on LAST, restarts in a later active step",
    "registered start inside step k >= 1 of a K-step call",
    "two worlds take one row in one step beside a world with -1",
    "starts_rows rewrite between registration and use",
    "restore while a stopped byte is set",
    "masked_reseed while a registration is set",
    "load from a step_many_states bank",
    "observe_* from a step_many_states bank",
)
DEAD_AVATAR_CONDITION = "a row with a dead avatar among the drawn rows"
REWARD_CONDITIONS = (
    "stopped by REWARD with steps left to skip",
    "returns with gamma != 1 paid after the first step the world ran",
    "non-zero reward on the step that leaves LAST",
)


# what the model's runs of a level's two unit programs must contain
UNIT_COVER_CONDITIONS = (
    "a listed call with bad entries, statistics registered",
    "a listed call names a world paused on LAST",
    "a listed until= call meets a stopped byte set under a different list",
    "a listed call with a registered start inside step k >= 1",
    "an episode finishes after an open one was cut",
    "an episode finishes inside step k >= 1 of a K-step call, statistics registered",
    "restore while statistics are registered",
    "restore changed a record, then a step skipped that world, a unit registered",
    "a registered view at orientation 0",
    "a registered view at orientation 1",
    "a registered view at orientation 2",
    "a registered view at orientation 3",
    "units_clear followed by submissions of every slot",
    "stats_set over a live registration",
    "non-zero total.counts at the end",
    "non-zero total.pairs at the end",
)
UNIT_DEAD_VIEWER = "a registered view of a dead viewer"
UNIT_OFF_THE_MAP = "a registered window cell off the map"


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
