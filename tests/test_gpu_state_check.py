"""The record check on the GPU: k_check_states judges rows where they lie.  No row the engine
produces is flagged; the device's verdicts are the host loop's on the same bytes, mutation by
mutation; a checked load leaves the world of a malformed row alone and names it at the next
synchronising call; valid edits made through `state_fields` pass, load and step; and a check
moves nothing of the engine's.

One rule for every test here: no malformed row is loaded or stepped unchecked.  A mutated row
gets its verdict on the host first, and goes near a load only with check=True."""
import numpy as np
import pytest
import torch

import states_recipe as R
import test_state_check_cpu as C
import test_state_rows_fixture_cpu as F
import util
from meltingpot_amd import engine, substrate

pytestmark = pytest.mark.gpu

E = engine
N = R.N


def _clean(eng, verdicts, what):
  v = verdicts.cpu().numpy()
  lay = eng.state_layout()
  assert not v.any(), (what, [(i, lay.describe(*x)) for i, x in enumerate(v) if x.any()][:4])


# ---- no false positives ------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_rows_the_engine_produces_pass(name):
  road = R.road(name)
  e = engine.Engine(R.pack(name), N, device=0)
  bank = road["all"]
  _clean(e, e.check_states(bank, fingerprint=road["fingerprint"]), "road")
  # row lists: repeats, ragged workgroups (1, 3, 7 rows), a non-contiguous pick
  for rows in ([3], [24, 0, 24], [1, 1, 5, 20, 7, 7, 13], list(range(0, 25, 3))):
    v = e.check_states(bank, rows=rows)
    assert v.shape == (len(rows), 2)
    _clean(e, v, rows)
  # after a reset, over 24 steps of one launch (auto-resets at step 17), after a load
  e.reset()
  _clean(e, e.check_states(e.save_worlds()), "reset")
  A = torch.from_numpy(road["actions"]).to(e.device)
  many = e.step_many(A, states=True)["states"]
  _clean(e, e.check_states(many.view(R.STEPS * N, -1)), "step_many")
  e.load_worlds(bank, [7, -1, 12, 24, 0])
  _clean(e, e.check_states(e.save_worlds()), "load")
  e.sync()
  util.no_faults(e)
  e.close()
  # frozen worlds: no auto-reset, eight steps past the end of the episode
  e = engine.Engine(R.pack(name), N, device=0, auto_reset=False)
  e.reset()
  many = e.step_many(A, states=True)["states"]
  _clean(e, e.check_states(many[-3:].reshape(3 * N, -1)), "frozen")
  e.sync()
  util.no_faults(e)
  e.close()


# ---- device equals host --------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_device_verdicts_are_the_host_loops(name):
  e = engine.Engine(R.pack(name), N, device=0)
  lay = substrate.SubstrateStateLayout(e.state_layout(), C.tables(name))
  assert e.state_layout().fields == C.layout(name).fields and e.state_layout().fingerprint == C.layout(name).fingerprint
  # every mutation of the CPU tests, of the fixture's real rows and of the states built by hand
  real, built = F.rows_of(name), C.built_rows(name)
  base = torch.from_numpy(np.concatenate([real, built])).to(e.device)
  muts = ([(m, m[3]) for m in C.all_mutations(name, real, F.dead_row(name))] +
          [(m, len(real) + m[3]) for m in C.all_mutations(name)])
  bank = torch.stack([base[row] for _, row in muts]).contiguous()
  muts = [m for m, _ in muts]
  for i, m in enumerate(muts):   # the mutation applied on the device, through the field views
    m[1](substrate.StateFields(bank[i:i + 1], lay))
  host = C.verdicts(name, bank.cpu().numpy())
  for m, v in zip(muts, host):   # (the host's verdict first: these are the CPU tests' own)
    assert tuple(int(x) for x in v) == m[2], (name, m[0])
  dev = e.check_states(bank).cpu().numpy()
  assert (dev == host).all(), [(m[0], d.tolist(), h.tolist()) for m, d, h in zip(muts, dev, host) if (d != h).any()]
  # and on the unmutated rows next to them, in one bank, picked by a row list
  both = torch.cat([bank, base])
  rows = list(range(len(both) - 1, -1, -1))
  dev = e.check_states(both, rows=rows).cpu().numpy()
  assert (dev == C.verdicts(name, both.cpu().numpy(), which=rows)).all()
  e.sync()
  e.close()


def test_a_row_index_outside_the_bank_is_reported_not_read():
  name = "coins"
  e = engine.Engine(R.pack(name), N, device=0)
  bank = torch.from_numpy(C.rows_of(name)).to(e.device)
  v = e.check_states(bank, rows=[0, len(bank), 2]).cpu().numpy()
  assert v.tolist() == [[0, 0], [-1, len(bank)], [0, 0]]
  with pytest.raises(ValueError, match=r"MpStatesCheck: rows\[1\] = %d" % len(bank)):
    e.sync()
  e.sync()   # reported once
  with pytest.raises(ValueError, match="fingerprint"):
    e.check_states(bank, fingerprint=5)
  e.close()


# ---- checked load ----------------------------------------------------------------------------------
def _tail_free(eng, rows):
  """`rows` without ctr[] and reward_fx (a load keeps the destination's)."""
  lay = eng.state_layout()
  keep = torch.ones(rows.shape[1], dtype=torch.bool, device=rows.device)
  keep[lay.field_offset("ctr"):lay.field_offset("reward_fx") + 4] = False
  return rows[:, keep]


@pytest.mark.parametrize("name,ring", [("clean_up", False), ("territory__rooms", False), ("clean_up", True)])
def test_checked_load_refuses_the_malformed_row_only(name, ring):
  cfg = substrate.get_config(name)
  kw = {"rollout_length": 2} if ring else {}
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=N, env_seed=41, **kw)
  twin = substrate.build(name, roles=cfg.default_player_roles, num_worlds=N, env_seed=41, **kw)
  eng = env._eng
  P, nact = env.num_players, env.action_spec()[0].num_values
  A = util.random_actions(np.random.default_rng(4), 6, N, P, nact)
  env.reset(); twin.reset()
  for k in range(3):
    env.step(A[k]); twin.step(A[k])
  states = env.save_state()
  for k in range(3, 6):
    env.step(A[k]); twin.step(A[k])
  f = env.state_fields(states)
  assert states.edited
  f.avatar_x[0, 0] = 255   # row 0: a living avatar off the map
  lay = env.state_layout()
  bad = (E.RULE_AVATAR_CELL, lay.field_offset("ax", 0))
  host = E.check_states_host(eng.pack_bytes, states.data.cpu().numpy(), fingerprint=states.fingerprint,
                             num_players=P)
  assert tuple(host[0]) == bad and not host[1:].any()   # on the host first
  assert env.check_states(states).cpu().numpy().tolist() == host.tolist()
  before = env.save_state().data.clone()
  src = [0, 3, -1, len(states), -1]   # world 0: the mutated row; 1: a good one; 2: none; 3: out of range
  ts = env.load_state(states, src)   # (edited: checked without being asked)
  # (the twin loads the good row alone, unchecked, from rows nobody edited)
  tw = twin.load_state(substrate.WorldStates(states.data.clone(), states.fingerprint), [-1, 3, -1, -1, -1],
                       check=False)
  after = env.save_state().data
  for w in (0, 2, 3, 4):
    assert torch.equal(after[w], before[w]), w
  assert torch.equal(_tail_free(eng, after[1:2]), _tail_free(eng, states.data[3:4]))
  if ring:   # the checked load wrote the slot an unchecked load writes
    assert ts.slot == tw.slot
  with pytest.raises(ValueError) as err:
    eng.sync()
  msg = str(err.value)
  assert "src[0]" in msg and "row 0," in msg and "rule 4" in msg and "world 0 " in msg, msg
  # the index out of range is the load's own report: the load runs behind the filter and writes
  # words 9-11 last, and the first sync left them (word 11 was the load's); then nothing is left
  with pytest.raises(ValueError, match=r"src\[3\]"):
    eng.sync()
  eng.sync()
  env.step(A[0]); twin.step(A[0])
  eng.sync()
  util.no_faults(eng)
  assert torch.equal(_tail_free(eng, env.save_state().data[1:2]), _tail_free(eng, twin.save_state().data[1:2]))
  env.close(); twin.close()


# ---- valid edits -----------------------------------------------------------------------------------
def _free_cell(fields, lay, row, planes):
  g = fields.grid[row].cpu().numpy()
  for y in range(1, lay.H - 1):
    for x in range(1, lay.W - 1):
      if all(g[p, y, x] == 0 for p in planes):
        return x, y
  raise AssertionError("no free cell")


@pytest.mark.parametrize("name", ["clean_up", "collaborative_cooking__cramped"])
def test_a_moved_avatar_passes_loads_and_steps(name):
  cfg = substrate.get_config(name)
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=2, env_seed=43)
  twin = substrate.build(name, roles=cfg.default_player_roles, num_worlds=2, env_seed=43)
  eng = env._eng
  P, nact = env.num_players, env.action_spec()[0].num_values
  env.reset(); twin.reset()
  A = util.random_actions(np.random.default_rng(5), 9, 2, P, nact)
  env.step(A[0]); twin.step(A[0])
  original = env.save_state()
  states = substrate.WorldStates(original.data.clone(), original.fingerprint)
  lay = env.state_layout()
  f = env.state_fields(states)
  AL = lay.avatar_layer
  cook = name.startswith("collaborative_cooking")
  ov = lay.state_layers[lay.state_id("inventory.empty")] if cook else -1
  p = 0
  x0, y0 = int(f.avatar_x[0, p]), int(f.avatar_y[0, p])
  planes = [AL, ov] if cook else [AL]
  # (a cell with nothing on it but floor: no wall, apple, water or counter)
  x1, y1 = _free_cell(f, lay, 0, [l for l in range(lay.L)
                                  if lay.layer_names[l] not in ("logic", "alternateLogic", "background")])
  for pl in planes:   # the avatar's byte — in the kitchen also its connected inventory piece
    f.grid[0, pl, y1, x1] = f.grid[0, pl, y0, x0]
    f.grid[0, pl, y0, x0] = 0
  f.avatar_x[0, p] = x1
  f.avatar_y[0, p] = y1
  host = E.check_states_host(eng.pack_bytes, states.data.cpu().numpy(), fingerprint=states.fingerprint, num_players=P)
  assert not host.any(), [lay.describe(*v) for v in host]
  assert not env.check_states(states).cpu().numpy().any()
  pos = env.observe_states(states, ("POSITION",))["POSITION"]
  assert pos[0, p].tolist() == [x1, y1] and torch.equal(pos[1], env.observe_states(original, ("POSITION",))["POSITION"][1])
  new = env.observe_states(states, ("WORLD.RGB",))["WORLD.RGB"]
  old = env.observe_states(original, ("WORLD.RGB",))["WORLD.RGB"]
  S = new.shape[1] // lay.H
  diff = (new[0] != old[0]).any(-1).cpu().numpy()
  assert diff.any()
  inside = np.zeros_like(diff)
  for x, y in ((x0, y0), (x1, y1)):
    inside[y * S:(y + 1) * S, x * S:(x + 1) * S] = True
  assert not (diff & ~inside).any() and torch.equal(new[1], old[1])
  # load (auto-checked: the rows are edited) into two substrates; NOOPs, then the same actions
  assert states.edited
  env.load_state(states, [0, 1]); twin.load_state(states, [0, 1])
  noop = np.zeros((2, P), np.int32)
  env.step(noop); twin.step(noop)
  eng.sync(); twin._eng.sync()
  util.no_faults(eng); util.no_faults(twin._eng)
  for k in range(1, 9):
    env.step(A[k]); twin.step(A[k])
  a, b = env.save_state().data, twin.save_state().data
  assert torch.equal(a, b)
  assert not env.check_states(env.save_state()).cpu().numpy().any()
  eng.sync()
  util.no_faults(eng)
  env.close(); twin.close()


def test_an_edited_seed_needs_the_orders_cache_cleared():
  """The cached orders are a function of (seed, episode, step): the check cannot tell a stale
  cache from a fresh one (both are permutations under the right step tag), so the rule of thumb
  is the documentation's — after editing seed, episode or step, set orders_step = 0."""
  name = "clean_up"
  cfg = substrate.get_config(name)
  env = substrate.build(name, roles=cfg.default_player_roles, num_worlds=2, env_seed=44)
  P, nact = env.num_players, env.action_spec()[0].num_values
  # (200 steps: clean_up's dirt only starts to spawn after 50, and the draws have to show)
  A = util.random_actions(np.random.default_rng(6), 200, 2, P, nact)
  env.reset()
  env.step(A[0])
  original = env.save_state()
  states = substrate.WorldStates(original.data.clone(), original.fingerprint)
  f = env.state_fields(states)
  f.seed[0] = int(f.seed[0]) ^ 0x5DEECE66D
  stale = env.check_states(states).cpu().numpy()
  assert not stale.any()   # (the check cannot tell: see the docstring)
  f.orders_step[0] = 0
  assert not env.check_states(states).cpu().numpy().any()

  def run(s):
    env.load_state(s, [0, 1])
    env.step_many(A[1:])
    return env.save_state().data.clone()
  lay = env.state_layout()
  edited, plain = run(states), run(original)
  planes = lay.grid_planes * lay.H * lay.W
  assert not torch.equal(edited[0, :planes], plain[0, :planes])   # another continuation
  assert torch.equal(_tail_free(env._eng, edited[1:2]), _tail_free(env._eng, plain[1:2]))   # world 1: untouched
  env._eng.sync()
  util.no_faults(env._eng)
  env.close()


# ---- nothing else moved ------------------------------------------------------------------------------
def test_a_check_changes_nothing_of_the_engine():
  name = "clean_up"
  e = engine.Engine(R.pack(name), N, device=0)
  ring = {k: e.bind_ring(k, slots=3) for k in (E.OBS_RGB, E.OBS_REWARD)}
  plain = {k: e.bind(k) for k in (E.OBS_WORLD_RGB, E.OBS_POSITION, E.OBS_STEP_TYPE, E.OBS_EVENTS)}
  A = torch.from_numpy(R.actions(e.P, e.num_actions)).to(e.device)
  e.reset()
  for s in range(4):
    e.step(A[s])
  bank = torch.from_numpy(C.rows_of(name)).to(e.device)
  before = (e.snapshot(), e.counters(), e.ring, {k: v.clone() for k, v in {**ring, **plain}.items()}, e.plan)
  e.check_states(bank)
  e.check_states(e.save_worlds(), rows=[4, 0])
  after = (e.snapshot(), e.counters(), e.ring, {**ring, **plain}, e.plan)
  assert (before[0] == after[0]).all() and before[1] == after[1] and before[2] == after[2] and before[4] == after[4]
  for k, v in before[3].items():
    assert torch.equal(v, after[3][k]), k
  e.sync()
  util.no_faults(e)
  e.close()
