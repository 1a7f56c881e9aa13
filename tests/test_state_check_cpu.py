"""The record check without a GPU: the layout the library tells (MpStateLayout) and the host-only
form of the check (MP_CHECK_HOST: the kernel's rule functions compiled for the host), on states
built by hand through the field views and on mutations of them with their exact verdicts; and the
Python surface on CPU tensors.  (Rows an engine saved are judged where an engine runs:
tests/test_gpu_state_check.py.)"""
import ctypes
import functools

import numpy as np
import pytest

import states_recipe as R
from meltingpot_amd import engine as E
from meltingpot_amd import pack as pack_lib
from meltingpot_amd import substrate as S

COOK = "collaborative_cooking__cramped"
MUSHROOMS = "externality_mushrooms__dense"
CASES = tuple(R.PACKS)


def base_name(name):
  return name


def pack_of(name):
  """The recipe's pack of a case."""
  return R.pack(name)


@functools.lru_cache(maxsize=None)
def layout(name):
  return E.state_layout(pack_of(name))


@functools.lru_cache(maxsize=None)
def tables(name):
  return pack_lib.loads(pack_of(name))


def rows_of(name):
  """Six well-formed rows of the level: the states built by hand, three times over."""
  return np.concatenate([built_rows(name)] * 3)


def verdicts(name, rows, **kw):
  return E.check_states_host(pack_of(name), rows, fingerprint=layout(name).fingerprint, **kw)


# ---- structure ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PACKS)
def test_layout_agrees_with_the_pack(name):
  lay, t = layout(name), tables(name)
  assert lay.tail_bytes == 400 and lay.layout_version == 1
  assert lay.H * lay.W * lay.L == t["init_grid"].size
  assert lay.L == len(bytes(t["layer_names"]).split(b"\0")) - 1
  assert lay.nstates == len(bytes(t["state_names"]).split(b"\0")) - 1
  assert lay.grid_planes >= lay.L
  planes = lay.H * lay.W * lay.grid_planes
  if lay.player_block < 0:
    assert lay.grid_bytes == planes
  else:   # the matrix games keep a block of 16 x 32 bytes behind the planes
    assert lay.player_block == (planes + 15) // 16 * 16 and lay.grid_bytes == lay.player_block + 16 * 32
  assert lay.grid_pad == (lay.grid_bytes + 15) // 16 * 16
  assert lay.world_stride % 64 == 0 and lay.world_stride >= lay.grid_pad + lay.tail_bytes
  assert lay.max_frames == R.LAST_STEP and lay.fingerprint != 0
  assert E.state_layout(R.pack(name)).fingerprint == lay.fingerprint != E.state_layout(engine_pack(name)).fingerprint
  # the fields tile the tail: no overlap, no gap
  spans = sorted((off, off + elem * count) for off, elem, count in lay.fields.values())
  assert spans[0][0] == 0 and spans[-1][1] == lay.tail_bytes
  assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
  assert lay.fields["seed"][1:] == (8, 1) and lay.fields["next_orders"][1:] == (2, 16) and lay.fields["ax"][1:] == (1, 16)


def test_layout_request_refusals():
  L = E.load_library()
  req = E.MpStateLayout(ctypes.sizeof(E.MpStateLayout))
  with pytest.raises(ValueError, match="bad MpConfig"):   # no engine and no pack: the host stage's refusal
    E._check(L, L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)), "layout")
  with pytest.raises(ValueError, match="fingerprint"):
    E.check_states_host(R.pack("coins"), rows_of("coins"), fingerprint=1)
  with pytest.raises(ValueError, match="rows of"):
    E.check_states_host(R.pack("coins"), rows_of("clean_up"))


def engine_pack(name):
  """The committed pack (the recipe's has episodes of 16 frames: another pack, another fingerprint)."""
  return E.load_pack(name)


def test_row_lists_and_bad_indices():
  rows = rows_of("clean_up")
  v = verdicts("clean_up", rows, which=[5, 0, 0, 3])
  assert v.shape == (4, 2) and not v.any()
  v = verdicts("clean_up", rows, which=[1, len(rows), -2])
  assert v.tolist() == [[0, 0], [-1, len(rows)], [-1, -2]]


# ---- states built by hand ------------------------------------------------------------------------
MARKINGS = {MUSHROOMS: ("avatar_marking.level_1", "ctimer", "flag1"),
            "territory__rooms": ("avatar_marking.level_1", None, None),
            R.MATRIX: ("avatarReadyToInteractMarker.notReady", "ctimer", "nozap")}


@functools.lru_cache(maxsize=None)
def built_rows(name):
  """uint8 [2, S]: a mid-episode state of the level built from nothing but the pack's initial map
  and the field views — every avatar on a spawn point (row 0), and the same with the last avatar
  dead (row 1).  What a user who constructs probe states would write."""
  lay, sl, t = layout(name), sub_layout(name), tables(name)
  name = base_name(name)
  rows = np.zeros((2, lay.world_stride), np.uint8)
  import torch
  f = S.StateFields(torch.from_numpy(rows), sl)
  f.grid[:, :lay.L] = torch.from_numpy(np.ascontiguousarray(t["init_grid"]).reshape(lay.L, lay.H, lay.W))
  cells = [int(c) for c in t["spawn_cells"]]
  assert len(cells) >= lay.P
  for r in range(2):
    for p in range(lay.P):
      x, y = cells[p] % lay.W, cells[p] // lay.W
      dead = r == 1 and p == lay.P - 1
      f.avatar_x[r, p], f.avatar_y[r, p], f.orientation[r, p], f.alive[r, p] = x, y, p % 4, 0 if dead else 1
      f.aflags[r, p] = 1   # movement allowed
      v = p * 0x1111   # every stream visits the avatars in index order (int16: the bits of the u16)
      f.next_orders[r, p] = v - 0x10000 if v >= 0x8000 else v
      if not dead:
        f.grid[r, lay.avatar_layer, y, x] = sl.avatar_states[p][0]
      if name in MARKINGS:   # a marker piece connected to the avatar, with a position of its own
        state, fx, fy = MARKINGS[name]
        if fx:
          getattr(f, fx)[r, p], getattr(f, fy)[r, p] = x, y
        if not dead:
          f.flag0[r, p] = 1
          f.grid[r, sl.state_layers[sl.state_id(state)], y, x] = sl.state_id(state)
      if name in (MUSHROOMS, "territory__rooms"):
        f.level[r, p] = 1
      if name == COOK:   # the inventory piece on the avatar's cell
        f.grid[r, sl.state_layers[sl.state_id("inventory.empty")], y, x] = sl.state_id("inventory.empty")
    f.step[r], f.frame[r], f.cont[r], f.started[r], f.episode[r], f.orders_step[r] = 1, 2, 1, 1, 1, 2
    f.seed[r] = 1234 + r
  return rows


@pytest.mark.parametrize("name", CASES)
def test_states_built_by_hand_are_well_formed(name):
  v = E.check_states_host(pack_of(name), built_rows(name))
  assert not v.any(), [layout(name).describe(*x) for x in v]
  # ... and so is a world that was never reset (zeros and a seed)
  blank = np.zeros((1, layout(name).world_stride), np.uint8)
  fields(name, blank).seed[0] = 99
  assert not E.check_states_host(pack_of(name), blank).any()


# ---- mutations -----------------------------------------------------------------------------------
def fields(name, rows):
  """StateFields over a CPU tensor that shares memory with the numpy array `rows`."""
  import torch
  return S.StateFields(torch.from_numpy(rows), S.SubstrateStateLayout(layout(name), tables(name)))


def sub_layout(name):
  return S.SubstrateStateLayout(layout(name), tables(name))


def free_cell(name, row, plane):
  """A cell (x, y) whose byte of every render plane is zero but the background's... simply: a
  cell empty on `plane` and on the avatar plane, away from every avatar."""
  lay = layout(name)
  g = row[:lay.grid_planes * lay.H * lay.W].reshape(lay.grid_planes, lay.H, lay.W)
  for y in range(lay.H):
    for x in range(lay.W):
      if g[plane, y, x] == 0 and g[lay.avatar_layer, y, x] == 0:
        return x, y
  raise AssertionError("no free cell")


def other_layer_state(name, plane):
  """A valid state id whose layer is not `plane`."""
  layer = tables(name)["state_layer"]
  for s in range(1, layout(name).nstates):
    if 0 <= int(layer[s]) != plane:
      return s
  raise AssertionError("no such state")


def generic_mutations(name, rows=None, dead_row=None):
  """(label, mutate(fields-of-one-row), expected (rule, offset), base row) on copies of row 0 of
  `rows` (step 1, MID, every avatar alive; default: the states built by hand) — or of the
  dead-avatar row."""
  if rows is None:
    rows, dead_row = built_rows(name), 1
  lay = layout(name)
  sl = sub_layout(name)
  AL = lay.avatar_layer
  base = rows[0]
  f0 = fields(name, base[None].copy())
  x0, y0 = int(f0.avatar_x[0, 0]), int(f0.avatar_y[0, 0])
  alive0 = int(f0.grid[0, AL, y0, x0])
  fx, fy = free_cell(name, base, AL)
  plane0 = 0 if AL != 0 else 1
  cx, cy = 0, 0
  out = []

  def add(label, fn, rule, offset, row=0):
    out.append((label, fn, (rule, offset), row))

  def setter(fieldname, value, idx=0):
    def fn(f):
      getattr(f, fieldname)[0][idx] = value
    return fn

  def scalar(fieldname, value):
    def fn(f):
      getattr(f, fieldname)[0] = value
    return fn

  def cell(plane, x, y, value):
    def fn(f):
      f.grid[0, plane, y, x] = value
    return fn

  add("plane byte = nstates", cell(plane0, cx, cy, lay.nstates), E.RULE_STATE_RANGE, lay.cell_offset(plane0, cx, cy))
  add("plane byte = 255", cell(lay.L - 1, 1, 0, 255), E.RULE_STATE_RANGE, lay.cell_offset(lay.L - 1, 1, 0))
  add("state of another layer", cell(plane0, cx, cy, other_layer_state(name, plane0)), E.RULE_STATE_LAYER,
      lay.cell_offset(plane0, cx, cy))
  add("aori = 4", setter("orientation", 4, lay.P - 1), E.RULE_TAIL_RANGE, lay.field_offset("aori", lay.P - 1))
  add("aalive = 2", setter("alive", 2), E.RULE_TAIL_RANGE, lay.field_offset("aalive", 0))
  add("step = max_frames + 1", scalar("step", lay.max_frames + 1), E.RULE_TAIL_RANGE, lay.field_offset("step"))
  add("done = 7", scalar("done", 7), E.RULE_TAIL_RANGE, lay.field_offset("done"))
  add("ax = W", setter("avatar_x", lay.W), E.RULE_AVATAR_CELL, lay.field_offset("ax", 0))
  add("ay = 255", setter("avatar_y", 255), E.RULE_AVATAR_CELL, lay.field_offset("ay", 0))
  add("avatar's cell emptied", cell(AL, x0, y0, 0), E.RULE_AVATAR_CELL, lay.cell_offset(AL, x0, y0))
  add("second copy of avatar 0", cell(AL, fx, fy, alive0), E.RULE_AVATAR_STRAY, lay.cell_offset(AL, fx, fy))
  add("orders_step = step + 2", scalar("orders_step", 3), E.RULE_ORDERS, lay.field_offset("orders_step"))

  def repeat_nibble(f):   # stream 1: position 1 names the avatar of position 0
    v = f.next_orders[0]   # (int16 [P]; plain tensor arithmetic: the GPU test applies it on the device)
    v[1] = (v[1] & ~0x00f0) | (v[0] & 0x00f0)
  add("repeated nibble", repeat_nibble, E.RULE_ORDERS, lay.field_offset("next_orders", 1))

  def two(f):   # rules 6 and 3 in one row: the smaller pair is reported
    f.orders_step[0] = 3
    f.orientation[0][0] = 9
  add("two violations", two, E.RULE_TAIL_RANGE, lay.field_offset("aori", 0))

  def two_same_rule(f):   # the smaller offset of one rule
    f.grid[0, plane0, 3, 2] = 255
    f.grid[0, plane0, 1, 4] = 254
  add("two violations of one rule", two_same_rule, E.RULE_STATE_RANGE, lay.cell_offset(plane0, 4, 1))

  if dead_row is not None:
    dead = rows[dead_row]
    fd = fields(name, dead[None].copy())
    p = int((fd.alive[0] == 0).nonzero()[0, 0])
    dx, dy = free_cell(name, dead, AL)
    add("dead avatar's state on the map", cell(AL, dx, dy, sl.avatar_states[p][0]), E.RULE_AVATAR_STRAY,
        lay.cell_offset(AL, dx, dy), row=dead_row)
  return out


def level_mutations(name, rows=None):
  """One mutation per level rule of the pack's level."""
  if rows is None:
    rows = built_rows(name)
  lay, sl = layout(name), sub_layout(name)
  case, name = name, base_name(name)
  out = []

  def add(label, fn, sub, offset, row=0):
    out.append((label, fn, (E.RULE_LEVEL, E.level_offset(sub, offset)), row))

  def kill(f, p):   # avatar p of the row leaves the map (its markers and pieces stay where they are)
    x, y = int(f.avatar_x[0, p]), int(f.avatar_y[0, p])
    f.alive[0][p] = 0
    f.grid[0, lay.avatar_layer, y, x] = 0

  def byte(fieldname, cname, value, p=0):
    k = list(lay.fields).index(cname)
    def fn(f):
      getattr(f, fieldname)[0][p] = value
    return fn, E.LEVEL_BYTE_FIELD + k, lay.field_offset(cname, p)

  if name == "clean_up":
    def fn(f):
      f.aux_count[0] = 10 ** 6
    add("aux_count past the threshold table", fn, E.LEVEL_AUX_COUNT, lay.field_offset("aux_count"))
    def neg(f):
      f.aux_count[0] = -1
    add("aux_count negative", neg, E.LEVEL_AUX_COUNT, lay.field_offset("aux_count"))
  if name == COOK:
    # the avatars never die here; a dead one's position is still used
    def fn(f):
      kill(f, 1)
      f.avatar_x[0][1] = 200
    add("a dead avatar off the map", fn, E.LEVEL_BYTE_FIELD + 0, lay.field_offset("ax", 1))
    def fn_y(f):
      kill(f, 0)
      f.avatar_y[0][0] = lay.H
    add("a dead avatar below the map", fn_y, E.LEVEL_BYTE_FIELD + 1, lay.field_offset("ay", 0))
    base = fields(case, rows[0][None].copy())
    x, y = int(base.avatar_x[0, 0]), int(base.avatar_y[0, 0])
    ov = sl.state_layers[sl.state_id("inventory.empty")]
    def lost(f):
      f.grid[0, ov, y, x] = 0
    add("an avatar without its inventory piece", lost, E.LEVEL_FOLLOWER, lay.cell_offset(ov, x, y))
  if name == "coop_mining":
    def fn(f):
      f.grid[0, lay.L, 0, 0] = 1 << lay.P   # hidden plane 0: the miner sets
    if lay.P < 8:
      add("a miner that is no avatar", fn, E.LEVEL_PLANE0, lay.cell_offset(lay.L, 0, 0))
  if name == "gift_refinements":
    for cname, p in (("flag0", 0), ("flag1", 1), ("level", lay.P - 1)):   # the three token types
      fn, sub, off = byte(cname, cname, 255, p=p)
      add(f"an inventory above the capacity ({cname})", fn, sub, off)
  if name == MUSHROOMS:
    fn, sub, off = byte("flag0", "flag0", 3, p=1)
    add("a marking state past level_2", fn, sub, off)
    fn, sub, off = byte("ctimer", "ctimer", lay.W)
    add("a marking's x off the map", fn, sub, off)
    fn, sub, off = byte("flag1", "flag1", 255, p=lay.P - 1)
    add("a marking's y off the map", fn, sub, off)
    fn, sub, off = byte("level", "level", 0)
    add("sanction level 0", fn, sub, off)
    base = fields(case, rows[0][None].copy())
    p = 0
    assert int(base.flag0[0, p]) > 0
    mx, my = int(base.ctimer[0, p]), int(base.flag1[0, p])
    mark_plane = sl.state_layers[sl.state_id("avatar_marking.level_1")]
    assert int(base.grid[0, mark_plane, my, mx]) != 0
    def lost(f):
      f.grid[0, mark_plane, my, mx] = 0
    add("a marking that is not on its cell", lost, E.LEVEL_MARKER_CELL, lay.cell_offset(mark_plane, mx, my))
  if name == "territory__rooms":
    def fn(f):
      f.grid[0, lay.L, 2, 3] = (lay.P + 1) << 3   # hidden plane A: claimedBy + 1 in bits 3-7
    add("a resource claimed by nobody's index", fn, E.LEVEL_PLANE0, lay.cell_offset(lay.L, 3, 2))
    fn, sub, off = byte("flag0", "flag0", 3)
    add("a marking state past level_2", fn, sub, off)
    fn, sub, off = byte("level", "level", 3, p=2)
    add("a sanction level the increments cannot reach", fn, sub, off)
    def orphan(f):   # a dead avatar whose marking stays on the map: its cell is still written
      p = lay.P - 1
      kill(f, p)
      f.flag0[0][p] = 1
      f.avatar_x[0][p] = lay.W
    add("an orphaned marking off the map", orphan, E.LEVEL_MARKER_OFF_MAP, lay.field_offset("ax", lay.P - 1))
  if name == R.MATRIX:
    base = fields(case, rows[0][None].copy())
    assert int(base.flag0[0, 0]) > 0
    mx, my = int(base.ctimer[0, 0]), int(base.nozap[0, 0])
    mark_plane = sl.state_layers[sl.state_id("avatarReadyToInteractMarker.notReady")]
    assert int(base.grid[0, mark_plane, my, mx]) != 0
    def lost(f):
      f.grid[0, mark_plane, my, mx] = 0
    add("a marker that is not on its cell", lost, E.LEVEL_MARKER_CELL, lay.cell_offset(mark_plane, mx, my))
    fn, sub, off = byte("nozap", "nozap", lay.H)
    add("a marker's y off the map", fn, sub, off)
    fn, sub, off = byte("ctimer", "ctimer", 250, p=1)
    add("a marker's x off the map", fn, sub, off)
  return out


def all_mutations(name, rows=None, dead_row=None):
  """Every mutation of the level, on `rows` (default: the states built by hand)."""
  if rows is None:
    rows, dead_row = built_rows(name), 1
  return generic_mutations(name, rows, dead_row) + level_mutations(name, rows)


def apply(name, mutation, rows=None):
  label, fn, want, row = mutation
  one = (built_rows(name) if rows is None else rows)[row][None].copy()
  fn(fields(name, one))
  return one


@pytest.mark.parametrize("name", CASES)
def test_mutations_get_their_exact_verdict(name):
  lay = layout(name)
  muts = all_mutations(name)
  bank = np.concatenate([apply(name, m) for m in muts])
  got = verdicts(name, bank)
  for m, v in zip(muts, got):
    assert tuple(int(x) for x in v) == m[2], (name, m[0], lay.describe(*v), "wanted", lay.describe(*m[2]))


# The level rules of DESIGN.md §3.9's audit table, by rule 7's sub-code: 1 + k = per-avatar byte
# array k of the tail (1 ax, 2 ay, 6 ctimer, 7 flag0, 8 flag1, 12 nozap, 13 level), 16 aux_count,
# 17 a plane rule, 19 / 20 a marker, 21 a connected piece.
AUDIT = {"clean_up": {16}, "commons_harvest__open": set(), "coins": set(),
         "territory__rooms": {7, 13, 17, 19}, R.MATRIX: {6, 12, 20}, "coop_mining": {17},
         "gift_refinements": {7, 8, 13}, COOK: {1, 2, 21}, MUSHROOMS: {6, 7, 8, 13, 20}}


def test_every_level_rule_of_the_audit_has_a_mutation():
  assert set(AUDIT) == set(R.PACKS)
  for base, subs in AUDIT.items():
    got = {m[2][1] >> 24 for case in CASES if base_name(case) == base for m in level_mutations(case)}
    assert got == subs, (base, sorted(got), sorted(subs))


def test_the_mushrooms_layer_takes_nothing_but_the_four_types():
  """A live mushroom's type indexes the pack's tables (step_mushroom.h:339-361).  No level rule
  bounds it: the decoder refuses a pack whose mushroom layer holds another state, so every other
  byte there is rule 1's or rule 2's."""
  name = MUSHROOMS
  lay, sl = layout(name), sub_layout(name)
  s0 = sl.state_id("mushroom.fullInternalityZeroExternality")
  live = sl.state_layers[s0]
  assert [s for s in range(lay.nstates) if sl.state_layers[s] == live] == [s0, s0 + 1, s0 + 2, s0 + 3]
  x, y = free_cell(name, built_rows(name)[0], live)
  bank = np.repeat(built_rows(name)[:1], 256, axis=0)
  fields(name, bank).grid[:, live, y, x] = __import__("torch").arange(256, dtype=__import__("torch").uint8)
  got = verdicts(name, bank)
  for s in range(256):
    want = 0 if s == 0 or s0 <= s < s0 + 4 else E.RULE_STATE_RANGE if s >= lay.nstates else E.RULE_STATE_LAYER
    assert int(got[s, 0]) == want and (want == 0 or int(got[s, 1]) == lay.cell_offset(live, x, y)), s


# ---- bytes that must not matter ------------------------------------------------------------------
def junk_unjudged(name, rows):
  """A copy of `rows` with random bytes wherever the check does not look: behind the planes (the
  padding, the matrix games' player block), behind the tail, ctr[], reward_fx, tail lanes >= P."""
  lay = layout(name)
  rng = np.random.default_rng(3)
  rows = rows.copy()
  n = len(rows)
  junk = lambda k: rng.integers(0, 256, (n, k), dtype=np.uint8)
  behind = lay.grid_planes * lay.H * lay.W
  rows[:, behind:lay.grid_pad] = junk(lay.grid_pad - behind)
  rows[:, lay.grid_pad + lay.tail_bytes:] = junk(lay.world_stride - lay.grid_pad - lay.tail_bytes)
  for cname in ("ctr", "reward_fx"):
    off, elem, count = lay.fields[cname]
    rows[:, lay.grid_pad + off:lay.grid_pad + off + elem * count] = junk(elem * count)
  for cname, (off, elem, count) in lay.fields.items():   # tail lanes >= P
    if count == 16 and lay.P < 16:
      lo = lay.grid_pad + off + elem * lay.P
      rows[:, lo:lay.grid_pad + off + elem * 16] = junk(elem * (16 - lay.P))
  return rows


@pytest.mark.parametrize("name", CASES)
def test_unjudged_bytes_take_any_value(name):
  lay = layout(name)
  rows = junk_unjudged(name, rows_of(name))
  assert (rows != rows_of(name)).any()
  v = verdicts(name, rows)
  assert not v.any(), [lay.describe(*x) for x in v]


# ---- the Python surface on CPU tensors -----------------------------------------------------------
def test_state_fields_are_views_and_the_edited_flag():
  import torch
  name = "clean_up"
  lay = layout(name)
  data = torch.from_numpy(rows_of(name).copy())
  states = S.WorldStates(data, lay.fingerprint)
  assert states.edited is False and states[1:3].edited is False
  f = S.StateFields(states.data, sub_layout(name))
  assert f.grid.shape == (len(states), lay.grid_planes, lay.H, lay.W) and f.grid.dtype == torch.uint8
  assert f.avatar_x.shape == (len(states), lay.P) and f.seed.dtype == torch.int64 and f.step.dtype == torch.int32
  assert f.ctr.shape == (len(states), 8) and f.next_orders.shape == (len(states), lay.P)
  for n in f.names:   # no copies
    v = getattr(f, n)
    lo, hi = states.data.data_ptr(), states.data.data_ptr() + states.data.numel()
    assert lo <= v.data_ptr() < hi, n
  f.step[2] = 7
  f.avatar_y[0, 1] = 9
  f.seed[1] = -5
  raw = states.data.numpy()
  assert raw[2, lay.field_offset("step")] == 7 and raw[0, lay.field_offset("ay", 1)] == 9
  assert raw[1, lay.field_offset("seed"):lay.field_offset("seed") + 8].tolist() == [251] + [255] * 7
  f.grid[3, 2, 4, 5] = 1
  assert raw[3, lay.cell_offset(2, 5, 4)] == 1

  class Eng:   # what Substrate.state_fields asks of its engine
    state_fingerprint = lay.fingerprint
    class info:
      world_state_bytes = lay.world_stride
    pack_bytes = R.pack(name)
    def state_layout(self):
      return lay
  sub = S.Substrate.__new__(S.Substrate)
  sub._eng = Eng()
  got = sub.state_fields(states)
  assert states.edited is True and got.step.data_ptr() == f.step.data_ptr()
  assert states[0].edited and states[:2].edited and states[[1, 0]].edited
  sl = sub.state_layout()
  assert len(sl.layer_names) == lay.L and sl.hidden_planes == lay.grid_planes - lay.L
  assert sl.state_layers[sl.avatar_states[0][0]] == lay.avatar_layer and sl.state_layers[sl.avatar_states[0][1]] == -1
  assert sl.state_id("avatar1.player1") == sl.avatar_states[0][0] and len(sl.avatar_states) == lay.P
  with pytest.raises(KeyError):
    sl.state_id("no.such")


def test_load_state_resolves_check():
  import torch
  name = "coins"
  lay = layout(name)
  calls = []

  class Eng:
    state_fingerprint = lay.fingerprint
    class info:
      world_state_bytes = lay.world_stride
    def use_current_stream(self):
      pass
    def load_worlds(self, bank, src, fingerprint=None, **kw):
      calls.append(kw)
  sub = S.Substrate.__new__(S.Substrate)
  sub._eng = Eng()
  sub._submissions = 0
  sub._emit = lambda ts: ts
  sub._timestep = lambda: None
  states = S.WorldStates(torch.from_numpy(rows_of(name).copy()), lay.fingerprint)
  sub.load_state(states, [0])
  sub.load_state(states, [0], check=True)
  sub.load_state(states, [0], check=False)
  states.edited = True
  sub.load_state(states, [0])
  sub.load_state(states, [0], check=False)
  sub.load_state(states[1:], [0])
  # (never edited: exactly the call of a load before there was a check)
  assert calls == [{}, {"check": True}, {}, {"check": True}, {}, {"check": True}]
  with pytest.raises(ValueError):
    sub.load_state(states, [0], check="yes")


def test_describe_names_the_field_or_the_cell():
  lay = layout("clean_up")
  assert lay.describe(0, 0) == "well-formed"
  assert "aori[3]" in lay.describe(E.RULE_TAIL_RANGE, lay.field_offset("aori", 3))
  assert "plane 4 cell (x=5, y=2)" in lay.describe(E.RULE_AVATAR_STRAY, lay.cell_offset(4, 5, 2))
  assert "aux_count" in lay.describe(E.RULE_LEVEL, E.level_offset(E.LEVEL_AUX_COUNT, lay.field_offset("aux_count")))
  assert "orders_step" in lay.describe(E.RULE_ORDERS, lay.field_offset("orders_step"))
