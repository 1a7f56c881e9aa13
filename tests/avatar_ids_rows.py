"""Hand-placed records for the AVATAR_IDS tests (test infrastructure): a real row of a level (the
fixture tests/golden/state_rows.npz, saved on a GPU by the recipe of tests/states_recipe.py) with
its avatars taken off the map and put back where a case wants them, through `StateFields`.  Player
0 is the viewer, players 1 and 2 the targets; every other player is parked alive on a free cell at
least 5 cells from the viewer (out of every ray's reach), so that the rows can be stepped.  A
hand-made record may put an avatar or a wall on any cell of the map, a border wall included."""
import functools
import os

import numpy as np

import avatar_ids_model as M
import ego_layer_model as EM
import states_recipe as R

HERE = os.path.dirname(os.path.abspath(__file__))
LEVELS = ("clean_up", "commons_harvest__open", "territory__rooms", "externality_mushrooms__dense")
DX, DY = M.DX, M.DY


def golden_rows(name):
  return dict(np.load(os.path.join(HERE, "golden", "state_rows.npz")))[name + "/rows"]


def viewer_at(H, W, o):
  """Where the viewer of orientation `o` stands so that 10 cells ahead, 2 behind and 6 to either
  side are cells of the map (the window reaches 9, 1, 5 and 5)."""
  return {0: (W // 2, H - 3), 1: (2, H // 2), 2: (W // 2, 2), 3: (W - 3, H // 2)}[o]


def offset(x, y, o, right, ahead):
  r = (o + 1) % 4
  return x + right * DX[r] + ahead * DX[o], y + right * DY[r] + ahead * DY[o]


@functools.lru_cache(maxsize=None)
def hand_rows(name):
  """(rows uint8 [M, S], what: a list of M strings, tags: {tag: [row indices]}) of a level.  Tags:
  "edge_in" / "edge_out" (a target on the window's last row or column / one cell outside),
  "corner_in", "footprint", "wall", "shadow" (the nearer of two in a ray), "side_wall", "map_corner",
  "dead_viewer", "dead_target", "all_dead", and "alive" (every row in which all P avatars live)."""
  pack = R.pack(name)
  H, W, _, (vl, vr, vf, vb), _ = EM.geometry(pack)
  assert (vl, vr, vf, vb) == (5, 5, 9, 1) and H >= 13 and W >= 13
  # the base: the fixture's first row in which every avatar lives and none is frozen or barred from zapping
  every = golden_rows(name)
  fe = M.fields_of(pack, every)
  good = fe.alive.numpy().all(1) & (fe.freeze.numpy() == 0).all(1) & (fe.nozap.numpy() == 0).all(1)
  assert good.any(), "no base row"
  base = every[int(np.flatnonzero(good)[0])][None]
  f0 = M.fields_of(pack, base)
  P = f0.avatar_x.shape[1]
  al = M.avatar_layer(pack)
  own = M.avatar_states(pack, P)
  state_of = {p: s for s, p in own.items()}
  wall_state = int(f0.grid[0, al, 0, 0])
  assert wall_state != 0 and wall_state not in own
  foot = M.footprint(pack)
  cases = []   # (what, tag, wanted: {p: (x, y, o)}, walls, dead players)

  def case(what, tag, viewer, targets=(), walls=(), dead=()):
    cases.append((what, tag, viewer, tuple(targets), tuple(walls), tuple(dead)))

  for o in range(4):
    x, y = viewer_at(H, W, o)
    v = (x, y, o)
    for label, right, ahead in (("ahead", 0, vf), ("behind", 0, -vb), ("left", -vl, 0), ("right", vr, 0)):
      step = (np.sign(right), np.sign(ahead))
      case(f"facing {o}: target on the window's last cell {label}", "edge_in", v, [offset(x, y, o, right, ahead) + (0,)])
      case(f"facing {o}: target one cell outside the window {label}", "edge_out", v,
           [offset(x, y, o, right + step[0], ahead + step[1]) + (0,)])
    for right, ahead in ((-vl, vf), (vr, vf), (-vl, -vb), (vr, -vb)):
      case(f"facing {o}: target on the window's corner ({right}, {ahead})", "corner_in", v,
           [offset(x, y, o, right, ahead) + (1,)])
    for j, (lat, fw, _) in enumerate(foot):
      case(f"facing {o}: target on footprint cell {j} ({lat}, {fw})", "footprint", v, [offset(x, y, o, lat, fw) + (2,)])
    case(f"facing {o}: target behind a wall", "wall", v, [offset(x, y, o, 0, 2) + (0,)], walls=[offset(x, y, o, 0, 1)])
    case(f"facing {o}: a nearer avatar shadows a farther one", "shadow", v,
         [offset(x, y, o, 0, 1) + (3,), offset(x, y, o, 0, 2) + (1,)])
    case(f"facing {o}: target on a side ray whose first cell is a wall", "side_wall", v,
         [offset(x, y, o, 1, 1) + (0,)], walls=[offset(x, y, o, 1, 0)])
    case(f"facing {o}: a dead viewer", "dead_viewer", v, [offset(x, y, o, 0, 1) + (0,)], dead=[0])
    case(f"facing {o}: a dead target", "dead_target", v, [offset(x, y, o, 0, 1) + (0,)], dead=[1])
  # a viewer on a corner of the map facing out: ahead and to one side the map ends
  for (x, y), o, side in (((0, 0), 0, 1), ((0, 0), 3, -1), ((W - 1, H - 1), 2, 1), ((W - 1, H - 1), 1, -1)):
    case(f"viewer on the map's corner {(x, y)} facing {o}", "map_corner", (x, y, o), [offset(x, y, o, side, 0) + (0,)])
  case("all avatars dead", "all_dead", viewer_at(H, W, 0) + (0,), dead=list(range(P)))

  rows = np.repeat(base, len(cases), axis=0)
  f = M.fields_of(pack, rows)   # (views of `rows`' memory, through torch.from_numpy)
  data = f.grid.numpy()
  assert np.shares_memory(data, rows)
  what, tags = [], {}
  for r, (text, tag, viewer, targets, walls, dead) in enumerate(cases):
    plane = data[r, al]
    for s in own:
      plane[plane == s] = 0
    for wx, wy in walls:
      plane[wy, wx] = wall_state
    wanted = {0: viewer}
    wanted.update({1 + k: t for k, t in enumerate(targets)})
    taken = {(x, y) for x, y, _ in wanted.values()}
    free = [(x, y) for y in range(H) for x in range(W)
            if plane[y, x] == 0 and (x, y) not in taken and max(abs(x - viewer[0]), abs(y - viewer[1])) >= 5]
    if W == H == 21 and name == "territory__rooms":   # (a torus: distances wrap)
      free = [(x, y) for x, y in free
              if max(min(abs(x - viewer[0]), W - abs(x - viewer[0])), min(abs(y - viewer[1]), H - abs(y - viewer[1]))) >= 5]
    for p in range(P):
      if p not in wanted:
        wanted[p] = free.pop(len(free) // 2 if p % 2 else 0) + (p % 4,)
    for p, (x, y, o) in wanted.items():
      assert 0 <= x < W and 0 <= y < H, (text, p, x, y)
      f.avatar_x[r, p], f.avatar_y[r, p], f.orientation[r, p] = x, y, o
      f.alive[r, p] = int(p not in dead)
      if p not in dead:
        plane[y, x] = state_of[p]
    what.append(text)
    tags.setdefault(tag, []).append(r)
    if not dead:
      tags.setdefault("alive", []).append(r)
  return rows, what, tags
