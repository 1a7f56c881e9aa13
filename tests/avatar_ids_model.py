"""AVATAR_IDS_IN_VIEW and AVATAR_IDS_IN_RANGE_TO_ZAP as numpy statements of their definitions (test
infrastructure, include/mp_engine.h: MpAvatarIds): the model the host twin and the kernels are held
to.  Loops over window cells and over footprint cells with their predecessors; the library is not
called.  IN_VIEW walks the window enumeration of tests/ego_layer_model.py (the same turned offsets,
the same torus wrap), so IN_VIEW[p][q] == 1 exactly when q's avatar shows on the avatar layer of
p's EGO_LAYER."""
import numpy as np

from meltingpot_amd import lower, pack as pack_lib

import ego_layer_model as EM


def avatar_layer(pack_bytes):
  return int(pack_lib.loads(pack_bytes)["hdr"][lower.HDR_AVATAR_LAYER])


def footprint(pack_bytes):
  """The zap footprint of a pack as a list of (lat, fw, pred): the cell lies `lat` to the avatar's
  right and `fw` ahead, and `pred` is the set of indices of the cells a ray passes before it.  The
  rays of Zapper:getWhoZappable (avatar_library.lua:780-824) with the Zapper's beamLength and
  beamRadius: the centre ray ahead; to either side the sideways ray, and from its i-th cell a ray
  ahead of length beamLength - i that has passed the sideways cells up to there.  None: the level
  has no Zapper."""
  t = pack_lib.loads(pack_bytes)
  if "zapper_i32" not in t:
    return None
  length, radius = (int(v) for v in np.asarray(t["zapper_i32"]).reshape(-1)[1:3])
  cells = []
  ray = set()
  for f in range(1, length + 1):
    cells.append((0, f, frozenset(ray)))
    ray.add(len(cells) - 1)
  for side in (-1, 1):
    sideways = set()
    for i in range(1, radius + 1):
      cells.append((side * i, 0, frozenset(sideways)))
      sideways.add(len(cells) - 1)
      ray = set(sideways)
      for f in range(1, length - i + 1):
        cells.append((side * i, f, frozenset(ray)))
        ray.add(len(cells) - 1)
  return cells


def avatar_states(pack_bytes, num_players):
  """{state: player}: the avatar states of the first `num_players` players."""
  t = pack_lib.loads(pack_bytes)
  out = {int(s): p for p, s in enumerate(np.asarray(t["avatar_alive_state"]).reshape(-1)[:num_players])}
  if "avatar_extra_alive" in t:
    extra = np.asarray(t["avatar_extra_alive"]).reshape(-1, 2)
    out.update({int(s): int(p) for s, p in extra if p < num_players})
  return out


DX, DY = (0, 1, 0, -1), (-1, 0, 1, 0)   # N E S W, N = decreasing y


def in_view(pack_bytes, avatar_x, avatar_y, orientation, alive):
  """int32 [R, P, P] from [R, P] arrays."""
  H, W, _, (vl, vr, vf, vb), torus = EM.geometry(pack_bytes)
  ax, ay, ao, al = (np.asarray(v).astype(np.int64) for v in (avatar_x, avatar_y, orientation, alive))
  R, P = ax.shape
  out = np.zeros((R, P, P), np.int32)
  for r in range(R):
    for p in range(P):
      if not al[r, p]:
        continue
      seen = set()
      for dy in range(-vf, vb + 1):        # window cell (vy, vx) = (dy + vf, dx + vl)
        for dx in range(-vl, vr + 1):
          tx = (dx, -dy, -dx, dy)[ao[r, p]]
          ty = (dy, dx, -dy, -dx)[ao[r, p]]
          x, y = ax[r, p] + tx, ay[r, p] + ty
          if torus:
            x, y = x % W, y % H
          elif not (0 <= x < W and 0 <= y < H):
            continue
          seen.add((int(x), int(y)))
      for q in range(P):
        out[r, p, q] = int(bool(al[r, q]) and (int(ax[r, q]), int(ay[r, q])) in seen)
  return out


def in_range(pack_bytes, plane, avatar_x, avatar_y, orientation, alive):
  """int32 [R, P, P] from the avatar_layer plane [R, H, W] and [R, P] arrays."""
  H, W, _, _, torus = EM.geometry(pack_bytes)
  cells = footprint(pack_bytes)
  assert cells is not None, "the level has no Zapper"
  plane = np.asarray(plane)
  ax, ay, ao, al = (np.asarray(v).astype(np.int64) for v in (avatar_x, avatar_y, orientation, alive))
  R, P = ax.shape
  owner = avatar_states(pack_bytes, P)
  out = np.zeros((R, P, P), np.int32)
  for r in range(R):
    for p in range(P):
      if not al[r, p]:
        continue
      o = int(ao[r, p])
      right = (o + 1) % 4
      where, stops = [], []
      for lat, fw, _ in cells:
        x = int(ax[r, p]) + lat * DX[right] + fw * DX[o]
        y = int(ay[r, p]) + lat * DY[right] + fw * DY[o]
        if torus:
          x, y = x % W, y % H
        on = 0 <= x < W and 0 <= y < H
        where.append((x, y) if on else None)
        stops.append(not on or plane[r, y, x] != 0)
      for j, (_, _, pred) in enumerate(cells):
        if where[j] is None or any(stops[k] for k in pred):
          continue
        x, y = where[j]
        q = owner.get(int(plane[r, y, x]))
        if q is not None:
          out[r, p, q] = 1
  return out


def fields_of(pack_bytes, rows, num_players=0):
  """`StateFields` of host rows (uint8 [R, S])."""
  import torch

  from meltingpot_amd import engine, substrate
  layout = engine.state_layout(pack_bytes, num_players=num_players)
  data = torch.from_numpy(np.ascontiguousarray(rows, np.uint8))
  return substrate.StateFields(data, substrate.SubstrateStateLayout(layout, pack_lib.loads(pack_bytes)))


def of_fields(pack_bytes, fields, zap=True):
  """(in_view, in_range or None) of a `StateFields` (host or device tensors)."""
  f = lambda v: v.cpu().numpy()
  P = f(fields.avatar_x).shape[1]
  x, y, o, a = f(fields.avatar_x), f(fields.avatar_y), f(fields.orientation), f(fields.alive)
  view = in_view(pack_bytes, x, y, o, a)
  if not zap:
    return view, None
  return view, in_range(pack_bytes, f(fields.grid)[:, avatar_layer(pack_bytes)], x, y, o, a)


def of_rows(pack_bytes, rows, zap=True, num_players=0):
  return of_fields(pack_bytes, fields_of(pack_bytes, rows, num_players), zap)
