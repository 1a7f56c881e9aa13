"""Class-indicator feature planes of a player's view (MpEgoPlanes) as one numpy statement of their
definition (test infrastructure): the model the host twin and the kernels are held to.  The class
planes come from the model's EGO_LAYER (tests/ego_layer_model.py) through the class table; the
facing planes from `avatar_x`, `avatar_y`, `orientation` and `alive`, with the same turned-offset
arrays as that model.  Nothing here comes from the library."""
import numpy as np

import ego_layer_model as EM


def class_planes(ego, classes, num_classes, layers=None):
  """uint8 [..., C, VH, VW] of views `ego`, int32 [..., VH, VW, L]: plane c is 1 where some counted
  layer holds an id of class c.  `layers`: the counted layer indices (None: all)."""
  ego = np.asarray(ego)
  L = ego.shape[-1]
  cls = np.asarray(classes, np.int64)[ego.astype(np.int64)]          # [..., VH, VW, L]
  counted = np.ones(L, bool) if layers is None else np.isin(np.arange(L), np.asarray(list(layers)))
  cls = np.where(counted, cls, -1)
  hit = (cls[..., None] == np.arange(int(num_classes))).any(axis=-2)   # [..., VH, VW, C]
  return np.moveaxis(hit, -1, -3).astype(np.uint8)


def facing_planes(pack_bytes, avatar_x, avatar_y, orientation, alive):
  """uint8 [R, P, 4, VH, VW]: plane d of viewer p is 1 at window cell (i, j) iff p is alive, the cell
  maps to a cell of the map, and a living avatar q stands there with (ori[q] - ori[p]) & 3 == d."""
  H, W, _, (vl, vr, vf, vb), torus = EM.geometry(pack_bytes)
  ax, ay = np.asarray(avatar_x).astype(np.int64), np.asarray(avatar_y).astype(np.int64)
  vo, live = np.asarray(orientation).astype(np.int64), np.asarray(alive).astype(bool)
  R, P = ax.shape
  dx = (np.arange(vl + vr + 1) - vl)[None, :]
  dy = (np.arange(vf + vb + 1) - vf)[:, None]
  dx, dy = np.broadcast_arrays(dx, dy)
  turned_x = np.stack([dx, -dy, -dx, dy])
  turned_y = np.stack([dy, dx, -dy, -dx])
  x = ax[:, :, None, None] + turned_x[vo]          # [R, P, VH, VW]
  y = ay[:, :, None, None] + turned_y[vo]
  if torus:
    x, y, inside = x % W, y % H, np.ones(x.shape, bool)
  else:
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
  inside = inside & live[:, :, None, None]
  out = np.zeros((R, P, 4) + x.shape[2:], np.uint8)
  for q in range(P):
    here = inside & live[:, q, None, None, None] & (x == ax[:, q, None, None, None]) & (y == ay[:, q, None, None, None])
    d = (vo[:, q, None] - vo) & 3                  # [R, P]
    for k in range(4):
      out[:, :, k] |= (here & (d == k)[:, :, None, None]).astype(np.uint8)
  return out


def planes(pack_bytes, grid, avatar_x, avatar_y, orientation, alive, classes, num_classes=None, layers=None,
           facing=False):
  """uint8 [R, P, C', VH, VW] of rows given by their fields."""
  C = int(np.max(classes)) + 1 if num_classes is None else int(num_classes)
  ego = EM.ego_layer(pack_bytes, grid, avatar_x, avatar_y, orientation, alive)
  out = class_planes(ego, classes, C, layers)
  if facing:
    out = np.concatenate([out, facing_planes(pack_bytes, np.asarray(avatar_x)[:, :ego.shape[1]],
                                             np.asarray(avatar_y)[:, :ego.shape[1]],
                                             np.asarray(orientation)[:, :ego.shape[1]],
                                             np.asarray(alive)[:, :ego.shape[1]])], axis=2)
  return np.ascontiguousarray(out)


def of_fields(pack_bytes, fields, classes, num_classes=None, layers=None, facing=False):
  """`planes` of a `StateFields` (host or device tensors)."""
  f = lambda v: v.cpu().numpy()
  return planes(pack_bytes, f(fields.grid), f(fields.avatar_x), f(fields.avatar_y), f(fields.orientation),
                f(fields.alive), classes, num_classes, layers, facing)


def of_rows(pack_bytes, rows, classes, num_classes=None, layers=None, facing=False, num_players=0):
  """`planes` of host rows (uint8 [R, S]) through the library's layout and `StateFields`."""
  import torch

  from meltingpot_amd import engine, pack as pack_lib, substrate
  layout = engine.state_layout(pack_bytes, num_players=num_players)
  data = torch.from_numpy(np.ascontiguousarray(rows, np.uint8))
  sl = substrate.SubstrateStateLayout(layout, pack_lib.loads(pack_bytes))
  return of_fields(pack_bytes, substrate.StateFields(data, sl), classes, num_classes, layers, facing)
