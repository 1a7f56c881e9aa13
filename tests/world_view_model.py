"""WORLD.LAYER and the world planes as numpy statements of their definitions (test infrastructure):
the model the host twins and the kernels are held to.  The world's value table comes from the pack's
`state_sprite` and row P of `view_sprite_map` through `pack.loads`; the planes and the tail come
from `state_fields`."""
import numpy as np

from meltingpot_amd import lower, pack as pack_lib


def geometry(pack_bytes):
  """(H, W, L) of a pack."""
  hdr = pack_lib.loads(pack_bytes)["hdr"]
  return int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W]), int(hdr[lower.HDR_L])


def sprite_maps(pack_bytes):
  """int32 [rows, nsprites]: `view_sprite_map`; row P is the world's, rows < P the viewers'."""
  t = pack_lib.loads(pack_bytes)
  return np.asarray(t["view_sprite_map"]).reshape(-1, int(t["hdr"][lower.HDR_NSPRITES]))


def table(pack_bytes, num_players):
  """int32 [256]: Wt, WORLD.LAYER's id of a plane byte."""
  t = pack_lib.loads(pack_bytes)
  nstates = int(t["hdr"][lower.HDR_NSTATES])
  ssprite = np.asarray(t["state_sprite"]).reshape(-1)
  world = sprite_maps(pack_bytes)[num_players]
  out = np.zeros(256, np.int32)
  for s in range(1, min(nstates, 256)):
    out[s] = 1 + world[ssprite[s]] if ssprite[s] >= 0 else 0
  return out


def num_ids(pack_bytes, num_players):
  return 1 + int(table(pack_bytes, num_players).max())


def world_layer(pack_bytes, grid, num_players):
  """int32 [R, H, W, L] of rows given by their grid (numpy [R, planes, H, W])."""
  _, _, L = geometry(pack_bytes)
  states = np.asarray(grid)[:, :L].astype(np.int64)
  return np.ascontiguousarray(table(pack_bytes, num_players)[states].transpose(0, 2, 3, 1)).astype(np.int32)


def world_planes(pack_bytes, grid, avatar_x, avatar_y, orientation, alive, classes, num_classes=None, layers=None,
                 facing=False):
  """uint8 [R, C', H, W]: the fields as numpy arrays, grid [R, planes, H, W], the others [R, P]."""
  H, W, L = geometry(pack_bytes)
  P = np.asarray(avatar_x).shape[1]
  classes = np.asarray(classes)
  C = int(classes.max()) + 1 if num_classes is None else int(num_classes)
  wl = world_layer(pack_bytes, grid, P)                    # [R, H, W, L]
  cls = classes[wl]
  cls = np.where((cls >= 0) & (cls < C), cls, -1)          # (an entry out of range counts as -1)
  counted = np.zeros(L, bool)
  counted[list(range(L)) if layers is None else list(layers)] = True
  R = wl.shape[0]
  out = np.zeros((R, C + (4 if facing else 0), H, W), np.uint8)
  for c in range(C):
    out[:, c] = ((cls == c) & counted[None, None, None, :]).any(-1)
  if facing:
    for r in range(R):
      for q in range(P):
        if alive[r, q]:
          out[r, C + int(orientation[r, q]), int(avatar_y[r, q]), int(avatar_x[r, q])] = 1
  return out


def _numpy(fields, num_players):
  f = lambda v: v.cpu().numpy()
  P = num_players
  return (f(fields.grid), f(fields.avatar_x)[:, :P], f(fields.avatar_y)[:, :P], f(fields.orientation)[:, :P],
          f(fields.alive)[:, :P])


def layer_of_fields(pack_bytes, fields, num_players):
  return world_layer(pack_bytes, _numpy(fields, num_players)[0], num_players)


def planes_of_fields(pack_bytes, fields, num_players, classes, num_classes=None, layers=None, facing=False):
  return world_planes(pack_bytes, *_numpy(fields, num_players), classes, num_classes, layers, facing)


def fields_of(pack_bytes, rows, num_players=0):
  """`StateFields` of host rows (uint8 [R, S]) through the library's layout, and P."""
  import torch

  from meltingpot_amd import engine, substrate
  layout = engine.state_layout(pack_bytes, num_players=num_players)
  data = torch.from_numpy(np.ascontiguousarray(rows, np.uint8))
  return substrate.StateFields(data, substrate.SubstrateStateLayout(layout, pack_lib.loads(pack_bytes))), layout.P


def layer_of_rows(pack_bytes, rows):
  f, P = fields_of(pack_bytes, rows)
  return layer_of_fields(pack_bytes, f, P)


def planes_of_rows(pack_bytes, rows, classes, num_classes=None, layers=None, facing=False):
  f, P = fields_of(pack_bytes, rows)
  return planes_of_fields(pack_bytes, f, P, classes, num_classes, layers, facing)
