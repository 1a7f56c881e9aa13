"""EGO_LAYER as one numpy statement of its definition (test infrastructure): the model the host
twin and the kernels are held to.  The value table comes from the pack's `state_sprite` and
`view_sprite_map` through `pack.loads`; the planes and the tail come from `state_fields`."""
import numpy as np

from meltingpot_amd import lower, pack as pack_lib

OOB = 256   # the table's OutOfBounds column


def geometry(pack_bytes):
  """(H, W, L, (left, right, forward, backward), torus) of a pack."""
  hdr = pack_lib.loads(pack_bytes)["hdr"]
  view = tuple(int(hdr[i]) for i in (lower.HDR_VL, lower.HDR_VR, lower.HDR_VF, lower.HDR_VB))
  return int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W]), int(hdr[lower.HDR_L]), view, int(hdr[lower.HDR_TOPOLOGY]) == 1


def lut(pack_bytes, num_players):
  """int32 [P, 257]: N.LAYER's id of (viewer, plane byte); column 256 is OutOfBounds."""
  t = pack_lib.loads(pack_bytes)
  hdr = t["hdr"]
  nstates, nsprites = int(hdr[lower.HDR_NSTATES]), int(hdr[lower.HDR_NSPRITES])
  ssprite = np.asarray(t["state_sprite"]).reshape(-1)
  vmap = np.asarray(t["view_sprite_map"]).reshape(-1, nsprites)
  out = np.zeros((num_players, 257), np.int32)
  for p in range(num_players):
    for s in range(1, min(nstates, 256)):
      out[p, s] = 1 + vmap[p, ssprite[s]] if ssprite[s] >= 0 else 0
    out[p, OOB] = 1 + vmap[p, 0]
  return out


def ego_layer(pack_bytes, grid, avatar_x, avatar_y, orientation, alive, north=False):
  """int32 [R, P, VH, VW, L] of rows given by their fields (numpy arrays: grid [R, planes, H, W],
  the others [R, P]).  north=True: the window is not turned (N.LAYER)."""
  H, W, L, (vl, vr, vf, vb), torus = geometry(pack_bytes)
  grid = np.asarray(grid)[:, :L].astype(np.int64)
  R, P = np.asarray(avatar_x).shape
  table = lut(pack_bytes, P)
  vo = np.zeros((R, P), np.int64) if north else np.asarray(orientation).astype(np.int64)
  dx = (np.arange(vl + vr + 1) - vl)[None, :]          # [1, VW]
  dy = (np.arange(vf + vb + 1) - vf)[:, None]          # [VH, 1]
  dx, dy = np.broadcast_arrays(dx, dy)                 # [VH, VW]
  turned_x = np.stack([dx, -dy, -dx, dy])              # [4, VH, VW]
  turned_y = np.stack([dy, dx, -dy, -dx])
  x = np.asarray(avatar_x).astype(np.int64)[:, :, None, None] + turned_x[vo]   # [R, P, VH, VW]
  y = np.asarray(avatar_y).astype(np.int64)[:, :, None, None] + turned_y[vo]
  if torus:
    x, y, inside = x % W, y % H, np.ones(x.shape, bool)
  else:
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
  inside &= np.asarray(alive).astype(bool)[:, :, None, None]
  r = np.arange(R)[:, None, None, None]
  states = grid[r, :, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]       # [R, P, VH, VW, L]
  states = np.where(inside[..., None], states, OOB)
  return table[np.arange(P)[None, :, None, None, None], states].astype(np.int32)


def of_fields(pack_bytes, fields, north=False):
  """`ego_layer` of a `StateFields` (host or device tensors)."""
  f = lambda v: v.cpu().numpy()
  return ego_layer(pack_bytes, f(fields.grid), f(fields.avatar_x), f(fields.avatar_y), f(fields.orientation),
                   f(fields.alive), north)


def of_rows(pack_bytes, rows, num_players=0, north=False):
  """`ego_layer` of host rows (uint8 [R, S]) through the library's layout and `StateFields`."""
  import torch

  from meltingpot_amd import engine, substrate
  layout = engine.state_layout(pack_bytes, num_players=num_players)
  data = torch.from_numpy(np.ascontiguousarray(rows, np.uint8))
  return of_fields(pack_bytes, substrate.StateFields(data, substrate.SubstrateStateLayout(layout, pack_lib.loads(pack_bytes))),
                   north)
