"""The hash of a player's view (MpViewHash) as one numpy statement of its definition (test
infrastructure): the model the host twin and the kernels are held to.  EGO_LAYER comes from
tests/ego_layer_model.py, never from the library; the arithmetic is plain uint64 numpy.  Also the
rows the CPU tests hash: records written from the CPU oracle's dump through `StateFields`."""
import numpy as np

import ego_layer_model as EM

U64 = np.uint64


def fmix64(h):
  """MurmurHash3's 64-bit finalizer on a uint64 array (numpy wraps mod 2^64)."""
  h = np.asarray(h, U64).copy()
  h ^= h >> U64(33)
  h *= U64(0xff51afd7ed558ccd)
  h ^= h >> U64(33)
  h *= U64(0xc4ceb9fe1a85ec53)
  h ^= h >> U64(33)
  return h


def view_hash(ego, layers=None, classes=None):
  """int64 [...]: V of views `ego`, int32 [..., VH, VW, L].  `layers`: the included layer indices
  (None: all); `classes`: an int array indexed by id (None: the ids themselves)."""
  ego = np.asarray(ego)
  L = ego.shape[-1]
  n = ego.shape[-3] * ego.shape[-2] * L
  v = ego.reshape(ego.shape[:-3] + (n,)).astype(np.int64)
  if classes is not None:
    v = np.asarray(classes, np.int64)[v]
  e = np.arange(n, dtype=U64)
  words = (v & 0xffffffff).astype(U64)           # (u32)v_e
  c = fmix64(((e + U64(1)) << U64(32)) | words)
  included = np.ones(L, bool) if layers is None else np.isin(np.arange(L), np.asarray(list(layers)))
  c = np.where(included[np.arange(n) % L], c, U64(0))
  return fmix64(c.sum(axis=-1, dtype=U64)).view(np.int64)


def of_rows(pack_bytes, rows, layers=None, classes=None, num_players=0):
  """int64 [R, P]: `view_hash` of the model's EGO_LAYER of host rows (uint8 [R, S])."""
  return view_hash(EM.of_rows(pack_bytes, rows, num_players), layers, classes)


def of_fields(pack_bytes, fields, layers=None, classes=None):
  """int64 [R, P]: `view_hash` of the model's EGO_LAYER of a `StateFields`."""
  return view_hash(EM.of_fields(pack_bytes, fields), layers, classes)


def num_ids(pack_bytes, num_players):
  """1 + the largest id the viewers' value tables hold: the length of a class table."""
  return int(EM.lut(pack_bytes, num_players).max()) + 1


def oracle_rows(pack_bytes, num_actions, seed, steps, keep, world=0):
  """(rows uint8 [len(keep), S], facings, dead): the records of one CPU-oracle world after each
  step count in `keep` of `steps` random steps (every action of the level; action 7, the beam, four
  times as likely as another) — the oracle's planes, positions, orientations and who is alive
  written through `StateFields`, which is all of a record that a view depends on.  `facings`: the set of orientations seen in the kept
  rows; `dead`: how many (row, player) viewers are off the grid in them."""
  import torch

  import util
  from meltingpot_amd import engine, pack as pack_lib, substrate
  layout = engine.state_layout(pack_bytes)
  sl = substrate.SubstrateStateLayout(layout, pack_lib.loads(pack_bytes))
  rows = np.zeros((len(keep), layout.world_stride), np.uint8)
  f = substrate.StateFields(torch.from_numpy(rows), sl)
  o = util.make_oracles(pack_bytes, 1, offset=world)[0]
  rng = np.random.default_rng(seed)
  weights = np.ones(num_actions)
  weights[min(7, num_actions - 1)] = 4
  weights /= weights.sum()
  facings, dead, at = set(), 0, 0
  try:
    o.reset()
    for k in range(1, steps + 1):
      o.step(rng.choice(num_actions, size=o.P, p=weights).astype(np.int32))
      if k in keep:
        grid, avat, _ = o.dump()
        f.grid[at, :layout.L] = torch.from_numpy(grid)
        for p in range(o.P):
          f.avatar_x[at, p], f.avatar_y[at, p] = int(avat[p, 0]), int(avat[p, 1])
          f.orientation[at, p], f.alive[at, p] = int(avat[p, 2]), int(avat[p, 3])
        facings |= {int(v) for v in avat[:, 2]}
        dead += int((avat[:, 3] == 0).sum())
        at += 1
  finally:
    o.close()
  assert at == len(keep)
  return rows, facings, dead
