"""The recipe the world-state observation tests share (test infrastructure): one pack per level
kernel with episodes of 16 frames, five worlds (a ragged last workgroup), 24 steps of seeded
actions that zap often.  On the CPU oracle this gives rows with a dead avatar in clean_up,
commons_harvest__open and externality_mushrooms__dense, and every world of every level is LAST at
step 16 and FIRST at step 17 — the tests assert that those rows are among the ones they compare."""
import functools

import numpy as np

import util
from meltingpot_amd import engine

PACKS = ("clean_up", "commons_harvest__open", "territory__rooms", "coins", "coop_mining",
         "gift_refinements", "externality_mushrooms__dense", "collaborative_cooking__cramped",
         "prisoners_dilemma_in_the_matrix__repeated")
DEAD_AVATARS = ("clean_up", "commons_harvest__open", "externality_mushrooms__dense")
MATRIX = "prisoners_dilemma_in_the_matrix__repeated"
N, STEPS, LAST_STEP = 5, 24, 16
SAVE_AT = (1, 8, 16, 17, 24)
E = engine


@functools.lru_cache(maxsize=None)
def pack(name):
  return util.patch_pack(engine.load_pack(name), MAXFRAMES=LAST_STEP)


def actions(num_players, num_actions, n=N):
  """int32 [STEPS, n, P]: weight 4 on action min(7, nact - 1), 1 on every other."""
  w = np.ones(num_actions)
  w[min(7, num_actions - 1)] = 4
  return util.random_actions(np.random.default_rng(7), STEPS, n, num_players, num_actions, w)


def record_kinds(eng):
  """The kinds that are functions of a record, as far as the engine's level has them (the pooled
  per-agent views apart: one per-agent view is bound at a time)."""
  kinds = [E.OBS_RGB, E.OBS_WORLD_RGB, E.OBS_LAYER, E.OBS_READY_TO_SHOOT, E.OBS_POSITION,
           E.OBS_ORIENTATION]
  if eng.info.num_resources > 0:
    kinds.append(E.OBS_INVENTORY)
  return tuple(kinds)


@functools.lru_cache(maxsize=None)
def road(name):
  """The loop of single steps with every record-function kind bound: after each step of SAVE_AT
  the saved rows (`banks[k]`, uint8 [N, S]), clones of the bound leaves (`views[k][kind]`), the
  step types and whether some avatar is dead.  Computed once and shared; treat it as read-only."""
  import torch
  e = engine.Engine(pack(name), N, device=0)
  bufs = {k: e.bind(k) for k in record_kinds(e)}
  A = actions(e.P, e.num_actions)
  dA = torch.from_numpy(A).to(e.device)
  e.reset()
  out = {"banks": {}, "views": {}, "step_type": {}, "dead": {}, "actions": A,
         "fingerprint": e.state_fingerprint, "kinds": record_kinds(e)}
  for s in range(1, STEPS + 1):
    e.step(dA[s - 1])
    if s in SAVE_AT:
      out["banks"][s] = e.save_worlds().clone()
      out["views"][s] = {k: v.clone() for k, v in bufs.items()}
      out["step_type"][s] = e.observe(E.OBS_STEP_TYPE).cpu().numpy().copy()
      out["dead"][s] = bool((e.dump()[1][:, :, 3] == 0).any())
  assert not e.fault_words()[:6].any()
  e.close()
  assert (out["step_type"][16] == 2).all() and (out["step_type"][17] == 0).all(), name
  if name in DEAD_AVATARS:
    assert any(out["dead"].values()), name
  out["all"] = torch.cat([out["banks"][s] for s in SAVE_AT])   # 25 rows: row i * N + w = world w after SAVE_AT[i]
  out["all_views"] = {k: torch.cat([out["views"][s][k] for s in SAVE_AT]) for k in out["kinds"]}
  return out
