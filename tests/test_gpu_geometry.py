"""Edited map and view geometries on the GPU (tests/geometry.py), every byte against the oracle:
world-view rows at the wave-pass boundaries (R = 64 // W changes between W = 16|17, 21|22 and
32|33; W = 64 and the 64 x 64 map), per-agent windows from 1 x 1 to 64 x 64 with left != right
and forward != backward, TORUS on levels that are BOUNDED in stock with the view's reach equal to
H or W, and a 64 x 64 window at a world count whose tickets per workgroup times tickets per batch
pass 2^32.  State, rewards and events after every step; RGB, RGB_POOL2/4/8, WORLD.RGB full and
pooled by 2/4/8 and LAYER at a few steps and the last; fused, unfused and under forced plans.
No fault word may be set after any of it."""
import numpy as np
import pytest
import torch

import geometry
import util
from meltingpot_amd import engine

pytestmark = pytest.mark.gpu

POOL_OF = {k: f for f, k in engine.OBS_RGB_POOL.items()}
# (WORLD.RGB factor, per-agent view, LAYER bound): every view of the variant across four engines
ALL_VIEWS = [(1, engine.OBS_RGB, True), (2, engine.OBS_RGB_POOL2, False),
             (4, engine.OBS_RGB_POOL4, False), (8, engine.OBS_RGB_POOL8, True)]
FEW_VIEWS = [(1, engine.OBS_RGB, True), (8, engine.OBS_RGB_POOL8, False)]
IDS = [geometry.variant_id(v) for v in geometry.ACCEPTED]


def _asymmetric(v):
  view = v.get("view")
  return view is not None and (view[0] != view[1] or view[2] != view[3])


def _actions(v, steps, n, P, nact, seed):
  """Random actions.  Asymmetric windows: no random turns, and every avatar turns right every
  fourth step, so each one has faced all four ways after step 12; beams only from then on (a
  zapped avatar stops turning), three times as likely as the other actions.  TORUS: beams
  three times as likely."""
  rng = np.random.default_rng(seed)
  turn, fire = geometry.turn_and_fire(v["name"])
  w = np.ones(nact)
  w[fire] = 3.0 if _asymmetric(v) or v.get("topology") == "TORUS" else 1.0
  if not _asymmetric(v):
    return util.random_actions(rng, steps, n, P, nact, w)
  w[geometry.turns(v["name"])] = 0.0
  calm = w.copy()
  calm[fire] = 0.0
  acts = np.concatenate([util.random_actions(rng, min(steps, 12), n, P, nact, calm),
                         util.random_actions(rng, max(steps - 12, 0), n, P, nact, w)])
  acts[3::4] = turn[0]
  return acts


def _events(rows, w):
  assert rows[w, 0, 1] == 0, "events dropped"
  return sorted(tuple(int(x) for x in r[:3]) for r in rows[w, 1:1 + int(rows[w, 0, 0])])


def _run(v, n, steps, setups=ALL_VIEWS, dev=None, unfused=None, seed=0, looks=()):
  """One engine per entry of `setups`, stepped with the same actions as n oracles."""
  blob = geometry.variant_pack(v)
  engs = [engine.Engine(blob, n, device=0, dev=dev, world_pool=kw, unfused=unfused)
          for kw, _, _ in setups]
  bufs = []
  for e, (kw, agent, layer) in zip(engs, setups):
    b = {engine.OBS_WORLD_RGB: e.bind(engine.OBS_WORLD_RGB), agent: e.bind(agent)}
    if layer:
      b[engine.OBS_LAYER] = e.bind(engine.OBS_LAYER)
    bufs.append(b)
  oracles = util.make_oracles(blob, n)
  P, nact = engs[0].P, engs[0].num_actions
  acts = _actions(v, steps, n, P, nact, seed)
  dacts = torch.from_numpy(acts).to(engs[0].device)
  faced = np.zeros((n, P, 4), bool)
  looks = set(looks) | {steps}
  try:
    for e in engs:
      e.reset()
    for o in oracles:
      o.reset()
    for s in range(steps):
      for e in engs:
        e.step(dacts[s])
      for o, a in zip(oracles, acts[s]):
        o.step(a)
      for e in engs if s + 1 in looks else engs[:1]:
        grid, avat, glob = e.dump()
        rew = e.observe(engine.OBS_REWARD).cpu().numpy()
        ev = e.observe(engine.OBS_EVENTS).cpu().numpy()
        for w, o in enumerate(oracles):
          og, oa, ogl = o.dump()
          assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), (s, w)
          assert np.array_equal(glob[w], ogl), (s, w)
          assert np.array_equal(rew[w], o.rewards()), (s, w)
          assert _events(ev, w) == o.events(), (s, w)
          faced[w, np.arange(P), oa[:, 2]] = True
      if s + 1 not in looks:
        continue
      world = [o.render_world() for o in oracles]
      agents = [np.stack([o.render_agent(p) for p in range(P)]) for o in oracles]
      layers = [np.stack([o.layer_view(p) for p in range(P)]) for o in oracles]
      for e, b, (kw, agent, layer) in zip(engs, bufs, setups):
        host = {k: t.cpu().numpy() for k, t in b.items()}
        for w in range(n):
          assert np.array_equal(host[engine.OBS_WORLD_RGB][w], engine.pool_rgb(world[w], kw)), \
              ("WORLD.RGB", kw, s, w)
          want = agents[w] if agent == engine.OBS_RGB else engine.pool_rgb(agents[w], POOL_OF[agent])
          assert np.array_equal(host[agent][w], want), ("RGB", agent, s, w)
          if layer:
            assert np.array_equal(host[engine.OBS_LAYER][w], layers[w]), ("LAYER", s, w)
        util.no_faults(e)
    if _asymmetric(v):
      assert faced.all(), "an avatar did not face all four ways"
  finally:
    for o in oracles:
      o.close()
    for e in engs:
      e.close()


@pytest.mark.parametrize("v", geometry.ACCEPTED, ids=IDS)
def test_variant_fused(v):
  """Every accepted variant, every view, the stock plans of the fused launch."""
  _run(v, 8, 24, looks=(1, 12))


def _pick(views=(), widths=(), tori=()):
  return [v for v in geometry.ACCEPTED if (v.get("view") in views and not v.get("topology")) or
          (v.get("width") in widths and "view" not in v) or (v.get("topology") and v.get("view") in tori)]


UNFUSED = _pick(views=[(0, 7, 3, 0), (3, 0, 0, 4), (31, 32, 32, 31), (0, 63, 0, 0)],
                widths=(17, 33, 64), tori=[(5, 5, 21, 1), (5, 17, 9, 1)])


@pytest.mark.parametrize("v", UNFUSED, ids=[geometry.variant_id(v) for v in UNFUSED])
def test_variant_unfused(v):
  """MpConfig.unfused = 1: the rules in one launch, each view drawn by a draw-only launch."""
  _run(v, 11, 20, FEW_VIEWS, unfused=True, seed=1, looks=(1,))


FORCED = _pick(views=[(0, 7, 3, 0), (3, 18, 1, 0), (31, 32, 32, 31)], widths=(16, 22, 64),
               tori=[(30, 0, 9, 1), None])


@pytest.mark.parametrize("dev", [
    {"batch_worlds": 1, "ring_batches": 6, "static_pct": 50, "max_groups": 4},
    {"batch_worlds": 3, "ring_batches": 2, "max_groups": 8, "world_waves": 1},
], ids=["single-world-batches", "several-batches-per-workgroup"])
@pytest.mark.parametrize("v", FORCED, ids=[geometry.variant_id(v) for v in FORCED])
def test_variant_forced_plans(v, dev):
  """Odd world counts under plans that pool batches and put several in one workgroup."""
  _run(v, 37, 20, FEW_VIEWS, dev=dev, seed=2, looks=(1,))


def test_layer_alone_on_the_largest_map():
  """LAYER alone is written by the stand-alone step kernels.  A 64 x 64 clean_up record (9
  layers, the marks and the scratch) is about 42 KB: four of them, 170 KB, do not fit a
  workgroup's 160 KB of LDS, so the launch runs two worlds per workgroup
  (step_worlds_per_group) — the path with fewer waves than kWorldsPerGroup."""
  v = dict(name="clean_up", width=64, height=64)
  blob = geometry.variant_pack(v)
  n, steps = 9, 12
  e = engine.Engine(blob, n, device=0)
  lay = e.bind(engine.OBS_LAYER)
  oracles = util.make_oracles(blob, n)
  acts = _actions(v, steps, n, e.P, e.num_actions, 4)
  try:
    e.reset()
    for o in oracles:
      o.reset()
    for s in range(steps):
      e.step(torch.from_numpy(acts[s]).to(e.device))
      for o, a in zip(oracles, acts[s]):
        o.step(a)
    grid, avat, glob = e.dump()
    got = lay.cpu().numpy()
    for w, o in enumerate(oracles):
      og, oa, ogl = o.dump()
      assert np.array_equal(grid[w], og) and np.array_equal(avat[w], oa), w
      assert np.array_equal(glob[w], ogl), w
      assert np.array_equal(got[w], np.stack([o.layer_view(p) for p in range(o.P)])), w
    util.no_faults(e)
  finally:
    for o in oracles:
      o.close()
    e.close()


def _first_inexact_ticket(d):
  """The first n for which magic_div(n, 2^32 // d + 1) is not n // d."""
  m, q = 2 ** 32 // d + 1, 0
  while ((q * d + d - 1) * m) >> 32 == q:
    q += 1
  return q * d + d - 1


def test_ticket_division_past_two_to_the_32():
  """A 64 x 64 window of 16 viewers, drawn by ONE workgroup in batches of 8 worlds: a batch is
  npb = 8 * 16 * 64 = 8192 tickets, one image row each (R = 64 / VW = 1).  The host's reciprocal
  alone gives ticket / npb one too large on the last ticket of each batch from batch 64 on
  (ticket 532479, where ticket * npb > 2^32): the last row of the last viewer of worlds 519 and
  527 would not be drawn.  The window (31, 32, 63, 0) puts that row through the viewer's own
  cell, inside the map, and the view is filled with a sentinel before the step, so a row left
  undrawn cannot pass for the oracle's.  frame_kernel.h magic_div_exact corrects the quotient."""
  P, VH, B = 16, 64, 8
  v = dict(name="commons_harvest__open", view=(31, 32, 63, 0), roles=("default",) * P)
  blob = geometry.variant_pack(v)
  npb = B * P * VH
  bad = _first_inexact_ticket(npb)
  n = B * (bad // npb + 2)
  e = engine.Engine(blob, n, device=0, dev={"batch_worlds": B, "ring_batches": 2, "max_groups": 1})
  out = e.bind(engine.OBS_RGB_POOL8)
  assert e.P == P and e.plan["workgroups"] == 1 and e.plan["batch_worlds"] == B, e.plan
  assert n * P * VH > bad and (n * P * VH - 1) * npb >= 2 ** 32
  hit = [(t // npb) * B + B - 1 for t in (bad, bad + npb)]   # worlds whose last row is that ticket
  assert hit == [519, 527] and n == 528
  sample = [0, 1, 511] + hit
  oracles = [util.make_oracles(blob, 1, offset=w)[0] for w in sample]
  rng = np.random.default_rng(9)
  acts = rng.integers(0, e.num_actions, size=(n, P), dtype=np.int32)
  try:
    e.reset()
    out.fill_(201)
    e.step(torch.from_numpy(acts).to(e.device))
    for o, w in zip(oracles, sample):
      o.reset()
      o.step(acts[w])
    got = out[sample].cpu().numpy()
    for i, (o, w) in enumerate(zip(oracles, sample)):
      want = engine.pool_rgb(np.stack([o.render_agent(p) for p in range(P)]), 8)
      assert not (want[P - 1, -1] == 201).all(), w   # (the sentinel is not what the row holds)
      assert np.array_equal(got[i], want), w
    util.no_faults(e)
  finally:
    for o in oracles:
      o.close()
    e.close()
