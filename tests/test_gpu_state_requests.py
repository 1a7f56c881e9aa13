"""The refusals of the saved-state requests on one engine: every malformed request of
tests/tools/make_state_request_refusals.py against tests/golden/state_request_refusals.json (return
code and message, byte for byte up to pointers; each is refused on the host, nothing is launched),
and the ValueError texts Engine's methods raise before a request is sent."""
import json
import os
import sys

import pytest
import torch

from meltingpot_amd import engine as E

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import make_state_request_refusals as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
  """The engine of the replay: 2 worlds of clean_up; `early` is what it answered before its reset."""
  c = T.DeviceCtx()
  c.early = T.replay(c.L, T.gpu_cases_before_reset(c))
  c.bank_ready()
  yield c
  c.close()


def test_device_refusals_are_the_recorded_ones(ctx):
  with open(T.GOLDEN) as f:
    golden = json.load(f)
  cases = T.gpu_cases(ctx)
  assert len({name for name, *_ in cases}) == len(cases) >= 250
  got = dict(ctx.early)
  got.update(T.replay(ctx.L, cases))
  host = {name for name, *_ in T.cpu_cases(T.HostCtx())}
  assert set(got) | host == set(golden), sorted(set(got) ^ (set(golden) - host))
  wrong = {n: (v, golden[n]) for n, v in got.items() if v != golden[n]}
  assert not wrong, wrong
  accepted = sorted(n for n, v in got.items() if v[0] == 0)
  assert accepted == ["episode_starts/null_bank_clears", "hash/mask_counts_not_validated"]
  torch.cuda.synchronize()
  assert not ctx.eng.fault_words()[:6].any()


def raised(fn, *args, **kwargs) -> str:
  with pytest.raises(ValueError) as err:
    fn(*args, **kwargs)
  return str(err.value)


def test_engine_value_error_texts(ctx):
  eng, bank = ctx.eng, ctx._bank
  S, dev = ctx.S, eng.device
  assert str(dev) == "cuda:0" and tuple(bank.shape) == (3, S)
  short, empty, f32 = bank[:, :100], bank[:0], bank.to(torch.float32)
  methods = {"check_states": lambda b: eng.check_states(b), "hash_states": lambda b: eng.hash_states(b),
             "load_worlds": lambda b: eng.load_worlds(b, [0, 1]),
             "observe_states": lambda b: eng.observe_states(b, E.OBS_LAYER),
             "observe_views": lambda b: eng.observe_views(b, E.OBS_LAYER, [0]),
             "observe_ego_layer": lambda b: eng.observe_ego_layer(b), "hash_views": lambda b: eng.hash_views(b),
             "observe_ego_planes": lambda b: eng.observe_ego_planes([0] * eng.num_layer_ids, b)}
  strided = torch.zeros((3, 2 * S), dtype=torch.uint8, device=dev)[:, ::2]
  for who, call in methods.items():
    live = who in ("observe_ego_layer", "hash_views", "observe_ego_planes")   # (None: the engine's worlds)
    for bad in [short, f32, bank.cpu().numpy(), strided] + ([] if live else [None]):
      assert raised(call, bad) == f"{who}: bank must be a contiguous uint8 tensor [M, {S}]", who
    assert raised(call, empty) == f"{who}: the bank has no rows", who
  assert raised(eng.save_worlds, []) == "save_worlds: no worlds to save"
  assert raised(eng.save_worlds, [0.5]) == "worlds must hold integers (got float64)"
  for out in (bank[:1], torch.zeros((2, S), dtype=torch.int32, device=dev), strided[:2], "x"):
    assert raised(eng.save_worlds, out=out) == f"save_worlds: out must be a contiguous uint8 tensor of shape (2, {S})"
  assert raised(eng.save_worlds, out=bank) == f"save_worlds: out must be a contiguous uint8 tensor of shape (2, {S})"
  assert raised(eng.save_worlds, [0], out=bank) == f"save_worlds: out must be a contiguous uint8 tensor of shape (1, {S})"

  assert raised(eng.check_states, bank, rows=[]) == "check_states: no rows to judge"
  assert raised(eng.check_states, bank, rows=torch.zeros(2)) == "rows must hold integers (got torch.float32)"
  i32 = torch.zeros((3, 2), dtype=torch.int32, device=dev)
  for out in (i32[:2], i32.to(torch.int64), i32.cpu(), torch.zeros((3, 4), dtype=torch.int32, device=dev)[:, ::2]):
    assert raised(eng.check_states, bank, out=out) == \
        "check_states: out must be a contiguous int32 tensor of shape (3, 2) on cuda:0"
  assert raised(eng.check_states, empty, rows=[], out=i32[:2]) == "check_states: the bank has no rows"
  assert raised(eng.check_states, bank, rows=[], out=i32[:2]) == "check_states: no rows to judge"

  assert raised(eng.hash_states, bank, rows=[]) == "hash_states: nothing to hash"
  assert raised(eng.hash_worlds, []) == "hash_worlds: nothing to hash"
  assert raised(eng.hash_worlds, [0.5]) == "worlds must hold integers (got float64)"
  i64 = torch.zeros(3, dtype=torch.int64, device=dev)
  for out in (i64[:2], i64.to(torch.int32), i64.cpu()):
    assert raised(eng.hash_states, bank, out=out) == \
        "hash_states: out must be a contiguous int64 tensor of shape (3,) on cuda:0"
  assert raised(eng.hash_worlds, out=i64) == "hash_worlds: out must be a contiguous int64 tensor of shape (2,) on cuda:0"
  assert raised(eng.hash_states, bank, out=i64, planes=[99]) == "hash: 99 is no grid plane (the rows have 9)"
  assert raised(eng.hash_states, bank, out=i64[:2], planes=[99]) == \
      "hash_states: out must be a contiguous int64 tensor of shape (3,) on cuda:0"

  assert raised(eng.load_worlds, bank, [0, 1, 2]) == "load_worlds: src must have 2 entries (got 3)"
  assert raised(eng.load_worlds, bank, [0.5, 1]) == "src must hold integers (got float64)"

  assert raised(eng.observe_states, bank, 99) == "observe_states: 99 is no observation kind"
  assert raised(eng.observe_states, bank, True) == "observe_states: True is no observation kind"
  assert raised(eng.observe_states, empty, 99) == "observe_states: the bank has no rows"
  assert raised(eng.observe_states, bank, E.OBS_LAYER, rows=[]) == "observe_states: no rows to draw"
  lshape = tuple(int(d) for d in eng.shapes[E.OBS_LAYER][0])
  layer = torch.zeros((3,) + lshape[1:], dtype=torch.int32, device=dev)
  for out in (layer[:2], layer.to(torch.int64), layer.cpu()):
    assert raised(eng.observe_states, bank, E.OBS_LAYER, out=out) == \
        f"observe_states: out must be a contiguous torch.int32 tensor of shape {(3,) + lshape[1:]} on cuda:0"
  assert raised(eng.observe_states, bank, E.OBS_READY_TO_SHOOT, out=layer) == \
      f"observe_states: out must be a contiguous torch.float64 tensor of shape (3, {eng.P}) on cuda:0"

  assert raised(eng.observe_views, bank, 99, [0]) == "observe_views: 99 is no observation kind"
  assert raised(eng.observe_views, bank, E.OBS_WORLD_RGB, [0]) == \
      "observe_views: OBS_WORLD_RGB is not a per-player kind (observe_states draws it)"
  assert raised(eng.observe_views, bank, E.OBS_WORLD_RGB, None) == \
      "observe_views: OBS_WORLD_RGB is not a per-player kind (observe_states draws it)"
  assert raised(eng.observe_views, bank, E.OBS_LAYER, None) == "observe_views: players is required"
  assert raised(eng.observe_views, bank, E.OBS_LAYER, []) == "observe_views: no views to draw"
  assert raised(eng.observe_views, bank, E.OBS_LAYER, [0, 1, 2], rows=[0, 1]) == \
      "observe_views: rows has 2 entries, players 3"
  for out in (layer[:2, 0], layer[:, 0], layer[:2, 0].contiguous().cpu()):
    assert raised(eng.observe_views, bank, E.OBS_LAYER, [0, 1], out=out) == \
        f"observe_views: out must be a contiguous torch.int32 tensor of shape {(2,) + lshape[2:]} on cuda:0"

  views = {"observe_ego_layer": (eng.observe_ego_layer, (), "draw", "int32", lshape[2:]),
           "hash_views": (eng.hash_views, (), "hash", "int64", ()),
           "observe_ego_planes": (eng.observe_ego_planes, ([0] * eng.num_layer_ids,), "draw", "uint8",
                                  eng.ego_planes_shape(1)[2:])}
  for who, (fn, args, verb, dtype, tail) in views.items():
    assert raised(fn, *args, bank, rows=[]) == f"{who}: no views to {verb}"
    assert raised(fn, *args, bank, players=[]) == f"{who}: no views to {verb}"
    assert raised(fn, *args, None, players=[]) == f"{who}: no views to {verb}"
    assert raised(fn, *args, bank, rows=[0, 1], players=[0, 1, 2]) == f"{who}: rows has 2 entries, players 3"
    assert raised(fn, *args, empty, rows=[]) == f"{who}: the bank has no rows"
    assert raised(fn, *args, bank, out=torch.zeros(1, device=dev)) == \
        f"{who}: out must be a contiguous {dtype} tensor of shape {(3, eng.P) + tuple(tail)} on cuda:0"
    assert raised(fn, *args, None, players=[0], out=torch.zeros(1)) == \
        f"{who}: out must be a contiguous {dtype} tensor of shape {(1,) + tuple(tail)} on cuda:0"

  rows = torch.zeros(2, dtype=torch.int32, device=dev)
  assert raised(eng.set_episode_starts, bank, rows, fresh=1) == "set_episode_starts: fresh must be True or False (got 1)"
  assert raised(eng.set_episode_starts, bank, rows.cpu()) == "set_episode_starts: rows lives on cpu, the engine on cuda:0"
  assert raised(eng.set_episode_starts, empty, rows, fresh=1) == "set_episode_starts: the bank has no rows"
  assert eng.episode_starts is None
  torch.cuda.synchronize()
  assert not eng.fault_words()[:6].any()
