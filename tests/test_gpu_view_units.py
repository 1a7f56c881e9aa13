"""The three registrations of every viewer's window on ONE engine (MpEgoLayer, MpViewHash,
MpEgoPlanes; Engine.bind_ego_layer / bind_view_hash / bind_ego_planes): the launches behind a
submission share their source fields and their ring slot, and every other test registers one unit
alone.  After each submission each registered tensor — the slot just written — equals its own draw
form of the live worlds; after one registration is cleared the other two still follow.  Every
comparison is exact equality."""
import numpy as np
import pytest
import torch

import util
from meltingpot_amd import engine

pytestmark = pytest.mark.gpu

E = engine
N = 3
SEED = 5


@pytest.mark.parametrize("T", [0, 2])
def test_three_registrations_on_one_engine_follow_every_submission(T):
  eng = E.Engine(E.load_pack("clean_up"), N, device=0)
  P = eng.P
  assert P == 7   # (odd: every second world's u64 [P] block of hashes starts off a 16-byte line)
  if T:
    eng.bind_ring(E.OBS_REWARD, slots=T)
  L = int(eng.info.num_layers)
  layers = [0, L - 1]
  assert L >= 3
  ids = eng.num_layer_ids
  hash_classes = torch.from_numpy((np.arange(ids) % 5).astype(np.int32)).to(eng.device)
  C = 5
  plane_classes = torch.from_numpy((np.arange(ids) % (C + 1) - 1).astype(np.int32)).to(eng.device)
  lead = (T,) if T else ()
  if T:
    ego = eng.bind_ego_layer_ring(slots=T)
  else:
    ego = eng.bind_ego_layer(torch.zeros(eng.ego_layer_shape, dtype=torch.int32, device=eng.device))
  hashes = eng.bind_view_hash(torch.zeros(lead + (N, P), dtype=torch.int64, device=eng.device), layers=layers,
                              classes=hash_classes)
  planes = eng.bind_ego_planes(torch.zeros(lead + eng.ego_planes_shape(C, True), dtype=torch.uint8, device=eng.device),
                               plane_classes, facing=True, num_classes=C)
  assert tuple(ego.shape) == lead + eng.ego_layer_shape
  registered = {"ego": ego, "hashes": hashes, "planes": planes}

  def draw():
    return {"ego": eng.observe_ego_layer(),
            "hashes": eng.hash_views(layers=layers, classes=hash_classes),
            "planes": eng.observe_ego_planes(plane_classes, facing=True, num_classes=C)}

  def check(what, cleared=()):
    want = draw()
    slot = eng.ring["last"] if T else None
    for name, reg in registered.items():
      if name in cleared:
        continue
      now = reg[slot] if T else reg
      assert now.shape == want[name].shape and now.dtype == want[name].dtype, (what, name)
      assert torch.equal(now, want[name]), (what, name, slot)
    return want

  rng = np.random.default_rng(SEED)

  def actions(*shape):
    a = util.random_actions(rng, 1, int(np.prod(shape)), P, eng.num_actions)
    return torch.from_numpy(a.reshape(shape + (P,))).to(eng.device)

  eng.reset()
  first = check("reset")
  saved = eng.save_worlds().clone()
  eng.step(actions(N))
  second = check("step")
  assert not torch.equal(first["ego"], second["ego"]) or not torch.equal(first["hashes"], second["hashes"])
  eng.step_many(actions(2, N))
  check("step_many")
  eng.load_worlds(saved, [2, -1, 0])
  loaded = check("load_worlds")
  assert torch.equal(loaded["ego"][0], first["ego"][2]) and torch.equal(loaded["planes"][2], first["planes"][0])
  # clearing one registration: its tensor is written no more, the other two still follow
  frozen = hashes.clone()
  assert eng.bind_view_hash(None) is None
  for k in range(2):   # (T = 2: both slots)
    eng.step(actions(N))
    check(("step, the hashes cleared", k), cleared=("hashes",))
  assert torch.equal(hashes, frozen)
  assert not torch.equal(eng.hash_views(layers=layers, classes=hash_classes), frozen[eng.ring["last"]] if T else frozen)
  eng.sync()
  assert not eng.fault_words()[:12].any(), eng.fault_words()[:12]   # (9 .. 11: a skipped index; none was)
  eng.close()
