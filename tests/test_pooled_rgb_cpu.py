"""Pooled per-agent RGB (MP_OBS_RGB_POOL2/4/8, `Substrate(..., rgb_pool=k)`) without a GPU:
the C ABI's kinds and the binding's agree, the keyword refuses
what it does not offer, and the numpy reference `engine.pool_rgb` is the contract's rule."""
import os
import re

import numpy as np
import pytest

from meltingpot_amd import engine, substrate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum():
  text = open(os.path.join(ROOT, "include", "mp_engine.h")).read()
  return {name: int(v) for name, v in re.findall(r"\b(MP_OBS_[A-Z0-9_]+)\s*=\s*(\d+)", text)}


def test_header_pooled_kinds_match_the_binding():
  kinds = _header_enum()
  assert kinds["MP_OBS_RGB_POOL2"] == engine.OBS_RGB_POOL2 == 21
  assert kinds["MP_OBS_RGB_POOL4"] == engine.OBS_RGB_POOL4 == 22
  assert kinds["MP_OBS_RGB_POOL8"] == engine.OBS_RGB_POOL8 == 23
  assert kinds["MP_OBS_KINDS"] == 24
  assert engine.OBS_RGB_POOL == {2: 21, 4: 22, 8: 23}


@pytest.mark.parametrize("bad", [0, 3, 16, -8, 2.5, True])
def test_rgb_pool_refuses_other_factors(bad):
  with pytest.raises(ValueError, match="rgb_pool"):
    substrate.build("clean_up", roles=("default",) * 7, num_worlds=4, rgb_pool=bad)


def test_pool_rgb_hand_computed_blocks():
  img = np.zeros((1, 8, 8, 3), np.uint8)
  img[0, :2, :2, 0] = [[1, 2], [3, 4]]        # 10 / 4 = 2.5 -> rounds up to 3
  img[0, :2, 2:4, 1] = [[0, 0], [0, 1]]       # 1 / 4 = 0.25 -> 0
  img[0, :2, 4:6, 2] = [[255, 255], [255, 254]]  # 1019 / 4 = 254.75 -> 255
  img[0, 2:4, :2, 0] = [[1, 1], [0, 0]]       # 2 / 4 = 0.5 -> 1 (half up)
  p2 = engine.pool_rgb(img, 2)
  assert p2.shape == (1, 4, 4, 3) and p2.dtype == np.uint8
  assert p2[0, 0, 0, 0] == 3
  assert p2[0, 0, 1, 1] == 0
  assert p2[0, 0, 2, 2] == 255
  assert p2[0, 1, 0, 0] == 1
  assert p2.sum() == 3 + 255 + 1
  # k = 8: one value per 8 x 8 block; 64 * 127 + 32 = 8160 -> (8128 + 32) // 64 = 127.5 -> 128
  blk = np.full((8, 8, 3), 127, np.uint8)
  blk[0, 0, :] = 159                          # sum 64 * 127 + 32
  assert engine.pool_rgb(blk, 8).tolist() == [[[128, 128, 128]]]
  blk[0, 0, :] = 158                          # one less: 127.48 -> 127
  assert engine.pool_rgb(blk, 8).tolist() == [[[127, 127, 127]]]
  # k = 4 on a gradient, against the rule written out
  rng = np.random.default_rng(3)
  g = rng.integers(0, 256, size=(2, 3, 16, 24, 3), dtype=np.uint8)
  want = np.zeros((2, 3, 4, 6, 3), np.uint8)
  for y in range(4):
    for x in range(6):
      s = g[:, :, 4 * y:4 * y + 4, 4 * x:4 * x + 4, :].astype(np.int64).sum(axis=(2, 3))
      want[:, :, y, x, :] = (s + 8) // 16
  assert np.array_equal(engine.pool_rgb(g, 4), want)
  assert np.array_equal(engine.pool_rgb(g, 1), g)
  with pytest.raises(ValueError):
    engine.pool_rgb(np.zeros((12, 12, 3), np.uint8), 8)
