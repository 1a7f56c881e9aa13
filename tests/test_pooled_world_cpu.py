"""Pooled WORLD.RGB (MpConfig.world_pool, `Substrate(..., world_rgb_pool=k)`) without a GPU: the
appended MpConfig field sits behind the ABI-8 layout, mp_create still takes the ABI-8
layout and refuses other factors before a device is touched, the keyword refuses what it does not
offer, and `engine.pool_rgb` pools world-shaped images (odd cell counts) by the contract's rule."""
import ctypes

import numpy as np
import pytest

from meltingpot_amd import engine, substrate

ABI8_CONFIG_BYTES = 72   # sizeof(MpConfig) of ABI 8 before world_pool was appended


def test_world_pool_is_the_last_mpconfig_field_and_matches_the_header():
  """(The mirror against the header as a compiler lays it out: tests/test_request_abi_cpu.py.)"""
  names = [f[0] for f in engine.MpConfig._fields_]
  assert names[-1] == "world_pool"
  assert names[:-1][-2:] == ["dev", "roles"]
  assert engine.MpConfig.world_pool.offset == ABI8_CONFIG_BYTES


def _create(cfg, blob):
  L = engine.load_library()
  h = ctypes.c_void_p()
  buf = ctypes.create_string_buffer(blob, len(blob))
  rc = L.mp_create(buf, len(blob), ctypes.byref(cfg), ctypes.byref(h))
  if rc == 0:   # (on a machine with a GPU: a created engine is released again)
    L.mp_destroy(h)
  return rc, L.mp_last_error()


def test_abi8_struct_size_keeps_todays_verdicts(clean_up_pack):
  cfg = engine.MpConfig(ABI8_CONFIG_BYTES, 0, 0, 1, 0, 0, None)
  rc, msg = _create(cfg, clean_up_pack)
  assert rc == -1 and b"num_worlds" in msg
  cfg.num_worlds = 4
  cfg.world_pool = 3   # beyond the ABI-8 struct: never read
  rc, msg = _create(cfg, b"not a pack" * 10)
  assert rc == -2, msg
  for size in (ABI8_CONFIG_BYTES - 4, ABI8_CONFIG_BYTES + 4, ctypes.sizeof(engine.MpConfig) + 8):
    cfg.struct_size = size
    assert _create(cfg, clean_up_pack)[0] == -1


@pytest.mark.parametrize("bad", [3, -1, 16, 6])
def test_world_pool_outside_the_factors_is_refused_before_any_device_call(clean_up_pack, bad):
  cfg = engine.MpConfig(ctypes.sizeof(engine.MpConfig), 0, 4, 1, 0, 0, None)
  cfg.world_pool = bad
  rc, msg = _create(cfg, clean_up_pack)
  assert rc == -1
  assert b"world_pool" in msg
  # (checked next to MpConfig.unfused: even a junk pack gets this verdict first)
  assert _create(cfg, b"not a pack" * 10) == (-1, msg)


def test_full_size_config_with_world_pool_reaches_the_pack_checks():
  for k in (0, 1, 2, 4, 8):
    cfg = engine.MpConfig(ctypes.sizeof(engine.MpConfig), 0, 4, 1, 0, 0, None)
    cfg.world_pool = k
    assert _create(cfg, b"not a pack" * 10)[0] == -2


@pytest.mark.parametrize("bad", [3, 16, -8, 2.5, True, "2"])
def test_engine_world_pool_is_validated_in_python(clean_up_pack, bad):
  with pytest.raises(ValueError, match="world_pool"):
    engine.Engine(clean_up_pack, 2, world_pool=bad)


@pytest.mark.parametrize("bad", [0, 3, 16, -8, 2.5, True])
def test_world_rgb_pool_refuses_other_factors(bad):
  with pytest.raises(ValueError, match="world_rgb_pool"):
    substrate.build("clean_up", roles=("default",) * 7, num_worlds=4, world_rgb_pool=bad)


def _blocks(img, k):
  """The rule written out, one block at a time."""
  h, w, c = img.shape
  out = np.zeros((h // k, w // k, c), np.uint8)
  for y in range(h // k):
    for x in range(w // k):
      s = img[k * y:k * y + k, k * x:k * x + k, :].astype(np.int64).sum(axis=(0, 1))
      out[y, x] = (s + (k * k) // 2) // (k * k)
  return out


@pytest.mark.parametrize("cells", [(17, 17), (5, 9)])   # coins; collaborative_cooking__cramped
def test_pool_rgb_on_world_images_with_odd_cell_counts(cells):
  rng = np.random.default_rng(cells[0] * 100 + cells[1])
  h, w = cells[0] * 8, cells[1] * 8
  imgs = rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
  for k in (2, 4, 8):
    got = engine.pool_rgb(imgs, k)
    assert got.shape == (3, h // k, w // k, 3) and got.dtype == np.uint8
    for i in range(3):
      assert np.array_equal(got[i], _blocks(imgs[i], k)), (cells, k, i)
  # hand-computed blocks at the last cell of the map: 8 x 8 of 100 with one pixel 131 -> 100.48
  # -> 100 at k = 8; its 2 x 2 block at k = 2: (3 * 100 + 131 + 2) // 4 = 108.25 -> 108
  img = np.full((h, w, 3), 100, np.uint8)
  img[h - 1, w - 1, 0] = 131
  img[h - 1, w - 2, 1] = 102   # 2 x 2 block: (3 * 100 + 102 + 2) // 4 = 101
  p8, p2 = engine.pool_rgb(img, 8), engine.pool_rgb(img, 2)
  assert p8.shape == (cells[0], cells[1], 3)
  assert p8[-1, -1].tolist() == [100, 100, 100] and int(p8.sum()) == 100 * p8.size
  assert p2[-1, -1].tolist() == [108, 101, 100]
  assert int(p2.astype(np.int64).sum()) == 100 * p2.size + 8 + 1
  # rounding half up on an odd-width row: a block summing to 2 of 4 -> 0.5 -> 1
  img = np.zeros((h, w, 3), np.uint8)
  img[0, w - 2:w, 2] = [1, 1]
  assert engine.pool_rgb(img, 2)[0, -1].tolist() == [0, 0, 1]
  assert engine.pool_rgb(img, 4)[0, -1].tolist() == [0, 0, 0]   # 2 / 16 -> 0.125 -> 0
