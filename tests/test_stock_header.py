"""The constants compiled into the stock frame kernels (csrc/stock.h, csrc/stock_clean_up.h) and
mp_create's selection of those kernels, on the host alone (an MpKernelVariant request without an engine: the
host-only pack decoder, no GPU): the committed header is what tools/make_stock_header.py writes from
the committed pack, byte for byte; the committed pack with its default player count selects the stock
kernels; a pack with one edited cell, one fewer player, another view window, other rule constants,
a padded record or MpDevOptions.generic_kernel is refused and runs the generic ones."""
import importlib.util
import os

import numpy as np
import pytest

import geometry
import util
from meltingpot_amd import engine, lower, pack as pack_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
  spec = importlib.util.spec_from_file_location(
      "make_stock_header", os.path.join(ROOT, "tools", "make_stock_header.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_committed_header_is_what_the_generator_writes():
  tool = _tool()
  for level in tool.LEVELS:
    with open(tool.header_path(level)) as f:
      committed = f.read()
    assert committed == tool.generate(level), f"stock_{level}.h is stale: run tools/make_stock_header.py"


def test_header_holds_the_packs_geometry(clean_up_pack):
  """A few of the folded values against the pack's own header table, read in Python."""
  tool = _tool()
  variant, text = tool.pack_fields(clean_up_pack)
  assert variant == engine.KERNEL_STOCK
  got = {}
  for line in text.splitlines():
    parts = line.split(" ")
    if parts[0] == "t":
      got[parts[1]] = parts[2]
  hdr = pack_lib.loads(clean_up_pack)["hdr"]
  for member, index in (("H", lower.HDR_H), ("W", lower.HDR_W), ("L", lower.HDR_L),
                        ("P_pack", lower.HDR_P), ("vl", lower.HDR_VL), ("vf", lower.HDR_VF),
                        ("sprite_size", lower.HDR_SPRITE)):
    assert int(got[member]) == int(hdr[index]), member
  assert int(got["P"]) == 7   # (the pack's default player count, of the 15 avatars it holds)
  assert int(got["world_stride"]) % 64 == 0 and int(got["grid_bytes"]) == 9 * 21 * 30


def test_stock_pack_selects_the_stock_kernels(clean_up_pack):
  assert engine.kernel_variant(clean_up_pack) == engine.KERNEL_STOCK
  assert engine.kernel_variant(clean_up_pack, num_players=7) == engine.KERNEL_STOCK
  # the same settings lowered again give the same bytes, hence the same kernels
  assert engine.kernel_variant(geometry.pack("clean_up")) == (
      engine.KERNEL_STOCK if geometry.pack("clean_up") == clean_up_pack else engine.KERNEL_GENERIC)


def _one_cell_edited(clean_up_pack):
  """One floor cell of the lowest layer's initial grid takes the state of its neighbour: no cell
  list, count or header field changes."""
  t = pack_lib.loads(clean_up_pack)
  grid = t["init_grid"].copy()
  flat = grid.reshape(-1)
  i = next(i for i in range(1, flat.size) if flat[i] != flat[i - 1])
  flat[i] = flat[i - 1]
  return util.patch_pack(clean_up_pack, tables={"init_grid": grid})


def test_edited_packs_are_refused(clean_up_pack, commons_pack):
  G = engine.KERNEL_GENERIC
  assert engine.kernel_variant(_one_cell_edited(clean_up_pack)) == G
  assert engine.kernel_variant(clean_up_pack, num_players=6) == G
  assert engine.kernel_variant(geometry.pack("clean_up", view=(1, 1, 1, 0))) == G
  assert engine.kernel_variant(geometry.pack("clean_up", width=32)) == G
  assert engine.kernel_variant(util.fertile_clean_up(clean_up_pack)) == G
  assert engine.kernel_variant(util.patch_pack(clean_up_pack, MAXFRAMES=100)) == G
  assert engine.kernel_variant(commons_pack) == G


def test_dev_options_force_the_generic_kernels(clean_up_pack):
  assert engine.kernel_variant(clean_up_pack, dev={"generic_kernel": 1}) == engine.KERNEL_GENERIC
  # a padded record is another world_stride, which is folded
  assert engine.kernel_variant(clean_up_pack, dev={"record_pad": 1}) == engine.KERNEL_GENERIC
  assert engine.kernel_variant(clean_up_pack, dev={"batch_worlds": 1}) == engine.KERNEL_STOCK


def test_bad_pack_is_an_error_not_a_variant(clean_up_pack):
  with pytest.raises((engine.EngineError, ValueError)):
    engine.kernel_variant(clean_up_pack[:-16])


def test_folded_members_exist_once_in_the_field_lists():
  """Every member the header pins is named exactly once in csrc/stock.h's lists (a member listed
  twice would compile, a member dropped from the list would silently stay run-time)."""
  tool = _tool()
  with open(tool.header_path("clean_up")) as f:
    members = [line.split("X(")[1].split(",")[0] for line in f if line.lstrip().startswith("X(")]
  assert len(members) == len(set(members)) and len(members) > 60
  with open(os.path.join(ROOT, "meltingpot_amd", "csrc", "stock.h")) as f:
    lists = f.read()
  for m in members:
    assert lists.count(f"X({m})") == 1, m
