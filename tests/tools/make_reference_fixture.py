#!/usr/bin/env python3
"""Writes tests/golden/reference_configs.pkl.xz: what the CPU tests read from the
reference's substrate config modules (configs/substrates/<name>.py), recorded once so
that the tests run without the reference tree (tests/refdata.py serves it):

  * per module: its upper-case constants (ACTION_SET, ASCII_MAP, CHAR_PREFAB_MAP,
    COOKING_TIME, ...) and `get_config()` (refshim's ConfigDict / Spec stand-ins);
  * the `build(roles, get_config())` lab2d settings of every (name, roles) in BUILDS,
    after random.seed(0) (coins.py draws its map size and coin colours in build(): the
    tests seed the same way);
  * coins.py's `get_ascii_map` for every width and height it can draw;
  * the reference's `game_object_utils.get_game_object_positions_from_map` of every
    character of the maps in MAP_POSITIONS.

Runs where the reference tree is:

  python tests/tools/make_reference_fixture.py [--reference DIR]
"""
import argparse
import lzma
import os
import pickle
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

import random  # noqa: E402

from meltingpot_amd import refshim  # noqa: E402


def constants(mod):
  """The module's upper-case names: data (maps, action sets, tables, numbers)."""
  return {k: v for k, v in vars(mod).items() if k.isupper() and not callable(v)}


def every_ascii_map(mod, config):
  """{(min_width, max_width, min_height, max_height, width, height): map} of the module's
  get_ascii_map, its two randint draws (width, then height) fixed to every outcome."""
  bounds = (config.min_width, config.max_width, config.min_height, config.max_height)
  maps, real = {}, mod.random.randint
  try:
    for w in range(config.min_width, config.max_width + 1):
      for h in range(config.min_height, config.max_height + 1):
        draws = iter((w, h))
        mod.random.randint = lambda a, b: next(draws)
        maps[bounds + (w, h)] = mod.get_ascii_map(*bounds)
  finally:
    mod.random.randint = real
  return maps


# every (name, roles) whose settings a test builds
BUILDS = {
    "bach_or_stravinsky_in_the_matrix__arena": [
        ("bach_fan",) * 8, ("bach_fan",) * 4 + ("stravinsky_fan",) * 4, ("default",) * 8,
        ("stravinsky_fan", "default", "bach_fan", "bach_fan", "default", "stravinsky_fan",
         "default", "bach_fan"),
        ("stravinsky_fan",) * 8],
    "bach_or_stravinsky_in_the_matrix__repeated": [
        ("bach_fan",) * 2, ("bach_fan", "stravinsky_fan"), ("default",) * 2,
        ("stravinsky_fan", "bach_fan"), ("stravinsky_fan",) * 2],
    "chicken_in_the_matrix__arena": [("default",) * 8],
    "chicken_in_the_matrix__repeated": [("default",) * 2],
    "clean_up": [("default",) * 7, ("default",) * 15],
    "coins": [("default",) * 2],
    "collaborative_cooking__asymmetric": [("default",) * 2],
    "collaborative_cooking__circuit": [("default",) * 2],
    "collaborative_cooking__cramped": [("default",) * 2],
    "collaborative_cooking__crowded": [("default",) * 9],
    "collaborative_cooking__figure_eight": [("default",) * 6],
    "collaborative_cooking__forced": [("default",) * 2],
    "collaborative_cooking__ring": [("default",) * 2],
    "commons_harvest__closed": [("default",) * 7, ("default",) * 16],
    "commons_harvest__open": [("default",) * 4, ("default",) * 5, ("default",) * 7,
                              ("default",) * 16],
    "commons_harvest__partnership": [("default",) * 7],
    "coop_mining": [("default",) * 6, ("default",) * 8, ("target",) * 8],
    "externality_mushrooms__dense": [("default",) * 5],
    "gift_refinements": [("default",) * 6, ("default",) * 8, ("target",) * 8],
    "prisoners_dilemma_in_the_matrix__arena": [("default",) * 8],
    "prisoners_dilemma_in_the_matrix__repeated": [("default",) * 2],
    "pure_coordination_in_the_matrix__arena": [("default",) * 8],
    "pure_coordination_in_the_matrix__repeated": [("default",) * 2],
    "rationalizable_coordination_in_the_matrix__arena": [("default",) * 8],
    "rationalizable_coordination_in_the_matrix__repeated": [("default",) * 2],
    "running_with_scissors_in_the_matrix__arena": [("default",) * 8],
    "running_with_scissors_in_the_matrix__one_shot": [("default",) * 2],
    "running_with_scissors_in_the_matrix__repeated": [("default",) * 2],
    "stag_hunt_in_the_matrix__arena": [("default",) * 8],
    "stag_hunt_in_the_matrix__repeated": [("default",) * 2],
    "territory__inside_out": [("default",) * 5],
    "territory__open": [("default",) * 9],
    "territory__rooms": [("default",) * 9],
}

# base modules whose constants the tests read (their levels' modules import them)
BASES = ("territory", "collaborative_cooking", "externality_mushrooms")

# (name, players) whose map tests/test_reference_kats.py visits
MAP_POSITIONS = [("clean_up", 7), ("territory__rooms", 9), ("commons_harvest__open", 16)]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reference", default=refshim.DEFAULT_REFERENCE_ROOT)
  args = ap.parse_args()
  modules, settings, positions = {}, {}, {}
  for name, all_roles in BUILDS.items():
    mod = refshim.load_config_module(name, args.reference)
    modules[name] = {"attrs": constants(mod), "config": mod.get_config()}
    for roles in all_roles:
      random.seed(0)
      settings[(name, roles)] = mod.build(roles, mod.get_config())
    if hasattr(mod, "get_ascii_map"):
      modules[name]["ascii_maps"] = every_ascii_map(mod, mod.get_config())
  for name in BASES:
    mod = refshim.load_config_module(name, args.reference)
    modules[name] = {"attrs": constants(mod), "config": mod.get_config()}
  gou = sys.modules["meltingpot.utils.substrates.game_object_utils"]
  for name, players in MAP_POSITIONS:
    ascii_map = settings[(name, ("default",) * players)]["simulation"]["map"]
    positions[(name, players)] = {
        ch: sorted((t.position.x, t.position.y)
                   for t in gou.get_game_object_positions_from_map(ascii_map, ch))
        for ch in sorted(set(ascii_map) - {"\n"})}
  fixture = {"modules": modules, "settings": settings, "map_positions": positions,
             "source": "configs/substrates/<name>.py of the reference, recorded by "
                       "tests/tools/make_reference_fixture.py"}
  out = os.path.join(ROOT, "tests", "golden", "reference_configs.pkl.xz")
  with lzma.open(out, "wb") as f:
    pickle.dump(fixture, f, protocol=4)
  print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
  main()
