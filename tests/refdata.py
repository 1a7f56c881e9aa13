"""The reference's substrate configs as the tests read them, from a recorded fixture.

tests/golden/reference_configs.pkl.xz (written by tests/tools/make_reference_fixture.py)
holds, per config module, the constants and `get_config()` the tests use, and the
`build(roles, config)` lab2d settings of every (name, roles) they build.  The calls
mirror `meltingpot_amd.refshim` (`load_config_module`, `build_settings`), so a test
reads the same values with or without the reference tree.  A (name, roles) that was
not recorded raises KeyError: add it to the generator's BUILDS and rerun it.
"""
import copy
import functools
import lzma
import os
import pickle
import random

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "reference_configs.pkl.xz")


@functools.lru_cache(maxsize=1)
def _fixture():
  with lzma.open(FIXTURE, "rb") as f:
    return pickle.load(f)


class ConfigModule:
  """What the tests use of `configs/substrates/<name>.py`: its constants as attributes,
  `get_config()` and `build(roles, config)` (fresh copies on every call, like the module),
  and for coins `get_ascii_map` with the module's `random`."""

  random = random   # the generator the module's functions draw from, as in the module

  def __init__(self, name):
    rec = _fixture()["modules"][name]
    self.__name__ = name
    self.__dict__.update(copy.deepcopy(rec["attrs"]))
    self._config = rec["config"]
    self._maps = rec.get("ascii_maps")

  def get_config(self):
    return copy.deepcopy(self._config)

  def build(self, roles, config=None):
    key = (self.__name__, tuple(roles))
    settings = _fixture()["settings"]
    if key not in settings:
      raise KeyError(f"{key} was not recorded: add it to tests/tools/make_reference_fixture.py")
    return copy.deepcopy(settings[key])

  def get_ascii_map(self, min_width, max_width, min_height, max_height):
    """coins.py:45-82: width, then height drawn with self.random.randint; the map the
    module's generator made for that size."""
    if self._maps is None:
      raise AttributeError(f"{self.__name__} has no get_ascii_map")
    width = self.random.randint(min_width, max_width)
    height = self.random.randint(min_height, max_height)
    return self._maps[(min_width, max_width, min_height, max_height, width, height)]


def load_config_module(name):
  return ConfigModule(name)


def build_settings(name, roles):
  """(settings, module, config) as `refshim.build_settings` returns them."""
  module = load_config_module(name)
  config = module.get_config()
  return module.build(tuple(roles), config), module, config


def map_positions(name, players):
  """{char: sorted [(x, y)]}: the reference's get_game_object_positions_from_map of every
  character of the (name, ('default',) * players) map."""
  return copy.deepcopy(_fixture()["map_positions"][(name, players)])
