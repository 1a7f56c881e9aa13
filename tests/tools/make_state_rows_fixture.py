"""Writes tests/golden/state_rows.npz: real world records of every recipe pack, for the CPU tests
of the record check (tests/test_state_rows_fixture_cpu.py).  Run once on a GPU:

    python tests/tools/make_state_rows_fixture.py

Per pack of states_recipe.PACKS: the rows of states_recipe.road(name)["all"] after steps 1 (MID),
16 (LAST) and 17 (FIRST, the auto-reset) of worlds 0 and 4, one more row with a dead avatar where
the recipe has one (states_recipe.DEAD_AVATARS), and the engine's state fingerprint — the CPU
test compares it with the host-only layout request's, so a change of the record layout asks for
a new fixture."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import states_recipe as R  # noqa: E402
from meltingpot_amd import engine  # noqa: E402

STEPS, WORLDS = (1, 16, 17), (0, 4)


def main():
  out = {}
  for name in R.PACKS:
    road = R.road(name)
    bank = road["all"].cpu().numpy()
    layout = engine.state_layout(R.pack(name))
    picks = [R.SAVE_AT.index(s) * R.N + w for s in STEPS for w in WORLDS]
    if name in R.DEAD_AVATARS:
      alive_at = layout.field_offset("aalive")
      dead = [i for i in range(len(bank)) if i not in picks and
              (bank[i, alive_at:alive_at + layout.P] == 0).any()]
      assert dead, name
      picks.append(dead[0])
    out[name + "/rows"] = bank[picks]
    out[name + "/fingerprint"] = np.array([road["fingerprint"]], np.uint64)
    print(name, out[name + "/rows"].shape)
  path = os.path.join(ROOT, "tests", "golden", "state_rows.npz")
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
  main()
