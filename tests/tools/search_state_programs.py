"""Searches the seeds of the state programs (api_programs.STATE_SEEDS) on the CPU, by the model alone:
per level the pair of seeds (one for the 6-world profile, one for the 23-world one) whose two
programs together hold the most of the conditions tests/test_api_programs_cpu.py asserts, the
smallest seeds first.  Prints the list to paste into api_programs.py and, per level, what is still
missing with the number of seeds tried.

  python tests/tools/search_state_programs.py [seeds for n = 6] [seeds for n = 23]

The defaults (40 and 12 seeds from 2000 on) find every level's pair but territory's, whose committed
seeds came from 160 and 30."""
import multiprocessing
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")]

import api_programs as ap   # noqa: E402
import states_recipe        # noqa: E402

FIRST_SEED = 2000


def required(pack):
  dead = (ap.DEAD_AVATAR_CONDITION,) if pack in states_recipe.DEAD_AVATARS else ()
  return ap.COVER_CONDITIONS + dead + ap.REWARD_CONDITIONS


def _covers(job):
  name, seeds = job
  profile = next(p for p in ap.STATE_PROFILES if p["name"] == name)
  out = []
  for seed in seeds:
    cover = ap.program_cover(ap.make_program(seed, profile))
    out.append((seed, {k for k in required(profile["pack"]) if cover[k] > 0}))
  return name, out


def main(small=40, large=12):
  jobs = [(p["name"], list(range(FIRST_SEED, FIRST_SEED + (small if p["n"] == 6 else large))))
          for p in ap.STATE_PROFILES if not p["stock"]]
  with multiprocessing.Pool(min(len(jobs), len(os.sched_getaffinity(0)))) as pool:
    found = dict(pool.map(_covers, jobs))
  seeds = {}
  for pack in ap.LEVEL_PACKS:
    a, b = (f"{pack}-states-n{n}" for n in ap.STATE_WORLD_COUNTS)
    need = set(required(pack))
    best = max(((len(need & (ca | cb)), -(sa + sb), sa, sb) for sa, ca in found[a] for sb, cb in found[b]))
    _, _, sa, sb = best
    seeds[a], seeds[b] = sa, sb
    got = dict(found[a])[sa] | dict(found[b])[sb]
    print(f"{pack}: seeds {sa}, {sb}; missing after {len(found[a])} x {len(found[b])} seeds: {sorted(need - got)}")
  print("STATE_SEEDS =", [seeds.get(p["name"], FIRST_SEED) for p in ap.STATE_PROFILES])


if __name__ == "__main__":
  main(*(int(a) for a in sys.argv[1:3]))
