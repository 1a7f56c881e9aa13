"""Searches the seeds of the unit programs (api_programs.UNIT_SEEDS) on the CPU, by the model alone:
per level the pair of seeds (one for the 6-world profile, one for the 23-world one) whose two
programs together hold the most of the conditions tests/test_api_programs_cpu.py asserts of them, the
smallest seeds first.  Prints the list to paste into api_programs.py and, per level, what is still
missing with the number of seeds tried.

  python tests/tools/search_unit_programs.py [seeds for n = 6] [seeds for n = 23]

The committed UNIT_SEEDS are what `python tests/tools/search_unit_programs.py 140 24` prints (two
minutes on eight cores); the defaults are a quick look."""
import multiprocessing
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")]

import api_programs as ap   # noqa: E402
import test_api_programs_cpu as tests   # noqa: E402  (the exemptions are listed there)

FIRST_SEED = 3000
WANTED = ap.UNIT_COVER_CONDITIONS + (ap.UNIT_DEAD_VIEWER, ap.UNIT_OFF_THE_MAP)


def _covers(job):
  name, seeds = job
  profile = next(p for p in ap.UNIT_PROFILES if p["name"] == name)
  out = []
  for seed in seeds:
    cover = ap.program_cover(ap.make_program(seed, profile))
    out.append((seed, {k for k in WANTED if cover[k] > 0}))
  return name, out


def main(small=40, large=12):
  jobs = [(p["name"], list(range(FIRST_SEED, FIRST_SEED + (small if p["n"] == 6 else large))))
          for p in ap.UNIT_PROFILES if not p["stock"]]
  with multiprocessing.Pool(min(len(jobs), len(os.sched_getaffinity(0)))) as pool:
    found = dict(pool.map(_covers, jobs))
  seeds = {}
  for pack in ap.LEVEL_PACKS:
    a, b = (f"{pack}-units-n{n}" for n in (6, 23))
    need = set(WANTED) - {k for k, _ in tests.UNIT_EXEMPT[pack]}
    best = max(((len(need & (ca | cb)), -(sa + sb), sa, sb) for sa, ca in found[a] for sb, cb in found[b]))
    _, _, sa, sb = best
    seeds[a], seeds[b] = sa, sb
    got = dict(found[a])[sa] | dict(found[b])[sb]
    print(f"{pack}: seeds {sa}, {sb}; missing after {len(found[a])} x {len(found[b])} seeds: {sorted(need - got)}")
  print("UNIT_SEEDS =", [seeds.get(p["name"], FIRST_SEED) for p in ap.UNIT_PROFILES])


if __name__ == "__main__":
  main(*(int(a) for a in sys.argv[1:3]))
