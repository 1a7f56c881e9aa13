"""What of the oracle's rules a run of tests reached (a measuring instrument, host code only).

  make -C oracle cov                                   # liboracle_cov.so, objects under oracle/cov/
  python tests/tools/oracle_coverage.py --reset        # forget earlier counts
  MP_ORACLE_LIB=$PWD/oracle/liboracle_cov.so python -m pytest tests/test_gpu_situations.py -m gpu
  python tests/tools/oracle_coverage.py --report out.md [--lines]

The report runs `gcov -b` over engine.c and the level files and prints, per file, how many
lines and branch directions there are and how many were never taken; with --lines also which
(`file:line` for a line never run, `file:line bN` for a direction never taken).  The `*_dump`,
`*_destroy` and accessor functions (non-static functions that read a `const Oracle*`) are left
out: they are how the tests look at a world, not rules.  --json writes the sets, so that two runs
can be compared (--only-in A.json B.json: what B reaches and A does not)."""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")
COV = os.path.join(ORACLE, "cov")
FILES = ("engine.c", "clean_up.c", "commons_harvest.c", "territory.c", "coins.c", "the_matrix.c",
         "coop_mining.c", "gift_refinements.c", "collaborative_cooking.c", "externality_mushrooms.c")


def _left_out(name, definition):
  if name.endswith(("_dump", "_destroy")):
    return True
  return not definition.lstrip().startswith("static") and "const Oracle*" in definition.split(")")[0]


def measure():
  """{file: {"lines": [n, ...], "missed_lines": [...], "branches": count, "missed_branches":
  ["line bK", ...]}} from the .gcda files under oracle/cov."""
  out = {}
  with tempfile.TemporaryDirectory(prefix="mp_gcov_") as tmp:
    for src in FILES:
      # (the objects name their sources relative to oracle/: gcov runs there, its files move out)
      subprocess.run(["gcov", "-b", "-c", "-o", COV, src], cwd=ORACLE, check=True,
                     stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
      for made in glob.glob(os.path.join(ORACLE, "*.gcov")):
        os.replace(made, os.path.join(tmp, os.path.basename(made)))
      path = os.path.join(tmp, src + ".gcov")
      if not os.path.exists(path):
        raise SystemExit(f"gcov wrote nothing for {src}: run the tests with MP_ORACLE_LIB set first")
      rec = {"lines": [], "missed_lines": [], "branches": 0, "missed_branches": []}
      skip, pending, line_no = False, None, 0
      for text in open(path, errors="replace"):
        m = re.match(r"function (\S+) called", text)
        if m:
          pending = m.group(1)
          continue
        m = re.match(r"\s*(\S+):\s*(\d+):(.*)", text)
        if m:
          count, line_no, code = m.group(1), int(m.group(2)), m.group(3)
          if pending is not None and line_no > 0:
            skip, pending = _left_out(pending, code), None
          if line_no == 0 or skip or count == "-":
            continue
          rec["lines"].append(line_no)
          if count.startswith(("#####", "=====")):
            rec["missed_lines"].append(line_no)
          continue
        m = re.match(r"branch\s+(\d+) (never executed|taken (\d+))", text)
        if m and not skip:
          rec["branches"] += 1
          if m.group(2) == "never executed" or int(m.group(3)) == 0:
            rec["missed_branches"].append(f"{line_no} b{m.group(1)}")
      out[src] = rec
  return out


def table(data, lines=False):
  rows = ["| file | lines | never run | % run | branch directions | never taken | % taken |",
          "|---|---|---|---|---|---|---|"]
  for src, r in data.items():
    n, m, b, mb = len(r["lines"]), len(r["missed_lines"]), r["branches"], len(r["missed_branches"])
    rows.append(f"| {src} | {n} | {m} | {100 * (n - m) / max(n, 1):.1f} | {b} | {mb} | {100 * (b - mb) / max(b, 1):.1f} |")
  if lines:
    for src, r in data.items():
      rows.append(f"\n{src}: lines never run: " + (", ".join(str(l) for l in r["missed_lines"]) or "none"))
      rows.append(f"{src}: directions never taken: " + (", ".join(r["missed_branches"]) or "none"))
  return "\n".join(rows) + "\n"


def only_in(a, b):
  """What run b reaches and run a does not."""
  rows = []
  for src in b:
    gained = sorted(set(a[src]["missed_lines"]) - set(b[src]["missed_lines"]))
    branches = [x for x in a[src]["missed_branches"] if x not in set(b[src]["missed_branches"])]
    rows.append(f"{src}: lines {', '.join(map(str, gained)) or 'none'}; directions {', '.join(branches) or 'none'}")
  return "\n".join(rows) + "\n"


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  ap.add_argument("--reset", action="store_true", help="delete the counts under oracle/cov")
  ap.add_argument("--report", metavar="FILE", help="write the table ('-': print it)")
  ap.add_argument("--lines", action="store_true", help="list the lines and directions too")
  ap.add_argument("--json", metavar="FILE", help="write the measured sets")
  ap.add_argument("--only-in", nargs=2, metavar=("A.json", "B.json"))
  args = ap.parse_args()
  if args.reset:
    for path in glob.glob(os.path.join(COV, "*.gcda")):
      os.unlink(path)
  if args.only_in:
    a, b = (json.load(open(p)) for p in args.only_in)
    sys.stdout.write(only_in(a, b))
  if args.report or args.json:
    data = measure()
    if args.json:
      with open(args.json, "w") as f:
        json.dump(data, f)
    if args.report:
      text = table(data, args.lines)
      if args.report == "-":
        sys.stdout.write(text)
      else:
        with open(args.report, "w") as f:
          f.write(text)


if __name__ == "__main__":
  main()
