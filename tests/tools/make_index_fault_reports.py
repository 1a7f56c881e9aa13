"""Writes tests/golden/index_fault_reports.json: what the next synchronising call answers after a
request whose index list held ONE entry out of range — the deferred reports of the fault words
(FAULT_STATE_INDEX, kFaultCheckWorld, kFaultStartWorld) — as {case name: [return code of mp_sync,
last-error text]}.  Run on the commit whose texts are to be pinned, on a GPU:

    python tests/tools/make_index_fault_reports.py

Every case issues one request on a clean_up engine of 2 worlds with a bank of 3 rows; the kernel
skips the bad element and writes the words (nothing faults), `mp_sync` reports them once, and a
second `mp_sync` answers MP_OK.  One case per index-fault code the API can reach (mp_common.h:
IndexFault; the refused row of a checked load, code 4, is told by the kFaultCheckWorld report), the
two forms of the episode-start report, and the checked load's.  The frame kernel's stall report and
the matrix reward report are not here: only an engine bug or one special level produces them.
tests/test_gpu_index_fault_reports.py replays `cases`; tests/test_index_fault_reports_cpu.py checks
the fixture's shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from meltingpot_amd import engine as E  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "index_fault_reports.json")
N, BANK_ROWS, K = 2, 3, 2
FAR_ROW, FAR_PLAYER, FAR_WORLD, BAD_ORIENTATION = 7, 99, 5, 7
PAIRS = {"view": (7, 8), "ego_layer": (11, 12), "view_hash": (13, 14), "ego_planes": (15, 16), "avatar_ids": (18, 19)}
# case name -> the index-fault code its report tells (None: a report with words of its own)
CODES = {"load/src": 1, "save/worlds": 2, "observe/rows": 3, "check/rows": 5, "hash/rows": 6,
         "listed/world": 9, "listed/repeat": 10, "ego_planes/classes": 17,
         "checked_load/malformed_row": None, "episode_starts/rows": None, "episode_starts/malformed_row": None}
for _name, (_row, _player) in PAIRS.items():
  CODES[f"{_name}/rows"], CODES[f"{_name}/players"] = _row, _player


class Ctx:
  """Two engines and what their cases share.  `eng`: clean_up, 2 worlds, reset; `bank`: 3 rows saved
  from it; `broken`: the bank with player 0's orientation of row 1 out of range (a malformed record).
  `short`: the same level with episodes of 2 frames, for the episode starts; `short_bank`,
  `short_broken` likewise."""

  def __init__(self):
    import torch
    import util
    from meltingpot_amd import substrate
    self.torch, self.keep = torch, []
    pack = E.load_pack("clean_up")
    self.eng = E.Engine(pack, N, device=0)
    self.short = E.Engine(util.patch_pack(pack, MAXFRAMES=2), N, device=0)
    for name, eng in (("bank", self.eng), ("short_bank", self.short)):
      eng.reset()
      bank = eng.save_worlds(torch.tensor([0, 1, 0]))
      broken = bank.clone()
      substrate.StateFields(broken, eng.state_layout()).orientation[1, 0] = BAD_ORIENTATION
      setattr(self, name, bank)
      setattr(self, name.replace("bank", "broken"), broken)
      eng.sync()
    self.L = self.eng._L

  def ints(self, *values):
    """An index list on the device, kept alive until `close` (the launches that read it run later)."""
    self.keep.append(self.torch.tensor(values, dtype=self.torch.int32, device=self.eng.device))
    return self.keep[-1]

  def close(self):
    self.torch.cuda.synchronize()
    self.eng.close()
    self.short.close()


def cases(c: Ctx):
  """[(name, engine, the call that issues the one request)]"""
  e, bank = c.eng, c.bank
  noop = c.torch.zeros((K, N, e.P), dtype=c.torch.int32, device=e.device)
  zeros = c.torch.zeros(e.num_layer_ids, dtype=c.torch.int32, device=e.device)
  wild = zeros.clone()
  wild[3] = 5
  good, far, strangers = c.ints(0, 1), c.ints(0, FAR_ROW), c.ints(0, FAR_PLAYER)
  out = [
      ("load/src", e, lambda: e.load_worlds(bank, c.ints(0, FAR_ROW))),
      ("save/worlds", e, lambda: e.save_worlds(c.ints(0, FAR_WORLD))),
      ("observe/rows", e, lambda: e.observe_states(bank, E.OBS_LAYER, rows=far)),
      ("check/rows", e, lambda: e.check_states(bank, rows=far)),
      ("hash/rows", e, lambda: e.hash_states(bank, rows=far)),
      ("view/rows", e, lambda: e.observe_views(bank, E.OBS_LAYER, good, rows=far)),
      ("view/players", e, lambda: e.observe_views(bank, E.OBS_LAYER, strangers, rows=good)),
      ("listed/world", e, lambda: e.step_many(noop, worlds=c.ints(0, FAR_WORLD))),
      ("listed/repeat", e, lambda: e.step_many(noop, worlds=c.ints(1, 1))),
      ("ego_planes/classes", e, lambda: e.observe_ego_planes(wild, bank, num_classes=1)),
      ("checked_load/malformed_row", e, lambda: e.load_worlds(c.broken, c.ints(0, 1), check=True)),
  ]
  draws = {"ego_layer": e.observe_ego_layer, "view_hash": e.hash_views,
           "ego_planes": lambda *a, **k: e.observe_ego_planes(zeros, *a, num_classes=1, **k),
           "avatar_ids": e.observe_avatar_ids}
  for name, draw in draws.items():
    out.append((f"{name}/rows", e, lambda draw=draw: draw(bank, rows=far)))
    out.append((f"{name}/players", e, lambda draw=draw: draw(bank, rows=good, players=strangers)))

  s = c.short
  still = c.torch.zeros((N, s.P), dtype=c.torch.int32, device=s.device)

  def starts(bank, rows, verdicts=None):
    """Registers the starts and steps through the end of the 2-frame episode into the first start."""
    s.reset()
    s.set_episode_starts(bank, rows, verdicts=verdicts)
    for _ in range(3):
      s.step(still)

  out.append(("episode_starts/rows", s, lambda: starts(c.short_bank, c.ints(FAR_ROW, -1))))
  out.append(("episode_starts/malformed_row", s,
              lambda: starts(c.short_broken, c.ints(-1, 1), s.check_states(c.short_broken))))
  assert sorted(n for n, *_ in out) == sorted(CODES)
  return out


def replay(c: Ctx, which):
  """{name: [mp_sync's return code, its text]} of `which`; every report is made once."""
  got = {}
  for name, eng, call in which:
    call()
    rc = int(c.L.mp_sync(eng._h))
    got[name] = [rc, (c.L.mp_last_error() or b"").decode() if rc else ""]
    assert int(c.L.mp_sync(eng._h)) == 0, (name, "reported twice")
  return got


def main():
  c = Ctx()
  got = replay(c, cases(c))
  c.close()
  assert all(rc == E.MP_ERR_INVALID and text for rc, text in got.values()), got
  with open(GOLDEN, "w") as f:
    json.dump(dict(sorted(got.items())), f, indent=1)
    f.write("\n")
  print(GOLDEN, len(got), "cases,", os.path.getsize(GOLDEN), "bytes")
  for name, (rc, text) in sorted(got.items()):
    print(name, rc, text)


if __name__ == "__main__":
  main()
