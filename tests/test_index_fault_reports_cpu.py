"""The shape of tests/golden/index_fault_reports.json (tests/tools/make_index_fault_reports.py
recorded it on a GPU; tests/test_gpu_index_fault_reports.py replays it): one entry per reachable
index-fault code, every one MP_ERR_INVALID told by mp_sync, and three texts spelt out by hand."""
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import make_index_fault_reports as T  # noqa: E402


@pytest.fixture(scope="module")
def golden():
  with open(T.GOLDEN) as f:
    return json.load(f)


def test_one_entry_per_reachable_code(golden):
  assert set(golden) == set(T.CODES)
  codes = sorted(c for c in T.CODES.values() if c is not None)
  assert codes == [c for c in range(1, 20) if c != 4]   # (4, a checked load's refused row: the kFaultCheckWorld report)
  for name, (rc, text) in golden.items():
    assert rc == T.E.MP_ERR_INVALID and text.startswith("mp_sync: "), name
    assert not re.search(r"0x[0-9a-f]{6,}", text), name   # no pointer in a report
  assert len({text for _, text in golden.values()}) == len(golden)


def test_the_five_pairs_share_one_sentence(golden):
  names = {"view": "MpStatesView", "ego_layer": "MpEgoLayer", "view_hash": "MpViewHash",
           "ego_planes": "MpEgoPlanes", "avatar_ids": "MpAvatarIds"}
  assert set(names) == set(T.PAIRS)
  for case, who in names.items():
    no_row = "not a row of the bank" + ("" if case == "view" else " (with no bank: no world of this engine)")
    assert golden[f"{case}/rows"][1] == (
        f"mp_sync: {who}: rows[1] = {T.FAR_ROW} is {no_row}; element 1 of the destination was left as it was")
    assert golden[f"{case}/players"][1] == (
        f"mp_sync: {who}: players[1] = {T.FAR_PLAYER} is not a player of this engine; element 1 of the "
        "destination was left as it was")


def test_the_table_says_what_it_should(golden):
  """Entries by hand, so that a fixture recorded from a broken library does not pass."""
  assert golden["ego_layer/rows"] == [
      -1, "mp_sync: MpEgoLayer: rows[1] = 7 is not a row of the bank (with no bank: no world of this engine); "
          "element 1 of the destination was left as it was"]
  assert golden["listed/repeat"] == [
      -1, "mp_sync: MpStepListed: worlds[1] = 1 repeats an earlier entry's world; the entry ran nothing and "
          "element 1 of every per-call tensor was left as it was"]
  assert golden["save/worlds"] == [
      -1, "mp_sync: MP_STATES_SAVE: worlds[1] = 5 is not a world of this engine; row 1 was left as it was"]
  assert golden["load/src"] == [
      -1, "mp_sync: MP_STATES_LOAD: src[1] = 7 is neither -1 nor a row of the bank; world 1 was left as it was"]
  assert golden["episode_starts/rows"] == [
      -1, "mp_sync: MpEpisodeStarts: rows[0] = 7 is neither -1 nor a row of the bank; world 0 took the level's "
          "own reset"]
  assert golden["checked_load/malformed_row"][1].startswith(
      "mp_sync: checked MP_STATES_LOAD: row 1, which src[1] names, is not a well-formed record (rule 3, ")
  assert golden["episode_starts/malformed_row"][1].startswith(
      "mp_sync: MpEpisodeStarts: row 1, which rows[1] names, is not a well-formed record (rule 3, ")
