"""The ValueError texts the Python layer raises before a saved-state request is sent, for the
callers that need no device: check_episode_starts, check_states_host, hash_states_host and the
three host view functions.  The texts are the ones these functions raised before the bank-row
front was shared; they are part of the interface (callers match on them)."""
import numpy as np
import pytest
import torch

from meltingpot_amd import engine as E


def raised(fn, *args, **kwargs) -> str:
  with pytest.raises(ValueError) as err:
    fn(*args, **kwargs)
  return str(err.value)


@pytest.fixture(scope="module")
def pack():
  return E.load_pack("clean_up")


@pytest.fixture(scope="module")
def stride(pack):
  return E.state_layout(pack).world_stride


def test_check_episode_starts_texts():
  S, N = 64, 2
  bank = torch.zeros((3, S), dtype=torch.uint8)
  rows = torch.zeros(N, dtype=torch.int32)
  verdicts = torch.zeros((3, 2), dtype=torch.int32)
  assert E.check_episode_starts(bank, rows, verdicts, N, S, "cpu") == 3
  assert E.check_episode_starts(bank, rows, None, N, S, "cpu") == 3
  assert raised(E.check_episode_starts, bank.numpy(), rows, None, N, S, "cpu") == \
      "set_episode_starts: bank must be a contiguous uint8 tensor [M, 64] (got uint8 (3, 64))"
  assert raised(E.check_episode_starts, None, rows, None, N, S, "cpu") == \
      "set_episode_starts: bank must be a contiguous uint8 tensor [M, 64] (got NoneType ())"
  assert raised(E.check_episode_starts, bank.to(torch.int32), rows, None, N, S, "cpu") == \
      "set_episode_starts: bank must be a contiguous uint8 tensor [M, 64] (got torch.int32 (3, 64))"
  assert raised(E.check_episode_starts, bank[:, :32], rows, None, N, S, "cpu") == \
      "set_episode_starts: bank must be a contiguous uint8 tensor [M, 64] (got torch.uint8 (3, 32))"
  assert raised(E.check_episode_starts, bank.t().contiguous().t(), rows, None, N, S, "cpu") == \
      "set_episode_starts: bank must be a contiguous uint8 tensor [M, 64] (got torch.uint8 (3, 64))"
  assert raised(E.check_episode_starts, bank[:0], rows, None, N, S, "cpu") == \
      "set_episode_starts: the bank has no rows"
  assert raised(E.check_episode_starts, bank, rows[:1], None, N, S, "cpu") == \
      "set_episode_starts: rows must be a contiguous int32 tensor [2], one row index per world (got torch.int32 (1,))"
  assert raised(E.check_episode_starts, bank, rows.to(torch.int64), None, N, S, "cpu") == \
      "set_episode_starts: rows must be a contiguous int32 tensor [2], one row index per world (got torch.int64 (2,))"
  assert raised(E.check_episode_starts, bank, rows, verdicts[:2], N, S, "cpu") == \
      "set_episode_starts: verdicts must be a contiguous int32 tensor [3, 2], check_states of the whole bank " \
      "(got torch.int32 (2, 2))"
  assert raised(E.check_episode_starts, bank, rows, verdicts, N, S, "cuda:0") == \
      "set_episode_starts: bank lives on cpu, the engine on cuda:0"
  # the order of the checks: the bank, its rows, the row list, the verdicts, the devices
  assert raised(E.check_episode_starts, bank[:0], rows[:1], None, N, S, "cuda:0") == \
      "set_episode_starts: the bank has no rows"
  assert raised(E.check_episode_starts, bank, rows[:1], verdicts[:2], N, S, "cuda:0").startswith(
      "set_episode_starts: rows must be")


@pytest.mark.parametrize("fn,who,verb", [(E.check_states_host, "check_states_host", "judge"),
                                         (E.hash_states_host, "hash_states_host", "hash")])
def test_host_bank_texts(pack, stride, fn, who, verb):
  rows = np.zeros((3, stride), np.uint8)
  assert raised(fn, pack, rows[0]) == f"{who}: rows must be a uint8 array [M, S]"
  assert raised(fn, pack, rows[:0]) == f"{who}: rows must be a uint8 array [M, S]"
  assert raised(fn, pack, rows[:, :100]) == f"{who}: rows of 100 bytes, the pack's are {stride}"
  assert raised(fn, pack, rows, which=[]) == f"{who}: no rows to {verb}"
  # the order of the checks: the bank's form, its row length, the count
  assert raised(fn, pack, rows[:0, :100], which=[]) == f"{who}: rows must be a uint8 array [M, S]"
  assert raised(fn, pack, rows[:, :100], which=[]) == f"{who}: rows of 100 bytes, the pack's are {stride}"


def test_hash_states_host_out_text(pack, stride):
  rows = np.zeros((3, stride), np.uint8)
  for out in (np.zeros(2, np.int64), np.zeros(3, np.int32), np.zeros(6, np.int64)[::2], [0, 0, 0]):
    assert raised(E.hash_states_host, pack, rows, out=out) == \
        "hash_states_host: out must be a contiguous int64 array of shape (3,)"
  assert raised(E.hash_states_host, pack, rows, which=[0, 1], out=np.zeros(3, np.int64)) == \
      "hash_states_host: out must be a contiguous int64 array of shape (2,)"


@pytest.mark.parametrize("who,verb", [("ego_layer_host", "draw"), ("hash_views_host", "hash"),
                                      ("ego_planes_host", "draw")])
def test_host_view_source_texts(pack, stride, who, verb):
  fn = getattr(E, who)
  args = (np.zeros(E.num_layer_ids_host(pack), np.int32),) if who == "ego_planes_host" else ()
  rows = np.zeros((3, stride), np.uint8)
  assert raised(fn, pack, rows[0], *args) == f"{who}: rows must be a uint8 array [M, S]"
  assert raised(fn, pack, rows[:0], *args) == f"{who}: rows must be a uint8 array [M, S]"
  assert raised(fn, pack, rows[:, :100], *args) == f"{who}: rows of 100 bytes, the pack's are {stride}"
  assert raised(fn, pack, rows, *args, which=[]) == f"{who}: no rows to {verb}"
  assert raised(fn, pack, rows, *args, players=[]) == f"{who}: no rows to {verb}"
  assert raised(fn, pack, rows, *args, players=[0, 1], which=[0, 1, 2]) == f"{who}: which has 3 entries, players 2"
  assert raised(fn, pack, rows[:, :100], *args, players=[0, 1], which=[0]) == \
      f"{who}: rows of 100 bytes, the pack's are {stride}"
