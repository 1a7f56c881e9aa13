"""The rule of the episode statistics (include/mp_engine.h: MpEpisodeStats) in numpy, written from
the issue's text and from nothing of the library's: fed per-step host copies of step_type, reward,
the raw event rows and the mask of the steps that ran.  Columns are given by NAME and decoded here
from the documented payload packing, not by the product's parser."""
import numpy as np

EVENT_ROWS = 128
# event name -> (MpEventType, {key: (payload 0 a / 1 b, shift, mask)})
FULL = 0xFFFFFFFF
EVENTS = {
    "zap": (1, {"source": (0, 0, FULL), "target": (1, 0, FULL)}),
    "edible_consumed": (2, {"player_index": (0, 0, FULL)}),
    "player_cleaned": (3, {"player_index": (0, 0, FULL)}),
    "claimed_resource": (4, {"player_index": (0, 0, FULL)}),
    "destroyed_resource": (5, {"player_index": (0, 0, FULL), "class": (1, 0, FULL)}),
    "sanctioning": (6, {"source": (0, 0, FULL), "target": (1, 0, FULL)}),
    "removal_due_to_sanctioning": (7, {"source": (0, 0, FULL), "target": (1, 0, FULL)}),
    "set_sanctioning_level": (8, {"player_index": (0, 0, FULL), "level": (1, 0, FULL)}),
    "coin_consumed": (10, {"player_index": (0, 0, FULL), "player_coin_type": (1, 1, FULL >> 1),
                           "coin_type": (1, 0, 1)}),
    "interaction": (11, {"row_player_idx": (0, 0, FULL), "col_player_idx": (1, 0, FULL)}),
    "collected_resource": (12, {"player_index": (0, 0, FULL), "class": (1, 0, FULL)}),
    "mining": (13, {"player": (0, 0, FULL), "ore_type": (1, 0, FULL)}),
    "extraction": (14, {"player": (0, 0, FULL), "ore_type": (1, 0, FULL)}),
    "extraction_pair": (15, {"player_a": (0, 0, FULL), "player_b": (1, 2, FULL >> 2), "ore_type": (1, 0, 3)}),
    "gift": (16, {"gifter_index": (0, 0, 15), "source_type": (0, 4, FULL >> 4), "receipient_index": (1, 0, 15),
                  "received_amount": (1, 4, FULL >> 4)}),
    "receiver_accepted_item": (17, {"player_index": (0, 0, FULL), "item": (1, 0, FULL)}),
    "item_dropped_into_pot": (18, {"player_index": (0, 0, FULL), "item": (1, 0, FULL)}),
    "cooked_food_collected_from_pot": (19, {"player_index": (0, 0, FULL), "cooked_item": (1, 0, FULL)}),
    "eating_mushroom": (20, {"player_index": (0, 0, FULL), "mushroom_type": (1, 0, FULL)}),
}


def decode(name):
  """"event.key", "event.key>other", each optionally "[key=value]" -> a dict."""
  test = None
  if name.endswith("]"):
    name, rest = name[:-1].split("[")
    key, value = rest.split("=")
    test = (key, int(value))
  event, key = name.split(".")
  other = None
  if ">" in key:
    key, other = key.split(">")
  type_, fields = EVENTS[event]
  return {"type": type_, "player": fields[key], "other": None if other is None else fields[other],
          "test": None if test is None else (fields[test[0]], test[1])}


def _field(row, where):
  payload, shift, mask = where
  return ((int(row[1 + payload]) & FULL) >> shift) & mask


def tally(rows, columns, pairs, P):
  """Event rows int32 [EVENT_ROWS, 4] of one world-step -> (counts [C, P], pairs [C2, P, P])."""
  counts = np.zeros((len(columns), P), np.int64)
  pair_counts = np.zeros((len(pairs), P, P), np.int64)
  n = min(max(int(rows[0, 0]), 0), EVENT_ROWS - 1)
  for row in rows[1:1 + n]:
    for c, name in enumerate(list(columns) + list(pairs)):
      d = decode(name)
      if int(row[0]) != d["type"]:
        continue
      if d["test"] is not None and _field(row, d["test"][0]) != d["test"][1]:
        continue
      p = _field(row, d["player"])
      if not 1 <= p <= P:
        continue
      if d["other"] is None:
        counts[c, p - 1] += 1
      else:
        q = _field(row, d["other"])
        if 1 <= q <= P:
          pair_counts[c - len(columns), p - 1, q - 1] += 1
  return counts, pair_counts


class Model:
  """The statistics of n worlds of P players."""

  def __init__(self, n, P, columns=(), pairs=()):
    self.n, self.P, self.columns, self.pairs = n, P, tuple(columns), tuple(pairs)
    C, C2 = len(self.columns), len(self.pairs)
    self.open = np.zeros(n, np.uint8)
    self.episodes = np.zeros(n, np.int32)
    self.dropped = np.zeros(n, np.int32)
    bank = lambda ints: {"returns": np.zeros((n, P), np.float64), "length": np.zeros(n, ints),
                         "counts": np.zeros((n, C, P), ints), "pairs": np.zeros((n, C2, P, P), ints)}
    self.running, self.last, self.total = bank(np.int32), bank(np.int32), bank(np.int64)

  def step(self, step_type, reward, events, ran=None):
    """One step: step_type [n], reward [n, P], events [n, EVENT_ROWS, 4] (None with no columns);
    ran: bool [n], the worlds whose step ran (None: all)."""
    for w in range(self.n):
      if ran is not None and not ran[w]:
        continue
      E = None if events is None else np.asarray(events[w])
      if E is not None:
        self.dropped[w] += int(E[0, 1])
      counts, pairs = tally(E, self.columns, self.pairs, self.P) if E is not None else (0, 0)
      st = int(step_type[w])
      run = self.running
      if st == 0:
        for key in run:
          run[key][w] = 0
        self.open[w] = 1
        run["counts"][w] += counts
        run["pairs"][w] += pairs
      elif self.open[w]:
        run["returns"][w] = run["returns"][w] + np.asarray(reward[w], np.float64)
        run["length"][w] += 1
        run["counts"][w] += counts
        run["pairs"][w] += pairs
        if st == 2:
          for key in run:
            self.last[key][w] = run[key][w]
            self.total[key][w] = self.total[key][w] + run[key][w]
          self.episodes[w] += 1
          self.open[w] = 0

  def arrays(self):
    return {"open": self.open, "episodes": self.episodes, "dropped": self.dropped, "running": self.running,
            "last": self.last, "total": self.total}


def flatten(arrays):
  """{name: numpy array} of a statistics dict (numpy arrays or torch tensors)."""
  out = {}
  for key, value in arrays.items():
    for sub, a in (value.items() if isinstance(value, dict) else [(None, value)]):
      out[key if sub is None else f"{key}.{sub}"] = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
  return out


def assert_equal(got, want, what=""):
  """Bitwise: every tensor of two statistics dicts."""
  got, want = flatten(got), flatten(want)
  assert got.keys() == want.keys()
  for key in want:
    assert got[key].dtype == want[key].dtype, (what, key, got[key].dtype, want[key].dtype)
    assert got[key].tobytes() == want[key].tobytes(), (what, key, got[key], want[key])
