"""Times step_many with stop conditions (profiles/r22_step_until.md) on one GPU, every figure
against the masked step_many of the same K in the same run.

    python tools/time_step_until.py [--packs clean_up] [--worlds 4096] [--steps 1,64] [--calls 128]
                                    [--rounds 7]

Scalars only (no view bound; step_many's default four per-step kinds).  Per pack and K, one JSON
line with median [min, max] µs a REQUEST over the rounds, measured as tools/time_step_active.py
measures (events on the engine's stream, every timed window enqueued behind a blocker so that the
events see device time; `device_bound` says whether the host kept up; one warm-up window per
variant, the variants alternated over the rounds, each on an engine of its own).  Variants:
  active   (a) step_many(A, active=1): the k_many_active_* kernels, which this feature leaves as
           they were;
  sums     (b) the new family with nothing to stop on: stopped= and returns= asked for, until=None;
  last     (c) until="last";
  reward   (d) until="reward": the reward is loaded back and waited for in every step;
  loop     (e) the host loop this replaces: K calls of step(A[k], active=~done), `done` updated
           from STEP_TYPE and read back once per step (the per-step synchronisation).  Wall-clock
           µs for the K steps, not device time: the loop's cost IS the host's.
The figures are to say what the CHECKS cost, not what a shortened rollout saves, so nothing may stay
stopped: the pack's episode length is set beyond the run (no world reaches LAST), and where a
request is long enough to hide it (K >= 16) `stopped` is cleared in front of every request — by
every variant, (a) included, which clears a tensor nobody reads, so that the differences do not
contain the 2 µs fill.  At K = 1 it is cleared between the windows only.  Random play is paid now
and then, so in (d) some worlds still stop inside a request; `stopped_worlds` is how many had when
the last request ended.
`per_step_us`: (b) - (a) and (d) - (c), medians, over K."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from meltingpot_amd import engine, lower  # noqa: E402
from meltingpot_amd import pack as pack_lib  # noqa: E402
from time_step_active import Blocker, timed  # noqa: E402

VARIANTS = {"active": {}, "sums": dict(returns=True), "last": dict(until="last", returns=True),
            "reward": dict(until="reward", returns=True)}


def host_loop(e, A, done):
  """The README's closed loop with a stop on LAST: one synchronisation a step."""
  done.zero_()
  for k in range(A.shape[0]):
    e.step(A[k], active=~done)
    done |= e.observe(engine.OBS_STEP_TYPE) == 2
    if bool(done.all()):
      break


def one_case(name, K, args, blocker):
  n = args.worlds
  calls = max(16, args.calls * 4 // max(4, K))
  tables = pack_lib.loads(engine.load_pack(name))
  tables["hdr"][lower.HDR_MAXFRAMES] = 1 << 24   # (no episode ends inside the run)
  pack = pack_lib.dumps(tables)
  rng = np.random.default_rng(0)
  probe = engine.Engine(pack, 1, device=0)
  nact, P = probe.num_actions, probe.P
  probe.close()
  A = torch.from_numpy(rng.integers(0, nact, (K, n, P), dtype=np.int32)).cuda()
  ones = torch.ones(n, dtype=torch.uint8, device=A.device)
  engines, outs, kws, clear = {}, {}, {}, {}
  for how, kw in VARIANTS.items():
    e = engine.Engine(pack, n, device=0)
    e.reset()
    kw = dict(kw, active=ones)
    clear[how] = torch.zeros(n, dtype=torch.uint8, device=A.device)
    if how != "active":
      kw["stopped"] = clear[how]
    out = e.step_many(A, **kw)
    if "returns" in out:
      kw["returns"] = out["returns"]
    engines[how], outs[how], kws[how] = e, out, kw
  times = {how: [] for how in VARIANTS}
  enqueue_ms = 0.0
  for _ in range(args.rounds):   # alternated over the rounds
    for how in VARIANTS:
      e, kw, mine = engines[how], kws[how], clear[how]
      mine.zero_()

      def request():
        if K >= 16:
          mine.zero_()
        e.step_many(A, out=outs[how], **kw)

      us, host_ms = timed(request, calls, blocker)
      times[how].append(us)
      enqueue_ms = max(enqueue_ms, host_ms)
  stopped_worlds = {how: int((kws[how]["stopped"] != 0).sum()) for how in VARIANTS if "stopped" in kws[how]}
  for e in engines.values():
    e.sync()
    assert not e.fault_words()[:40].any()
    e.close()
  # (e) the host loop, wall-clock
  e = engine.Engine(pack, n, device=0)
  e.reset()
  done = torch.zeros(n, dtype=torch.bool, device=A.device)
  loop_calls = max(4, calls // 8)
  loop = []
  for r in range(args.rounds + 1):   # (the first round warms up)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(loop_calls):
      host_loop(e, A, done)
    torch.cuda.synchronize()
    if r:
      loop.append((time.perf_counter() - t0) * 1e6 / loop_calls)
  assert not e.fault_words()[:40].any()
  e.close()
  times["loop"] = loop
  res = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
  return {"pack": name, "worlds": n, "K": K, "calls": calls, "device": torch.cuda.get_device_name(0),
          "blocker_ms": round(blocker.ms, 1), "enqueue_ms": round(enqueue_ms, 1),
          "device_bound": bool(enqueue_ms < blocker.ms), "us_per_request": res,
          "per_step_us": {"sums_minus_active": round((res["sums"][0] - res["active"][0]) / K, 3),
                          "reward_minus_last": round((res["reward"][0] - res["last"][0]) / K, 3)},
          "ratio_to_active": {k: round(v[0] / res["active"][0], 3) for k, v in res.items()},
          "stopped_worlds": stopped_worlds}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--packs", default="clean_up")
  ap.add_argument("--worlds", type=int, default=4096)
  ap.add_argument("--steps", default="1,64")
  ap.add_argument("--calls", type=int, default=128)
  ap.add_argument("--fills", type=int, default=60, help="2 GiB fills of the blocker in front of a window")
  ap.add_argument("--rounds", type=int, default=7)
  args = ap.parse_args()
  blocker = Blocker(args.fills)
  for name in args.packs.split(","):
    for K in (int(k) for k in args.steps.split(",")):
      print(json.dumps(one_case(name, K, args, blocker)), flush=True)


if __name__ == "__main__":
  main()
