"""Builds libmp_engine.so (hand-written HIP for gfx950) in-tree with hipcc.

The shared library is the product's only compute path; there is no fallback.
`hipcc` cross-compiles without a GPU, so this runs in the CPU container too.
"""

from __future__ import annotations

import concurrent.futures
import fcntl
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libmp_engine.so")
# The units, the slowest to compile first (the frame kernels take most of a build's time, and at
# most MAX_JOBS compilers run at once).
# The engine's host side is six units that share engine_state.h: mp_engine.hip (the engine object,
# its life cycle, the submission path and the deferred fault reports), engine_atlas.hip (the sprite
# atlas, host only), engine_requests.hip (what mp_snapshot / mp_restore carry, and the two
# carriers), engine_views.hip (the four requests about every viewer's window), engine_outputs.hip
# (mapped views: mp_alloc_output and its kin, which need no engine) and mp_place.hip (the tuner,
# mp_place_output, mp_box_fill and their two kernels).
# The kernels' units: frame_wpool<k>.hip: the WORLD.RGB-pooled frame kernels, one unit per factor so
# that they compile in parallel with frame.hip; frame_stock.hip: the kernels with a committed
# pack's constants compiled in, likewise; state_check.hip: the record check, which includes no step
# header; state_hash.hip: the record hash, likewise; step_starts.hip: the single-step kernels with
# registered episode starts, a unit of its own so that step_kernels.hip's are what they were;
# state_view.hip: the renderer of one (row, player) view, likewise; step_active.hip and
# step_until.hip: the K-step kernels under a device mask and with stop conditions, and
# step_listed.hip: the K-step kernels of a world list, one unit each so that every unit has one
# caller of each level's step; all three instantiate the one body of step_masked.h;
# episode_stats.hip: the launch behind every submission of an engine with registered episode
# statistics, which includes no step header; ego_layer.hip: the EGO_LAYER draw and the launch
# behind every submission of an engine with the leaf registered; view_hash.hip: the hash of every
# player's view, likewise a draw and a launch behind every submission; ego_planes.hip: the class
# and facing planes of every player's view, likewise; avatar_ids.hip: whom every player sees and
# could zap, likewise; world_view.hip: WORLD.LAYER and the world planes, the whole map in place of the
# viewers' windows, likewise; these five take what they share — the staged record, the launch plan, the
# host twin's loop — from view_unit.h.  The six step units take the nine levels from step_levels.h
# and the K-step ones their row helpers from step_rows.h.
SOURCES = ("frame.hip", "frame_wpool2.hip", "frame_wpool4.hip", "frame_wpool8.hip", "frame_stock.hip",
           "step_many.hip", "step_active.hip", "step_until.hip", "step_listed.hip", "step_kernels.hip",
           "step_starts.hip", "state_obs.hip", "state_view.hip", "state_check.hip", "state_hash.hip",
           "episode_stats.hip", "ego_layer.hip", "view_hash.hip", "ego_planes.hip", "avatar_ids.hip", "world_view.hip",
           "mp_engine.hip", "engine_atlas.hip", "engine_requests.hip", "engine_views.hip", "engine_outputs.hip",
           "mp_place.hip", "pack_decode.hip")
HEADERS = ("mp_common.h", "engine_state.h", "stock.h", "stock_clean_up.h", "pack_decode.h", "frame_kernel.h", "frame_wpool.h", "step_common.h", "step_clean_up.h", "step_commons.h",
           "step_territory.h", "step_coins.h", "step_matrix.h", "step_coop.h", "step_gift.h", "step_cook.h", "step_mushroom.h", "step_load.h", "step_one.h", "step_levels.h", "step_rows.h", "step_masked.h", "step_many.h", "step_until.h", "step_listed.h", "state_obs.h", "state_obs_rules.h", "state_view.h", "state_check.h", "state_hash.h", "episode_stats.h", "ego_layer.h", "view_hash.h", "ego_planes.h", "avatar_ids.h", "view_unit.h", "world_view.h", "../../include/mp_engine.h",
           "../../include/mp_pack.h", "exports.map")
ARCH = "gfx950"


def _stale() -> bool:
  if not os.path.exists(LIB_PATH):
    return True
  built = os.path.getmtime(LIB_PATH)
  for f in SOURCES + HEADERS:
    if os.path.getmtime(os.path.join(CSRC, f)) > built:
      return True
  return False


def build_engine(force: bool = False, verbose: bool = False) -> str:
  """Compiles the engine if missing or stale; returns the library path."""
  if not force and not _stale():
    return LIB_PATH
  hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  if not os.path.exists(hipcc):
    raise RuntimeError("hipcc not found: cannot build libmp_engine.so")
  os.makedirs(LIB_DIR, exist_ok=True)
  # One builder at a time (N ranks of `bench.py --gpus N` import this together),
  # and readers never see a half-written library: compile aside, then rename.
  with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
    fcntl.flock(lock, fcntl.LOCK_EX)
    if not force and not _stale():  # another process built it while we waited
      return LIB_PATH
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    # one object per source (kept under lib/obj: a change to mp_engine.hip does not
    # recompile the frame kernel's 40 s), then one link
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    newest_header = max(os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS)
    objects, todo = [], []
    for src in SOURCES:
      path = os.path.join(CSRC, src)
      obj = os.path.join(obj_dir, os.path.splitext(src)[0] + ".o")
      objects.append(obj)
      if (force or not os.path.exists(obj) or
          os.path.getmtime(obj) < max(os.path.getmtime(path), newest_header)):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC",
               "-fvisibility=hidden", "-c", "-o", obj + f".{os.getpid()}.tmp", path]
        todo.append((obj, cmd))
    # at most MAX_JOBS compilers at a time, started in SOURCES' order as earlier ones end
    limit = max(1, int(os.environ.get("MAX_JOBS", 16)))

    def compile_one(job):
      if verbose:
        print(" ".join(job[1]))
      return subprocess.run(job[1]).returncode

    with concurrent.futures.ThreadPoolExecutor(max_workers=limit) as pool:
      codes = list(pool.map(compile_one, todo))
    failed = [obj for (obj, _), rc in zip(todo, codes) if rc != 0]
    for obj, _ in todo:
      part = obj + f".{os.getpid()}.tmp"
      if obj not in failed and os.path.exists(part):
        os.replace(part, obj)
      elif os.path.exists(part):
        os.remove(part)
    if failed:
      raise RuntimeError(f"hipcc failed on {[os.path.basename(o) for o in failed]}")
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC",
           f"-Wl,--version-script={os.path.join(CSRC, 'exports.map')}", "-o", tmp] + objects
    if verbose:
      print(" ".join(cmd).replace(tmp, LIB_PATH))
    try:
      subprocess.run(cmd, check=True)
      os.replace(tmp, LIB_PATH)
    finally:
      # (this hipcc leaves its offload-bundle intermediates next to the output)
      for name in os.listdir(LIB_DIR):
        if name.startswith(os.path.basename(tmp)) or ".hipv4-" in name or ".host-x86_64-" in name:
          os.remove(os.path.join(LIB_DIR, name))
  return LIB_PATH
