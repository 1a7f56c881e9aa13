"""CPU-side checks of the drop-in boundary: libmp_engine.so builds (hipcc
cross-compiles gfx950 without a GPU), loads, exports every symbol that
include/mp_engine.h declares, and fails loudly — no CPU fallback — when asked
to compute without a device."""
import ctypes

import numpy as np
import os
import re
import subprocess

import pytest

from meltingpot_amd import _build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
  text = open(os.path.join(ROOT, "include", "mp_engine.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return sorted(set(re.findall(r"\b(mp_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
  assert _declared_symbols() == sorted(engine.ABI_SYMBOLS)


def test_library_builds_loads_and_exports_every_declared_symbol():
  L = engine.load_library()
  for name in _declared_symbols():
    assert hasattr(L, name), f"{name} declared in mp_engine.h but not exported"
  assert L.mp_abi_version() == engine.MP_ABI_VERSION == 8


def test_library_exports_exactly_the_declared_symbols():
  """A C-ABI boundary exports its ABI and nothing else: the library is compiled with
  -fvisibility=hidden and linked against csrc/exports.map, so `nm -D` shows the header's
  mp_* entry points only (no launch_frame, plan_frame, timed_launches_us ...)."""
  path = _build.build_engine()
  out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                       check=True).stdout
  exported = sorted(line.split()[-1] for line in out.splitlines()
                    if line.split() and line.split()[-2] in ("T", "D", "B", "R"))
  assert exported == _declared_symbols()


def test_library_contains_gfx950_code_object():
  path = _build.build_engine()
  out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", path],
                       capture_output=True, text=True).stdout
  assert "gfx950" in out
  # the three hot kernels are in the fat binary
  blob = open(path, "rb").read()
  for kernel in (b"k_step_clean_up", b"k_step_commons", b"k_step_territory", b"k_frame"):
    assert kernel in blob


def test_no_cpu_fallback(clean_up_pack):
  import torch
  if torch.cuda.is_available():
    pytest.skip("a GPU is present")
  with pytest.raises(engine.EngineError, match="no HIP device"):
    engine.Engine(clean_up_pack, 2)


def test_bad_arguments_are_rejected_before_touching_a_device(clean_up_pack):
  L = engine.load_library()
  cfg = engine.MpConfig(ctypes.sizeof(engine.MpConfig), 0, 0, 1, 0, 0, None)
  h = ctypes.c_void_p()
  buf = ctypes.create_string_buffer(clean_up_pack, len(clean_up_pack))
  assert L.mp_create(buf, len(clean_up_pack), ctypes.byref(cfg), ctypes.byref(h)) == -1
  assert b"num_worlds" in L.mp_last_error()
  cfg.num_worlds = 4
  junk = ctypes.create_string_buffer(b"not a pack" * 10, 100)
  assert L.mp_create(junk, 100, ctypes.byref(cfg), ctypes.byref(h)) == -2
  cfg.struct_size = 3
  assert L.mp_create(buf, len(clean_up_pack), ctypes.byref(cfg), ctypes.byref(h)) == -1


def test_product_never_imports_the_oracle():
  """oracle/ is test infrastructure: nothing under meltingpot_amd/ may touch it."""
  pkg = os.path.join(ROOT, "meltingpot_amd")
  for dirpath, _, files in os.walk(pkg):
    for f in files:
      if f.endswith((".py", ".hip", ".h")):
        src = open(os.path.join(dirpath, f)).read()
        assert "import oracle" not in src and "from oracle" not in src, f
        assert "liboracle" not in src, f


def _create_rc(blob, num_players=0, roles=None):
  L = engine.load_library()
  cfg = engine.MpConfig(ctypes.sizeof(engine.MpConfig), 0, 2, 1, 0, 0, None, num_players, 0, 0, 0)
  if roles is not None:
    cfg.roles = (ctypes.c_int32 * len(roles))(*roles)
  h = ctypes.c_void_p()
  buf = ctypes.create_string_buffer(bytes(blob), len(blob))
  rc = L.mp_create(buf, len(blob), ctypes.byref(cfg), ctypes.byref(h))
  return rc, L.mp_last_error().decode()


def _variant(t, **kw):
  """mp_create's verdict on the pack tables `t` with each named table edited by its function."""
  from meltingpot_amd import pack
  bad = dict(t)
  for k, fn in kw.items():
    v = t[k].copy(); fn(v); bad[k] = v
  return _create_rc(pack.dumps(bad))


def _set(index, value):
  return lambda v: v.__setitem__(index, value)


def test_malformed_packs_are_refused_before_a_device_is_touched(clean_up_pack, territory_pack):
  """mp_create takes arbitrary bytes: truncated blobs, overflowing counts, missing
  or mistyped tables and out-of-range indices must come back as MP_ERR_PACK (-2),
  never as a crash.  (Without a GPU a well-formed pack gets as far as
  MP_ERR_NO_DEVICE, -3: everything below is checked on the host first, rule constants
  included.)"""
  import struct
  import torch
  from meltingpot_amd import lower, pack
  good = -3 if not torch.cuda.is_available() else 0
  rc, _ = _create_rc(clean_up_pack)
  assert rc == good
  # truncation, bad magic
  assert _create_rc(clean_up_pack[:-16])[0] == -2
  assert _create_rc(b"XPK1" + clean_up_pack[4:])[0] == -2
  # an entry whose count * size overflows 64 bits / whose offset leaves the blob
  hdr_size, entry_size = 16, 64
  blob = bytearray(clean_up_pack)
  struct.pack_into("<Q", blob, hdr_size + 40, 0xFFFFFFFFFFFFFFF0)   # entry 0: count
  assert _create_rc(blob)[0] == -2
  blob = bytearray(clean_up_pack)
  struct.pack_into("<Q", blob, hdr_size + 48, len(blob) + 16)       # entry 0: offset
  assert _create_rc(blob)[0] == -2
  blob = bytearray(clean_up_pack)
  struct.pack_into("<Q", blob, hdr_size + 48, 8)                    # inside the entry table
  assert _create_rc(blob)[0] == -2
  # missing / mistyped / short tables, indices out of range
  t = pack.loads(clean_up_pack)
  for name in ("state_layer", "apple_cells", "view_sprite_map", "init_spawn_mask", "cu_states"):
    bad = {k: v for k, v in t.items() if k != name}
    rc, msg = _create_rc(pack.dumps(bad))
    assert rc == -2, (name, rc, msg)
  bad = dict(t); bad["state_layer"] = t["state_layer"].astype(np.float64)
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["init_grid"] = t["init_grid"][:-5]
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["apple_cells"] = t["apple_cells"].copy(); bad["apple_cells"][3] = 21 * 30
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["spawn_cells"] = t["spawn_cells"].copy(); bad["spawn_cells"][0] = -1
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["init_grid"] = t["init_grid"].copy(); bad["init_grid"][7] = 250
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["cu_i32"] = t["cu_i32"].copy(); bad["cu_i32"][5] = 0     # ee_interval: % 0
  rc, msg = _create_rc(pack.dumps(bad))
  assert rc == -2 and "clean_up constants out of engine range" in msg, msg
  bad = dict(t); bad["hdr"] = t["hdr"].copy(); bad["hdr"][lower.HDR_NHITS] = 30
  assert _create_rc(pack.dumps(bad))[0] == -2
  # player counts
  assert _create_rc(clean_up_pack, num_players=16)[0] == -1
  assert _create_rc(clean_up_pack, num_players=15)[0] == good
  t3 = pack.loads(territory_pack)
  bad = dict(t3); bad["resource_cells"] = t3["resource_cells"].copy(); bad["resource_cells"][0] = 10**6
  rc, msg = _create_rc(pack.dumps(bad))
  assert rc == -2 and "table 'resource_cells' is missing, too long or leaves the map" in msg, msg


def test_malformed_matrix_packs_are_refused():
  """The *_in_the_matrix tables: lengths follow from R and the colour intervals,
  classes and states are range-checked, all on the host."""
  import torch
  from meltingpot_amd import engine, pack
  good = -3 if not torch.cuda.is_available() else 0
  blob = engine.load_pack("running_with_scissors_in_the_matrix__arena")
  assert _create_rc(blob)[0] == good
  t = pack.loads(blob)
  for name in ("mx_i32", "mx_f64", "mx_states", "mx_thr", "mx_player_i32", "mx_player_f64",
               "resource_class", "resource_cells"):
    bad = {k: v for k, v in t.items() if k != name}
    rc, msg = _create_rc(pack.dumps(bad))
    assert rc == -2, (name, rc, msg)
  def variant(**kw):
    return _variant(t, **kw)[0]
  assert variant(mx_i32=lambda v: v.__setitem__(0, 4)) == -2       # R > 3
  assert variant(mx_i32=lambda v: v.__setitem__(0, 2)) == -2       # R that the tables do not fit
  assert variant(mx_i32=lambda v: v.__setitem__(16, 0)) == -2      # intervalLength 0: % 0
  assert variant(mx_i32=lambda v: v.__setitem__(18, 7)) == -2      # initialHealth > 3 (2 bits)
  assert variant(mx_i32=lambda v: v.__setitem__(21, 9)) == -2      # hit index
  assert variant(resource_class=lambda v: v.__setitem__(5, 4)) == -2
  assert variant(resource_cells=lambda v: v.__setitem__(0, 24 * 25)) == -2
  assert variant(mx_states=lambda v: v.__setitem__(3, 255)) == -2
  bad = dict(t); bad["mx_f64"] = t["mx_f64"][:-1]
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["resource_class"] = t["resource_class"][:-1]
  assert _create_rc(pack.dumps(bad))[0] == -2


def test_malformed_mushroom_packs_are_refused():
  """externality_mushrooms: tables missing, short or leaving the map are refused on the host
  (its rule constants: test_mushroom_rule_constants_out_of_engine_range_are_refused)."""
  import torch
  from meltingpot_amd import engine, pack
  good = -3 if not torch.cuda.is_available() else 0
  blob = engine.load_pack("externality_mushrooms__dense")
  assert _create_rc(blob)[0] == good
  t = pack.loads(blob)
  for name in ("em_states", "em_i32", "em_f64", "em_thr", "mushroom_cells", "zapper_i32"):
    bad = {k: v for k, v in t.items() if k != name}
    rc, msg = _create_rc(pack.dumps(bad))
    assert rc == -2, (name, rc, msg)
  for name, keep in (("em_i32", 29), ("em_thr", 20), ("em_states", 7)):
    bad = dict(t); bad[name] = t[name][:keep]
    assert _create_rc(pack.dumps(bad))[0] == -2, name
  bad = dict(t); bad["mushroom_cells"] = t["mushroom_cells"].copy(); bad["mushroom_cells"][7] = 14 * 23
  assert _create_rc(pack.dumps(bad))[0] == -2
  bad = dict(t); bad["mushroom_cells"] = np.concatenate([t["mushroom_cells"]] * 2)   # 462 sites: four a lane
  assert _create_rc(pack.dumps(bad))[0] == -2



@pytest.mark.parametrize("name, table, index, value, message", [
    ("commons_harvest__open", "ch_i32", 0, 33, "commons_harvest constants"),   # 33 regrowth classes
    ("territory__open", "tr_i32", 7, 3, "territory constants"),                # three health levels
    ("coop_mining", "cm_i32", 6, 2, "coop_mining constants"),                  # a third ore type
    ("collaborative_cooking__ring", "cc_i32", 1, 31, "collaborative_cooking constants"),  # cooking time
    ("gift_refinements", "gr_i32", 6, 16, "gift_refinements constants"),       # capacity beyond 4 bits
    ("externality_mushrooms__dense", "em_i32", 1, 2, "externality_mushrooms constants"),  # health 2
])
def test_rule_constants_out_of_engine_range_are_refused_on_the_host(name, table, index, value, message):
  """A substrate's rule constants are checked before a device is touched (MP_ERR_PACK, not
  MP_ERR_NO_DEVICE, on a machine without one)."""
  from meltingpot_amd import pack
  rc, msg = _variant(pack.loads(engine.load_pack(name)), **{table: _set(index, value)})
  assert rc == -2 and message in msg, msg


def test_player_counts_and_roles_a_pack_cannot_run_are_refused_on_the_host():
  rc, msg = _create_rc(engine.load_pack("coins"), num_players=1)
  assert rc == -2 and "coins tables missing or out of engine range" in msg, msg
  blob = engine.load_pack("bach_or_stravinsky_in_the_matrix__arena")
  roles = [0] * 16   # (MP_MAX_PLAYERS)
  roles[1] = 99
  rc, msg = _create_rc(blob, roles=roles)
  assert rc == -1 and "role 99 of player 2 is outside" in msg, msg


def test_colour_intervals_with_a_gap_are_refused():
  """TheMatrix:getColorInterval asserts (components.lua:282-290): a pack whose intervals
  leave a gap inside the payable range is refused by mp_create (what it reports at run
  time: tests/test_gpu_matrix.py)."""
  from meltingpot_amd import pack
  t = pack.loads(engine.load_pack("prisoners_dilemma_in_the_matrix__repeated"))
  R, NI = int(t["mx_i32"][0]), int(t["mx_i32"][19])
  def gap(f):
    iv = f[5 + 2 * R * R:5 + 2 * R * R + 2 * NI].reshape(NI, 2)
    iv[1] = (1.5, 2.0)                                 # nothing holds [1.0, 1.5)
  rc, msg = _variant(t, mx_f64=gap)
  assert rc == -2 and "resultIndicatorColorIntervals" in msg, msg


def test_mushroom_rule_constants_out_of_engine_range_are_refused():
  """What step_mushroom.h builds on is checked at mp_create: a zap destroys a mushroom
  (health 1), two sanction levels, consecutive mushroom states, delays that fit the age
  plane, a Zapper that pays nothing and leaves removal to the marking."""
  import torch
  from meltingpot_amd import pack
  good = -3 if not torch.cuda.is_available() else 0
  blob = engine.load_pack("externality_mushrooms__dense")
  t = pack.loads(blob)
  def refused(**kw):
    rc, msg = _variant(t, **kw)
    assert rc == -2 and re.search("externality_mushrooms|Zapper", msg), (kw, rc, msg)
  refused(em_i32=_set(1, 2))           # initialHealth 2
  refused(em_i32=_set(3, 3))           # three levels
  refused(em_i32=_set(5, 0))           # intervalLength 0
  refused(em_i32=_set(16, 300))        # a delay the age byte cannot count
  refused(em_i32=_set(8, 9))           # nine spores
  refused(em_i32=_set(20, 4))          # typeToDestroy out of range
  refused(em_i32=_set(25, 300))        # a freeze beyond a byte
  refused(em_states=lambda v: v.__setitem__(1, int(v[0]) + 2))   # types not consecutive
  refused(zapper_i32=_set(4, 1))       # Zapper removes
  refused(zapper_f64=_set(0, -1.0))    # Zapper pays
  assert _create_rc(blob)[0] == good
