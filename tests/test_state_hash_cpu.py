"""The state hash without a GPU (MpStatesHash: MP_HASH_HOST and MP_HASH_MASK, the kernel's own
function compiled for the host).  The byte mask is rebuilt here in numpy from nothing but
`engine.state_layout` and the rules include/mp_engine.h states, the function is restated in numpy
u64 arithmetic, and both are held against the library on rows of random bytes (the hash does not
need well-formed rows); flipping every byte of a row in turn changes the hash exactly where the
mask is set.  (Rows an engine saved are hashed where an engine runs: tests/test_gpu_state_hash.py.)"""
import ctypes
import functools

import numpy as np
import pytest

from meltingpot_amd import engine as E

MATRIX_REPEATED = "prisoners_dilemma_in_the_matrix__repeated"
MATRIX_ARENA = "prisoners_dilemma_in_the_matrix__arena"
# (pack, num_players): the arena with 3 of its 8 players, so that the `< P` cut of the per-avatar
# fields differs from the pack's own player count
CASES = (("coins", 0), ("collaborative_cooking__cramped", 0), ("clean_up", 0), (MATRIX_REPEATED, 0),
         (MATRIX_ARENA, 3))
IDS = [f"{name}-P{p}" if p else name for name, p in CASES]
BOOKKEEPING = ("ctr", "reward_fx", "orders_step", "next_orders")
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def pack(name):
  return E.load_pack(name)


@functools.lru_cache(maxsize=None)
def layout(name, players):
  return E.state_layout(pack(name), num_players=players)


def numpy_mask(lay, planes=None, fields=None):
  """The byte mask of a spec from the layout alone, by the rules of include/mp_engine.h."""
  m = np.zeros(lay.world_stride, np.uint8)
  hw = lay.H * lay.W
  default = planes is None and fields is None
  for p in (range(lay.grid_planes) if default else (planes or ())):
    m[p * hw:(p + 1) * hw] = 0xFF
  names = [n for n in lay.fields if n not in BOOKKEEPING] if default else [f for f in (fields or ()) if f != "player_block"]
  if lay.player_block >= 0 and (default or "player_block" in (fields or ())):
    m[lay.player_block:lay.grid_bytes] = 0xFF
  for n in names:
    off, elem, count = lay.fields[n]
    if count == 16:   # a per-avatar array: the avatars that play
      count = lay.P
    m[lay.grid_pad + off:lay.grid_pad + off + elem * count] = 0xFF
  return m


def fmix64(h):
  """(numpy u64 arrays: arithmetic wraps at 2^64)"""
  h = h.copy()
  h ^= h >> np.uint64(33)
  h *= np.uint64(0xff51afd7ed558ccd)
  h ^= h >> np.uint64(33)
  h *= np.uint64(0xc4ceb9fe1a85ec53)
  h ^= h >> np.uint64(33)
  return h


def numpy_hash(rows, mask):
  """int64 [R]: H of uint8 rows [R, S] under a uint8 byte mask [S]."""
  with np.errstate(over="ignore"):
    w = np.ascontiguousarray(rows).view("<u4").astype(np.uint64)
    m = np.ascontiguousarray(mask).view("<u4").astype(np.uint64)
    j = np.arange(1, m.size + 1, dtype=np.uint64) << np.uint64(32)
    c = fmix64(j[None, :] | (w & m[None, :]))
    c[:, m == 0] = 0
    return fmix64(c.sum(axis=1, dtype=np.uint64)).view(np.int64)


def random_rows(lay, n, seed):
  return np.random.default_rng(seed).integers(0, 256, (n, lay.world_stride), dtype=np.uint8)


def test_request_size_and_ctypes_mirror():
  """The hash rows' kind is no observation kind.  (The request's size and mirror:
  tests/test_request_abi_cpu.py.)"""
  assert E.STEP_ROW_HASH not in E.STEP_ROW_KINDS and E.STEP_ROW_HASH != E.STEP_ROW_STATE


def test_numpy_fmix64_is_the_published_one():
  # MurmurHash3's 64-bit finalizer: fmix64(1), fmix64(2^64 - 1) by exact integer arithmetic
  def exact(h):
    h ^= h >> 33; h = h * 0xff51afd7ed558ccd & M64
    h ^= h >> 33; h = h * 0xc4ceb9fe1a85ec53 & M64
    return h ^ h >> 33
  with np.errstate(over="ignore"):
    got = fmix64(np.array([1, M64, 0, 0x0123456789abcdef], np.uint64))
  assert [int(v) for v in got] == [exact(1), exact(M64), 0, exact(0x0123456789abcdef)]


@pytest.mark.parametrize("name,players", CASES, ids=IDS)
def test_masks_equal_the_numpy_restatement(name, players):
  lay = layout(name, players)
  hw = lay.H * lay.W
  assert lay.world_stride % 16 == 0
  if players:
    assert lay.P == players
  mask = lambda **kw: E.state_hash_mask(pack(name), num_players=players, **kw)
  default = mask()
  assert default.dtype == np.uint8 and default.shape == (lay.world_stride,) and set(np.unique(default)) <= {0, 0xFF}
  assert np.array_equal(default, numpy_mask(lay))
  # what every spec leaves out: the gap in front of the level's block, the padding, what follows the tail
  block = lay.player_block if lay.player_block >= 0 else lay.grid_bytes
  assert not default[lay.grid_planes * hw:block].any() and not default[lay.grid_bytes:lay.grid_pad].any()
  assert not default[lay.grid_pad + lay.tail_bytes:].any()
  for f in BOOKKEEPING:
    off, elem, count = lay.fields[f]
    assert not default[lay.grid_pad + off:lay.grid_pad + off + elem * count].any(), f
  off = lay.fields["ax"][0]
  assert default[lay.grid_pad + off:lay.grid_pad + off + lay.P].all() and not default[lay.grid_pad + off + lay.P:lay.grid_pad + off + 16].any()
  planes = (0, lay.grid_planes - 1)
  assert np.array_equal(mask(planes=planes), numpy_mask(lay, planes=planes))
  fields = ("ax", "ay", "step", "seed") + (("player_block",) if lay.player_block >= 0 else ())
  assert np.array_equal(mask(fields=fields), numpy_mask(lay, fields=fields))
  assert np.array_equal(mask(planes=(1,), fields=("achange",)), numpy_mask(lay, planes=(1,), fields=("achange",)))
  # a single plane whose end is not word aligned
  odd = [p for p in range(lay.grid_planes) if ((p + 1) * hw) % 4]
  if hw % 4:
    assert odd
  for p in odd[:1]:
    one = mask(planes=(p,))
    assert np.array_equal(one, numpy_mask(lay, planes=(p,))) and int(one.sum()) == 0xFF * hw
    word = one[(p + 1) * hw // 4 * 4:][:4]
    assert word.any() and not word.all()   # the plane ends inside this word
  ctr = mask(fields=("ctr",))
  assert np.array_equal(ctr, numpy_mask(lay, fields=("ctr",))) and int(ctr.sum()) == 0xFF * 32
  orders = mask(fields=("next_orders",))   # a per-avatar field of two-byte elements
  assert int(orders.sum()) == 0xFF * 2 * lay.P


def test_the_layout_facts_the_masks_rest_on():
  facts = {("coins", 0): (289, 2432), ("collaborative_cooking__cramped", 0): (45, 896), ("clean_up", 0): (630, 6080),
           (MATRIX_REPEATED, 0): (345, 4416), (MATRIX_ARENA, 3): (600, 6912)}
  for (name, players), (hw, stride) in facts.items():
    lay = layout(name, players)
    assert (lay.H * lay.W, lay.world_stride) == (hw, stride), name
  assert layout("clean_up", 0).grid_bytes == 5670 and layout("clean_up", 0).grid_pad == 5680
  assert layout(MATRIX_REPEATED, 0).player_block == 3456 and layout(MATRIX_ARENA, 3).player_block == 6000
  cramped = layout("collaborative_cooking__cramped", 0)
  assert cramped.world_stride - cramped.grid_pad - cramped.tail_bytes == 32


@pytest.mark.parametrize("name,players", CASES, ids=IDS)
def test_hashes_equal_the_numpy_restatement(name, players):
  lay = layout(name, players)
  rows = random_rows(lay, 7, 11)
  host = lambda **kw: E.hash_states_host(pack(name), rows, num_players=players, **kw)
  got = host()
  assert got.dtype == np.int64 and got.shape == (7,) and len(set(got.tolist())) == 7
  assert np.array_equal(got, numpy_hash(rows, numpy_mask(lay)))
  which = [6, 0, 0, 3]
  assert np.array_equal(host(which=which), got[which])
  planes, fields = (lay.grid_planes - 1,), ("ax", "ay", "ctr")
  assert np.array_equal(host(planes=planes, fields=fields), numpy_hash(rows, numpy_mask(lay, planes, fields)))
  assert np.array_equal(host(planes=(0,)), numpy_hash(rows, numpy_mask(lay, planes=(0,))))
  # excluded bytes do not count, whatever they hold
  noise = rows.copy()
  keep = numpy_mask(lay) != 0
  noise[:, ~keep] = random_rows(lay, 7, 12)[:, ~keep]
  assert np.array_equal(E.hash_states_host(pack(name), noise, num_players=players), got)


@pytest.mark.parametrize("name", ["collaborative_cooking__cramped", "coins"])
def test_every_byte_flip_changes_the_hash_exactly_where_the_mask_is_set(name):
  lay = layout(name, 0)
  S = lay.world_stride
  row = random_rows(lay, 1, 5)[0]
  bank = np.repeat(row[None, :], S + 1, axis=0)   # row i: byte i flipped; row S: the row itself
  bank[np.arange(S), np.arange(S)] ^= np.uint8(0x40)
  for spec in ({}, {"planes": (lay.grid_planes - 1,), "fields": ("ay", "ctr")}):
    h = E.hash_states_host(pack(name), bank, **spec)
    mask = E.state_hash_mask(pack(name), **spec)
    assert np.array_equal(h[:S] != h[S], mask != 0), spec
    assert len(set(h[:S][mask != 0].tolist())) == int((mask != 0).sum())   # and no two flips collide


def test_host_form_refusals():
  name = "coins"
  lay = layout(name, 0)
  rows = random_rows(lay, 4, 3)
  with pytest.raises(ValueError, match="fingerprint"):
    E.hash_states_host(pack(name), rows, fingerprint=lay.fingerprint ^ 1)
  with pytest.raises(ValueError, match="rows of"):
    E.hash_states_host(pack(name), rows[:, :-16])
  # unknown names and planes
  for kw in ({"fields": ("apples",)}, {"planes": (lay.grid_planes,)}, {"planes": (-1,)}, {"fields": ("player_block",)},
             {"planes": (), "fields": ()}):
    with pytest.raises(ValueError, match="hash"):
      E.hash_states_host(pack(name), rows, **kw)
    with pytest.raises(ValueError, match="hash"):
      E.state_hash_mask(pack(name), **kw)
  # the library's own refusals of a bad mask bit, an unknown flag, an unknown op: the raw request
  L = E.load_library()
  keep = E._host_config(pack(name))
  out = np.full(4, -7, np.int64)

  def request(op=E.MP_HASH_HOST, **fields):
    req = E.MpStatesHash(ctypes.sizeof(E.MpStatesHash), op, lay.fingerprint)
    req.pack, req.pack_len, req.cfg = ctypes.addressof(keep[0]), len(pack(name)), ctypes.pointer(keep[1])
    req.bank, req.bank_rows, req.count = rows.ctypes.data, 4, 4
    req.out, req.out_bytes = out.ctypes.data, out.nbytes
    for k, v in fields.items():
      setattr(req, k, v)
    return L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)), L.mp_last_error().decode()

  assert request()[0] == 0 and np.array_equal(out, numpy_hash(rows, numpy_mask(lay)))
  out[:] = -7
  for word, fields in (("names no plane", dict(flags=E.MP_HASH_CUSTOM, plane_mask=1 << lay.grid_planes)),
                       ("names no field", dict(flags=E.MP_HASH_CUSTOM, field_mask=1 << len(lay.fields))),
                       ("no player block", dict(flags=E.MP_HASH_CUSTOM | E.MP_HASH_PLAYER_BLOCK, plane_mask=1)),
                       ("includes no byte", dict(flags=E.MP_HASH_CUSTOM)),
                       ("default spec", dict(flags=0, plane_mask=1)),
                       ("default spec", dict(flags=4)),
                       ("unknown op", dict(op=9)),
                       ("at least 1", dict(count=0)),
                       ("without a row list", dict(count=5, out_bytes=40)),
                       ("need", dict(out_bytes=24)),
                       ("NULL bank", dict(bank=None)),
                       ("NULL out", dict(out=None)),
                       ("aligned", dict(out=out.ctypes.data + 4, count=3)),
                       ("struct_size", dict(struct_size=96))):
    rc, msg = request(**fields)
    assert rc == E.MP_ERR_INVALID and "MpStatesHash" in msg and word in msg, (word, rc, msg)
  assert (out == -7).all()   # nothing was written
  # MP_HASH_ROWS and MP_HASH_WORLDS need an engine
  for op in (E.MP_HASH_ROWS, E.MP_HASH_WORLDS):
    rc, msg = request(op=op)
    assert rc == E.MP_ERR_INVALID and "engine" in msg
  # an index outside the bank: its element stays, the others are hashed, the call says so
  want = numpy_hash(rows, numpy_mask(lay))
  for bad in (4, -1, 1 << 30):
    out[:] = -7
    with pytest.raises(ValueError, match=r"rows\[1\] = %d is not a row of the bank" % bad):
      E.hash_states_host(pack(name), rows, which=[2, bad, 0, 3], out=out)
    assert out.tolist() == [want[2], -7, want[0], want[3]]
  # a mask buffer that is too small
  req = E.MpStatesHash(ctypes.sizeof(E.MpStatesHash), E.MP_HASH_MASK)
  req.pack, req.pack_len, req.cfg = ctypes.addressof(keep[0]), len(pack(name)), ctypes.pointer(keep[1])
  small = np.zeros(lay.world_stride - 1, np.uint8)
  req.out, req.out_bytes = small.ctypes.data, small.nbytes
  assert L.mp_snapshot(None, ctypes.addressof(req), ctypes.sizeof(req)) == E.MP_ERR_INVALID
  assert "mask of a row" in L.mp_last_error().decode() and not small.any()


def test_c_wrappers_compile_and_agree(tmp_path):
  """include/mp_state_hash.h as a C program: the struct's size, and the host form's value."""
  import os
  import subprocess
  from meltingpot_amd import _build
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  lay = layout("coins", 0)
  rows = random_rows(lay, 2, 21)
  (tmp_path / "pack.bin").write_bytes(pack("coins"))
  (tmp_path / "rows.bin").write_bytes(rows.tobytes())
  src = tmp_path / "hash.c"
  src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "mp_state_hash.h"\n'
                 "static void* slurp(const char* p, long* n) { FILE* f = fopen(p, \"rb\"); fseek(f, 0, SEEK_END); *n = ftell(f);\n"
                 "  rewind(f); void* b = malloc(*n); if (fread(b, 1, *n, f) != (size_t)*n) return NULL; fclose(f); return b; }\n"
                 "int main(int argc, char** argv) {\n"
                 "  long np, nr; void* pack = slurp(argv[1], &np); void* rows = slurp(argv[2], &nr);\n"
                 "  MpConfig cfg; memset(&cfg, 0, sizeof cfg); cfg.struct_size = sizeof cfg; cfg.num_worlds = 1; cfg.auto_reset = 1;\n"
                 "  MpStateLayout lay; memset(&lay, 0, sizeof lay); lay.struct_size = sizeof lay; lay.pack = pack; lay.pack_len = np; lay.cfg = &cfg;\n"
                 "  if (mp_snapshot(NULL, &lay, sizeof lay)) return 2;\n"
                 "  uint64_t h[2] = {0, 0};\n"
                 "  int rc = mp_hash_states_host(pack, np, &cfg, rows, 2, NULL, 2, h, lay.fingerprint, NULL);\n"
                 "  MpHashSpec spec = {1, 0, MP_HASH_CUSTOM};\n"
                 "  uint8_t* mask = calloc(lay.world_stride, 1); long set = 0;\n"
                 "  int rc2 = mp_state_hash_mask(NULL, pack, np, &cfg, mask, lay.world_stride, &spec);\n"
                 "  for (int i = 0; i < lay.world_stride; ++i) set += mask[i] == 0xFF;\n"
                 "  printf(\"%zu %d %llu %llu %d %ld %d\\n\", sizeof(MpStatesHash), rc, (unsigned long long)h[0],\n"
                 "         (unsigned long long)h[1], rc2, set, MP_STEP_ROW_HASH);\n"
                 "  return 0;\n}\n")
  exe = tmp_path / "hash"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe),
                  _build.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_build.LIB_PATH)}"], check=True)
  E.load_library()
  out = subprocess.run([str(exe), str(tmp_path / "pack.bin"), str(tmp_path / "rows.bin")], capture_output=True,
                       text=True, check=True).stdout.split()
  want = numpy_hash(rows, numpy_mask(lay)).view(np.uint64)
  assert out == ["104", "0", str(int(want[0])), str(int(want[1])), "0", str(lay.H * lay.W), str(E.STEP_ROW_HASH)]
