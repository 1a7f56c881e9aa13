"""Writes tests/golden/state_request_refusals.json: what the library answers to malformed requests
about saved world states — MpStatesObserve, MpStatesView, MpStatesCheck, MpStatesHash,
MpEpisodeStarts, MpWorldStates (save, load) and the draws of MpEgoLayer, MpViewHash, MpEgoPlanes —
as {case name: [return code, normalised last-error text]}.  Run on the commit whose behaviour is to
be pinned, on a GPU:

    python tests/tools/make_state_request_refusals.py          # every case
    python tests/tools/make_state_request_refusals.py --cpu    # only the cases that need no device

Both also write tests/golden/request_dispatch.json, the same pairs for `dispatch_cases`: every
request's size through each of the two carriers with a NULL engine, a size no request has, and a
NULL buffer — which handler, if any, a (carrier, size) pair reaches.  No device is needed.

Every case is refused on the host before any launch (a few are accepted without a launch and pin
that: code 0, empty text).  A case breaks the one or two rules its name says; every other pointer
of its request is device memory large enough for it.  The list is this module's `cpu_cases` and
`gpu_cases`; tests/test_state_requests_cpu.py and tests/test_gpu_state_requests.py replay it."""
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from meltingpot_amd import engine as E  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "state_request_refusals.json")
DISPATCH = os.path.join(ROOT, "tests", "golden", "request_dispatch.json")
CARRIERS = ("mp_snapshot", "mp_restore")
ODD_SIZE = 8   # a buffer no request is the size of
N, BANK_ROWS = 2, 3
VIEWS = {"ego_layer": E.MpEgoLayer, "view_hash": E.MpViewHash, "ego_planes": E.MpEgoPlanes}


def normalise(text: str) -> str:
  """Pointers are PTR; what follows "runs past the end of its allocation" is the allocator's."""
  text = re.sub(r"0x[0-9a-f]+", "PTR", text)
  cut = "runs past the end of its allocation"
  return text[:text.index(cut) + len(cut)] if cut in text else text


def send_bytes(L, carrier: str, handle, address, size: int):
  """[return code, normalised text] of `size` bytes at `address` (None: a NULL buffer), read the way
  engine._check reads it."""
  rc = getattr(L, carrier)(handle, address, size)
  return [int(rc), normalise((L.mp_last_error() or b"").decode()) if rc else ""]


def send(L, carrier: str, handle, req):
  """`send_bytes` of one request."""
  return send_bytes(L, carrier, handle, ctypes.addressof(req), ctypes.sizeof(req))


def make(struct, **fields):
  req = struct(ctypes.sizeof(struct))
  for k, v in fields.items():
    setattr(req, k, v)
  return req


def aligned_host(nbytes: int):
  """(a 64-byte aligned address of `nbytes` bytes of plain host memory, what keeps it alive)"""
  a = np.zeros(nbytes + 64, np.uint8)
  return (a.ctypes.data + 63) & ~63, a


class HostCtx:
  """What the cases without a device share: the pack, its config, three zeroed rows."""

  def __init__(self):
    self.L = E.load_library()
    self.pack = E.load_pack("clean_up")
    self.keep = E._host_config(self.pack)
    self.pack_ptr, self.pack_len = ctypes.addressof(self.keep[0]), len(self.pack)
    self.cfg = ctypes.pointer(self.keep[1])
    self.cfg_ptr = ctypes.cast(self.cfg, ctypes.c_void_p)
    lay = E.state_layout(self.pack)
    self.S, self.fp, self.P = lay.world_stride, lay.fingerprint, lay.P
    self.num_ids = E.num_layer_ids_host(self.pack)
    self.bank, self._bank = aligned_host(BANK_ROWS * self.S)
    self.out_bytes = 1 << 20
    self.out, self._out = aligned_host(self.out_bytes)
    self._rows = np.array([0, 1, 2, 0], np.int32)
    self._far = np.array([0, 7, 0, 0], np.int32)
    self._players = np.zeros(4, np.int32)
    self._strangers = np.array([0, 99, 0, 0], np.int32)
    self._classes = np.zeros(self.num_ids, np.int32)
    self._wild = np.full(self.num_ids, 5, np.int32)
    self.rows, self.far, self.players = self._rows.ctypes.data, self._far.ctypes.data, self._players.ctypes.data
    self.strangers, self.classes, self.wild = (self._strangers.ctypes.data, self._classes.ctypes.data,
                                               self._wild.ctypes.data)


def view_extra(struct, c):
  """The fields a well-formed MpViewHash / MpEgoPlanes has beyond MpEgoLayer's."""
  if struct is E.MpEgoLayer:
    return {}
  extra = dict(classes=c.classes, classes_len=c.num_ids)
  if struct is E.MpEgoPlanes:
    extra.update(num_classes=1)
  return extra


def cpu_cases(c: HostCtx):
  """[(name, carrier, handle, request)]: the NULL-engine refusals and the host forms."""
  pack = dict(pack=c.pack_ptr, pack_len=c.pack_len)
  out = []

  def add(name, carrier, req):
    out.append((name, carrier, None, req))

  add("observe/null_engine", "mp_snapshot", make(E.MpStatesObserve))
  add("view/null_engine", "mp_snapshot", make(E.MpStatesView))
  add("episode_starts/null_engine", "mp_restore", make(E.MpEpisodeStarts))
  add("save/null_engine", "mp_snapshot", make(E.MpWorldStates, op=E.MP_STATES_SAVE))
  add("load/null_engine", "mp_restore", make(E.MpWorldStates, op=E.MP_STATES_LOAD))

  def check(**over):
    f = dict(op=E.MP_CHECK_HOST, fingerprint=c.fp, cfg=c.cfg, bank=c.bank, bank_rows=BANK_ROWS, count=2,
             out=c.out, out_bytes=c.out_bytes, **pack)
    f.update(over)
    return make(E.MpStatesCheck, **f)

  add("check/rows_without_engine", "mp_snapshot", check(op=E.MP_CHECK_ROWS))
  add("check/filter_without_engine", "mp_snapshot", check(op=E.MP_CHECK_FILTER))
  add("check_host/struct_size", "mp_snapshot", check(struct_size=8))
  add("check_host/op_unknown", "mp_snapshot", check(op=9))
  add("check_host/null_bank", "mp_snapshot", check(bank=None))
  add("check_host/null_out", "mp_snapshot", check(out=None))
  add("check_host/count_0", "mp_snapshot", check(count=0))
  add("check_host/bank_rows_0", "mp_snapshot", check(bank_rows=0))
  add("check_host/no_rows_count_over", "mp_snapshot", check(count=4))
  add("check_host/out_bytes", "mp_snapshot", check(out_bytes=8))
  add("check_host/out_align", "mp_snapshot", check(out=c.out + 2))
  add("check_host/rows_align", "mp_snapshot", check(rows=c.rows + 2))
  add("check_host/null_cfg", "mp_snapshot", check(cfg=None))
  add("check_host/fingerprint", "mp_snapshot", check(fingerprint=c.fp ^ 1))
  add("check_host/two_count_0_then_out_bytes", "mp_snapshot", check(count=0, out_bytes=0))
  add("check_host/two_null_cfg_then_fingerprint", "mp_snapshot", check(cfg=None, fingerprint=c.fp ^ 1))

  def hash_(**over):
    f = dict(op=E.MP_HASH_HOST, fingerprint=c.fp, cfg=c.cfg, bank=c.bank, bank_rows=BANK_ROWS, count=2,
             out=c.out, out_bytes=c.out_bytes, **pack)
    f.update(over)
    return make(E.MpStatesHash, **f)

  add("hash/rows_without_engine", "mp_snapshot", hash_(op=E.MP_HASH_ROWS))
  add("hash/worlds_without_engine", "mp_snapshot", hash_(op=E.MP_HASH_WORLDS))
  add("hash_host/struct_size", "mp_snapshot", hash_(struct_size=8))
  add("hash_host/op_unknown", "mp_snapshot", hash_(op=9))
  add("hash_host/flags_unknown", "mp_snapshot", hash_(flags=4))
  add("hash_host/default_spec_with_planes", "mp_snapshot", hash_(plane_mask=1))
  add("hash_host/null_out", "mp_snapshot", hash_(out=None))
  add("hash_host/null_bank", "mp_snapshot", hash_(bank=None))
  add("hash_host/count_0", "mp_snapshot", hash_(count=0))
  add("hash_host/bank_rows_0", "mp_snapshot", hash_(bank_rows=0))
  add("hash_host/no_rows_count_over", "mp_snapshot", hash_(count=4))
  add("hash_host/out_bytes", "mp_snapshot", hash_(out_bytes=8))
  add("hash_host/out_align", "mp_snapshot", hash_(out=c.out + 4))
  add("hash_host/rows_align", "mp_snapshot", hash_(rows=c.rows + 2))
  add("hash_host/null_cfg", "mp_snapshot", hash_(cfg=None))
  add("hash_host/spec_no_plane", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM, plane_mask=1 << 40))
  add("hash_host/spec_no_byte", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM))
  add("hash_host/fingerprint", "mp_snapshot", hash_(fingerprint=c.fp ^ 1))
  add("hash_host/row_outside", "mp_snapshot", hash_(rows=c.far))
  add("hash_host/two_null_out_then_null_bank", "mp_snapshot", hash_(out=None, bank=None))
  add("hash_host/two_out_bytes_then_fingerprint", "mp_snapshot", hash_(out_bytes=8, fingerprint=c.fp ^ 1))
  add("hash_mask/counts_not_validated", "mp_snapshot", hash_(op=E.MP_HASH_MASK, count=0, bank_rows=0, bank=None))
  add("hash_mask/out_bytes", "mp_snapshot", hash_(op=E.MP_HASH_MASK, out_bytes=8))
  add("hash_mask/spec_no_byte", "mp_snapshot", hash_(op=E.MP_HASH_MASK, flags=E.MP_HASH_CUSTOM))
  add("hash_mask/null_cfg", "mp_snapshot", hash_(op=E.MP_HASH_MASK, cfg=None))
  add("hash_mask/two_null_out_then_out_bytes", "mp_snapshot", hash_(op=E.MP_HASH_MASK, out=None, out_bytes=0))

  for name, struct in VIEWS.items():
    def view(**over):
      f = dict(op=3, fingerprint=c.fp, cfg=c.cfg_ptr, bank=c.bank, bank_rows=BANK_ROWS, count=2, dst=c.out,
               dst_bytes=c.out_bytes, **pack)
      f.update(view_extra(struct, c))
      f.update(over)
      return make(struct, **f)

    add(f"{name}/draw_without_engine", "mp_snapshot", view(op=1))
    add(f"{name}/register_without_engine", "mp_snapshot", view(op=2))
    add(f"{name}_host/struct_size", "mp_snapshot", view(struct_size=8))
    add(f"{name}_host/op_unknown", "mp_snapshot", view(op=9))
    add(f"{name}_host/reserved", "mp_snapshot", view(reserved=1))
    add(f"{name}_host/null_pack", "mp_snapshot", view(pack=None))
    add(f"{name}_host/null_cfg", "mp_snapshot", view(cfg=None))
    add(f"{name}_host/null_dst", "mp_snapshot", view(dst=None))
    add(f"{name}_host/null_bank", "mp_snapshot", view(bank=None))
    add(f"{name}_host/count_0", "mp_snapshot", view(count=0))
    add(f"{name}_host/bank_rows_0", "mp_snapshot", view(bank_rows=0))
    add(f"{name}_host/no_rows_count_over", "mp_snapshot", view(count=4))
    add(f"{name}_host/fingerprint", "mp_snapshot", view(fingerprint=c.fp ^ 1))
    add(f"{name}_host/dst_bytes", "mp_snapshot", view(dst_bytes=4))
    add(f"{name}_host/rows_align", "mp_snapshot", view(rows=c.rows + 2))
    add(f"{name}_host/players_align", "mp_snapshot", view(players=c.players + 2))
    add(f"{name}_host/row_outside", "mp_snapshot", view(rows=c.far))
    add(f"{name}_host/player_outside", "mp_snapshot", view(players=c.strangers))
    add(f"{name}_host/two_count_0_then_fingerprint", "mp_snapshot", view(count=0, fingerprint=c.fp ^ 1))
    add(f"{name}_host/two_fingerprint_then_dst_bytes", "mp_snapshot", view(fingerprint=c.fp ^ 1, dst_bytes=4))
    add(f"{name}_host/two_dst_bytes_then_rows_align", "mp_snapshot", view(dst_bytes=4, rows=c.rows + 2))
    if struct is not E.MpEgoLayer:
      add(f"{name}_host/classes_len", "mp_snapshot", view(classes_len=3))
      add(f"{name}_host/layer_mask", "mp_snapshot", view(layer_mask=1 << 40))
    if struct is E.MpEgoPlanes:
      add(f"{name}_host/class_outside", "mp_snapshot", view(classes=c.wild))
  return out


class DeviceCtx:
  """What the cases with an engine share: one clean_up engine of N worlds, a bank of BANK_ROWS rows
  (attached by `bank_ready` after the one reset), index lists, one large destination, plain host
  memory, and addresses 4, 8 and 16 bytes in front of the end of a device allocation."""

  def __init__(self):
    import torch
    self.torch = torch
    self.eng = E.Engine(E.load_pack("clean_up"), N, device=0)
    self.L, self.h = self.eng._L, self.eng._h
    self.S, self.P, self.fp = int(self.eng.info.world_state_bytes), self.eng.P, self.eng.state_fingerprint
    dev = self.eng.device
    self.num_ids = self.eng.num_layer_ids
    self._rows = torch.tensor([0, 1, 2, 0], dtype=torch.int32, device=dev)
    self._src = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    self._players = torch.zeros(4, dtype=torch.int32, device=dev)
    self._classes = torch.zeros(self.num_ids, dtype=torch.int32, device=dev)
    self._verdicts = torch.zeros((BANK_ROWS, 2), dtype=torch.int32, device=dev)
    self.out_bytes = 8 << 20
    self._out = torch.zeros(self.out_bytes, dtype=torch.uint8, device=dev)
    self._spare = torch.zeros((BANK_ROWS, self.S), dtype=torch.uint8, device=dev)   # (before the reset: no rows yet)
    self.rows, self.src, self.players = self._rows.data_ptr(), self._src.data_ptr(), self._players.data_ptr()
    self.classes, self.verdicts, self.out = self._classes.data_ptr(), self._verdicts.data_ptr(), self._out.data_ptr()
    self.bank = self._spare.data_ptr()
    self.host, self._host = aligned_host(self.out_bytes)
    assert self.out % 256 == 0 and self.bank % 16 == 0
    end = self.allocation_end(self.out)
    self.tail4, self.tail8, self.tail16 = end - 4, end - 8, end - 16

  def allocation_end(self, ptr: int) -> int:
    """The end of the device allocation `ptr` lies in (torch's allocator hands out parts of them)."""
    for seg in self.torch.cuda.memory_snapshot():
      if seg["address"] <= ptr < seg["address"] + seg["total_size"]:
        assert not seg.get("is_expandable", False), "an expandable segment is no single allocation"
        return seg["address"] + seg["total_size"]
    raise AssertionError("the tensor lies in no segment of torch's allocator")

  def bank_ready(self):
    self.eng.reset()
    self._bank = self.eng.save_worlds(self.torch.tensor([0, 1, 0]))
    self.torch.cuda.synchronize()
    self.bank = self._bank.data_ptr()
    assert self.bank % 16 == 0

  def close(self):
    self.torch.cuda.synchronize()
    self.eng.close()


def view_draw(struct, c: DeviceCtx, **over):
  f = dict(op=1, fingerprint=c.fp, bank=c.bank, bank_rows=BANK_ROWS, count=2, dst=c.out, dst_bytes=c.out_bytes)
  f.update(view_extra(struct, c))
  f.update(over)
  return make(struct, **f)


def gpu_cases_before_reset(c: DeviceCtx):
  """[(name, carrier, handle, request)] for an engine that has never been reset."""
  out = [("save/never_reset", "mp_snapshot", c.h,
          make(E.MpWorldStates, op=E.MP_STATES_SAVE, count=N, bank=c.out, bank_bytes=c.out_bytes)),
         ("hash/worlds_never_reset", "mp_snapshot", c.h,
          make(E.MpStatesHash, op=E.MP_HASH_WORLDS, count=N, out=c.out, out_bytes=c.out_bytes)),
         ("hash/two_never_reset_then_out_host", "mp_snapshot", c.h,
          make(E.MpStatesHash, op=E.MP_HASH_WORLDS, count=N, out=c.host, out_bytes=c.out_bytes))]
  for name, struct in VIEWS.items():
    out.append((f"{name}/live_never_reset", "mp_snapshot", c.h, view_draw(struct, c, bank=None, bank_rows=0)))
  return out


def gpu_cases(c: DeviceCtx):
  """[(name, carrier, handle, request)] for the engine after its reset, `c.bank` saved from it."""
  out = []

  def add(name, carrier, req):
    out.append((name, carrier, c.h, req))

  def extents(prefix, carrier, build, fields):
    """Per field (name, tail address): plain host memory, and an extent that leaves its allocation."""
    for field, tail in fields:
      add(f"{prefix}/{field}_host", carrier, build(**{field: c.host}))
      add(f"{prefix}/{field}_past_end", carrier, build(**{field: tail}))

  def observe(**over):
    f = dict(kind=E.OBS_LAYER, fingerprint=c.fp, bank=c.bank, bank_rows=BANK_ROWS, count=2, dst=c.out,
             dst_bytes=c.out_bytes)
    f.update(over)
    return make(E.MpStatesObserve, **f)

  def view(**over):
    f = dict(kind=E.OBS_LAYER, fingerprint=c.fp, bank=c.bank, bank_rows=BANK_ROWS, count=2, players=c.players,
             dst=c.out, dst_bytes=c.out_bytes)
    f.update(over)
    return make(E.MpStatesView, **f)

  for prefix, build in (("observe", observe), ("view", view)):
    add(f"{prefix}/struct_size", "mp_snapshot", build(struct_size=8))
    add(f"{prefix}/null_bank", "mp_snapshot", build(bank=None))
    add(f"{prefix}/null_dst", "mp_snapshot", build(dst=None))
    add(f"{prefix}/count_0", "mp_snapshot", build(count=0))
    add(f"{prefix}/bank_rows_0", "mp_snapshot", build(bank_rows=0))
    add(f"{prefix}/no_rows_count_over", "mp_snapshot", build(count=4))
    add(f"{prefix}/fingerprint", "mp_snapshot", build(fingerprint=c.fp ^ 1))
    add(f"{prefix}/kind_over", "mp_snapshot", build(kind=99))
    add(f"{prefix}/kind_negative", "mp_snapshot", build(kind=-1))
    add(f"{prefix}/kind_transition", "mp_snapshot", build(kind=E.OBS_REWARD))
    add(f"{prefix}/kind_absent", "mp_snapshot", build(kind=E.OBS_INVENTORY))
    add(f"{prefix}/dst_bytes", "mp_snapshot", build(dst_bytes=8))
    add(f"{prefix}/dst_align_4", "mp_snapshot", build(dst=c.out + 2))
    add(f"{prefix}/dst_align_8", "mp_snapshot", build(kind=E.OBS_READY_TO_SHOOT, dst=c.out + 4))
    add(f"{prefix}/rows_align", "mp_snapshot", build(rows=c.rows + 2))
    add(f"{prefix}/bank_align", "mp_snapshot", build(bank=c.bank + 8))
    add(f"{prefix}/two_count_0_then_fingerprint", "mp_snapshot", build(count=0, fingerprint=c.fp ^ 1))
    add(f"{prefix}/two_fingerprint_then_kind", "mp_snapshot", build(fingerprint=c.fp ^ 1, kind=99))
    add(f"{prefix}/two_dst_bytes_then_dst_align", "mp_snapshot", build(dst_bytes=8, dst=c.out + 2))
    add(f"{prefix}/two_dst_align_then_bank_align", "mp_snapshot", build(dst=c.out + 2, bank=c.bank + 8))
    add(f"{prefix}/two_bank_host_then_dst_host", "mp_snapshot", build(bank=c.host, dst=c.host))
  add("observe/dst_align_pooled", "mp_snapshot", observe(kind=E.OBS_RGB_POOL2, dst=c.out + 4))
  add("observe/two_null_bank_then_count_0", "mp_snapshot", observe(bank=None, count=0))
  extents("observe", "mp_snapshot", lambda **o: observe(count=4, **{"rows": c.rows, **o}),
          (("bank", c.tail16), ("rows", c.tail8), ("dst", c.tail16)))
  add("view/reserved", "mp_snapshot", view(reserved=(ctypes.c_uint64 * 2)(0, 1)))
  add("view/null_players", "mp_snapshot", view(players=None))
  add("view/world_rgb", "mp_snapshot", view(kind=E.OBS_WORLD_RGB))
  add("view/players_align", "mp_snapshot", view(players=c.players + 2))
  add("view/two_reserved_then_null_bank", "mp_snapshot", view(reserved=(ctypes.c_uint64 * 2)(1, 0), bank=None))
  add("view/two_null_dst_then_null_players", "mp_snapshot", view(dst=None, players=None))
  add("view/two_rows_align_then_players_align", "mp_snapshot", view(rows=c.rows + 2, players=c.players + 2))
  extents("view", "mp_snapshot", lambda **o: view(count=4, **{"rows": c.rows, **o}),
          (("bank", c.tail16), ("rows", c.tail8), ("players", c.tail8), ("dst", c.tail16)))

  def check(**over):
    f = dict(op=E.MP_CHECK_ROWS, fingerprint=c.fp, bank=c.bank, bank_rows=BANK_ROWS, count=2, out=c.out,
             out_bytes=c.out_bytes)
    f.update(over)
    return make(E.MpStatesCheck, **f)

  add("check/struct_size", "mp_snapshot", check(struct_size=8))
  add("check/op_unknown", "mp_snapshot", check(op=9))
  add("check/host_with_engine", "mp_snapshot", check(op=E.MP_CHECK_HOST))
  add("check/null_bank", "mp_snapshot", check(bank=None))
  add("check/null_out", "mp_snapshot", check(out=None))
  add("check/count_0", "mp_snapshot", check(count=0))
  add("check/bank_rows_0", "mp_snapshot", check(bank_rows=0))
  add("check/no_rows_count_over", "mp_snapshot", check(count=4))
  add("check/filter_without_src", "mp_snapshot", check(op=E.MP_CHECK_FILTER, count=N))
  add("check/out_bytes", "mp_snapshot", check(out_bytes=8))
  add("check/filter_out_bytes", "mp_snapshot", check(op=E.MP_CHECK_FILTER, count=N, rows=c.src, out_bytes=4))
  add("check/out_align", "mp_snapshot", check(out=c.out + 2))
  add("check/rows_align", "mp_snapshot", check(rows=c.rows + 2))
  add("check/fingerprint", "mp_snapshot", check(fingerprint=c.fp ^ 1))
  add("check/filter_count", "mp_snapshot", check(op=E.MP_CHECK_FILTER, count=3, rows=c.rows))
  add("check/bank_align", "mp_snapshot", check(bank=c.bank + 8))
  add("check/two_op_unknown_then_null_bank", "mp_snapshot", check(op=9, bank=None))
  add("check/two_out_bytes_then_fingerprint", "mp_snapshot", check(out_bytes=8, fingerprint=c.fp ^ 1))
  add("check/two_fingerprint_then_filter_count", "mp_snapshot",
      check(op=E.MP_CHECK_FILTER, count=3, rows=c.rows, fingerprint=c.fp ^ 1))
  add("check/two_fingerprint_then_bank_align", "mp_snapshot", check(fingerprint=c.fp ^ 1, bank=c.bank + 8))
  add("check/two_bank_align_then_out_host", "mp_snapshot", check(bank=c.bank + 8, out=c.host))
  extents("check", "mp_snapshot", lambda **o: check(count=4, **{"rows": c.rows, **o}),
          (("bank", c.tail16), ("rows", c.tail8), ("out", c.tail16)))

  def hash_(**over):
    f = dict(op=E.MP_HASH_ROWS, fingerprint=c.fp, bank=c.bank, bank_rows=BANK_ROWS, count=2, out=c.out,
             out_bytes=c.out_bytes)
    f.update(over)
    return make(E.MpStatesHash, **f)

  def worlds(**over):
    return hash_(**{"op": E.MP_HASH_WORLDS, "bank": None, "bank_rows": 0, "count": N, **over})

  add("hash/struct_size", "mp_snapshot", hash_(struct_size=8))
  add("hash/op_unknown", "mp_snapshot", hash_(op=9))
  add("hash/host_with_engine", "mp_snapshot", hash_(op=E.MP_HASH_HOST))
  add("hash/flags_unknown", "mp_snapshot", hash_(flags=4))
  add("hash/default_spec_with_fields", "mp_snapshot", hash_(field_mask=1))
  add("hash/null_out", "mp_snapshot", hash_(out=None))
  add("hash/null_bank", "mp_snapshot", hash_(bank=None))
  add("hash/count_0", "mp_snapshot", hash_(count=0))
  add("hash/bank_rows_0", "mp_snapshot", hash_(bank_rows=0))
  add("hash/worlds_count_0", "mp_snapshot", worlds(count=0))
  add("hash/no_rows_count_over", "mp_snapshot", hash_(count=4))
  add("hash/worlds_count_not_n", "mp_snapshot", worlds(count=1))
  add("hash/out_bytes", "mp_snapshot", hash_(out_bytes=8))
  add("hash/out_align", "mp_snapshot", hash_(out=c.out + 4))
  add("hash/rows_align", "mp_snapshot", hash_(rows=c.rows + 2))
  add("hash/spec_no_plane", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM, plane_mask=1 << 40))
  add("hash/spec_no_field", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM, field_mask=1 << 31))
  add("hash/spec_no_player_block", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM | E.MP_HASH_PLAYER_BLOCK))
  add("hash/spec_no_byte", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM))
  add("hash/fingerprint", "mp_snapshot", hash_(fingerprint=c.fp ^ 1))
  add("hash/worlds_ignore_fingerprint_refuse_out_host", "mp_snapshot", worlds(fingerprint=c.fp ^ 1, out=c.host))
  add("hash/bank_align", "mp_snapshot", hash_(bank=c.bank + 8))
  add("hash/mask_counts_not_validated", "mp_snapshot",
      hash_(op=E.MP_HASH_MASK, count=0, bank_rows=0, bank=None, out=c.host))
  add("hash/mask_out_bytes", "mp_snapshot", hash_(op=E.MP_HASH_MASK, out=c.host, out_bytes=8))
  add("hash/two_flags_then_null_out", "mp_snapshot", hash_(flags=4, out=None))
  add("hash/two_null_out_then_null_bank", "mp_snapshot", hash_(out=None, bank=None))
  add("hash/two_out_bytes_then_out_align", "mp_snapshot", hash_(out_bytes=8, out=c.out + 4))
  add("hash/two_out_align_then_spec", "mp_snapshot", hash_(out=c.out + 4, flags=E.MP_HASH_CUSTOM))
  add("hash/two_spec_then_fingerprint", "mp_snapshot", hash_(flags=E.MP_HASH_CUSTOM, fingerprint=c.fp ^ 1))
  add("hash/two_fingerprint_then_bank_align", "mp_snapshot", hash_(fingerprint=c.fp ^ 1, bank=c.bank + 8))
  extents("hash", "mp_snapshot", lambda **o: hash_(count=4, **{"rows": c.rows, **o}),
          (("bank", c.tail16), ("rows", c.tail8), ("out", c.tail16)))
  extents("hash/worlds", "mp_snapshot", lambda **o: worlds(count=4, **{"rows": c.rows, **o}),
          (("rows", c.tail8), ("out", c.tail16)))

  def starts(**over):
    f = dict(fingerprint=c.fp, bank=c.bank, rows=c.src, verdicts=c.verdicts, bank_rows=BANK_ROWS)
    f.update(over)
    return make(E.MpEpisodeStarts, **f)

  add("episode_starts/struct_size", "mp_restore", starts(struct_size=8))
  add("episode_starts/null_bank_clears", "mp_restore", starts(bank=None, bank_rows=0, rows=None, fresh=7))
  add("episode_starts/bank_rows_0", "mp_restore", starts(bank_rows=0))
  add("episode_starts/null_rows", "mp_restore", starts(rows=None))
  add("episode_starts/fresh", "mp_restore", starts(fresh=2))
  add("episode_starts/fingerprint", "mp_restore", starts(fingerprint=c.fp ^ 1))
  add("episode_starts/bank_align", "mp_restore", starts(bank=c.bank + 8))
  add("episode_starts/rows_align", "mp_restore", starts(rows=c.src + 2))
  add("episode_starts/verdicts_align", "mp_restore", starts(verdicts=c.verdicts + 2))
  add("episode_starts/two_bank_rows_0_then_null_rows", "mp_restore", starts(bank_rows=0, rows=None))
  add("episode_starts/two_fresh_then_fingerprint", "mp_restore", starts(fresh=2, fingerprint=c.fp ^ 1))
  add("episode_starts/two_fingerprint_then_bank_align", "mp_restore", starts(fingerprint=c.fp ^ 1, bank=c.bank + 8))
  add("episode_starts/two_bank_align_then_rows_align", "mp_restore", starts(bank=c.bank + 8, rows=c.src + 2))
  add("episode_starts/two_rows_align_then_bank_host", "mp_restore", starts(rows=c.src + 2, bank=c.host))
  extents("episode_starts", "mp_restore", starts,
          (("bank", c.tail16), ("rows", c.tail4), ("verdicts", c.tail8)))

  def save(**over):
    f = dict(op=E.MP_STATES_SAVE, worlds=c.src, count=N, bank=c.out, bank_bytes=c.out_bytes)
    f.update(over)
    return make(E.MpWorldStates, **f)

  add("save/struct_size", "mp_snapshot", save(struct_size=8))
  add("save/through_mp_restore", "mp_restore", save())
  add("save/op_unknown", "mp_snapshot", save(op=9))
  add("save/null_dst", "mp_snapshot", save(bank=None))
  add("save/count_0", "mp_snapshot", save(count=0))
  add("save/count_not_n", "mp_snapshot", save(worlds=None, count=1))
  add("save/bank_bytes", "mp_snapshot", save(bank_bytes=8))
  add("save/two_count_not_n_then_bank_bytes", "mp_snapshot", save(worlds=None, count=1, bank_bytes=8))
  add("save/two_bank_bytes_then_dst_host", "mp_snapshot", save(bank_bytes=8, bank=c.host))
  add("save/two_dst_host_then_worlds_host", "mp_snapshot", save(bank=c.host, worlds=c.host))
  extents("save", "mp_snapshot", save, (("bank", c.tail16), ("worlds", c.tail4)))

  def load(**over):
    f = dict(op=E.MP_STATES_LOAD, fingerprint=c.fp, bank=c.bank, bank_rows=BANK_ROWS, src=c.src)
    f.update(over)
    return make(E.MpWorldStates, **f)

  add("load/struct_size", "mp_restore", load(struct_size=8))
  add("load/through_mp_snapshot", "mp_snapshot", load())
  add("load/null_bank", "mp_restore", load(bank=None))
  add("load/null_src", "mp_restore", load(src=None))
  add("load/bank_rows_0", "mp_restore", load(bank_rows=0))
  add("load/fingerprint", "mp_restore", load(fingerprint=c.fp ^ 1))
  add("load/two_null_src_then_fingerprint", "mp_restore", load(src=None, fingerprint=c.fp ^ 1))
  add("load/two_fingerprint_then_bank_host", "mp_restore", load(fingerprint=c.fp ^ 1, bank=c.host))
  add("load/two_bank_host_then_src_host", "mp_restore", load(bank=c.host, src=c.host))
  extents("load", "mp_restore", load, (("bank", c.tail16), ("src", c.tail4)))

  for name, struct in VIEWS.items():
    def draw(**over):
      return view_draw(struct, c, **over)

    add(f"{name}/host_with_engine", "mp_snapshot", draw(op=3))
    add(f"{name}/count_0", "mp_snapshot", draw(count=0))
    add(f"{name}/bank_rows_0", "mp_snapshot", draw(bank_rows=0))
    add(f"{name}/no_rows_count_over", "mp_snapshot", draw(count=4))
    add(f"{name}/live_no_rows_count_over", "mp_snapshot", draw(bank=None, bank_rows=0, count=3))
    add(f"{name}/fingerprint", "mp_snapshot", draw(fingerprint=c.fp ^ 1))
    add(f"{name}/dst_bytes", "mp_snapshot", draw(dst_bytes=4))
    add(f"{name}/rows_align", "mp_snapshot", draw(rows=c.rows + 2))
    add(f"{name}/players_align", "mp_snapshot", draw(players=c.players + 2))
    add(f"{name}/bank_align", "mp_snapshot", draw(bank=c.bank + 8))
    add(f"{name}/two_count_0_then_fingerprint", "mp_snapshot", draw(count=0, fingerprint=c.fp ^ 1))
    add(f"{name}/two_fingerprint_then_dst_bytes", "mp_snapshot", draw(fingerprint=c.fp ^ 1, dst_bytes=4))
    add(f"{name}/two_rows_align_then_bank_align", "mp_snapshot", draw(rows=c.rows + 2, bank=c.bank + 8))
    add(f"{name}/two_bank_align_then_dst_host", "mp_snapshot", draw(bank=c.bank + 8, dst=c.host))
    fields = [("bank", c.tail16), ("rows", c.tail8), ("players", c.tail8), ("dst", c.tail16)]
    if struct is not E.MpEgoLayer:
      fields.insert(3, ("classes", c.tail16))
    extents(name, "mp_snapshot", lambda **o: draw(count=4, **{"rows": c.rows, "players": c.players, **o}), fields)
    extents(f"{name}/live", "mp_snapshot",
            lambda **o: draw(bank=None, bank_rows=0, count=4, **{"rows": c.rows, **o}),
            (("rows", c.tail8), ("dst", c.tail16)))
  return out


def dispatch_cases():
  """[(name, carrier, request or None, size)], all with a NULL engine: each request, zero but for its
  struct_size, through each carrier; ODD_SIZE bytes; a NULL buffer of a request's size."""
  requests = [q.struct for q in E.REQUESTS]
  assert ODD_SIZE not in [ctypes.sizeof(s) for s in requests]
  out = []
  for carrier in CARRIERS:
    for struct in requests:
      out.append((f"{struct.__name__}/{carrier}", carrier, make(struct), ctypes.sizeof(struct)))
    out.append((f"odd_size/{carrier}", carrier, (ctypes.c_uint8 * ODD_SIZE)(), ODD_SIZE))
    out.append((f"null_buffer/{carrier}", carrier, None, ctypes.sizeof(E.MpStatesObserve)))
  return out


def replay_dispatch(L, cases):
  return {name: send_bytes(L, carrier, None, None if req is None else ctypes.addressof(req), size)
          for name, carrier, req, size in cases}


def replay(L, cases):
  return {name: send(L, carrier, handle, req) for name, carrier, handle, req in cases}


def record_cpu():
  c = HostCtx()
  return replay(c.L, cpu_cases(c))


def record_gpu():
  c = DeviceCtx()
  got = replay(c.L, gpu_cases_before_reset(c))
  c.bank_ready()
  got.update(replay(c.L, gpu_cases(c)))
  c.close()
  return got


def main():
  got = {}
  if os.path.exists(GOLDEN):
    with open(GOLDEN) as f:
      got = json.load(f)
  got.update(record_cpu())
  if "--cpu" not in sys.argv[1:]:
    got.update(record_gpu())
  with open(GOLDEN, "w") as f:
    json.dump(dict(sorted(got.items())), f, indent=1)
    f.write("\n")
  refused = sum(1 for rc, _ in got.values() if rc)
  print(GOLDEN, len(got), "cases,", refused, "refused,", os.path.getsize(GOLDEN), "bytes")
  dispatch = replay_dispatch(E.load_library(), dispatch_cases())
  with open(DISPATCH, "w") as f:
    json.dump(dict(sorted(dispatch.items())), f, indent=1)
    f.write("\n")
  print(DISPATCH, len(dispatch), "cases,", os.path.getsize(DISPATCH), "bytes")


if __name__ == "__main__":
  main()
