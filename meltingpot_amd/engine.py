"""ctypes binding of libmp_engine.so (C ABI: include/mp_engine.h).

Thin by design: the engine is the product, this module only moves pointers.
PyTorch-ROCm supplies device memory for action / observation tensors and the
stream; nothing here computes or measures (where a bound view is allocated and
which launch plan suits it are the library's business: mp_place_output, mp_tune).
There is no CPU fallback — constructing an `Engine` without a GPU (or without the
built library) raises.

Reference boundary replaced: `dmlab2d.Lab2d(...)` / `dmlab2d.Environment(...)`
(meltingpot/utils/substrates/builder.py:179-187).
"""

from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from meltingpot_amd import _build

OBS_RGB = 0
OBS_WORLD_RGB = 1
OBS_REWARD = 2
OBS_READY_TO_SHOOT = 3
OBS_AUX0 = 4
OBS_STEP_TYPE = 5
OBS_DISCOUNT = 6
OBS_COLLECTIVE_REWARD = 7
OBS_POSITION = 8
OBS_ORIENTATION = 9
OBS_EVENTS = 10
# debug observations (produced while bound, or with debug_observations=True)
OBS_AUX1 = 11  # clean_up: PLAYER_CLEANED
OBS_AUX2 = 12  # clean_up: PLAYER_ATE_APPLE
OBS_AUX3 = 13  # clean_up: NUM_OTHERS_PLAYER_ZAPPED_THIS_STEP
OBS_AUX4 = 14  # clean_up: NUM_OTHERS_WHO_ATE_THIS_STEP
OBS_ZAP_MATRIX = 15
OBS_LAYER = 16
OBS_INVENTORY = 17                 # *_in_the_matrix: "N.INVENTORY" f64 [N, P, R]
OBS_INTERACTION_INVENTORIES = 18   # "N.INTERACTION_INVENTORIES" f64 [N, P, 2, R]
# *_in_the_matrix debug cumulants f64 [N, P, 1 + 3 R] (the_matrix.py:22-60); columns:
OBS_MATRIX_CUMULANTS = 19
# *_in_the_matrix: f64 [N, P, 2], (row_reward, col_reward) of the latest interaction of
# player p — the rest of the 'interaction' event's payload (include/mp_engine.h)
OBS_INTERACTION_REWARDS = 20
# "N.RGB" pooled by k = 2, 4, 8 (k x k box average, rounded half up: `pool_rgb`), u8
# [N, P, VH * S / k, VW * S / k, 3]; drawn by the frame launch itself, the full image is never
# written.  One per-agent view (OBS_RGB or one pooled kind) can be bound at a time.
OBS_RGB_POOL2 = 21
OBS_RGB_POOL4 = 22
OBS_RGB_POOL8 = 23
OBS_RGB_POOL = {2: OBS_RGB_POOL2, 4: OBS_RGB_POOL4, 8: OBS_RGB_POOL8}
# the pixel views (placed / tuned like one another when large)
PIXEL_KINDS = (OBS_RGB, OBS_WORLD_RGB, OBS_RGB_POOL2, OBS_RGB_POOL4, OBS_RGB_POOL8)


def pool_rgb(images, k: int) -> np.ndarray:
  """What OBS_RGB_POOL<k> holds for full images `images` (u8 [..., H, W, 3], H and W
  multiples of k): every byte the k x k block average of the full image, rounded half up —
  (sum + k*k // 2) // (k*k), the rule lower._fit applies to sprite art."""
  a = np.asarray(images)
  if k == 1:
    return a.astype(np.uint8, copy=True)
  *lead, h, w, c = a.shape
  if h % k or w % k:
    raise ValueError(f"an image of {h} x {w} does not pool by {k}")
  s = a.astype(np.uint32).reshape(*lead, h // k, k, w // k, k, c).sum(axis=(-4, -2))
  return ((s + (k * k) // 2) // (k * k)).astype(np.uint8)


def matrix_cumulant_names(num_resources: int):
  """Reference observation names of the columns of OBS_MATRIX_CUMULANTS."""
  names = ["INTERACTED_THIS_STEP"]
  for k in range(1, num_resources + 1):
    names += [f"COLLECTED_RESOURCE_{k}", f"DESTROYED_RESOURCE_{k}",
              f"ARGMAX_INTERACTION_INVENTORY_WAS_{k}"]
  return names
EVENT_ROWS = 128  # MP_EVENT_ROWS: 1 header row + up to 127 events per world-step
# MpEventType -> (reference event name, payload keys)  (include/mp_engine.h)
EVENT_TYPES = {
    1: ("zap", ("source", "target")),
    2: ("edible_consumed", ("player_index",)),
    3: ("player_cleaned", ("player_index",)),
    4: ("claimed_resource", ("player_index",)),
    5: ("destroyed_resource", ("player_index",)),
    6: ("sanctioning", ("source", "target")),
    7: ("removal_due_to_sanctioning", ("source", "target")),
    8: ("set_sanctioning_level", ("player_index", "level")),
    9: ("AvatarStarted", ()),
    # payload b = player_coin_type << 1 | coin_type, indices of the two coin colours
    10: ("coin_consumed", ("player_index", "types")),
    # the_matrix: + row_reward, col_reward, row_inventory, col_inventory
    # (the_matrix/components.lua:789-797), read from OBS_INTERACTION_REWARDS and
    # OBS_INTERACTION_INVENTORIES of the same step by `Engine.events`
    11: ("interaction", ("row_player_idx", "col_player_idx")),
    12: ("collected_resource", ("player_index", "class")),
    # coop_mining/components.lua:196,210,220 (ore_type: 1 iron, 2 gold)
    13: ("mining", ("player", "ore_type")),
    14: ("extraction", ("player", "ore_type")),
    # payload b = player_b << 2 | ore_type (decoded by `Engine.events`)
    15: ("extraction_pair", ("player_a", "player_b", "ore_type")),
    # gift_refinements/components.lua:174-181; a = gifter_index | source_type << 4,
    # b = receipient_index | received_amount << 4 (decoded by `Engine.events`, which adds the
    # two avatars' roles from the pack's "agent_roles"; the reference's spelling of
    # "receipient" is kept)
    16: ("gift", ("gifter_index", "gifter_role", "receipient_index", "receipient_role",
                  "source_type", "received_amount")),
    # collaborative_cooking/components.lua:325-328, 397-400, 412-415 (item: 1 tomato, 2 dish,
    # 3 soup; decoded to the reference's strings by `Engine.events`)
    # externality_mushrooms/components.lua:72-74 (the type decoded to its state's name by
    # `Engine.events`)
    20: ("eating_mushroom", ("player_index", "mushroom_type")),
    17: ("receiver_accepted_item", ("player_index", "item")),
    18: ("item_dropped_into_pot", ("player_index", "item")),
    19: ("cooked_food_collected_from_pot", ("player_index", "cooked_item")),
}
COOKING_ITEMS = ("empty", "tomato", "dish", "soup")
# the live states of externality_mushrooms' mushroom prefab (externality_mushrooms.py:520-545)
MUSHROOM_TYPES = ("fullInternalityZeroExternality", "halfInternalityHalfExternality",
                  "zeroInternalityFullExternality", "negativeInternalityNegativeExternality")

COUNTER_NAMES = ("world_steps", "agent_steps", "episodes", "reward_sum_x1024",
                 "zaps", "aux0", "respawns", "bad_actions")

MP_ERR_INVALID = -1
MP_ERR_NO_DEVICE = -3
MP_ABI_VERSION = 8

# Every symbol include/mp_engine.h declares (tests check the library exports
# exactly these).
ABI_SYMBOLS = (
    "mp_abi_version", "mp_last_error", "mp_create", "mp_destroy", "mp_info",
    "mp_set_stream", "mp_bind_output", "mp_reset", "mp_step", "mp_step_host",
    "mp_step_fields", "mp_step_fields_host",
    "mp_observe", "mp_obs_bytes", "mp_dump", "mp_snapshot_bytes",
    "mp_snapshot", "mp_restore", "mp_counters", "mp_sync", "mp_fault_words",
    "mp_alloc_output", "mp_free_output", "mp_tune", "mp_place_output",
    "mp_bind_output_ring", "mp_set_retired_va_limit",
    "mp_torch_alloc", "mp_torch_free", "mp_box_fill")

# MpKernelVariant.variant: the frame kernels an engine runs
KERNEL_GENERIC, KERNEL_STOCK = 0, 1


class MpDevOptions(ctypes.Structure):
  """Test / development overrides of the launch plan (include/mp_engine.h);
  product code never passes one."""
  _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in (
      "batch_worlds", "waves", "feeders", "max_groups", "scratch_cells",
      "no_composite_cache", "max_composites", "verbose", "late_feeder_prio",
      "ring_batches", "static_pct", "world_waves", "store_sc1", "head", "no_next_orders",
      "record_pad", "pace", "team", "generic_kernel")]


class MpConfig(ctypes.Structure):
  _fields_ = [
      ("struct_size", ctypes.c_uint32),
      ("device", ctypes.c_int32),
      ("num_worlds", ctypes.c_int32),
      ("auto_reset", ctypes.c_int32),
      ("world_offset", ctypes.c_uint64),
      ("base_seed", ctypes.c_uint64),
      ("stream", ctypes.c_void_p),
      ("num_players", ctypes.c_int32),
      ("debug_observations", ctypes.c_int32),
      ("unfused", ctypes.c_int32),
      ("literal_base_seed", ctypes.c_int32),
      ("dev", ctypes.POINTER(MpDevOptions)),
      ("roles", ctypes.POINTER(ctypes.c_int32)),
      # 0 / 1: OBS_WORLD_RGB is the full image; 2, 4, 8: pooled by that factor (`pool_rgb`).
      # Appended to the ABI-8 layout, whose struct_size mp_create still takes (as 1).
      ("world_pool", ctypes.c_int32),
  ]


class MpInfo(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in (
      "abi_version", "substrate", "num_worlds", "num_players", "num_actions",
      "map_h", "map_w", "num_layers", "sprite_size", "view_h", "view_w",
      "max_frames", "world_state_bytes", "fused", "num_resources",
      "num_action_fields", "plan_batch_worlds", "plan_ring_batches", "plan_owned_batches",
      "plan_pooled_batches", "plan_groups", "plan_store_sc1", "plan_feeders", "plan_waves",
      "ring_slots", "ring_next", "plan_pace", "visible_layers", "plan_team", "plan_late_priority")] + [("retired_va_bytes", ctypes.c_int64),
                                      ("retired_va_limit", ctypes.c_int64)]


class MpPlacement(ctypes.Structure):
  _fields_ = [("candidates", ctypes.c_int32), ("picked", ctypes.c_int32),
              ("us", ctypes.c_float * 32), ("stepped", ctypes.c_int32),
              ("requested", ctypes.c_int32), ("out_of_memory", ctypes.c_int32),
              ("early_exit", ctypes.c_int32), ("setup_ms", ctypes.c_float)]


class MpBoxFill(ctypes.Structure):
  _fields_ = [("bytes", ctypes.c_uint64), ("memset_us", ctypes.c_float),
              ("product_order_us", ctypes.c_float), ("front_4k_us", ctypes.c_float),
              ("groups", ctypes.c_int32), ("waves", ctypes.c_int32), ("span_bytes", ctypes.c_uint32)]


# World-state requests (include/mp_engine.h: MpWorldStates), carried by mp_snapshot / mp_restore
MP_STATES_FINGERPRINT, MP_STATES_SAVE, MP_STATES_LOAD = 1, 2, 3


class MpKernelVariant(ctypes.Structure):
  """Which frame kernels an engine runs / a pack would get (include/mp_engine.h), carried by
  mp_snapshot."""
  _fields_ = [("struct_size", ctypes.c_uint32), ("variant", ctypes.c_int32),
              ("pack", ctypes.c_void_p), ("pack_len", ctypes.c_uint64),
              ("cfg", ctypes.POINTER(MpConfig)), ("fields", ctypes.c_void_p),
              ("fields_cap", ctypes.c_uint64)]


class MpWorldStates(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("op", ctypes.c_int32),
              ("fingerprint", ctypes.c_uint64), ("worlds", ctypes.c_void_p),
              ("src", ctypes.c_void_p), ("bank", ctypes.c_void_p), ("bank_bytes", ctypes.c_uint64),
              ("count", ctypes.c_int32), ("bank_rows", ctypes.c_int32)]


_SNAPSHOT, _RESTORE = "mp_snapshot", "mp_restore"   # the two carriers of a request


def _send(L, handle, req, carrier: Optional[str] = None, label: Optional[str] = None):
  """Sends the request struct `req` to engine `handle` (None: a host form) through its carrier in
  REQUESTS (through `carrier`, for the one request that has both), and returns it (with its
  outputs); raises like every call."""
  carrier = carrier or _CARRIER[type(req)]
  _check(L, getattr(L, carrier)(handle, ctypes.addressof(req), ctypes.sizeof(req)),
         f"{carrier} ({label or type(req).__name__})")
  return req


def _request(L, handle, struct, head, fields, carrier: Optional[str] = None, label: Optional[str] = None):
  """One request of type `struct`: struct_size, then `head` in the order of its fields, then `fields`."""
  req = struct(ctypes.sizeof(struct), *head)
  for k, v in fields.items():
    setattr(req, k, v)
  return _send(L, handle, req, carrier, label)


def world_states_request(L, handle, op: int, **fields) -> MpWorldStates:
  """Runs one MpWorldStates request on engine `handle` (MP_STATES_LOAD through mp_restore, the
  others through mp_snapshot) and returns it (with its outputs); raises like every call."""
  if op == MP_STATES_LOAD:
    return _request(L, handle, MpWorldStates, (op,), fields, _RESTORE, "MP_STATES_LOAD")
  return _request(L, handle, MpWorldStates, (op,), fields, _SNAPSHOT)


# Observations of bank rows (include/mp_engine.h: MpStatesObserve), carried by mp_snapshot
class MpStatesObserve(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_int32),
              ("fingerprint", ctypes.c_uint64), ("bank", ctypes.c_void_p), ("rows", ctypes.c_void_p),
              ("dst", ctypes.c_void_p), ("dst_bytes", ctypes.c_uint64), ("bank_rows", ctypes.c_int32),
              ("count", ctypes.c_int32), ("reserved", ctypes.c_uint64)]


# the kinds that are functions of a world's record: what observe_states draws from saved rows
STATE_OBS_KINDS = PIXEL_KINDS + (OBS_LAYER, OBS_READY_TO_SHOOT, OBS_POSITION, OBS_ORIENTATION,
                                 OBS_INVENTORY)


def states_observe_request(L, handle, **fields) -> MpStatesObserve:
  """Runs one MpStatesObserve request on engine `handle`; raises like every call."""
  return _request(L, handle, MpStatesObserve, (), fields)


# Sampled (row, player) views of bank rows (include/mp_engine.h: MpStatesView), carried by mp_snapshot
class MpStatesView(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_int32),
              ("fingerprint", ctypes.c_uint64), ("bank", ctypes.c_void_p), ("rows", ctypes.c_void_p),
              ("players", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("dst_bytes", ctypes.c_uint64),
              ("bank_rows", ctypes.c_int32), ("count", ctypes.c_int32), ("reserved", ctypes.c_uint64 * 2)]


def states_view_request(L, handle, **fields) -> MpStatesView:
  """Runs one MpStatesView request on engine `handle`; raises like every call."""
  return _request(L, handle, MpStatesView, (), fields)


# EGO_LAYER, the layer view in the avatar's own frame (include/mp_engine.h: MpEgoLayer), carried by
# mp_snapshot
MP_EGO_DRAW, MP_EGO_REGISTER, MP_EGO_HOST = 1, 2, 3
OBS_EGO_LAYER = -1   # no MpObsKind: the Python layers' handle for the leaf where leaves map to kinds
OBS_AVATAR_IDS = -2  # likewise: "AVATAR_IDS_IN_VIEW" and "AVATAR_IDS_IN_RANGE_TO_ZAP"


# What MpEgoLayer, MpViewHash, MpEgoPlanes and MpAvatarIds begin with (csrc/engine_views.hip:
# ViewRequest): the head, one int32 of the request's own, then the host form's pack
_VIEW_HEAD = [("struct_size", ctypes.c_uint32), ("op", ctypes.c_int32), ("fingerprint", ctypes.c_uint64),
              ("bank", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("players", ctypes.c_void_p),
              ("dst", ctypes.c_void_p), ("dst_bytes", ctypes.c_uint64), ("bank_rows", ctypes.c_int32),
              ("count", ctypes.c_int32), ("slot_stride", ctypes.c_uint64), ("slots", ctypes.c_int32)]
_VIEW_PACK = [("pack", ctypes.c_void_p), ("pack_len", ctypes.c_uint64), ("cfg", ctypes.c_void_p)]
_VIEW_CLASSES = (_VIEW_HEAD + [("classes_len", ctypes.c_int32)] + _VIEW_PACK +
                 [("layer_mask", ctypes.c_uint64), ("classes", ctypes.c_void_p), ("num_ids", ctypes.c_int32)])


class MpEgoLayer(ctypes.Structure):
  _fields_ = _VIEW_HEAD + [("reserved", ctypes.c_int32)] + _VIEW_PACK + [("reserved2", ctypes.c_uint64 * 3)]


def ego_layer_request(L, handle, op: int, **fields) -> MpEgoLayer:
  """Runs one MpEgoLayer request on engine `handle` (None: the host form); raises like every call."""
  return _request(L, handle, MpEgoLayer, (int(op),), fields)


# The layout of a record and the check of edited records (include/mp_engine.h: MpStateLayout,
# MpStatesCheck), carried by mp_snapshot
class MpStateField(ctypes.Structure):
  _fields_ = [("name", ctypes.c_char * 16), ("offset", ctypes.c_int32), ("elem_bytes", ctypes.c_int32),
              ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_LAYOUT_INTS = ("map_h", "map_w", "num_layers", "num_players", "num_states", "grid_planes", "grid_bytes",
                "grid_pad", "world_stride", "tail_bytes", "max_frames", "avatar_layer", "substrate",
                "player_block")


class MpStateLayout(ctypes.Structure):
  _fields_ = ([("struct_size", ctypes.c_uint32), ("layout_version", ctypes.c_uint32),
               ("pack", ctypes.c_void_p), ("pack_len", ctypes.c_uint64), ("cfg", ctypes.POINTER(MpConfig))] +
              [(n, ctypes.c_int32) for n in _LAYOUT_INTS] + [("reserved", ctypes.c_int32 * 2)] +
              [("fingerprint", ctypes.c_uint64), ("fields", ctypes.POINTER(MpStateField)),
               ("fields_cap", ctypes.c_int32), ("num_fields", ctypes.c_int32)])


MP_CHECK_ROWS, MP_CHECK_HOST, MP_CHECK_FILTER = 1, 2, 3


class MpStatesCheck(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("op", ctypes.c_int32), ("fingerprint", ctypes.c_uint64),
              ("pack", ctypes.c_void_p), ("pack_len", ctypes.c_uint64), ("cfg", ctypes.POINTER(MpConfig)),
              ("bank", ctypes.c_void_p), ("bank_rows", ctypes.c_int32), ("count", ctypes.c_int32),
              ("rows", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_bytes", ctypes.c_uint64),
              ("reserved", ctypes.c_uint64)]


# The rules of a check (include/mp_engine.h: MpStatesCheck).  A verdict is
# (rule, offset word): (0, 0) for a well-formed row.
RULE_OK = 0
RULE_STATE_RANGE = 1     # a render plane's byte is no state of the pack
RULE_STATE_LAYER = 2     # a render plane's byte is a state of another layer
RULE_TAIL_RANGE = 3      # aori, aalive, done, cont, started, step
RULE_AVATAR_CELL = 4     # a living avatar is off the map, or not where the tail says
RULE_AVATAR_STRAY = 5    # an avatar's state where the tail does not put that avatar
RULE_ORDERS = 6          # the cached visiting orders
RULE_LEVEL = 7           # a level's own rule; the offset word's top byte is its sub-code
RULE_NAMES = {RULE_OK: "well-formed", RULE_STATE_RANGE: "a plane byte that is no state of the pack",
              RULE_STATE_LAYER: "a state in another layer's plane", RULE_TAIL_RANGE: "a tail value out of range",
              RULE_AVATAR_CELL: "a living avatar that is not where the tail says",
              RULE_AVATAR_STRAY: "an avatar state where the tail does not put that avatar",
              RULE_ORDERS: "the cached visiting orders", RULE_LEVEL: "a level rule"}
# RULE_LEVEL sub-codes
LEVEL_BYTE_FIELD = 1     # + k: per-avatar byte array k of the tail outside the level's range (1 .. 14)
LEVEL_AUX_COUNT = 16
LEVEL_PLANE0, LEVEL_PLANE1 = 17, 18
LEVEL_MARKER_OFF_MAP, LEVEL_MARKER_CELL, LEVEL_FOLLOWER = 19, 20, 21
LEVEL_NAMES = {LEVEL_AUX_COUNT: "aux_count outside the level's table", LEVEL_PLANE0: "a plane byte the level cannot take",
               LEVEL_PLANE1: "a plane byte the level cannot take",
               LEVEL_MARKER_OFF_MAP: "a marker on the map whose position is no cell",
               LEVEL_MARKER_CELL: "a marker on the map whose cell of the marker plane is empty",
               LEVEL_FOLLOWER: "an avatar without its connected piece on its cell"}


def level_offset(sub: int, offset: int) -> int:
  """The offset word of a RULE_LEVEL verdict."""
  return (int(sub) << 24) | (int(offset) & 0xffffff)


class StateLayout:
  """What the bytes of a saved row are (an MpStateLayout request): `H`, `W`, `L` (render planes),
  `P`, `nstates`, `grid_planes` (render + hidden), `grid_bytes`, `grid_pad` (where the tail
  starts), `world_stride` (a row's bytes), `tail_bytes`, `max_frames`, `avatar_layer`,
  `player_block` (the matrix games' per-player block, else -1), `layout_version`, `fingerprint`,
  and `fields`: name -> (offset from grid_pad, element bytes, element count) of every member of
  the tail, as the library itself lists them."""

  def __init__(self, req: MpStateLayout, fields):
    self.H, self.W, self.L, self.P = req.map_h, req.map_w, req.num_layers, req.num_players
    self.nstates = req.num_states
    for n in _LAYOUT_INTS[5:]:
      setattr(self, n, int(getattr(req, n)))
    self.layout_version = int(req.layout_version)
    self.fingerprint = int(req.fingerprint)
    self.fields = {f.name.decode(): (int(f.offset), int(f.elem_bytes), int(f.count)) for f in fields}

  def field_offset(self, name: str, index: int = 0) -> int:
    """Byte offset in a row of element `index` of tail field `name`."""
    off, elem, count = self.fields[name]
    if not 0 <= index < count:
      raise IndexError(f"{name} has {count} elements")
    return self.grid_pad + off + elem * index

  def cell_offset(self, plane: int, x: int, y: int) -> int:
    """Byte offset in a row of cell (x, y) of plane `plane`."""
    return (plane * self.H + y) * self.W + x

  def describe(self, rule: int, offset: int) -> str:
    """A verdict in words: the rule, and the field or the plane and cell its offset names."""
    rule, offset = int(rule), int(offset) & 0xffffffff
    if rule == RULE_OK:
      return "well-formed"
    if rule == -1:
      return f"row index {offset - (1 << 32) if offset >= 1 << 31 else offset} is no row of the bank"
    what = RULE_NAMES.get(rule, f"rule {rule}")
    if rule == RULE_LEVEL:
      sub, offset = offset >> 24, offset & 0xffffff
      what = LEVEL_NAMES.get(sub, "a per-avatar byte outside the level's range")
    return f"rule {rule}: {what} at {self.where(offset)}"

  def where(self, offset: int) -> str:
    """The plane and cell, or the tail field and element, of byte `offset` of a row."""
    hw = self.H * self.W
    if offset < self.grid_planes * hw:
      plane, cell = divmod(offset, hw)
      kind = "plane" if plane < self.L else "hidden plane"
      return f"{kind} {plane} cell (x={cell % self.W}, y={cell // self.W})"
    if offset < self.grid_pad:
      return f"byte {offset} (behind the planes)"
    t = offset - self.grid_pad
    for name, (off, elem, count) in self.fields.items():
      if off <= t < off + elem * count:
        return f"{name}[{(t - off) // elem}]" if count > 1 else name
    return f"byte {offset}"


def _layout_request(L, handle, pack_bytes=None, num_players: int = 0, dev=None) -> StateLayout:
  fields = (MpStateField * 64)()
  req = MpStateLayout(ctypes.sizeof(MpStateLayout))
  req.fields = ctypes.cast(fields, ctypes.POINTER(MpStateField))
  req.fields_cap = 64
  keep = None
  if handle is None:
    keep = _host_config(pack_bytes, num_players, dev)
    req.pack, req.pack_len, req.cfg = ctypes.addressof(keep[0]), len(pack_bytes), ctypes.pointer(keep[1])
  _send(L, handle, req)
  return StateLayout(req, fields[:req.num_fields])


def _host_config(pack_bytes: bytes, num_players: int = 0, dev=None):
  """(pack buffer, MpConfig, options) of a host-only request; keep the tuple alive over the call."""
  cfg = MpConfig(ctypes.sizeof(MpConfig), 0, 1, 1, 0, 0, None, int(num_players))
  opts = None
  if dev:
    opts = MpDevOptions(ctypes.sizeof(MpDevOptions), max_composites=-1)
    for k, v in dev.items():
      setattr(opts, k, int(v))
    cfg.dev = ctypes.pointer(opts)
  return ctypes.create_string_buffer(pack_bytes, len(pack_bytes)), cfg, opts


def state_layout(pack_bytes: bytes, *, num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> StateLayout:
  """The layout of the rows an engine created on this pack would save, worked out on the host (an
  MpStateLayout request without an engine: no GPU needed)."""
  return _layout_request(load_library(), None, pack_bytes, num_players, dev)


def check_states_host(pack_bytes: bytes, rows, *, fingerprint: Optional[int] = None, which=None,
                      num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """Verdicts int32 [R, 2] = (rule, offset word) of host rows (uint8 [M, S] array) against the
  pack, by the library's host-only check (MP_CHECK_HOST: the kernel's own rule functions compiled
  for the host; no GPU needed).  `which`: the rows to judge (default: all).  `fingerprint`: the
  rows' (default: the pack's)."""
  layout, keep, bank, idx, _, count = _host_source("check_states_host", "judge", pack_bytes, rows, which, None,
                                                   num_players, dev)
  out = np.zeros((count, 2), np.int32)
  req = MpStatesCheck(ctypes.sizeof(MpStatesCheck), MP_CHECK_HOST,
                      layout.fingerprint if fingerprint is None else int(fingerprint))
  req.pack, req.pack_len, req.cfg = ctypes.addressof(keep[0]), len(pack_bytes), ctypes.pointer(keep[1])
  req.bank, req.bank_rows, req.count = bank.ctypes.data, int(bank.shape[0]), count
  req.rows = None if idx is None else idx.ctypes.data
  req.out, req.out_bytes = out.ctypes.data, out.nbytes
  _send(load_library(), None, req)
  return out


def _host_source(who: str, verb: str, pack_bytes: bytes, rows, which, players, num_players, dev):
  """What the host forms marshal alike: the host bank, `which` and `players` as int32 arrays (or
  None), the count.  Returns (layout, the pack and config to keep alive over the call, bank, which,
  players, count)."""
  bank = np.ascontiguousarray(rows, np.uint8)
  if bank.ndim != 2 or bank.shape[0] < 1:
    raise ValueError(f"{who}: rows must be a uint8 array [M, S]")
  keep = _host_config(pack_bytes, num_players, dev)
  layout = _layout_request(load_library(), None, pack_bytes, num_players, dev)
  if bank.shape[1] != layout.world_stride:
    raise ValueError(f"{who}: rows of {bank.shape[1]} bytes, the pack's are {layout.world_stride}")
  idx = None if which is None else np.ascontiguousarray(np.asarray(which).reshape(-1), np.int32)
  ply = None if players is None else np.ascontiguousarray(np.asarray(players).reshape(-1), np.int32)
  count = int(ply.size) if ply is not None else bank.shape[0] if idx is None else int(idx.size)
  if count < 1:
    raise ValueError(f"{who}: no rows to {verb}")
  return layout, keep, bank, idx, ply, count


def _view_host_source(who: str, verb: str, pack_bytes: bytes, rows, players, which, fingerprint, num_players, dev):
  """What ego_layer_host, hash_views_host and ego_planes_host marshal alike: the host bank, `which`
  and `players` as int32 arrays, the count.  Returns (layout, the result's leading shape — (R,) or
  (R, P) —, the request's source fields, what must stay alive over the call)."""
  layout, keep, bank, idx, ply, count = _host_source(who, verb, pack_bytes, rows, which, players, num_players, dev)
  if idx is not None and int(idx.size) != count:
    raise ValueError(f"{who}: which has {int(idx.size)} entries, players {count}")
  fields = dict(fingerprint=layout.fingerprint if fingerprint is None else int(fingerprint),
                pack=ctypes.addressof(keep[0]), pack_len=len(pack_bytes),
                cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p), bank=bank.ctypes.data,
                bank_rows=int(bank.shape[0]), rows=None if idx is None else idx.ctypes.data,
                players=None if ply is None else ply.ctypes.data, count=count)
  return layout, (count,) + ((layout.P,) if ply is None else ()), fields, (keep, bank, idx, ply)


def ego_layer_host(pack_bytes: bytes, rows, players=None, *, which=None, fingerprint: Optional[int] = None,
                   num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """EGO_LAYER of host rows (uint8 [M, S] array) by the library's host-only form (MP_EGO_HOST: the
  kernels' own value function compiled for the host; no GPU needed).  `which`: the rows to draw, in
  order, repeats allowed (default: all).  `players` None: int32 [R, P, VH, VW, L], every viewer of
  each row; else R ints, and the result is int32 [R, VH, VW, L], the view of player players[i] of
  the i-th drawn row.  `fingerprint`: the rows' (default: the pack's)."""
  layout, lead, src, _alive = _view_host_source("ego_layer_host", "draw", pack_bytes, rows, players, which,
                                                fingerprint, num_players, dev)
  out = np.zeros(lead + _view_window(pack_bytes) + (layout.L,), np.int32)
  ego_layer_request(load_library(), None, MP_EGO_HOST, dst=out.ctypes.data, dst_bytes=out.nbytes, **src)
  return out


# The hash of world records (include/mp_engine.h: MpStatesHash), carried by mp_snapshot
MP_HASH_ROWS, MP_HASH_WORLDS, MP_HASH_HOST, MP_HASH_MASK = 1, 2, 3, 4
MP_HASH_CUSTOM, MP_HASH_PLAYER_BLOCK = 1, 2
# the tail fields the default spec leaves out: the destination engine's bookkeeping, and the
# cached visiting orders, which may be present or absent
HASH_BOOKKEEPING = ("ctr", "reward_fx", "orders_step", "next_orders")


class MpStatesHash(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("op", ctypes.c_int32), ("fingerprint", ctypes.c_uint64),
              ("pack", ctypes.c_void_p), ("pack_len", ctypes.c_uint64), ("cfg", ctypes.POINTER(MpConfig)),
              ("bank", ctypes.c_void_p), ("bank_rows", ctypes.c_int32), ("count", ctypes.c_int32),
              ("rows", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_bytes", ctypes.c_uint64),
              ("plane_mask", ctypes.c_uint64), ("field_mask", ctypes.c_uint32), ("flags", ctypes.c_int32),
              ("reserved", ctypes.c_uint64)]


def hash_spec(layout: StateLayout, planes=None, fields=None):
  """(plane_mask, field_mask, flags) of an MpStatesHash request.  `planes`: an iterable of grid
  plane indices; `fields`: an iterable of tail field names (`layout.fields`' keys), plus
  "player_block" for the level's block.  Both None: the default spec, "the state".  If one is
  given, a None other means none of them.  ValueError for a plane or a name the layout has not."""
  if planes is None and fields is None:
    return 0, 0, 0
  plane_mask, field_mask, flags = 0, 0, MP_HASH_CUSTOM
  for p in (() if planes is None else planes):
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= int(p) < layout.grid_planes:
      raise ValueError(f"hash: {p!r} is no grid plane (the rows have {layout.grid_planes})")
    if int(p) >= 64:
      raise ValueError("hash: a custom spec names planes below 64")
    plane_mask |= 1 << int(p)
  names = list(layout.fields)
  if isinstance(fields, str):
    fields = (fields,)
  for f in (() if fields is None else fields):
    if f == "player_block":
      if layout.player_block < 0:
        raise ValueError("hash: this level keeps no player block")
      flags |= MP_HASH_PLAYER_BLOCK
    elif f in names:
      field_mask |= 1 << names.index(f)
    else:
      raise ValueError(f"hash: {f!r} is no field of the tail; it has {names} (and 'player_block')")
  if plane_mask == 0 and field_mask == 0 and not flags & MP_HASH_PLAYER_BLOCK:
    raise ValueError("hash: the spec includes no byte")
  return plane_mask, field_mask, flags


def _hash_request(op: int, spec, fingerprint: int = 0) -> MpStatesHash:
  req = MpStatesHash(ctypes.sizeof(MpStatesHash), op, int(fingerprint))
  req.plane_mask, req.field_mask, req.flags = spec
  return req


def state_hash_mask(pack_bytes: bytes, planes=None, fields=None, num_players: int = 0,
                    dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """The byte mask of a hash spec, uint8 [S]: 0xFF where a byte of a row counts (MP_HASH_MASK
  without an engine: no GPU needed).  `planes`, `fields`: see `hash_spec`."""
  L = load_library()
  layout = _layout_request(L, None, pack_bytes, num_players, dev)
  keep = _host_config(pack_bytes, num_players, dev)
  out = np.zeros(layout.world_stride, np.uint8)
  req = _hash_request(MP_HASH_MASK, hash_spec(layout, planes, fields))
  req.pack, req.pack_len, req.cfg = ctypes.addressof(keep[0]), len(pack_bytes), ctypes.pointer(keep[1])
  req.out, req.out_bytes = out.ctypes.data, out.nbytes
  _send(L, None, req)
  return out


def hash_states_host(pack_bytes: bytes, rows, which=None, planes=None, fields=None, num_players: int = 0,
                     dev: Optional[Dict[str, int]] = None, fingerprint: Optional[int] = None,
                     out: Optional[np.ndarray] = None) -> np.ndarray:
  """int64 [R]: the 64-bit state hash (the u64's bits) of host rows (uint8 [M, S] array) by the
  library's host-only form (MP_HASH_HOST: the kernel's own function compiled for the host; no GPU
  needed).  `which`: the rows to hash, in order, repeats allowed (default: all); an index outside
  the bank raises ValueError and leaves its element of `out` as it was.  `planes`, `fields`: the
  spec (`hash_spec`; both None: "the state").  `fingerprint`: the rows' (default: the pack's).
  Hashes compare only between rows of one fingerprint, hashed with one spec."""
  layout, keep, bank, idx, _, count = _host_source("hash_states_host", "hash", pack_bytes, rows, which, None,
                                                   num_players, dev)
  if out is None:
    out = np.zeros(count, np.int64)
  elif (not isinstance(out, np.ndarray) or out.dtype != np.int64 or out.shape != (count,) or
        not out.flags.c_contiguous):
    raise ValueError(f"hash_states_host: out must be a contiguous int64 array of shape {(count,)}")
  req = _hash_request(MP_HASH_HOST, hash_spec(layout, planes, fields),
                      layout.fingerprint if fingerprint is None else fingerprint)
  req.pack, req.pack_len, req.cfg = ctypes.addressof(keep[0]), len(pack_bytes), ctypes.pointer(keep[1])
  req.bank, req.bank_rows, req.count = bank.ctypes.data, int(bank.shape[0]), count
  req.rows = None if idx is None else idx.ctypes.data
  req.out, req.out_bytes = out.ctypes.data, out.nbytes
  _send(load_library(), None, req)
  return out


# The hash of each player's view (include/mp_engine.h: MpViewHash), carried by mp_snapshot
MP_VIEWHASH_DRAW, MP_VIEWHASH_REGISTER, MP_VIEWHASH_HOST = 1, 2, 3


class MpViewHash(ctypes.Structure):
  _fields_ = _VIEW_CLASSES + [("reserved", ctypes.c_int32), ("reserved2", ctypes.c_uint64 * 3)]


def view_hash_request(L, handle, op: int, **fields) -> MpViewHash:
  """Runs one MpViewHash request on engine `handle` (None: the host form); raises like every call.
  The returned request's `num_ids` is the length a class table must have."""
  return _request(L, handle, MpViewHash, (int(op),), fields)


def view_layer_mask(layers, num_layers: int) -> int:
  """MpViewHash.layer_mask of `layers`: None (every layer: 0) or an iterable of layer indices.
  ValueError for an index the view has not, and for an empty choice."""
  if layers is None:
    return 0
  if isinstance(layers, (int, np.integer)) and not isinstance(layers, bool):
    layers = (layers,)
  mask = 0
  for l in layers:
    if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or not 0 <= int(l) < num_layers:
      raise ValueError(f"hash_views: {l!r} is no layer of the view (it has {num_layers})")
    mask |= 1 << int(l)
  if mask == 0:
    raise ValueError("hash_views: layers includes no layer (None means every layer)")
  return mask


def _view_classes(classes, num_ids: int) -> np.ndarray:
  """`classes` as the contiguous int32 [num_ids] host table of an MpViewHash request."""
  a = np.asarray(classes)
  if a.ndim != 1 or a.size != num_ids or not np.issubdtype(a.dtype, np.integer):
    raise ValueError(f"hash_views: classes must be {num_ids} integers, one per layer id (num_layer_ids); got "
                     f"{a.dtype} {a.shape}")
  return np.ascontiguousarray(a, np.int32)


def num_layer_ids_host(pack_bytes: bytes, *, num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> int:
  """The number of ids "LAYER" and "EGO_LAYER" can hold for this pack, 1 + the largest: the length of
  a `classes` table of `hash_views_host` (an MpViewHash question without an engine: no GPU needed)."""
  keep = _host_config(pack_bytes, num_players, dev)
  req = view_hash_request(load_library(), None, MP_VIEWHASH_HOST, pack=ctypes.addressof(keep[0]),
                          pack_len=len(pack_bytes), cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p))
  return int(req.num_ids)


def hash_views_host(pack_bytes: bytes, rows, players=None, *, which=None, layers=None, classes=None,
                    fingerprint: Optional[int] = None, num_players: int = 0,
                    dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """The 64-bit hash (the u64's bits, int64) of each player's view of host rows (uint8 [M, S]
  array) by the library's host-only form (MP_VIEWHASH_HOST: the kernels' own function compiled for
  the host; no GPU needed).  `which`: the rows to hash, in order, repeats allowed (default: all).
  `players` None: int64 [R, P], every viewer of each row; else R ints, and the result is int64 [R],
  the hash of player players[i] of the i-th row.  `layers`: the layer indices that count (None:
  all); `classes`: int32 [num_layer_ids_host(pack)] mapping every id to its class (None: the ids
  themselves).  `fingerprint`: the rows' (default: the pack's)."""
  layout, lead, src, _alive = _view_host_source("hash_views_host", "hash", pack_bytes, rows, players, which,
                                                fingerprint, num_players, dev)
  cls = None if classes is None else _view_classes(classes, num_layer_ids_host(pack_bytes, num_players=num_players,
                                                                               dev=dev))
  out = np.zeros(lead, np.int64)
  view_hash_request(load_library(), None, MP_VIEWHASH_HOST, layer_mask=view_layer_mask(layers, layout.L),
                    classes=None if cls is None else cls.ctypes.data, classes_len=0 if cls is None else int(cls.size),
                    dst=out.ctypes.data, dst_bytes=out.nbytes, **src)
  return out


# Class-indicator feature planes of each player's view (include/mp_engine.h: MpEgoPlanes), carried
# by mp_snapshot
MP_EGOPLANES_DRAW, MP_EGOPLANES_REGISTER, MP_EGOPLANES_HOST = 1, 2, 3
EGO_PLANES_MAX_CLASSES = 64


class MpEgoPlanes(ctypes.Structure):
  _fields_ = _VIEW_CLASSES + [("num_classes", ctypes.c_int32), ("facing", ctypes.c_int32),
                              ("reserved", ctypes.c_int32), ("reserved2", ctypes.c_uint64 * 3)]


def ego_planes_request(L, handle, op: int, **fields) -> MpEgoPlanes:
  """Runs one MpEgoPlanes request on engine `handle` (None: the host form); raises like every call.
  The returned request's `num_ids` is the length a class table must have."""
  return _request(L, handle, MpEgoPlanes, (int(op),), fields)


def _plane_classes(classes, num_ids: int, num_classes) -> Tuple[np.ndarray, int]:
  """(`classes` as the contiguous int32 [num_ids] host table of an MpEgoPlanes request, C).  C is
  `num_classes`, by default 1 + the largest entry; every entry must lie in [-1, C), 1 <= C <= 64."""
  a = np.asarray(classes)
  if a.ndim != 1 or a.size != num_ids or not np.issubdtype(a.dtype, np.integer):
    raise ValueError(f"ego_planes: classes must be {num_ids} integers, one per layer id (num_layer_ids); got "
                     f"{a.dtype} {a.shape}")
  C = int(a.max()) + 1 if num_classes is None else int(num_classes)
  if not 1 <= C <= EGO_PLANES_MAX_CLASSES:
    raise ValueError(f"ego_planes: num_classes {C} is outside [1, {EGO_PLANES_MAX_CLASSES}]"
                     + (" (by default 1 + the largest entry of classes)" if num_classes is None else ""))
  bad = np.nonzero((a < -1) | (a >= C))[0]
  if bad.size:
    raise ValueError(f"ego_planes: classes[{int(bad[0])}] = {int(a[bad[0]])} is outside [-1, num_classes = {C})")
  return np.ascontiguousarray(a, np.int32), C


def _view_window(pack_bytes: bytes) -> Tuple[int, int]:
  """(VH, VW) of the pack's per-agent view."""
  from . import lower, pack as pack_lib
  hdr = pack_lib.loads(pack_bytes)["hdr"]
  return (int(hdr[lower.HDR_VF]) + int(hdr[lower.HDR_VB]) + 1, int(hdr[lower.HDR_VL]) + int(hdr[lower.HDR_VR]) + 1)


def layer_id_names_host(pack_bytes: bytes, *, num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> Tuple[str, ...]:
  """What every id of "LAYER" and "EGO_LAYER" shows: a tuple of `num_layer_ids_host(pack)` strings,
  "" for id 0 (nothing) and the name of sprite i - 1 for id i ("OutOfBounds" is id 1).  No GPU."""
  from . import pack as pack_lib
  names = bytes(pack_lib.loads(pack_bytes)["sprite_names"]).split(b"\0")[:-1]
  n = num_layer_ids_host(pack_bytes, num_players=num_players, dev=dev)
  return ("",) + tuple(names[i].decode() if i < len(names) else "" for i in range(n - 1))


def ego_planes_host(pack_bytes: bytes, rows, classes, players=None, *, which=None, layers=None, facing: bool = False,
                    num_classes: Optional[int] = None, fingerprint: Optional[int] = None, num_players: int = 0,
                    dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """The class and facing planes of each player's view of host rows (uint8 [M, S] array) by the
  library's host-only form (MP_EGOPLANES_HOST: the kernels' own functions compiled for the host;
  no GPU needed): uint8 [R, P, C', VH, VW], or [R, C', VH, VW] with `players` (R ints: player
  players[i] of the i-th row).  `classes`: `num_layer_ids_host(pack)` ints in [-1, C) mapping every
  id to its class (-1: none); C = `num_classes`, by default 1 + the largest; C' = C + 4 with
  `facing`.  `which`: the rows, in order, repeats allowed (default: all).  `layers`: the layer
  indices that count (None: all).  `fingerprint`: the rows' (default: the pack's)."""
  layout, lead, src, _alive = _view_host_source("ego_planes_host", "draw", pack_bytes, rows, players, which,
                                                fingerprint, num_players, dev)
  cls, C = _plane_classes(classes, num_layer_ids_host(pack_bytes, num_players=num_players, dev=dev), num_classes)
  mask = view_layer_mask(layers, layout.L)
  out = np.zeros(lead + (C + (4 if facing else 0),) + _view_window(pack_bytes), np.uint8)
  ego_planes_request(load_library(), None, MP_EGOPLANES_HOST, layer_mask=mask, classes=cls.ctypes.data,
                     classes_len=int(cls.size), num_classes=C, facing=int(bool(facing)), dst=out.ctypes.data,
                     dst_bytes=out.nbytes, **src)
  return out


# WORLD.LAYER and the world planes: the world ops of MpEgoLayer and MpEgoPlanes (include/mp_engine.h),
# the whole map in place of the viewers' windows
MP_EGO_WORLD_DRAW, MP_EGO_WORLD_REGISTER, MP_EGO_WORLD_HOST = 4, 5, 6
MP_EGOPLANES_WORLD_DRAW, MP_EGOPLANES_WORLD_REGISTER, MP_EGOPLANES_WORLD_HOST = 4, 5, 6
OBS_WORLD_LAYER = -3   # no MpObsKind: the Python layers' handle for the "WORLD.LAYER" leaf


def _world_map(pack_bytes: bytes) -> Tuple[int, int]:
  """(H, W) of the pack's map."""
  from . import lower, pack as pack_lib
  hdr = pack_lib.loads(pack_bytes)["hdr"]
  return int(hdr[lower.HDR_H]), int(hdr[lower.HDR_W])


def _world_host_source(who: str, pack_bytes: bytes, rows, which, fingerprint, num_players, dev):
  layout, lead, src, alive = _view_host_source(who, "draw", pack_bytes, rows, None, which, fingerprint,
                                               num_players, dev)
  return layout, lead[:1], src, alive


def num_world_layer_ids_host(pack_bytes: bytes, *, num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> int:
  """The number of ids "WORLD.LAYER" can hold for this pack, 1 + the largest: the length of a
  `classes` table of `world_planes_host` (an MpEgoPlanes question without an engine: no GPU needed)."""
  keep = _host_config(pack_bytes, num_players, dev)
  req = ego_planes_request(load_library(), None, MP_EGOPLANES_WORLD_HOST, pack=ctypes.addressof(keep[0]),
                           pack_len=len(pack_bytes), cfg=ctypes.cast(ctypes.pointer(keep[1]), ctypes.c_void_p))
  return int(req.num_ids)


def world_layer_id_names_host(pack_bytes: bytes, *, num_players: int = 0,
                              dev: Optional[Dict[str, int]] = None) -> Tuple[str, ...]:
  """What every id of "WORLD.LAYER" shows: "" for id 0 (nothing) and the name of sprite i - 1 for id
  i, after the WORLD's sprite map.  No GPU."""
  from . import pack as pack_lib
  names = bytes(pack_lib.loads(pack_bytes)["sprite_names"]).split(b"\0")[:-1]
  n = num_world_layer_ids_host(pack_bytes, num_players=num_players, dev=dev)
  return ("",) + tuple(names[i].decode() if i < len(names) else "" for i in range(n - 1))


def world_layer_host(pack_bytes: bytes, rows, *, which=None, fingerprint: Optional[int] = None,
                     num_players: int = 0, dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """WORLD.LAYER — the layer view of the whole map, int32 [R, H, W, L], north up — of host rows
  (uint8 [M, S] array) by the library's host-only form (MP_EGO_WORLD_HOST: the kernel's own value
  function compiled for the host; no GPU needed).  `which`: the rows to draw, in order, repeats
  allowed (default: all).  `fingerprint`: the rows' (default: the pack's)."""
  layout, lead, src, _alive = _world_host_source("world_layer_host", pack_bytes, rows, which, fingerprint,
                                                 num_players, dev)
  out = np.zeros(lead + _world_map(pack_bytes) + (layout.L,), np.int32)
  ego_layer_request(load_library(), None, MP_EGO_WORLD_HOST, dst=out.ctypes.data, dst_bytes=out.nbytes, **src)
  return out


def world_planes_host(pack_bytes: bytes, rows, classes, *, which=None, layers=None, facing: bool = False,
                      num_classes: Optional[int] = None, fingerprint: Optional[int] = None, num_players: int = 0,
                      dev: Optional[Dict[str, int]] = None) -> np.ndarray:
  """The class and facing planes of the whole map of host rows (uint8 [M, S] array) by the
  library's host-only form (MP_EGOPLANES_WORLD_HOST; no GPU needed): uint8 [R, C', H, W].  `classes`:
  `num_world_layer_ids_host(pack)` ints in [-1, C) mapping every id of "WORLD.LAYER" to its class
  (-1: none); C = `num_classes`, by default 1 + the largest; C' = C + 4 with `facing` (plane C + d:
  a living avatar that faces d stands there, 0 = N).  `which`: the rows, in order, repeats allowed
  (default: all).  `layers`: the layer indices that count (None: all)."""
  layout, lead, src, _alive = _world_host_source("world_planes_host", pack_bytes, rows, which, fingerprint,
                                                 num_players, dev)
  cls, C = _plane_classes(classes, num_world_layer_ids_host(pack_bytes, num_players=num_players, dev=dev),
                          num_classes)
  mask = view_layer_mask(layers, layout.L)
  out = np.zeros(lead + (C + (4 if facing else 0),) + _world_map(pack_bytes), np.uint8)
  ego_planes_request(load_library(), None, MP_EGOPLANES_WORLD_HOST, layer_mask=mask, classes=cls.ctypes.data,
                     classes_len=int(cls.size), num_classes=C, facing=int(bool(facing)), dst=out.ctypes.data,
                     dst_bytes=out.nbytes, **src)
  return out


# Whom each player sees and whom it could zap (include/mp_engine.h: MpAvatarIds), carried by mp_snapshot
MP_AVATARIDS_DRAW, MP_AVATARIDS_REGISTER, MP_AVATARIDS_HOST = 1, 2, 3


class MpAvatarIds(ctypes.Structure):
  _fields_ = (_VIEW_HEAD + [("reserved", ctypes.c_int32)] + _VIEW_PACK +
              [("dst_zap", ctypes.c_void_p), ("dst_zap_bytes", ctypes.c_uint64), ("reserved2", ctypes.c_uint64 * 3)])


def avatar_ids_request(L, handle, op: int, **fields) -> MpAvatarIds:
  """Runs one MpAvatarIds request on engine `handle` (None: the host form); raises like every call."""
  return _request(L, handle, MpAvatarIds, (int(op),), fields)


def has_zapper(pack_bytes: bytes) -> bool:
  """Does the pack's level carry the reference's Zapper (clean_up, commons_harvest, territory,
  externality_mushrooms)?  Without one there is no AVATAR_IDS_IN_RANGE_TO_ZAP."""
  from . import pack as pack_lib
  return "zapper_i32" in pack_lib.loads(pack_bytes)


def avatar_ids_host(pack_bytes: bytes, rows, players=None, *, which=None, view: bool = True, zap: bool = True,
                    fingerprint: Optional[int] = None, num_players: int = 0, dev: Optional[Dict[str, int]] = None):
  """AVATAR_IDS_IN_VIEW and AVATAR_IDS_IN_RANGE_TO_ZAP of host rows (uint8 [M, S] array) by the
  library's host-only form (MP_AVATARIDS_HOST: the kernels' own functions compiled for the host; no
  GPU needed).  Returns (in_view, in_range): int32 [R, P, P] each, row p the 0/1 vector of viewer p
  over the player slots, or [R, P] with `players` (R ints: player players[i] of the i-th row);
  None in the place of one not asked for (`view`, `zap`).  `which`: the rows, in order, repeats
  allowed (default: all).  A level without a Zapper raises ValueError for `zap`.  `fingerprint`:
  the rows' (default: the pack's)."""
  if not view and not zap:
    raise ValueError("avatar_ids_host: neither view nor zap is asked for")
  layout, lead, src, _alive = _view_host_source("avatar_ids_host", "draw", pack_bytes, rows, players, which,
                                                fingerprint, num_players, dev)
  out_v = np.zeros(lead + (layout.P,), np.int32) if view else None
  out_z = np.zeros(lead + (layout.P,), np.int32) if zap else None
  avatar_ids_request(load_library(), None, MP_AVATARIDS_HOST,
                     dst=None if out_v is None else out_v.ctypes.data, dst_bytes=0 if out_v is None else out_v.nbytes,
                     dst_zap=None if out_z is None else out_z.ctypes.data,
                     dst_zap_bytes=0 if out_z is None else out_z.nbytes, **src)
  return out_v, out_z


# Action sequences (include/mp_engine.h: MpStepMany), carried by mp_restore
STEP_MANY_MAX = 4096   # MP_STEP_MANY_MAX
# the five kinds step_many returns by name, in MpStepMany.per_step's order
STEP_MANY_NAMES = {"reward": OBS_REWARD, "collective_reward": OBS_COLLECTIVE_REWARD,
                   "step_type": OBS_STEP_TYPE, "discount": OBS_DISCOUNT, "events": OBS_EVENTS}
STEP_MANY_KINDS = tuple(STEP_MANY_NAMES)
_STEP_MANY_KIND_OF = STEP_MANY_NAMES


class MpStepMany(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("steps", ctypes.c_int32),
              ("fields", ctypes.c_int32), ("reserved", ctypes.c_int32),
              ("actions", ctypes.c_void_p), ("actions_step_bytes", ctypes.c_uint64),
              ("per_step", ctypes.c_void_p * 5), ("per_step_bytes", ctypes.c_uint64 * 5)]


# ... with per-step rows of any non-pixel kind (MpStepTrajectory)
class MpStepRow(ctypes.Structure):
  _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("rows", ctypes.c_void_p),
              ("step_bytes", ctypes.c_uint64)]


class MpStepTrajectory(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("steps", ctypes.c_int32),
              ("fields", ctypes.c_int32), ("num_rows", ctypes.c_int32),
              ("actions", ctypes.c_void_p), ("actions_step_bytes", ctypes.c_uint64),
              ("rows", ctypes.POINTER(MpStepRow))]


# MpStepRow.kind of the per-step world states (MP_STEP_ROW_STATE): no observation kind
STEP_ROW_STATE = 0x100
# ... and of the per-step state hashes (MP_STEP_ROW_HASH)
STEP_ROW_HASH = 0x102

# the kinds a step_many request may stack per step: every kind but the pixel ones
STEP_ROW_KINDS = tuple(k for k in range(OBS_RGB_POOL8 + 1) if k not in PIXEL_KINDS)


def step_row(shapes, key):
  """A key of step_many's result (one of STEP_MANY_NAMES, or an OBS_* kind) as (kind, shape of
  one world's part of a row, dtype), from `shapes` (Engine.shapes)."""
  kind = STEP_MANY_NAMES.get(key, key)
  shape, dtype = shapes[kind]
  return kind, tuple(shape[1:]), dtype


def check_step_rows(observations, *, steps: Optional[int] = None, shapes=None, out=None,
                    taken=()) -> tuple:
  """The kind, shape and dtype rules of Engine.step_many's observations=, without an engine:
  returns the kinds as a tuple of ints.  Each is an OBS_* kind other than a pixel kind, named
  once (`taken`: kinds the call already stacks under keep= / events=).  With `steps` = K,
  `shapes` (kind -> (shape, dtype), as Engine.shapes) and `out` (kind -> tensor) every given
  tensor must have the kind's dtype and shape (K,) + shape, with steps that do not overlap.
  ValueError otherwise."""
  kinds = []
  for kind in observations:
    if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)):
      raise ValueError(f"step_many: observations= takes OBS_* kinds (got {kind!r})")
    kind = int(kind)
    if kind in PIXEL_KINDS:
      raise ValueError(f"step_many: kind {kind} is a pixel kind; a K-step launch draws no frames. "
                       "Intermediate frames are what step() with a rollout ring "
                       "(bind_ring) writes")
    if kind not in STEP_ROW_KINDS:
      raise ValueError(f"step_many: {kind} is no observation kind")
    if kind in kinds or kind in taken:
      raise ValueError(f"step_many: kind {kind} is named twice")
    kinds.append(kind)
  if out is not None and shapes is not None and steps is not None:
    for kind in kinds:
      buf = out.get(kind)
      if buf is None:
        continue
      shape, dtype = shapes[kind]
      want = (int(steps),) + tuple(int(d) for d in shape)
      if (not hasattr(buf, "stride") or str(buf.dtype) != str(dtype) or
          tuple(int(d) for d in buf.shape) != want):
        raise ValueError(f"step_many: out[{kind}] must be a {dtype} tensor of shape {want} "
                         f"(got {getattr(buf, 'dtype', type(buf))} {tuple(getattr(buf, 'shape', ()))})")
      _step_distance(buf, f"out[{kind}]")
  return tuple(kinds)


def check_step_many(shape, dtype, num_worlds: int, num_players: int, *, repeat=None,
                    num_fields: Optional[int] = None) -> int:
  """The shape and dtype rules of Engine.step_many's actions, without an engine: returns K.
  [K, N, P] integers (or [K, N, P, A] with num_fields = A), or one block [N, P] ([N, P, A]) with
  repeat = K; 1 <= K <= STEP_MANY_MAX.  ValueError otherwise."""
  shape = tuple(int(d) for d in shape)
  block = (num_worlds, num_players) + ((int(num_fields),) if num_fields else ())
  name = str(dtype)
  if "int" not in name or "float" in name:
    raise ValueError(f"step_many: actions must hold integers (got {name})")
  if repeat is not None:
    if shape != block:
      raise ValueError(f"step_many: with repeat= the actions are one block of shape {block} (got {shape})")
    K = int(repeat)
  else:
    if len(shape) != len(block) + 1 or shape[1:] != block:
      raise ValueError(f"step_many: actions must have shape (K,) + {block} (got {shape})")
    K = shape[0]
  if not 1 <= K <= STEP_MANY_MAX:
    raise ValueError(f"step_many: K = {K} is outside [1, {STEP_MANY_MAX}]")
  return K


# ... under a device mask that says, per step and per world, whether the world runs (MpStepActive)
class MpStepActive(ctypes.Structure):
  _fields_ = MpStepTrajectory._fields_ + [("active", ctypes.c_void_p), ("active_step_bytes", ctypes.c_uint64),
                                          ("reserved", ctypes.c_uint64 * 5)]


def check_step_active(active, steps: int, num_worlds: int):
  """The dtype and shape rules of the active= mask of Engine.step / Engine.step_many, without an
  engine: bytes (uint8) or booleans of shape [K, N] with K = `steps`, or [N] (the same row at
  every step).  A torch tensor is taken as it is and may be a column slice [:, a:b] of a wider
  one (each row contiguous, rows at least N apart); a numpy array must be uint8 or bool; a
  nested list may hold booleans or integers.  Returns (mask, step_bytes): the tensor itself, or
  a contiguous numpy uint8 array for host data, and the distance between two steps' rows in
  bytes (0: one row for every step).  ValueError otherwise."""
  K, N = int(steps), int(num_worlds)
  def bad(got):
    return ValueError(f"active= must be a uint8 or bool mask of shape ({K}, {N}) or ({N},) (got {got})")
  if hasattr(active, "data_ptr"):   # a torch tensor
    name, shape = str(active.dtype), tuple(int(d) for d in active.shape)
    if name not in ("torch.uint8", "torch.bool") or shape not in ((K, N), (N,)):
      raise bad(f"{name} {shape}")
    if N > 1 and int(active.stride(-1)) != 1:
      raise ValueError(f"active=: a step's row must be contiguous (strides {tuple(active.stride())})")
    if len(shape) == 1:
      return active, 0
    if K > 1 and int(active.stride(0)) < N:
      raise ValueError(f"active=: the steps' rows overlap (stride {int(active.stride(0))} < {N})")
    return active, (int(active.stride(0)) if K > 1 else N)
  listed = not isinstance(active, np.ndarray)
  a = np.asarray(active)
  ok = a.dtype in (np.uint8, np.bool_) or (listed and a.dtype.kind in "iu")
  if not ok or a.shape not in ((K, N), (N,)):
    raise bad(f"{a.dtype} {a.shape}")
  a = np.ascontiguousarray(a != 0, np.uint8)
  return a, (0 if a.ndim == 1 else N)


# ... in which a world that ends its episode, or is paid, stops there (MpStepUntil)
MP_STOP_LAST, MP_STOP_REWARD = 1, 2
STOP_NAMES = {"last": MP_STOP_LAST, "reward": MP_STOP_REWARD}


class MpStepUntil(ctypes.Structure):
  # (MpStepActive without its `reserved`, where the new fields begin)
  _fields_ = MpStepActive._fields_[:-1] + [("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                                           ("stopped", ctypes.c_void_p), ("ran", ctypes.c_void_p),
                                           ("returns", ctypes.c_void_p), ("gamma", ctypes.c_double),
                                           ("reserved", ctypes.c_uint64 * 5)]


def check_step_until(num_worlds: int, num_players: int, *, until=None, stopped=None, ran=None,
                     returns=None, gamma=1.0, device=None) -> int:
  """The rules of the until=, stopped=, returns= and gamma= arguments of Engine.step_many (and of
  the ran / returns tensors it reuses from out=), without an engine.  until: None, "last",
  "reward" or an iterable of these names.  stopped: a contiguous uint8 tensor [N].  ran: a
  contiguous int32 tensor [N].  returns: None, a bool, or a contiguous float64 tensor [N, P].
  gamma: a finite number.  device: where the tensors must live (None: not checked).  Returns the
  MP_STOP_* bits of until=.  ValueError, naming the argument, otherwise."""
  N, P = int(num_worlds), int(num_players)
  try:
    names = () if until is None else (until,) if isinstance(until, str) else tuple(until)
  except TypeError:
    raise ValueError(f"until= knows {tuple(STOP_NAMES)} or an iterable of them (got {until!r})") from None
  stop = 0
  for name in names:
    if not isinstance(name, str) or name not in STOP_NAMES:
      raise ValueError(f"until= knows {tuple(STOP_NAMES)} (got {name!r})")
    stop |= STOP_NAMES[name]
  def tensor(value, arg, dtype, shape):
    if not hasattr(value, "data_ptr"):
      raise ValueError(f"{arg}= must be a {dtype} tensor of shape {shape} (got {type(value).__name__})")
    got = tuple(int(d) for d in value.shape)
    if str(value.dtype) != f"torch.{dtype}" or got != shape:
      raise ValueError(f"{arg}= must be a {dtype} tensor of shape {shape} (got {value.dtype} {got})")
    if not value.is_contiguous():
      raise ValueError(f"{arg}= must be contiguous (strides {tuple(value.stride())})")
    if device is not None and value.device != device:
      raise ValueError(f"{arg}= lives on {value.device}, the engine on {device}")
  if stopped is not None:
    tensor(stopped, "stopped", "uint8", (N,))
  if ran is not None:
    tensor(ran, "ran", "int32", (N,))
  if returns is not None and not isinstance(returns, (bool, np.bool_)):
    tensor(returns, "returns", "float64", (N, P))
  try:
    finite = bool(np.isfinite(float(gamma)))
  except (TypeError, ValueError):
    finite = False
  if not finite:
    raise ValueError(f"gamma= must be a finite number (got {gamma!r})")
  return stop


# ... launched with one wave per entry of a device list of world indices (MpStepListed)
class MpStepListed(ctypes.Structure):
  _fields_ = MpStepUntil._fields_ + [("worlds", ctypes.c_void_p), ("count", ctypes.c_int32),
                                     ("reserved2", ctypes.c_int32), ("reserved3", ctypes.c_uint64 * 3)]


def check_step_listed(worlds, num_worlds: int, num_players: int, *, actions=None, repeat=None,
                      num_fields: Optional[int] = None, active=None, lengths=None, out=None,
                      shapes=None) -> int:
  """The rules of the worlds= list of Engine.step / Engine.step_many, and of the tensors that go with
  it, without an engine: returns M, the number of entries.  worlds: 1-D integers (a tensor, an
  array or a list), 1 <= M <= num_worlds (more entries than worlds must repeat one); the VALUES are
  checked on the device.  Everything else the call takes per world has M columns, not N — actions
  ([K, M, P], or [M, P] with repeat=K; anything with .shape and .dtype, or array-like), active
  ([K, M] or [M]), lengths (integers [M]) and, with `shapes` (kind -> (shape, dtype), as
  Engine.shapes), every tensor of `out` (a step_many result: rows (K, M) + shape[1:], "ran" [M],
  "returns" [M, P]; its "stopped" stays [N]).  ValueError otherwise."""
  N, P = int(num_worlds), int(num_players)
  if hasattr(worlds, "data_ptr"):
    name, shape = str(worlds.dtype), tuple(int(d) for d in worlds.shape)
    ok = name in ("torch.int8", "torch.int16", "torch.int32", "torch.int64", "torch.uint8")
  else:
    w = np.asarray(worlds)
    name, shape = str(w.dtype), w.shape
    ok = np.issubdtype(w.dtype, np.integer) and w.dtype != np.bool_
  if len(shape) == 1 and int(shape[0]) == 0:   # (an empty list has no dtype to speak of)
    raise ValueError("worlds= names no world")
  if not ok or len(shape) != 1:
    raise ValueError(f"worlds= must be 1-D integers, one world index per entry (got {name} {tuple(shape)})")
  M = int(shape[0])
  if M < 1:
    raise ValueError("worlds= names no world")
  if M > N:
    raise ValueError(f"worlds= has {M} entries for {N} worlds: more entries than worlds must repeat one")
  K = None
  if actions is not None:
    a = actions if hasattr(actions, "shape") and hasattr(actions, "dtype") else np.asarray(actions)
    try:
      K = check_step_many(a.shape, a.dtype, M, P, repeat=repeat, num_fields=num_fields)
    except ValueError as e:
      raise ValueError(f"{e}; with worlds= the actions have one column per entry ({M}), not per world") from None
  elif repeat is not None:
    K = int(repeat)
  if active is not None:
    if K is None:
      raise ValueError("check_step_listed: active= is checked against the actions' K")
    check_step_active(active, K, M)
  if lengths is not None:
    n = lengths if hasattr(lengths, "shape") else np.asarray(lengths)
    kind = str(n.dtype)
    if "int" not in kind or tuple(int(d) for d in n.shape) != (M,):
      raise ValueError(f"lengths= must be an int tensor of shape ({M},), one per entry of worlds= (got {kind} "
                       f"{tuple(n.shape)})")
  if out is not None:
    for key, buf in out.items():
      if buf is None or key == "stopped":
        continue
      if key == "ran":
        want = (M,)
      elif key == "returns":
        want = (M, P)
      elif key == "hashes":
        want = None if K is None else (K, M)
      elif key == "states":
        want = None if K is None else (K, M, int(buf.shape[-1]))
      elif shapes is not None and K is not None:
        kind = STEP_MANY_NAMES.get(key, key)
        if kind not in shapes:
          continue
        want = (K, M) + tuple(int(d) for d in shapes[kind][0][1:])
      else:
        want = None
      if want is not None and tuple(int(d) for d in buf.shape) != want:
        raise ValueError(f"out[{key!r}] must have shape {want} with worlds= of {M} entries (got "
                         f"{tuple(int(d) for d in buf.shape)})")
  return M


# Registered episode starts (include/mp_engine.h: MpEpisodeStarts), carried by mp_restore
class MpEpisodeStarts(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("fresh", ctypes.c_int32), ("fingerprint", ctypes.c_uint64),
              ("bank", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("verdicts", ctypes.c_void_p),
              ("bank_rows", ctypes.c_int32), ("reserved", ctypes.c_int32), ("reserved2", ctypes.c_uint64 * 3)]


def _is_bank(bank, state_bytes: int) -> bool:
  """Whether `bank` is a contiguous uint8 tensor [M, state_bytes]."""
  import torch
  return (isinstance(bank, torch.Tensor) and bank.dtype == torch.uint8 and bank.dim() == 2 and
          int(bank.shape[1]) == int(state_bytes) and bank.is_contiguous())


def check_episode_starts(bank, rows, verdicts, num_worlds: int, state_bytes: int, device) -> int:
  """The argument rules of Engine.set_episode_starts, without an engine: `bank` a contiguous uint8
  tensor [M, state_bytes] with M >= 1, `rows` a contiguous int32 tensor [num_worlds], `verdicts`
  None or a contiguous int32 tensor [M, 2], all on `device`.  Returns M.  ValueError otherwise."""
  import torch
  device = torch.device(device)
  def on_device(x):
    return x.device.type == device.type and (device.index is None or x.device.index == device.index)
  def describe(x):
    return f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}"
  if not _is_bank(bank, state_bytes):
    raise ValueError(f"set_episode_starts: bank must be a contiguous uint8 tensor [M, {int(state_bytes)}] "
                     f"(got {describe(bank)})")
  M = int(bank.shape[0])
  if M < 1:
    raise ValueError("set_episode_starts: the bank has no rows")
  if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or tuple(rows.shape) != (int(num_worlds),) or
      not rows.is_contiguous()):
    raise ValueError(f"set_episode_starts: rows must be a contiguous int32 tensor [{int(num_worlds)}], one row "
                     f"index per world (got {describe(rows)})")
  if verdicts is not None and (not isinstance(verdicts, torch.Tensor) or verdicts.dtype != torch.int32 or
                               tuple(verdicts.shape) != (M, 2) or not verdicts.is_contiguous()):
    raise ValueError(f"set_episode_starts: verdicts must be a contiguous int32 tensor [{M}, 2], check_states of "
                     f"the whole bank (got {describe(verdicts)})")
  for name, x in (("bank", bank), ("rows", rows), ("verdicts", verdicts)):
    if x is not None and not on_device(x):
      raise ValueError(f"set_episode_starts: {name} lives on {x.device}, the engine on {device}")
  return M


# Episode statistics on the device (include/mp_engine.h: MpEpisodeStats), carried by mp_restore
STATS_MAX_COLUMNS, STATS_MAX_PAIRS = 32, 4
MP_STATS_REGISTER, MP_STATS_CLEAR, MP_STATS_TALLY, MP_STATS_HOST = 1, 2, 3, 4


class MpEventColumn(ctypes.Structure):
  _fields_ = [("type", ctypes.c_int32), ("player_payload", ctypes.c_uint8), ("player_shift", ctypes.c_uint8),
              ("filter_payload", ctypes.c_uint8), ("filter_shift", ctypes.c_uint8),
              ("player_mask", ctypes.c_uint32), ("filter_mask", ctypes.c_uint32), ("filter_value", ctypes.c_uint32),
              ("other_shift", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3), ("other_mask", ctypes.c_uint32),
              ("reserved2", ctypes.c_uint32)]


class MpStatsBank(ctypes.Structure):
  _fields_ = [("returns", ctypes.c_void_p), ("length", ctypes.c_void_p), ("counts", ctypes.c_void_p),
              ("pairs", ctypes.c_void_p)]


class MpEpisodeStats(ctypes.Structure):
  _fields_ = [("struct_size", ctypes.c_uint32), ("op", ctypes.c_int32), ("num_columns", ctypes.c_int32),
              ("num_pairs", ctypes.c_int32), ("columns", ctypes.c_void_p), ("pairs", ctypes.c_void_p),
              ("open", ctypes.c_void_p), ("episodes", ctypes.c_void_p), ("dropped", ctypes.c_void_p),
              ("running", MpStatsBank), ("last", MpStatsBank), ("total", MpStatsBank),
              ("steps", ctypes.c_int32), ("count", ctypes.c_int32), ("num_players", ctypes.c_int32),
              ("reserved", ctypes.c_int32), ("step_type", ctypes.c_void_p), ("reward", ctypes.c_void_p),
              ("events", ctypes.c_void_p), ("active", ctypes.c_void_p), ("ran", ctypes.c_void_p),
              ("reserved2", ctypes.c_uint64 * 2)]


class Request(NamedTuple):
  """One request that mp_snapshot and mp_restore tell apart by its size: its mirror, the carriers
  that take it, and whether its handler is reached without an engine."""
  struct: type
  snapshot: bool
  restore: bool
  null_engine: bool


# The 18 requests, in the order and with the flags of csrc/engine_requests.hip's kRequests
# (tests/test_request_abi_cpu.py holds the two tables, and every mirror above, to the library).
REQUESTS = (
    Request(MpKernelVariant, True, False, True),
    Request(MpWorldStates, True, True, False),    # (world_states_request: the carrier follows the op)
    Request(MpStatesObserve, True, False, True),
    Request(MpStatesView, True, False, True),
    Request(MpEgoLayer, True, False, True),
    Request(MpViewHash, True, False, True),
    Request(MpEgoPlanes, True, False, True),
    Request(MpAvatarIds, True, False, True),
    Request(MpStateLayout, True, False, True),
    Request(MpStatesCheck, True, False, True),
    Request(MpStatesHash, True, False, True),
    Request(MpStepMany, False, True, True),
    Request(MpStepTrajectory, False, True, True),
    Request(MpEpisodeStarts, False, True, True),
    Request(MpStepActive, False, True, True),
    Request(MpStepUntil, False, True, True),
    Request(MpStepListed, False, True, True),
    Request(MpEpisodeStats, False, True, True),
)
# mirror -> its carrier, for the requests that have one
_CARRIER = {q.struct: _SNAPSHOT if q.snapshot else _RESTORE for q in REQUESTS if q.snapshot != q.restore}


_FULL = 0xFFFFFFFF
# event name -> payload key -> (payload: 0 a / 1 b, shift, mask): where each key of EVENT_TYPES lies
# in a raw event row (gift's two roles are the host's: they are no payload)
EVENT_FIELDS = {
    "zap": {"source": (0, 0, _FULL), "target": (1, 0, _FULL)},
    "edible_consumed": {"player_index": (0, 0, _FULL)},
    "player_cleaned": {"player_index": (0, 0, _FULL)},
    "claimed_resource": {"player_index": (0, 0, _FULL)},
    "destroyed_resource": {"player_index": (0, 0, _FULL), "class": (1, 0, _FULL)},
    "sanctioning": {"source": (0, 0, _FULL), "target": (1, 0, _FULL)},
    "removal_due_to_sanctioning": {"source": (0, 0, _FULL), "target": (1, 0, _FULL)},
    "set_sanctioning_level": {"player_index": (0, 0, _FULL), "level": (1, 0, _FULL)},
    "AvatarStarted": {},
    "coin_consumed": {"player_index": (0, 0, _FULL), "types": (1, 0, _FULL), "player_coin_type": (1, 1, _FULL >> 1),
                      "coin_type": (1, 0, 1)},
    "interaction": {"row_player_idx": (0, 0, _FULL), "col_player_idx": (1, 0, _FULL)},
    "collected_resource": {"player_index": (0, 0, _FULL), "class": (1, 0, _FULL)},
    "mining": {"player": (0, 0, _FULL), "ore_type": (1, 0, _FULL)},
    "extraction": {"player": (0, 0, _FULL), "ore_type": (1, 0, _FULL)},
    "extraction_pair": {"player_a": (0, 0, _FULL), "player_b": (1, 2, _FULL >> 2), "ore_type": (1, 0, 3)},
    "gift": {"gifter_index": (0, 0, 15), "source_type": (0, 4, _FULL >> 4), "receipient_index": (1, 0, 15),
             "received_amount": (1, 4, _FULL >> 4)},
    "eating_mushroom": {"player_index": (0, 0, _FULL), "mushroom_type": (1, 0, _FULL)},
    "receiver_accepted_item": {"player_index": (0, 0, _FULL), "item": (1, 0, _FULL)},
    "item_dropped_into_pot": {"player_index": (0, 0, _FULL), "item": (1, 0, _FULL)},
    "cooked_food_collected_from_pot": {"player_index": (0, 0, _FULL), "cooked_item": (1, 0, _FULL)},
}
EVENT_PLAYER_KEYS = ("source", "target", "player_index", "row_player_idx", "col_player_idx", "player", "player_a",
                     "player_b", "gifter_index", "receipient_index")
_EVENT_IDS = {name: type_ for type_, (name, _) in EVENT_TYPES.items()}
# MPK_SUBSTRATE_* -> the event types the level's rules can push (the push_event sites of
# csrc/step_<level>.h and step_common.h's zap)
LEVEL_EVENT_TYPES = {
    1: (9, 1, 2, 3),                  # clean_up
    2: (9, 1, 2),                     # commons_harvest
    3: (9, 1, 4, 5, 6, 7, 8),         # territory
    4: (9, 1, 10),                    # coins
    5: (9, 1, 5, 11, 12),             # *_in_the_matrix
    6: (9, 1, 13, 14, 15),            # coop_mining
    7: (9, 1, 16),                    # gift_refinements
    8: (9, 1, 17, 18, 19),            # collaborative_cooking
    9: (9, 1, 6, 7, 8, 20),           # externality_mushrooms
}
_COLUMN_NAME = re.compile(r"^(\w+)\.(\w+)(?:>(\w+))?(?:\[(\w+)=(-?\d+)\])?$")


def parse_event_column(name: str):
  """A column name as (MpEventColumn, is_pair): "zap.source" counts zap events per source player,
  "zap.target" per target, "mining.player[ore_type=2]" only those whose ore_type is 2, and
  "zap.source>target" is a pair column, [P, P] at (source, target).  ValueError for a name that does
  not parse, an unknown event or key, a key that holds no player, or a pair whose two players lie in
  one payload."""
  m = _COLUMN_NAME.match(name) if isinstance(name, str) else None
  if not m:
    raise ValueError(f"event column {name!r}: expected \"event.key\", \"event.key[key=value]\" or \"event.key>key\"")
  event, key, other, fkey, fvalue = m.groups()
  if event not in EVENT_FIELDS:
    raise ValueError(f"event column {name!r}: unknown event {event!r} (known: {sorted(EVENT_FIELDS)})")
  fields = EVENT_FIELDS[event]
  for k in (key, other):
    if k is not None and (k not in fields or k not in EVENT_PLAYER_KEYS):
      players = [f for f in fields if f in EVENT_PLAYER_KEYS]
      raise ValueError(f"event column {name!r}: {k!r} is no player-valued key of {event!r} (it has {players})")
  col = MpEventColumn()
  col.type = _EVENT_IDS[event]
  col.player_payload, col.player_shift, col.player_mask = fields[key]
  if other is not None:
    payload, col.other_shift, col.other_mask = fields[other]
    if payload == col.player_payload:
      raise ValueError(f"event column {name!r}: {key!r} and {other!r} lie in the same payload")
  if fkey is not None:
    if fkey not in fields:
      raise ValueError(f"event column {name!r}: {fkey!r} is no key of {event!r} (it has {sorted(fields)})")
    payload, col.filter_shift, col.filter_mask = fields[fkey]
    col.filter_payload = payload + 1
    if int(fvalue) < 0 or int(fvalue) > col.filter_mask:
      raise ValueError(f"event column {name!r}: {fkey!r} cannot be {fvalue}")
    col.filter_value = int(fvalue)
  return col, other is not None


def level_event_columns(substrate: int):
  """The default columns of a level (MPK_SUBSTRATE_*): for every event type its rules can push, one
  unfiltered column per player-valued payload key; no pair columns."""
  names = []
  for type_ in LEVEL_EVENT_TYPES[int(substrate)]:
    event, _ = EVENT_TYPES[type_]
    names += [f"{event}.{key}" for key in EVENT_FIELDS[event] if key in EVENT_PLAYER_KEYS]
  return tuple(names)


def _column_array(names, limit: int, pair: bool, what: str):
  names = tuple(names)
  if len(names) > limit:
    raise ValueError(f"{what}: at most {limit} {'pair ' if pair else ''}columns (got {len(names)})")
  cols = (MpEventColumn * max(len(names), 1))()
  for i, name in enumerate(names):
    cols[i], is_pair = parse_event_column(name)
    if is_pair != pair:
      raise ValueError(f"{what}: {name!r} is {'a pair column: name it in pairs=' if is_pair else 'no pair column'}")
  return names, cols


STATS_BANKS = ("running", "last", "total")


def episode_stats_arrays(num_worlds: int, num_players: int, num_columns: int, num_pairs: int, empty):
  """The statistics tensors of an MpEpisodeStats request, zeroed, as a dict: `empty(shape, dtype
  name)` allocates one ("uint8", "int32", "int64", "float64")."""
  N, P, C, C2 = int(num_worlds), int(num_players), int(num_columns), int(num_pairs)
  out = {"open": empty((N,), "uint8"), "episodes": empty((N,), "int32"), "dropped": empty((N,), "int32")}
  for bank in STATS_BANKS:
    ints = "int64" if bank == "total" else "int32"
    out[bank] = {"returns": empty((N, P), "float64"), "length": empty((N,), ints),
                 "counts": empty((N, C, P), ints), "pairs": empty((N, C2, P, P), ints)}
  return out


def _stats_request(op: int, cols, ncols: int, pairs, npairs: int, arrays, ptr) -> MpEpisodeStats:
  req = MpEpisodeStats(ctypes.sizeof(MpEpisodeStats), op, ncols, npairs)
  req.columns = ctypes.addressof(cols) if ncols else None
  req.pairs = ctypes.addressof(pairs) if npairs else None
  if arrays is not None:
    req.open, req.episodes, req.dropped = ptr(arrays["open"]), ptr(arrays["episodes"]), ptr(arrays["dropped"])
    for bank in STATS_BANKS:
      b = getattr(req, bank)
      b.returns, b.length = ptr(arrays[bank]["returns"]), ptr(arrays[bank]["length"])
      b.counts = ptr(arrays[bank]["counts"]) if ncols else None
      b.pairs = ptr(arrays[bank]["pairs"]) if npairs else None
  return req


def episode_stats_host(stats, step_type, reward, events, columns=(), pairs=(), active=None, ran=None):
  """The rule of MpEpisodeStats applied on the host, by the library's own functions compiled for the
  host (no engine, no device): folds K steps of n worlds — step_type int32 [K, n], reward float64
  [K, n, P], events int32 [K, n, EVENT_ROWS, 4] (None with no columns), active uint8 [K, n] or
  None, ran int32 [n] or None — into `stats`, numpy arrays laid out as episode_stats_arrays gives
  them (see numpy_episode_stats), in place.  Returns `stats`."""
  L = load_library()
  names, cols = _column_array(columns, STATS_MAX_COLUMNS, False, "episode_stats_host")
  pnames, pcols = _column_array(pairs, STATS_MAX_PAIRS, True, "episode_stats_host")
  step_type = np.ascontiguousarray(step_type, np.int32)
  K, n = step_type.shape
  reward = np.ascontiguousarray(reward, np.float64)
  P = int(reward.shape[2])
  if reward.shape != (K, n, P):
    raise ValueError(f"episode_stats_host: reward must be [K, n, P] = {(K, n, P)} (got {reward.shape})")
  keep = [step_type, reward]
  def host(x, dtype, shape, what):
    if x is None:
      return None
    x = np.ascontiguousarray(x, dtype)
    if x.shape != shape:
      raise ValueError(f"episode_stats_host: {what} must have shape {shape} (got {x.shape})")
    keep.append(x)
    return x.ctypes.data
  def ptr(a):
    if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
      raise ValueError("episode_stats_host: the statistics must be contiguous numpy arrays")
    return a.ctypes.data
  want = episode_stats_arrays(n, P, len(names), len(pnames), lambda shape, dtype: (shape, dtype))
  for key, value in want.items():
    for sub, (shape, dtype) in (value.items() if isinstance(value, dict) else [(None, value)]):
      a = stats[key] if sub is None else stats[key][sub]
      if not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != np.dtype(dtype):
        raise ValueError(f"episode_stats_host: stats[{key!r}]{'' if sub is None else '[' + repr(sub) + ']'} must be a "
                         f"{dtype} array of shape {shape}")
  req = _stats_request(MP_STATS_HOST, cols, len(names), pcols, len(pnames), stats, ptr)
  req.steps, req.count, req.num_players = K, n, P
  req.step_type, req.reward = step_type.ctypes.data, reward.ctypes.data
  req.events = host(events, np.int32, (K, n, EVENT_ROWS, 4), "events")
  req.active = host(active, np.uint8, (K, n), "active")
  req.ran = host(ran, np.int32, (n,), "ran")
  _send(L, None, req)
  return stats


def numpy_episode_stats(num_worlds: int, num_players: int, num_columns: int, num_pairs: int = 0):
  """Zeroed host statistics for episode_stats_host."""
  return episode_stats_arrays(num_worlds, num_players, num_columns, num_pairs,
                              lambda shape, dtype: np.zeros(shape, dtype))


class EpisodeStats:
  """The live statistics tensors of a registration (Engine.set_episode_stats): `.open` uint8 [N],
  `.episodes` and `.dropped` int32 [N], and the banks `.running`, `.last`, `.total`, each a dict of
  "returns" float64 [N, P], "length" [N], "counts" [N, C, P], "pairs" [N, C2, P, P] (int32; int64
  in total).  `.columns` / `.pairs` are the names; `.index(name)` a column's (or pair's) index.
  The tensors are written by the device behind every submission: read them in stream order."""

  def __init__(self, columns, pairs, arrays):
    self.columns, self.pair_columns = tuple(columns), tuple(pairs)
    self.arrays = arrays
    self.open, self.episodes, self.dropped = arrays["open"], arrays["episodes"], arrays["dropped"]
    self.running, self.last, self.total = arrays["running"], arrays["last"], arrays["total"]

  def index(self, name: str) -> int:
    if name in self.columns:
      return self.columns.index(name)
    if name in self.pair_columns:
      return self.pair_columns.index(name)
    raise ValueError(f"{name!r} is no registered column (columns {self.columns}, pairs {self.pair_columns})")

  def slice(self, lo: int, hi: int) -> "EpisodeStats":
    """Worlds [lo, hi) of every tensor, in place (a mixture hands each member its slice)."""
    cut = {k: ({s: v[lo:hi] for s, v in a.items()} if isinstance(a, dict) else a[lo:hi])
           for k, a in self.arrays.items()}
    return EpisodeStats(self.columns, self.pair_columns, cut)


def _step_distance(tensor, what: str) -> int:
  """Bytes between tensor[k] and tensor[k + 1] of a tensor that may be non-contiguous along its
  first dimension only (a column slice [:, a:b] of a wider tensor)."""
  if not tensor[0].is_contiguous():
    raise ValueError(f"step_many: {what} may be non-contiguous along K only (each step's block "
                     f"must be contiguous; strides {tuple(tensor.stride())})")
  block = int(tensor[0].numel())
  if tensor.shape[0] == 1:
    return block * tensor.element_size()
  if tensor.stride(0) < block:
    raise ValueError(f"step_many: the steps of {what} overlap (stride {tensor.stride(0)} < {block})")
  return int(tensor.stride(0)) * tensor.element_size()


class EngineError(RuntimeError):
  pass


_lib = None


def load_library(build: bool = True) -> ctypes.CDLL:
  """Loads libmp_engine.so (building it with hipcc first if needed)."""
  global _lib
  if _lib is not None:
    return _lib
  # torch first: its wheel bundles its own HIP runtime, and a process must end up
  # with ONE — loaded the other way round (this library pulling in /opt/rocm's
  # runtime, torch its own afterwards) the second runtime finds no device
  try:
    import torch  # noqa: F401
  except ImportError:
    pass
  path = _build.LIB_PATH
  override = os.environ.get("MP_ENGINE_LIB")  # developer A/B runs of another build
  if override:
    path = override
  elif build:
    path = _build.build_engine()
  if not os.path.exists(path):
    raise EngineError(
        f"{path} is missing: build it with `python -c 'import __graft_entry__ "
        "as g; g.build()'` (hipcc --offload-arch=gfx950). There is no fallback.")
  L = ctypes.CDLL(path)
  vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
  L.mp_abi_version.restype = i32
  L.mp_last_error.restype = ctypes.c_char_p
  L.mp_create.restype = i32
  L.mp_create.argtypes = [vp, u64, ctypes.POINTER(MpConfig),
                          ctypes.POINTER(vp)]
  L.mp_destroy.restype = None
  L.mp_destroy.argtypes = [vp]
  L.mp_info.restype = i32
  L.mp_info.argtypes = [vp, ctypes.POINTER(MpInfo)]
  L.mp_set_stream.restype = i32
  L.mp_set_stream.argtypes = [vp, vp]
  L.mp_bind_output.restype = i32
  L.mp_bind_output.argtypes = [vp, i32, vp]
  L.mp_reset.restype = i32
  L.mp_reset.argtypes = [vp, vp, vp]
  L.mp_step.restype = i32
  L.mp_step.argtypes = [vp, vp]
  L.mp_step_host.restype = i32
  L.mp_step_host.argtypes = [vp, vp]
  L.mp_step_fields.restype = i32
  L.mp_step_fields.argtypes = [vp, vp]
  L.mp_step_fields_host.restype = i32
  L.mp_step_fields_host.argtypes = [vp, vp]
  L.mp_observe.restype = i32
  L.mp_observe.argtypes = [vp, i32, vp]
  L.mp_obs_bytes.restype = u64
  L.mp_obs_bytes.argtypes = [vp, i32]
  L.mp_dump.restype = i32
  L.mp_dump.argtypes = [vp, vp, vp, vp]
  L.mp_snapshot_bytes.restype = u64
  L.mp_snapshot_bytes.argtypes = [vp]
  L.mp_snapshot.restype = i32
  L.mp_snapshot.argtypes = [vp, vp, u64]
  L.mp_restore.restype = i32
  L.mp_restore.argtypes = [vp, vp, u64]
  L.mp_counters.restype = i32
  L.mp_counters.argtypes = [vp, vp]
  L.mp_sync.restype = i32
  L.mp_sync.argtypes = [vp]
  L.mp_alloc_output.restype = i32
  L.mp_alloc_output.argtypes = [i32, u64, u64, ctypes.POINTER(vp)]
  L.mp_free_output.restype = i32
  L.mp_free_output.argtypes = [i32, vp]
  L.mp_tune.restype = i32
  L.mp_tune.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
  L.mp_place_output.restype = i32
  L.mp_place_output.argtypes = [vp, i32, i32, u64, ctypes.POINTER(vp), ctypes.POINTER(MpPlacement)]
  L.mp_fault_words.restype = i32
  L.mp_fault_words.argtypes = [vp, vp]
  L.mp_bind_output_ring.restype = i32
  L.mp_bind_output_ring.argtypes = [vp, i32, vp, u64, i32]
  L.mp_box_fill.restype = i32
  L.mp_box_fill.argtypes = [vp, i32, i32, ctypes.POINTER(MpBoxFill)]
  L.mp_set_retired_va_limit.restype = i32
  L.mp_set_retired_va_limit.argtypes = [ctypes.c_int64]
  _lib = L
  return L


def kernel_variant(pack_bytes: bytes, *, num_players: int = 0,
                   dev: Optional[Dict[str, int]] = None) -> int:
  """KERNEL_STOCK if an engine created on this pack would run the frame kernels that have the
  committed pack's constants compiled in, KERNEL_GENERIC otherwise — mp_create's own selection,
  made on the host (an MpKernelVariant request without an engine: no GPU needed)."""
  return pack_fields(pack_bytes, num_players=num_players, dev=dev)[0]


def pack_fields(pack_bytes: bytes, *, num_players: int = 0, dev: Optional[Dict[str, int]] = None,
                want_fields: bool = False):
  """(variant, text): `kernel_variant`'s answer and, with `want_fields`, the pack's value of every
  scalar a stock kernel folds as "<group> <member> <C literal>" lines (tools/make_stock_header.py)."""
  L = load_library()
  cfg = MpConfig(ctypes.sizeof(MpConfig), 0, 1, 1, 0, 0, None, int(num_players))
  if dev:
    opts = MpDevOptions(ctypes.sizeof(MpDevOptions), max_composites=-1)
    for k, v in dev.items():
      setattr(opts, k, int(v))
    cfg.dev = ctypes.pointer(opts)
  buf = ctypes.create_string_buffer(pack_bytes, len(pack_bytes))
  out = ctypes.create_string_buffer(1 << 16) if want_fields else None
  req = MpKernelVariant(ctypes.sizeof(MpKernelVariant), 0, ctypes.addressof(buf), len(pack_bytes),
                        ctypes.pointer(cfg), ctypes.addressof(out) if out else None,
                        len(out) if out else 0)
  _send(L, None, req)
  return req.variant, (out.value.decode() if out else "")


def _check(L, rc: int, what: str):
  if rc == 0:
    return
  msg = (L.mp_last_error() or b"").decode()
  if rc == MP_ERR_INVALID:
    raise ValueError(f"{what}: {msg}")  # the reference raises ValueError too
  raise EngineError(f"{what} failed ({rc}): {msg}")


class Engine:
  """N worlds of one substrate on one GPU.  All buffers are torch tensors on
  that GPU; calls enqueue work on torch's current stream and do not sync."""

  def __init__(self, pack_bytes: bytes, num_worlds: int, *, device: int = 0,
               auto_reset: bool = True, world_offset: int = 0,
               base_seed: int = 0, literal_seed: bool = False, num_players: int = 0,
               debug_observations: bool = False, unfused: Optional[bool] = None,
               dev: Optional[Dict[str, int]] = None,
               roles: Optional[Sequence[int]] = None, placements: int = 8,
               world_pool: int = 1):
    """`num_players` = 0: the pack's default count (its header; all the avatars
    it holds unless tools/make_packs.py says otherwise); else the first
    `num_players` avatars play (the reference's num_players = len(roles)).
    `base_seed`: world w is seeded base_seed + w (mod 2**64); base_seed 0 selects
    the benchmark's fixed per-world seeds unless `literal_seed` says that 0 is a
    seed like any other (MpConfig.literal_base_seed: the Substrate API's env_seed).
    `unfused`: True = one launch for the rules and one per view, False = one
    fused launch per step, None = the engine's choice for the substrate
    (`info.fused` reports it).  `dev`: MpDevOptions fields by name — tests and
    tools/ only (launch-plan overrides; results never depend on them).  `roles`:
    one index per player into the pack's "role_names" (MpConfig.roles; only for
    substrates whose config has more than one valid role) — see
    `pack_role_names`.  `world_pool` = k in (2, 4, 8): OBS_WORLD_RGB is the world
    image pooled by k (`pool_rgb`), drawn so by every launch (MpConfig.world_pool); 1 = full."""
    if (isinstance(world_pool, bool) or not isinstance(world_pool, (int, np.integer)) or
        int(world_pool) not in (0, 1, 2, 4, 8)):
      raise ValueError(f"world_pool must be 1, 2, 4 or 8 (got {world_pool!r})")
    self.world_pool = max(1, int(world_pool))   # (0 means the full image, as in MpConfig)
    import torch  # device memory + streams only
    self._torch = torch
    # candidates `place` tries for a bound pixel view (1: the first allocation, its
    # plan tuned; 0: the first allocation, stock plan)
    self.placements = placements
    # memory `place` may keep alive while it probes (0: a quarter of the device's free
    # memory) — one process per GPU sets nothing; ranks that SHARE a device set their share
    self.place_max_bytes = 0
    self.placement: Dict[int, dict] = {}
    self._L = load_library()
    if not torch.cuda.is_available():
      # still go through mp_create so that the C ABI reports the error
      pass
    self._pack = ctypes.create_string_buffer(pack_bytes, len(pack_bytes))
    self.pack_bytes = pack_bytes
    stream = None
    if torch.cuda.is_available():
      torch.cuda.set_device(device)
      stream = torch.cuda.current_stream(device).cuda_stream
    cfg = MpConfig(ctypes.sizeof(MpConfig), device, num_worlds,
                   1 if auto_reset else 0, world_offset, int(base_seed) % (1 << 64), stream,
                   int(num_players), 1 if debug_observations else 0,
                   0 if unfused is None else (1 if unfused else 2),
                   1 if literal_seed else 0, None, None, self.world_pool)
    if roles is not None:
      if num_players and len(roles) != num_players:
        raise ValueError(f"{len(roles)} roles for {num_players} players")
      self._roles = (ctypes.c_int32 * len(roles))(*[int(r) for r in roles])
      cfg.roles = ctypes.cast(self._roles, ctypes.POINTER(ctypes.c_int32))
      cfg.num_players = len(roles)
    if dev:
      opts = MpDevOptions(ctypes.sizeof(MpDevOptions), max_composites=-1)
      for k, v in dev.items():
        if not hasattr(opts, k) or k == "struct_size":
          raise ValueError(f"unknown MpDevOptions field {k!r}")
        setattr(opts, k, int(v))
      self._dev = opts   # kept alive for mp_create
      cfg.dev = ctypes.pointer(opts)
    handle = ctypes.c_void_p()
    rc = self._L.mp_create(self._pack, len(pack_bytes), ctypes.byref(cfg),
                           ctypes.byref(handle))
    self._h = None
    _check(self._L, rc, "mp_create")
    self._h = handle
    info = MpInfo()
    _check(self._L, self._L.mp_info(self._h, ctypes.byref(info)), "mp_info")
    self.info = info
    self.device = torch.device("cuda", device)
    self.N, self.P = info.num_worlds, info.num_players
    self.num_actions = info.num_actions
    S = info.sprite_size
    self.shapes = {
        OBS_RGB: ((self.N, self.P, info.view_h * S, info.view_w * S, 3), torch.uint8),
        OBS_WORLD_RGB: ((self.N, info.map_h * S // self.world_pool, info.map_w * S // self.world_pool,
                         3), torch.uint8),
        OBS_REWARD: ((self.N, self.P), torch.float64),
        OBS_READY_TO_SHOOT: ((self.N, self.P), torch.float64),
        OBS_AUX0: ((self.N, self.P), torch.float64),
        OBS_STEP_TYPE: ((self.N,), torch.int32),
        OBS_DISCOUNT: ((self.N,), torch.float64),
        OBS_COLLECTIVE_REWARD: ((self.N,), torch.float64),
        OBS_POSITION: ((self.N, self.P, 2), torch.int32),
        OBS_ORIENTATION: ((self.N, self.P), torch.int32),
        OBS_EVENTS: ((self.N, EVENT_ROWS, 4), torch.int32),
        OBS_AUX1: ((self.N, self.P), torch.float64),
        OBS_AUX2: ((self.N, self.P), torch.float64),
        OBS_AUX3: ((self.N, self.P), torch.float64),
        OBS_AUX4: ((self.N, self.P), torch.float64),
        OBS_ZAP_MATRIX: ((self.N, self.P, self.P), torch.float64),
        OBS_LAYER: ((self.N, self.P, info.view_h, info.view_w, info.num_layers),
                    torch.int32),
        OBS_INVENTORY: ((self.N, self.P, info.num_resources), torch.float64),
        OBS_INTERACTION_INVENTORIES: ((self.N, self.P, 2, info.num_resources), torch.float64),
        OBS_MATRIX_CUMULANTS: ((self.N, self.P, 1 + 3 * info.num_resources), torch.float64),
        OBS_INTERACTION_REWARDS: ((self.N, self.P, 2), torch.float64),
        **{kind: ((self.N, self.P, info.view_h * S // k, info.view_w * S // k, 3), torch.uint8)
           for k, kind in OBS_RGB_POOL.items()},
    }
    self._bound: Dict[int, "torch.Tensor"] = {}
    self._episode_starts = None
    self._stats = None           # the registered EpisodeStats (set_episode_stats)
    self._stats_scratch = {}     # the rows a K-step request carries for it without being asked

  @property
  def fused(self) -> bool:
    """Whether a step with the views bound right now is ONE launch (rules and
    pixels fused) — MpConfig.unfused; the engine's own choice depends on the view."""
    info = MpInfo()
    _check(self._L, self._L.mp_info(self._h, ctypes.byref(info)), "mp_info")
    return bool(info.fused)

  @property
  def plan(self) -> Dict[str, int]:
    """The launch plan of a step with the pixel views bound right now (MpInfo.plan_*)."""
    info = MpInfo()
    _check(self._L, self._L.mp_info(self._h, ctypes.byref(info)), "mp_info")
    return {"batch_worlds": info.plan_batch_worlds, "ring_batches": info.plan_ring_batches,
            "owned_batches": info.plan_owned_batches, "pooled_batches": info.plan_pooled_batches,
            "workgroups": info.plan_groups, "sc1_stores": info.plan_store_sc1,
            "feeders": info.plan_feeders, "waves": info.plan_waves, "pace": info.plan_pace,
            "xcd_teams": info.plan_team, "late_feeder_priority": info.plan_late_priority,
            # 1: the stepping launches of the full views run the kernels with the committed pack's
            # constants compiled in (MpKernelVariant)
            "stock": self._kernel_variant()}

  def _kernel_variant(self) -> int:
    req = MpKernelVariant(ctypes.sizeof(MpKernelVariant))
    # (an older build under MP_ENGINE_LIB does not know the request: generic kernels only)
    if self._L.mp_snapshot(self._h, ctypes.addressof(req), ctypes.sizeof(req)) != 0:
      return KERNEL_GENERIC
    return int(req.variant)

  # -- lifetime ------------------------------------------------------------
  def close(self):
    if getattr(self, "_h", None):
      self._L.mp_destroy(self._h)
      self._h = None
      self._bound.clear()

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  # -- events ------------------------------------------------------------------
  def events(self, world: int = 0):
    """env.events() of one world for the last reset()/step(): a list of
    (name, {key: value}) in canonical (sorted) order — the engine resolves a step's
    beams in parallel, so rows carry no order of their own.

    Payloads are the keys of the reference's events.  The_matrix's 'interaction'
    carries row_player_idx, col_player_idx, row_reward, col_reward (floats) and
    row_inventory, col_inventory (float64 arrays of R) as in the reference
    (the_matrix/components.lua:789-797)."""
    return self.events_all(worlds=[world])[0]

  def events_all(self, worlds=None):
    """events() of every world (or of `worlds`), from one device read per kind: a
    list of lists."""
    if worlds is None:
      worlds, pick = list(range(self.N)), (lambda t: t)
    else:
      worlds = [int(w) for w in worlds]
      index = self._torch.as_tensor(worlds, dtype=self._torch.long, device=self.device)
      pick = lambda t: t.index_select(0, index)   # (only these worlds cross to the host)
    rows = pick(self.observe(OBS_EVENTS)).cpu().numpy()
    extra = None
    if self.info.num_resources and any(
        (rows[i, 1:1 + int(rows[i, 0, 0]), 0] == 11).any() for i in range(len(worlds))):
      extra = (pick(self.observe(OBS_INTERACTION_REWARDS)).cpu().numpy(),
               pick(self.observe(OBS_INTERACTION_INVENTORIES)).cpu().numpy())
    roles = pack_agent_roles(self.pack_bytes) if (rows[:, 1:, 0] == 16).any() else None
    return [self._decode_events(rows[i], w, None if extra is None else (extra[0][i], extra[1][i]),
                                roles)
            for i, w in enumerate(worlds)]

  @staticmethod
  def _decode_events(rows, world, interaction=None, agent_roles=None):
    """`interaction`: this world's ([P, 2] rewards, [P, 2, R] inventories) when a row
    of type 11 is present; `agent_roles`: the avatars' agentRole strings (gift_refinements)."""
    n = int(rows[0, 0])
    if rows[0, 1]:
      raise EngineError(f"world {world}: {int(rows[0, 1])} events beyond the "
                        f"{EVENT_ROWS - 1} rows of MP_OBS_EVENTS were dropped")
    out = []
    for t, a, b, _ in sorted(tuple(int(v) for v in r) for r in rows[1:1 + n]):
      name, keys = EVENT_TYPES[t]
      if t == 5 and b:   # the_matrix's destroyed_resource names the class too (components.lua:178)
        keys = ("player_index", "class")
      payload = dict(zip(keys, (a, b)))
      if t == 15:
        payload = {"player_a": a, "player_b": b >> 2, "ore_type": b & 3}
      if t == 16:
        payload = {"gifter_index": a & 15, "receipient_index": b & 15,
                   "source_type": a >> 4, "received_amount": b >> 4}
        if agent_roles:
          payload.update(gifter_role=agent_roles[(a & 15) - 1],
                         receipient_role=agent_roles[(b & 15) - 1])
      if t == 20:
        payload = {"player_index": a, "mushroom_type": MUSHROOM_TYPES[b - 1]}
      if t in (17, 18, 19):
        payload = {"player_index": a, keys[1]: COOKING_ITEMS[b],
                   **({"receiver": "Receiver"} if t == 17 else {"pot": "CookingPot"})}
      if t == 11 and interaction is not None:
        rewards, inventories = interaction
        payload.update(row_reward=float(rewards[a - 1, 0]), col_reward=float(rewards[a - 1, 1]),
                       row_inventory=inventories[a - 1, 0].copy(),
                       col_inventory=inventories[b - 1, 0].copy())
      out.append((name, payload))
    return out

  # -- buffers -------------------------------------------------------------
  def empty(self, kind: int):
    shape, dtype = self.shapes[kind]
    return self._torch.empty(shape, dtype=dtype, device=self.device)

  def _wrap(self, kind: int, ptr: int, leading: int = 0):
    """A tensor of `kind`'s shape (with `leading` slots in front, if any) over
    engine-library memory (mp_alloc_output / mp_place_output); the memory is released
    (mp_free_output) with the tensor."""
    t = self._torch
    shape, dtype = self.shapes[kind]
    if leading:
      shape = (leading,) + tuple(shape)
    nbytes = int(np.prod(shape)) * t.empty((), dtype=dtype).element_size()
    L, dev_index = self._L, self.device.index or 0

    class _Owner:   # torch keeps this object alive for as long as the tensor's storage
      __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1",
                                  "data": (ptr, False), "version": 2}

      def __del__(self):
        L.mp_free_output(dev_index, ctypes.c_void_p(ptr))

    flat = t.as_tensor(_Owner(), device=self.device)
    return flat.view(dtype).view(shape)

  def empty_mapped(self, kind: int, chunk_bytes: int):
    """A tensor for `kind` whose memory is one virtual range mapped onto separate
    physical chunks of `chunk_bytes` (mp_alloc_output; outside torch's allocator).
    None if the driver refuses."""
    shape, dtype = self.shapes[kind]
    nbytes = int(np.prod(shape)) * self._torch.empty((), dtype=dtype).element_size()
    ptr = ctypes.c_void_p()
    if self._L.mp_alloc_output(self.device.index or 0, nbytes, chunk_bytes, ctypes.byref(ptr)) != 0:
      return None
    try:
      return self._wrap(kind, ptr.value)
    except (RuntimeError, TypeError):
      self._L.mp_free_output(self.device.index or 0, ptr)
      return None

  # A pixel view of at least this many bytes is PLACED (see `place`), not just allocated
  PLACE_MIN_BYTES = 64 << 20

  def place(self, kind: int, candidates: Optional[int] = None, max_bytes: int = 0):
    """Allocates AND BINDS the tensor of a pixel view where this engine's launch
    writes it fastest (mp_place_output: up to `candidates` buffers mapped from 2 MB
    physical chunks, never more than `max_bytes` alive — 0: a quarter of the free
    memory —, each timed with dry launches under the plan that suits it; the fastest
    kept, the others released before the call returns).  The same launch takes
    99 - 122 us (clean_up WORLD.RGB) depending on WHERE its output lies, a property
    of the buffer's physical pages (profiles/r04_write_fronts.md).  What was measured
    stays in `self.placement[kind]`.  A caller that brings its own tensor to `bind`
    gets the speed of that tensor (and the plan tuned to it: mp_tune)."""
    k = self.placements if candidates is None else candidates
    max_bytes = max_bytes or self.place_max_bytes
    ptr, rep = ctypes.c_void_p(), MpPlacement()
    _check(self._L, self._L.mp_place_output(self._h, kind, k, max_bytes, ctypes.byref(ptr),
                                            ctypes.byref(rep)), "mp_place_output")
    try:
      tensor = self._wrap(kind, ptr.value)
    except Exception:
      # the placed buffer must not stay bound (and mapped) behind a failed wrap
      self._L.mp_bind_output(self._h, kind, None)
      self._L.mp_free_output(self.device.index or 0, ptr)
      raise
    self._bound[kind] = tensor
    self.placement[kind] = {"candidates": rep.candidates, "requested": rep.requested,
                            "picked": rep.picked,
                            "dry_launch_us": [round(rep.us[i], 1) for i in range(rep.candidates)],
                            # (every fourth candidate is one plain allocation: mp_place_output)
                            "kind": "plain allocation" if rep.picked % 4 == 3 else "mapped 2 MB",
                            "probe": "stepped behind a copy" if rep.stepped else "dry",
                            "out_of_memory": rep.out_of_memory,
                            "early_exit": {0: None, 1: "round within 3 %",
                                           2: "outlier found"}.get(rep.early_exit),
                            "setup_s": round(rep.setup_ms / 1e3, 3)}
    return tensor

  def tune(self) -> float:
    """The launch plan that suits the pixel views bound right now (mp_tune); returns
    its dry-launch time in us (0.0 when nothing is fused)."""
    us = ctypes.c_double()
    _check(self._L, self._L.mp_tune(self._h, ctypes.byref(us)), "mp_tune")
    return us.value

  def bind(self, kind: int, tensor=None):
    """Binds (and returns) a tensor refreshed by every reset()/step().  Without a
    tensor the engine allocates one — a large pixel view through `place` (unless
    `self.placements` <= 1).  A large pixel view the caller brings gets the launch
    plan tuned to it (mp_tune: a few dry launches)."""
    shape, dtype = self.shapes[kind]
    big = (kind in PIXEL_KINDS and
           int(np.prod(shape)) >= self.PLACE_MIN_BYTES)
    if tensor is None:
      if big and self.placements > 1:
        try:
          return self.place(kind)
        except EngineError as e:
          # no virtual-memory mappings to be had (driver, fragmentation, the bound on
          # retired address space): an ordinary allocation with its plan tuned — slower
          # on most boxes, never a failure to bind
          self.placement[kind] = {"candidates": 0, "kind": "torch allocation (placing failed)",
                                  "error": str(e)}
      tensor = self.empty(kind)
    assert tuple(tensor.shape) == shape and tensor.dtype == dtype
    assert tensor.is_contiguous() and tensor.device == self.device
    _check(self._L, self._L.mp_bind_output(self._h, kind, tensor.data_ptr()),
           "mp_bind_output")
    self._bound[kind] = tensor
    if big and self.placements > 0:
      _check(self._L, self._L.mp_tune(self._h, None), "mp_tune")
    return tensor

  def bind_ring(self, kind: int, tensor=None, slots: Optional[int] = None, tune: bool = True):
    """A rollout ring for `kind` (mp_bind_output_ring): submission t since the ring was
    bound — every reset() and step() — writes slot t % T of `tensor` [T, *shape(kind)].
    All ring-bound kinds share T and the position, so slot s of every kind is the same
    step.  The learner keeps what it was handed: a slot is not written again for T
    submissions, nothing is cloned, and moving on a slot costs a pointer store.  Without
    a tensor one is allocated (`slots` = T; a large pixel view from scattered 2 MB chunks,
    `empty_ring`).  `tune`: time the launch plans on every slot of a large pixel view now
    (once; the timed launches draw into the slots).  (Round 5 also searched a fast set of
    chunks for EVERY slot — 32 slots, 215 candidate sets, 30 s of set-up for 2 %: removed.)"""
    shape, dtype = self.shapes[kind]
    t = self._torch
    if tensor is None:
      if not slots or slots < 1:
        raise ValueError("bind_ring needs a tensor or a positive number of slots")
      tensor = self.empty_ring(kind, int(slots))
    if tuple(tensor.shape[1:]) != tuple(shape) or tensor.dtype != dtype:
      raise ValueError(f"a ring for kind {kind} is [T, {', '.join(map(str, shape))}] {dtype}, "
                       f"got {tuple(tensor.shape)} {tensor.dtype}")
    if slots is not None and int(slots) != tensor.shape[0]:
      raise ValueError(f"{tensor.shape[0]} slots in the tensor, {slots} asked for")
    if not tensor[0].is_contiguous() or tensor.device != self.device:
      raise ValueError("the slots of a ring must be contiguous and on the engine's device")
    # (one slot: any stride that holds it)
    stride = tensor.stride(0) * tensor.element_size() if tensor.shape[0] > 1 else (
        -(-int(np.prod(shape)) * tensor.element_size() // 256) * 256)
    if stride % 256:
      raise ValueError(f"slot stride {stride} B is not a multiple of 256: pad the kind's last axes "
                       "or use Engine.empty_ring")
    _check(self._L, self._L.mp_bind_output_ring(self._h, kind, tensor.data_ptr(), stride,
                                                tensor.shape[0]), "mp_bind_output_ring")
    self._bound[kind] = tensor
    big = kind in PIXEL_KINDS and int(np.prod(shape)) >= self.PLACE_MIN_BYTES
    if tune and big and self.placements > 0:
      _check(self._L, self._L.mp_tune(self._h, None), "mp_tune")
    return tensor

  def empty_ring(self, kind: int, slots: int):
    """[slots, *shape(kind)] whose slots start 256 bytes apart-aligned (the stride
    mp_bind_output_ring wants): for the kinds whose bytes per slot are not a multiple of
    256 the tensor is a view into a padded allocation."""
    shape, dtype = self.shapes[kind]
    t = self._torch
    item = t.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape))
    if (kind in PIXEL_KINDS and n * item >= self.PLACE_MIN_BYTES and
        self.placements > 0 and (n * item) % 256 == 0):
      # a large pixel view: scattered 2 MB chunks, like a placed single buffer — the frame
      # launch writes those evenly; an ordinary allocation is physically contiguous in large
      # pieces and 10 - 15 % slower on about half the boxes (profiles/r05_alloc_method.md)
      ptr = ctypes.c_void_p()
      if self._L.mp_alloc_output(self.device.index or 0, n * item * int(slots), 2 << 20,
                                 ctypes.byref(ptr)) == 0:
        try:
          return self._wrap(kind, ptr.value, leading=int(slots))
        except (RuntimeError, TypeError):
          self._L.mp_free_output(self.device.index or 0, ptr)
    padded = -(-n * item // 256) * 256 // item
    flat = t.empty((int(slots), padded), dtype=dtype, device=self.device)
    return flat[:, :n].view((int(slots),) + tuple(shape)) if padded != n else flat.view(
        (int(slots),) + tuple(shape))

  @property
  def ring(self) -> Dict[str, int]:
    """{"slots": T (0: no ring), "next": the slot the next reset()/step() writes,
    "last": the slot written last}."""
    info = MpInfo()
    _check(self._L, self._L.mp_info(self._h, ctypes.byref(info)), "mp_info")
    T = info.ring_slots
    return {"slots": T, "next": info.ring_next, "last": (info.ring_next + T - 1) % T if T else 0}

  @property
  def retired_va(self) -> Dict[str, int]:
    """Address space this process has retired with released mapped views, and the bound."""
    info = MpInfo()
    _check(self._L, self._L.mp_info(self._h, ctypes.byref(info)), "mp_info")
    return {"bytes": info.retired_va_bytes, "limit": info.retired_va_limit}

  def unbind(self, kind: int):
    _check(self._L, self._L.mp_bind_output(self._h, kind, None),
           "mp_bind_output")
    self._bound.pop(kind, None)

  def use_current_stream(self):
    s = self._torch.cuda.current_stream(self.device).cuda_stream
    _check(self._L, self._L.mp_set_stream(self._h, s), "mp_set_stream")

  # -- episode control -----------------------------------------------------
  def reset(self, seeds: Optional[Sequence[int]] = None, mask=None):
    sp = mp = None
    if seeds is not None:
      seeds = np.ascontiguousarray(seeds, np.uint64)
      assert seeds.shape == (self.N,)
      sp = seeds.ctypes.data
    if mask is not None:
      mask = np.ascontiguousarray(mask, np.uint8)
      assert mask.shape == (self.N,)
      mp = mask.ctypes.data
    _check(self._L, self._L.mp_reset(self._h, sp, mp), "mp_reset")

  def step(self, actions, active=None, worlds=None):
    """actions: int32 cuda tensor [N, P] of discrete action ids.
    active: a mask [N] (see step_many): only the worlds it selects step, the others are not
    touched.  It is the K = 1 masked request of step_many.
    worlds: a list of M world indices (see step_many): actions [M, P], entry i steps world
    worlds[i] and no other world is touched (active, if given, is then [M]).  It is the K = 1
    listed request of step_many."""
    t = self._torch
    if worlds is not None:
      a = actions if isinstance(actions, t.Tensor) else np.asarray(actions)
      M = check_step_listed(worlds, self.N, self.P)
      if tuple(a.shape) != (M, self.P):
        raise ValueError(f"actions must have shape {(M, self.P)}, one row per entry of worlds=")
      self.step_many(a[None], keep=(), active=active, worlds=worlds)
      return
    if active is not None:
      a = actions if isinstance(actions, t.Tensor) else np.asarray(actions)
      if tuple(a.shape) != (self.N, self.P):
        raise ValueError(f"actions must have shape {(self.N, self.P)}")
      self.step_many(a[None], keep=(), active=active)
      return
    if isinstance(actions, t.Tensor) and actions.is_cuda:
      assert actions.dtype == t.int32 and actions.is_contiguous()
      assert tuple(actions.shape) == (self.N, self.P)
      _check(self._L, self._L.mp_step(self._h, actions.data_ptr()), "mp_step")
    else:
      a = np.ascontiguousarray(actions, np.int32)
      if a.shape != (self.N, self.P):
        raise ValueError(f"actions must have shape {(self.N, self.P)}")
      _check(self._L, self._L.mp_step_host(self._h, a.ctypes.data),
             "mp_step_host")

  def step_fields(self, fields):
    """The raw action surface of dmlab2d: `fields` int32 [N, P, A], one value per
    field of the avatar's actionOrder (A = info.num_action_fields) — a cuda tensor
    (mp_step_fields) or a host array (mp_step_fields_host, ranges validated)."""
    t = self._torch
    shape = (self.N, self.P, self.info.num_action_fields)
    if isinstance(fields, t.Tensor) and fields.is_cuda:
      assert fields.dtype == t.int32 and fields.is_contiguous()
      assert tuple(fields.shape) == shape
      _check(self._L, self._L.mp_step_fields(self._h, fields.data_ptr()), "mp_step_fields")
    else:
      a = np.ascontiguousarray(fields, np.int32)
      if a.shape != shape:
        raise ValueError(f"fields must have shape {shape}")
      _check(self._L, self._L.mp_step_fields_host(self._h, a.ctypes.data),
             "mp_step_fields_host")

  def step_many(self, actions, *, repeat: Optional[int] = None, fields: bool = False,
                keep=("reward", "collective_reward", "step_type", "discount"), events: bool = False,
                observations=(), out=None, states=False, hashes=False, active=None,
                until=None, stopped=None, returns=False, gamma: float = 1.0, worlds=None):
    """K steps of every world in ONE launch, bit-identical to K calls of step() (fields=True:
    step_fields()) with actions[0] .. actions[K - 1]; returns the per-step transitions.

    actions: integers [K, N, P] ([K, N, P, A] with fields=True), or one block [N, P] with
    repeat=K (action repeat).  A device int32 tensor is read in place and may be
    non-contiguous along K only (a column slice [:, a:b] of a wider tensor); a host array is
    uploaded once.  1 <= K <= STEP_MANY_MAX.
    keep: which of "reward" f64 [K, N, P], "collective_reward" f64 [K, N], "step_type" i32
    [K, N], "discount" f64 [K, N] to stack per step; events=True adds "events" i32
    [K, N, EVENT_ROWS, 4] (rows beyond a header's count are not written).  Returned as a dict
    by name; out= (a previous result) reuses its tensors.  The in-place / bound buffers hold
    step K's values as after K steps; pixel views, a bound LAYER and a ring slot are written
    once, from the final state.
    observations: OBS_* kinds other than the pixel kinds (OBS_LAYER, OBS_READY_TO_SHOOT,
    OBS_POSITION, OBS_INVENTORY, ...) to stack per step as well, each returned under its kind as
    a tensor of shape (K,) + self.shapes[kind]: row k is what the kind's in-place (or bound)
    buffer holds after step k of the loop of step(), carried from row k - 1 wherever step k
    writes nothing (a frozen world; OBS_INTERACTION_REWARDS between interactions).  OBS_LAYER
    need not be bound.  A debug kind must be produced (bound, or debug_observations).
    states: True (or a tensor under out["states"]) adds "states", uint8 [K, N, S] with S =
    info.world_state_bytes: row k of a started world is what save_worlds() gives after step k of
    the loop (a world never reset writes nothing).  Each [k] loads with load_worlds and draws
    with observe_states like any bank.
    hashes: True (or a tensor under out["hashes"]) adds "hashes", int64 [K, N]: row k of a started
    world is hash_worlds() after step k of the loop — the hash (default spec) of what the state
    row's row k holds, at 8 bytes a world-step (a world never reset writes nothing).
    active: a mask of the world-steps to run, uint8 or bool [K, N], or [N] (the same row at every
    step); a device tensor is read in place and may be a column slice [:, a:b], a host array or
    a nested list is uploaded once.  World w runs step k only where active[k, w] is non-zero;
    elsewhere it is not touched (its record, counters, in-place outputs and events stay what they
    were), and row k of everything stacked per step repeats row k - 1 (row 0: the buffer as it was
    before the call) — so rewards of skipped steps REPEAT: sum them under the mask.  The result
    equals the loop of step(actions[k], active=active[k]).  Refused with a rollout ring bound.
    None: exactly the request issued without it.
    until: "last", "reward" or an iterable of both: a world stops INSIDE the call on the step that
    leaves it on LAST (step_type 2), or that pays some player a non-zero reward, and skips the
    steps behind it exactly as active= skips a step (it stands on the step that stopped it; its
    rows repeat).  The call equals the loop of step(actions[k], active=active[k] & (stopped == 0))
    with stopped updated from what each step left.
    stopped: a device uint8 tensor [N], read and written in place: a world whose byte is non-zero
    on entry does not run in this call and keeps its byte; a world that stops gets its reason bits
    (MP_STOP_LAST = 1, MP_STOP_REWARD = 2).  Hand the same tensor to call after call and the
    condition persists without the host; zero a byte and the world runs again (a world stopped on
    LAST then takes its reset, or its registered episode start).  None: every world starts
    unstopped and a new tensor is returned.
    returns: True, or a float64 tensor [N, P] to write in place: the sum over the steps world w
    ran, in step order, of gamma ** j * reward (j counts the steps that ran), every multiply and add
    rounded in float64 on its own.  It is this call's sum.
    With any of until=, stopped=, returns= the result gains "stopped" (uint8 [N]) and "ran" (int32
    [N]: the steps each world ran in this call; out["ran"] is reused), and "returns" when asked
    for; with none of them the call issues exactly the request it issues without them.
    worlds: a list of M world indices, 1 <= M <= N — a device int32 tensor [M] is read in place, a
    host list or array is uploaded once.  The launch then has one wave per ENTRY (ceil(M / 4)
    workgroups whatever N is) and entry i steps world worlds[i]; a world no entry names is not
    touched, as under a mask.  Everything per world above has M columns, by entry: actions
    [K, M, P], active [K, M] or [M], every stacked tensor (K, M) + ..., "states" [K, M, S],
    "hashes" [K, M], "ran" [M], "returns" [M, P], and row k of entry i is what the masked call over
    all N worlds leaves in row k of world worlds[i].  "stopped" stays [N], by WORLD: it is the
    tensor that persists over calls, which may name different lists; it is part of the result
    only with until=, stopped= or returns=.  An entry that is no world, or that repeats an earlier
    entry's world (the lowest entry steps it), runs nothing and leaves its elements of every
    tensor as they were; the next synchronising call raises ValueError once, naming it.  Refused
    with a rollout ring bound.  None: exactly the request issued without it.
    Enqueued on the current stream; does not synchronise."""
    t = self._torch
    listed = worlds is not None
    C = self.N   # the columns of every per-call tensor: N, or the entries of worlds=
    if listed:
      C = check_step_listed(worlds, self.N, self.P)
      if isinstance(worlds, t.Tensor) and worlds.device != self.device:
        raise ValueError(f"step_many: worlds= lives on {worlds.device}, the engine on {self.device}")
      if isinstance(worlds, t.Tensor) and worlds.dtype == t.int32 and worlds.is_contiguous():
        wl = worlds
      else:
        wl = self._device_ints(worlds, "worlds")
    stopping = until is not None or stopped is not None or (returns is not None and returns is not False)
    if stopping:
      stop = check_step_until(self.N, self.P, until=until, stopped=stopped, gamma=gamma, device=self.device)
      check_step_until(C, self.P, returns=returns, ran=None if out is None else out.get("ran"),
                       device=self.device)
    elif float(gamma) != 1.0:
      raise ValueError("step_many: gamma= goes with returns=")
    A = int(self.info.num_action_fields) if fields else None
    if isinstance(actions, t.Tensor) and actions.is_cuda:
      if actions.dtype != t.int32:
        raise ValueError(f"step_many: a device tensor of actions must be int32 (got {actions.dtype})")
      K = check_step_many(actions.shape, actions.dtype, C, self.P, repeat=repeat, num_fields=A)
      if actions.device != self.device:
        raise ValueError(f"step_many: actions live on {actions.device}, the engine on {self.device}")
    else:
      a = actions.cpu().numpy() if isinstance(actions, t.Tensor) else np.asarray(actions)
      K = check_step_many(a.shape, a.dtype, C, self.P, repeat=repeat, num_fields=A)
      actions = t.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.device)
    astep = 0 if repeat is not None else _step_distance(actions, "actions")
    if repeat is not None and not actions.is_contiguous():
      raise ValueError("step_many: the repeated block of actions must be contiguous")
    mask = None
    if active is not None:
      mask, mask_step = check_step_active(active, K, C)
      if isinstance(mask, np.ndarray):
        mask = t.from_numpy(mask).to(self.device)
      elif mask.device != self.device:
        raise ValueError(f"step_many: active= lives on {mask.device}, the engine on {self.device}")
    names = [k for k in STEP_MANY_KINDS if k in tuple(keep) or (k == "events" and events)]
    unknown = [k for k in keep if k not in STEP_MANY_KINDS[:4]]
    if unknown:
      raise ValueError(f"step_many: keep= knows {STEP_MANY_KINDS[:4]} (got {unknown})")
    kinds = check_step_rows(observations, taken=[STEP_MANY_NAMES[n] for n in names])
    states = bool(states) or (out is not None and out.get("states") is not None)
    hashes = bool(hashes) or (out is not None and out.get("hashes") is not None)
    # (registered episode statistics read the REWARD, STEP_TYPE and EVENTS rows of the launch: rows
    # nobody asked for go to scratch tensors of the engine's and stay out of the result)
    hidden = []
    if self._stats is not None:
      need = ["reward", "step_type"] + (["events"] if self._stats.columns or self._stats.pair_columns else [])
      hidden = [n for n in need if n not in names and STEP_MANY_NAMES[n] not in kinds]
    keys = names + list(kinds) + (["states"] if states else []) + (["hashes"] if hashes else []) + hidden
    rows = (MpStepRow * len(keys))()
    result = {}
    for i, key in enumerate(keys):
      if i >= len(keys) - len(hidden):
        kind, per_world, dtype = step_row(self.shapes, key)
        buf = self._stats_scratch.get(key)
        if buf is None or tuple(buf.shape) != (K, C) + per_world:
          buf = self._stats_scratch[key] = t.empty((K, C) + per_world, dtype=dtype, device=self.device)
        rows[i].kind, rows[i].rows, rows[i].step_bytes = kind, buf.data_ptr(), _step_distance(buf, key)
        continue
      if key == "states":
        kind, per_world, dtype = STEP_ROW_STATE, (int(self.info.world_state_bytes),), t.uint8
      elif key == "hashes":
        kind, per_world, dtype = STEP_ROW_HASH, (), t.int64
      else:
        kind, per_world, dtype = step_row(self.shapes, key)
      shape = (K, C) + per_world
      buf = None if out is None else out.get(key)
      if buf is None:
        buf = t.empty(shape, dtype=dtype, device=self.device)
      elif (not isinstance(buf, t.Tensor) or buf.dtype != dtype or tuple(buf.shape) != shape or
            buf.device != self.device):
        raise ValueError(f"step_many: out[{key!r}] must be a {dtype} tensor of shape {shape} on {self.device}")
      rows[i].kind = kind
      rows[i].rows = buf.data_ptr()
      rows[i].step_bytes = _step_distance(buf, f"out[{key!r}]")
      result[key] = buf
    self.use_current_stream()
    if stopping:
      ran = None if out is None else out.get("ran")
      if ran is None:
        ran = t.empty((C,), dtype=t.int32, device=self.device)
      if stopped is None:
        stopped = t.zeros((self.N,), dtype=t.uint8, device=self.device)
      if returns is True:
        returns = None if out is None else out.get("returns")
        if returns is None:
          returns = t.empty((C, self.P), dtype=t.float64, device=self.device)
        else:
          check_step_until(C, self.P, returns=returns, device=self.device)
      kind = MpStepListed if listed else MpStepUntil
      req = kind(ctypes.sizeof(kind), K, 1 if fields else 0, len(rows))
      if active is not None:
        req.active = mask.data_ptr()
        req.active_step_bytes = mask_step
      req.stop = stop
      req.stopped = stopped.data_ptr()
      req.ran = ran.data_ptr()
      req.gamma = float(gamma)
      result["stopped"], result["ran"] = stopped, ran
      if returns is not None and returns is not False:
        req.returns = returns.data_ptr()
        result["returns"] = returns
    elif listed:   # (the stopping request with nothing that stops a world)
      req = MpStepListed(ctypes.sizeof(MpStepListed), K, 1 if fields else 0, len(rows))
      req.gamma = 1.0
      if self._stats is not None:   # (which steps ran is read from it)
        ran = self._stats_scratch.get("ran")
        if ran is None or tuple(ran.shape) != (C,):
          ran = self._stats_scratch["ran"] = t.empty((C,), dtype=t.int32, device=self.device)
        req.ran = ran.data_ptr()
      if active is not None:
        req.active = mask.data_ptr()
        req.active_step_bytes = mask_step
    elif active is not None:
      req = MpStepActive(ctypes.sizeof(MpStepActive), K, 1 if fields else 0, len(rows))
      req.active = mask.data_ptr()
      req.active_step_bytes = mask_step
    else:
      req = MpStepTrajectory(ctypes.sizeof(MpStepTrajectory), K, 1 if fields else 0, len(rows))
    req.actions = actions.data_ptr()
    req.actions_step_bytes = astep
    req.rows = rows
    if listed:
      req.worlds = wl.data_ptr()
      req.count = C
    _send(self._L, self._h, req)
    self._state_args = (actions, result, mask, wl if listed else None)   # (kept until the next call: the launch may not have run yet)
    return result

  def observe(self, kind: int, out=None):
    if out is None:
      out = self.empty(kind)
    _check(self._L, self._L.mp_observe(self._h, kind, out.data_ptr()),
           "mp_observe")
    return out

  def observe_host(self, kind: int) -> np.ndarray:
    """Observation `kind` of all worlds as a host array (synchronises)."""
    return self.observe(kind).cpu().numpy()

  # -- introspection -------------------------------------------------------
  def dump(self):
    i = self.info
    grid = np.zeros((self.N, i.num_layers, i.map_h, i.map_w), np.uint8)
    avat = np.zeros((self.N, self.P, 8), np.int32)
    glob = np.zeros((self.N, 8), np.int32)
    _check(self._L, self._L.mp_dump(self._h, grid.ctypes.data,
                                    avat.ctypes.data, glob.ctypes.data),
           "mp_dump")
    return grid, avat, glob

  def snapshot(self) -> np.ndarray:
    n = int(self._L.mp_snapshot_bytes(self._h))
    buf = np.zeros(n, np.uint8)
    _check(self._L, self._L.mp_snapshot(self._h, buf.ctypes.data, n),
           "mp_snapshot")
    return buf

  def restore(self, buf: np.ndarray):
    buf = np.ascontiguousarray(buf, np.uint8)
    _check(self._L, self._L.mp_restore(self._h, buf.ctypes.data, buf.size),
           "mp_restore")

  # -- world states (include/mp_engine.h: MpWorldStates requests) --
  @property
  def state_fingerprint(self) -> int:
    """MP_STATES_FINGERPRINT: rows saved by this engine load into engines with the same value."""
    return int(world_states_request(self._L, self._h, MP_STATES_FINGERPRINT).fingerprint)

  def _device_ints(self, values, what: str):
    """`values` as a contiguous int32 tensor on the engine's device."""
    t = self._torch
    if isinstance(values, t.Tensor):
      if values.dtype not in (t.int8, t.int16, t.int32, t.int64, t.uint8):
        raise ValueError(f"{what} must hold integers (got {values.dtype})")
      return values.to(device=self.device, dtype=t.int32).contiguous().reshape(-1)
    a = np.asarray(values)
    if a.size and not np.issubdtype(a.dtype, np.integer):
      raise ValueError(f"{what} must hold integers (got {a.dtype})")
    return t.from_numpy(np.ascontiguousarray(a.reshape(-1), np.int32)).to(self.device)

  def _rows(self, values, what: str):
    """None, or `values` as `_device_ints` gives them."""
    return None if values is None else self._device_ints(values, what)

  def _bank(self, who: str, bank) -> int:
    """M of `bank`, which must be a contiguous uint8 tensor [M, S] with M >= 1."""
    S = int(self.info.world_state_bytes)
    if not _is_bank(bank, S):
      raise ValueError(f"{who}: bank must be a contiguous uint8 tensor [M, {S}]")
    if bank.shape[0] < 1:
      raise ValueError(f"{who}: the bank has no rows")
    return int(bank.shape[0])

  def _fingerprint(self, fingerprint: Optional[int]) -> int:
    """The rows' fingerprint: the caller's, by default this engine's."""
    return self.state_fingerprint if fingerprint is None else int(fingerprint)

  def _out(self, who: str, out, shape, dtype, *, torch_name: bool = False, anywhere: bool = False):
    """`out` of a request: a new tensor, or the caller's once it is contiguous and has the shape, the
    dtype and (unless `anywhere`) the device.  `torch_name`: the message says "torch.int32", not "int32"."""
    t = self._torch
    if out is None:
      return t.empty(shape, dtype=dtype, device=self.device)
    if (not isinstance(out, t.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or
        not out.is_contiguous() or not (anywhere or out.device == self.device)):
      raise ValueError(f"{who}: out must be a contiguous {dtype if torch_name else str(dtype).split('.')[-1]} "
                       f"tensor of shape {shape}" + ("" if anywhere else f" on {self.device}"))
    return out

  def save_worlds(self, worlds=None, out=None):
    """Row i of a uint8 [M, S] device tensor = the record of world worlds[i] (None: every world,
    M = N); S = info.world_state_bytes.  `out`: the tensor to write (allocated when None).
    Enqueued on the current stream; does not synchronise."""
    t = self._torch
    self.use_current_stream()
    S = int(self.info.world_state_bytes)
    w = self._rows(worlds, "worlds")
    M = self.N if w is None else int(w.numel())
    if M < 1:
      raise ValueError("save_worlds: no worlds to save")
    out = self._out("save_worlds", out, (M, S), t.uint8, anywhere=True)
    world_states_request(self._L, self._h, MP_STATES_SAVE, worlds=None if w is None else w.data_ptr(),
                         count=M, bank=out.data_ptr(), bank_bytes=out.numel())
    self._state_args = w   # (kept until the next call: the launch may not have run yet)
    return out

  def state_layout(self) -> StateLayout:
    """What the bytes of this engine's rows are (an MpStateLayout request)."""
    if getattr(self, "_layout", None) is None:
      self._layout = _layout_request(self._L, self._h)
    return self._layout

  def check_states(self, bank, rows=None, out=None, fingerprint: Optional[int] = None):
    """Verdicts int32 [R, 2] = (rule, offset word) of rows of `bank` (uint8 [M, S] device tensor),
    judged where they lie by one launch: (0, 0) is a well-formed row, anything else names the
    smallest rule the row breaks (RULE_*) and the byte (`state_layout().describe`).  rows: the
    rows to judge, in order, repeats allowed (None: every row).  Nothing of the engine's is
    written.  `fingerprint`: the rows' (default: this engine's).  Enqueued on the current stream;
    does not synchronise."""
    M = self._bank("check_states", bank)
    r = self._rows(rows, "rows")
    count = M if r is None else int(r.numel())
    if count < 1:
      raise ValueError("check_states: no rows to judge")
    out = self._out("check_states", out, (count, 2), self._torch.int32)
    fp = self._fingerprint(fingerprint)
    self.use_current_stream()
    req = MpStatesCheck(ctypes.sizeof(MpStatesCheck), MP_CHECK_ROWS, fp)
    req.bank, req.bank_rows, req.count = bank.data_ptr(), M, count
    req.rows = None if r is None else r.data_ptr()
    req.out, req.out_bytes = out.data_ptr(), out.numel() * 4
    _send(self._L, self._h, req)
    self._check_args = (bank, r, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def _hash(self, what: str, op: int, bank, index, out, planes, fields, fingerprint: int):
    """One MpStatesHash request (`index`: the rows or worlds, or None; `bank`: None for the
    engine's own records)."""
    r = self._rows(index, "rows" if bank is not None else "worlds")
    count = (int(bank.shape[0]) if bank is not None else self.N) if r is None else int(r.numel())
    if count < 1:
      raise ValueError(f"{what}: nothing to hash")
    out = self._out(what, out, (count,), self._torch.int64)
    spec = hash_spec(self.state_layout(), planes, fields)
    self.use_current_stream()
    req = _hash_request(op, spec, fingerprint)
    if bank is not None:
      req.bank, req.bank_rows = bank.data_ptr(), int(bank.shape[0])
    req.count = count
    req.rows = None if r is None else r.data_ptr()
    req.out, req.out_bytes = out.data_ptr(), count * 8
    _send(self._L, self._h, req)
    self._hash_args = (bank, r, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def hash_states(self, bank, rows=None, out=None, planes=None, fields=None, fingerprint: Optional[int] = None):
    """int64 [R] device tensor: the 64-bit state hash (the u64's bits) of rows of `bank` (uint8
    [M, S] device tensor from save_worlds or step_many(states=True)), computed where the rows lie
    by one launch.  Two records hash alike iff they agree in every byte a state's future and its
    observations depend on: ctr[] and reward_fx (the destination engine's bookkeeping), the
    cached visiting orders, the padding and the bytes of avatars >= P do not count.  `torch.unique(
    h, return_inverse=True)` is the dedup.  rows: the rows to hash, in order, repeats allowed (None:
    every row).  planes / fields: a custom spec (`hash_spec`) — an iterable of grid planes, an
    iterable of tail field names plus "player_block"; both None: "the state".  The first request
    with a NEW custom spec waits for the stream once to install its mask; the default spec and a
    repeated custom spec only enqueue.  Nothing of the engine's is written.  Hashes compare only
    between rows of one fingerprint, hashed with one spec.  `fingerprint`: the rows' (default:
    this engine's).  Enqueued on the current stream; does not synchronise."""
    self._bank("hash_states", bank)
    return self._hash("hash_states", MP_HASH_ROWS, bank, rows, out, planes, fields, self._fingerprint(fingerprint))

  def hash_worlds(self, worlds=None, out=None, planes=None, fields=None):
    """int64 [M] device tensor: `hash_states` of the records of `worlds` (None: every world, M =
    N) where they lie — equal to hash_states(save_worlds(worlds)) without the copy."""
    return self._hash("hash_worlds", MP_HASH_WORLDS, None, worlds, out, planes, fields, 0)

  def load_worlds(self, bank, src, fingerprint: Optional[int] = None, check: bool = False):
    """World w starts from row src[w] of `bank` (uint8 [M, S] device tensor from save_worlds, of
    this engine or another with the same state_fingerprint); src[w] = -1 leaves world w alone.
    One launch, shaped like a masked reset: the bound views and ring slot are written by it.
    `fingerprint`: the rows' (default: this engine's).  check=True: the rows src names are judged
    first (`check_states`' rules, one more launch) and a world whose row is malformed is left as
    it is; the next synchronising call (`sync`) raises ValueError naming the world, the row and
    the rule.  Enqueued on the current stream."""
    M = self._bank("load_worlds", bank)
    s = self._device_ints(src, "src")
    if s.numel() != self.N:
      raise ValueError(f"load_worlds: src must have {self.N} entries (got {s.numel()})")
    fp = self._fingerprint(fingerprint)
    self.use_current_stream()
    if check:
      checked = self._torch.empty_like(s)
      req = MpStatesCheck(ctypes.sizeof(MpStatesCheck), MP_CHECK_FILTER, fp)
      req.bank, req.bank_rows, req.count = bank.data_ptr(), M, self.N
      req.rows, req.out, req.out_bytes = s.data_ptr(), checked.data_ptr(), self.N * 4
      _send(self._L, self._h, req)
      loaded = checked
    else:
      loaded = s
    world_states_request(self._L, self._h, MP_STATES_LOAD, bank=bank.data_ptr(), bank_rows=M,
                         src=loaded.data_ptr(), fingerprint=fp)
    self._state_args = (s, loaded)   # (kept until the next call: the launches may not have run yet)

  # -- episode starts (include/mp_engine.h: an MpEpisodeStarts request) --
  def set_episode_starts(self, bank, rows, *, fresh: bool = False, verdicts=None,
                         fingerprint: Optional[int] = None):
    """From now on a world that auto-resets starts from row rows[w] of `bank` (uint8 [M, S] device
    tensor from save_worlds or step_many(states=True)) instead of the level's own first frame;
    rows[w] = -1 keeps the level's reset.  `rows`: int32 [N] device tensor, read by every later
    step (each of the K steps of step_many too) at the moment a world's episode ends — rewrite it
    whenever you like.  A started world is what load_worlds of the row gives (FIRST, the row's
    observations; the world keeps its own counters), and the start counts as an episode.
    verdicts: check_states(bank) of the whole bank — a row whose verdict is not (0, 0) is never
    read.  A bad index or a refused row gives the level's own reset, and the next synchronising
    call raises ValueError naming world, index and rule.  fresh=True: the started world keeps its
    own seed and episode count, so worlds that share a row draw differently.  `fingerprint`: the
    rows' (default: this engine's).  The engine keeps references to the tensors and never writes
    the bank.  While set, a step with a bound pixel view is two launches (`fused` is False).
    No launch; does not synchronise."""
    M = check_episode_starts(bank, rows, verdicts, self.N, int(self.info.world_state_bytes), self.device)
    if not isinstance(fresh, (bool, np.bool_)):
      raise ValueError(f"set_episode_starts: fresh must be True or False (got {fresh!r})")
    fp = self._fingerprint(fingerprint)
    req = MpEpisodeStarts(ctypes.sizeof(MpEpisodeStarts), 1 if fresh else 0, fp)
    req.bank, req.rows, req.bank_rows = bank.data_ptr(), rows.data_ptr(), M
    req.verdicts = None if verdicts is None else verdicts.data_ptr()
    _send(self._L, self._h, req)
    self._episode_starts = {"bank": bank, "rows": rows, "verdicts": verdicts, "fresh": bool(fresh),
                            "fingerprint": fp}

  def clear_episode_starts(self):
    """Episodes start from the level's own map again; the engine's launches are what they were."""
    req = MpEpisodeStarts(ctypes.sizeof(MpEpisodeStarts))
    _send(self._L, self._h, req)
    self._episode_starts = None

  @property
  def episode_starts(self):
    """The registration as a dict (bank, rows, verdicts, fresh, fingerprint), or None."""
    return None if self._episode_starts is None else dict(self._episode_starts)

  # -- episode statistics (include/mp_engine.h: an MpEpisodeStats request) --
  def event_columns(self):
    """The default columns of this engine's level: for every event type its rules can push, one
    unfiltered column per player-valued payload key ("zap.source", "zap.target", ...)."""
    return level_event_columns(int(self.info.substrate))

  def _torch_ptr(self, x):
    return x.data_ptr()

  def set_episode_stats(self, columns="default", pairs=(), out: Optional[EpisodeStats] = None) -> EpisodeStats:
    """From now on every submission (reset, step, step_fields, step_many in every form,
    load_worlds) is followed on the same stream, without synchronisation, by ONE launch that folds
    what it wrote into per-world statistics on the device: per-player returns, lengths and event
    counts of the running episode, of the last finished one and of all finished ones (the rule:
    include/mp_engine.h, MpEpisodeStats).  columns: names like "zap.source",
    "mining.player[ore_type=2]" ("default": event_columns(); (): returns and lengths only);
    pairs: pair columns like "zap.source>target".  out: an EpisodeStats whose tensors to use (a
    mixture hands each member a slice of one set); None allocates zeroed ones.  Returns the
    EpisodeStats; read its tensors in stream order.  A K-step call then carries the REWARD,
    STEP_TYPE and (with columns) EVENTS rows even when not asked for: the EVENTS row is K x
    columns x 2 KB.  None clears the registration (clear_episode_stats)."""
    if columns is None:
      self.clear_episode_stats()
      return None
    t = self._torch
    names, cols = _column_array(self.event_columns() if isinstance(columns, str) and columns == "default" else columns,
                                STATS_MAX_COLUMNS, False, "set_episode_stats")
    pnames, pcols = _column_array(pairs, STATS_MAX_PAIRS, True, "set_episode_stats")
    want = episode_stats_arrays(self.N, self.P, len(names), len(pnames),
                                lambda shape, dtype: (shape, getattr(t, dtype)))
    if out is None:
      arrays = episode_stats_arrays(self.N, self.P, len(names), len(pnames),
                                    lambda shape, dtype: t.zeros(shape, dtype=getattr(t, dtype), device=self.device))
      out = EpisodeStats(names, pnames, arrays)
    else:
      if tuple(out.columns) != names or tuple(out.pair_columns) != pnames:
        raise ValueError("set_episode_stats: out= was made for other columns")
      for key, value in want.items():
        for sub, (shape, dtype) in (value.items() if isinstance(value, dict) else [(None, value)]):
          a = out.arrays[key] if sub is None else out.arrays[key][sub]
          if (not isinstance(a, t.Tensor) or tuple(a.shape) != shape or a.dtype != dtype or
              a.device != self.device or not a.is_contiguous()):
            raise ValueError(f"set_episode_stats: out.{key}{'' if sub is None else '[' + repr(sub) + ']'} must be "
                             f"a contiguous {dtype} tensor of shape {shape} on {self.device}")
    req = _stats_request(MP_STATS_REGISTER, cols, len(names), pcols, len(pnames), out.arrays, self._torch_ptr)
    _send(self._L, self._h, req)
    self._stats = out
    self._stats_scratch = {}
    return out

  def clear_episode_stats(self):
    """No statistics launch any more: the engine issues exactly the launches it issued before."""
    req = MpEpisodeStats(ctypes.sizeof(MpEpisodeStats), MP_STATS_CLEAR)
    _send(self._L, self._h, req)
    self._stats = None
    self._stats_scratch = {}

  @property
  def episode_stats(self) -> Optional[EpisodeStats]:
    return self._stats

  episode_stats_host = staticmethod(episode_stats_host)

  def tally_events(self, events_rows, columns=None, active=None, ran=None, out=None, pairs=()):
    """Event counts of raw event rows, on the device: events_rows int32 [K, M, EVENT_ROWS, 4] (what
    step_many(events=True) returns; [M, EVENT_ROWS, 4] is K = 1) -> int32 [M, C, P], the rows of
    every column (None: event_columns()) summed over the steps that ran: all of them, or those
    where active ([K, M] uint8 / bool) is non-zero, of them the first ran[i] (int32 [M]).  With
    pairs= returns (counts, pairs int32 [M, C2, P, P]).  The kernel of the episode statistics
    without the episode logic; one launch, no synchronisation."""
    t = self._torch
    names, cols = _column_array(self.event_columns() if columns is None else columns, STATS_MAX_COLUMNS, False,
                                "tally_events")
    pnames, pcols = _column_array(pairs, STATS_MAX_PAIRS, True, "tally_events")
    ev = events_rows
    if not isinstance(ev, t.Tensor):
      ev = t.from_numpy(np.ascontiguousarray(ev, np.int32)).to(self.device)
    if ev.dim() == 3:
      ev = ev[None]
    if (ev.dtype != t.int32 or ev.dim() != 4 or tuple(ev.shape[2:]) != (EVENT_ROWS, 4) or ev.device != self.device):
      raise ValueError(f"tally_events: events_rows must be int32 [K, M, {EVENT_ROWS}, 4] on {self.device}")
    ev = ev.contiguous()
    K, M = int(ev.shape[0]), int(ev.shape[1])
    if K < 1 or M < 1:
      raise ValueError("tally_events: no event rows")
    def dev(x, dtype, shape, what):
      if x is None:
        return None
      if not isinstance(x, t.Tensor):
        x = t.from_numpy(np.ascontiguousarray(x)).to(self.device)
      if x.dtype == t.bool:
        x = x.to(t.uint8)
      if x.dtype != dtype or tuple(x.shape) != shape or x.device != self.device:
        raise ValueError(f"tally_events: {what} must be a {dtype} tensor of shape {shape} on {self.device}")
      return x.contiguous()
    active = dev(active, t.uint8, (K, M), "active")
    ran = dev(ran, t.int32, (M,), "ran")
    shape = (M, len(names), self.P)
    if out is None:
      out = t.empty(shape, dtype=t.int32, device=self.device)
    elif (not isinstance(out, t.Tensor) or out.dtype != t.int32 or tuple(out.shape) != shape or
          out.device != self.device or not out.is_contiguous()):
      raise ValueError(f"tally_events: out must be a contiguous int32 tensor of shape {shape} on {self.device}")
    pout = t.empty((M, len(pnames), self.P, self.P), dtype=t.int32, device=self.device)
    self.use_current_stream()
    req = _stats_request(MP_STATS_TALLY, cols, len(names), pcols, len(pnames), None, None)
    req.running.counts = out.data_ptr() if names else None
    req.running.pairs = pout.data_ptr() if pnames else None
    req.events, req.steps, req.count = ev.data_ptr(), K, M
    req.active = None if active is None else active.data_ptr()
    req.ran = None if ran is None else ran.data_ptr()
    _send(self._L, self._h, req)
    self._tally_args = (ev, active, ran, out, pout)   # (kept until the next call: the launch may not have run yet)
    return (out, pout) if pnames else out

  def observe_states(self, bank, kind: int, rows=None, out=None, fingerprint: Optional[int] = None):
    """Observation `kind` of rows of `bank` (uint8 [M, S] device tensor from save_worlds or
    step_many(states=True)[k], of this engine or another with the same state_fingerprint),
    drawn where the rows lie: no world is loaded and nothing of the engine's — records, outputs,
    ring, plans — is written.  rows: the rows to draw, in order, repeats allowed (None: every row
    of the bank).  Returns a tensor of shape (count,) + self.shapes[kind][0][1:] (`out`: the tensor to
    write).  `kind` is one of STATE_OBS_KINDS: a pixel view, OBS_LAYER, OBS_READY_TO_SHOOT,
    OBS_POSITION, OBS_ORIENTATION, OBS_INVENTORY — equal to what observe() / a load_worlds of the
    row gives; the transition kinds are not functions of a record and are refused.
    `fingerprint`: the rows' (default: this engine's).  Enqueued on the current stream."""
    M = self._bank("observe_states", bank)
    if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or int(kind) not in self.shapes:
      raise ValueError(f"observe_states: {kind!r} is no observation kind")
    kind = int(kind)
    r = self._rows(rows, "rows")
    count = M if r is None else int(r.numel())
    if count < 1:
      raise ValueError("observe_states: no rows to draw")
    shape, dtype = self.shapes[kind]
    out = self._out("observe_states", out, (count,) + tuple(int(d) for d in shape[1:]), dtype, torch_name=True)
    self.use_current_stream()
    states_observe_request(self._L, self._h, kind=kind, fingerprint=self._fingerprint(fingerprint),
                           bank=bank.data_ptr(), bank_rows=M, rows=None if r is None else r.data_ptr(),
                           count=count, dst=out.data_ptr(), dst_bytes=out.numel() * out.element_size())
    self._state_args = (bank, r, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def observe_views(self, bank, kind: int, players, rows=None, out=None,
                    fingerprint: Optional[int] = None):
    """Observation `kind` of ONE player of each sampled row of `bank` (as observe_states' bank):
    element i is the view of player players[i] of row rows[i] (None: rows 0 .. count - 1) — the
    (state, player) samples of a replay minibatch, without the other players' views and without
    an [R, P, ...] intermediate.  Returns a tensor of shape (count,) + self.shapes[kind][0][2:]
    (`out`: the tensor to write; a pixel kind's may start on any byte), equal to
    observe_states(bank, kind, rows)[arange(count), players].  `kind`: a per-player kind of
    STATE_OBS_KINDS (not OBS_WORLD_RGB).  Rows and (row, player) pairs may repeat.  Nothing of the
    engine's is written and no device memory of the engine's is allocated.  A row or player index
    out of range leaves its element as it was; the next synchronising call raises ValueError.
    `fingerprint`: the rows' (default: this engine's).  Enqueued on the current stream."""
    M = self._bank("observe_views", bank)
    if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or int(kind) not in self.shapes:
      raise ValueError(f"observe_views: {kind!r} is no observation kind")
    kind = int(kind)
    if kind == OBS_WORLD_RGB:
      raise ValueError("observe_views: OBS_WORLD_RGB is not a per-player kind (observe_states draws it)")
    if players is None:
      raise ValueError("observe_views: players is required")
    p = self._device_ints(players, "players")
    r = self._rows(rows, "rows")
    count = int(p.numel())
    if count < 1:
      raise ValueError("observe_views: no views to draw")
    if r is not None and int(r.numel()) != count:
      raise ValueError(f"observe_views: rows has {int(r.numel())} entries, players {count}")
    shape, dtype = self.shapes[kind]
    out = self._out("observe_views", out, (count,) + tuple(int(d) for d in shape[2:]), dtype, torch_name=True)
    self.use_current_stream()
    states_view_request(self._L, self._h, kind=kind, fingerprint=self._fingerprint(fingerprint),
                        bank=bank.data_ptr(), bank_rows=M, rows=None if r is None else r.data_ptr(),
                        players=p.data_ptr(), count=count, dst=out.data_ptr(),
                        dst_bytes=out.numel() * out.element_size())
    self._state_args = (bank, r, p, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def _view_source(self, who: str, verb: str, bank, rows, players, fingerprint):
    """What observe_ego_layer, hash_views and observe_ego_planes read: the checked `bank` (None: the
    engine's worlds), `rows` and `players` as device ints, the count.  Returns (count, rows,
    players, the request's source fields)."""
    there = self.N if bank is None else self._bank(who, bank)
    p = self._rows(players, "players")
    r = self._rows(rows, "rows")
    count = int(p.numel()) if p is not None else int(r.numel()) if r is not None else there
    if count < 1:
      raise ValueError(f"{who}: no views to {verb}")
    if r is not None and int(r.numel()) != count:
      raise ValueError(f"{who}: rows has {int(r.numel())} entries, players {count}")
    fields = dict(fingerprint=self._fingerprint(fingerprint), bank=None if bank is None else bank.data_ptr(),
                  bank_rows=0 if bank is None else there,
                  rows=None if r is None else r.data_ptr(), players=None if p is None else p.data_ptr(), count=count)
    return count, r, p, fields

  @staticmethod
  def _view_ring(out, ring: bool, block: int):
    """The destination fields of a registration: `out` holds one block of `block` bytes, or with
    `ring` T slots of one along its first axis."""
    T = int(out.shape[0]) if ring else 0
    stride = (out.stride(0) * out.element_size() if T > 1 else block) if ring else 0
    return dict(dst=out.data_ptr(), dst_bytes=(T - 1) * stride + block if ring else block, slot_stride=stride,
                slots=T)

  @property
  def ego_layer_shape(self):
    """The shape of the EGO_LAYER leaf, [N, P, VH, VW, L] (OBS_LAYER's; int32)."""
    return tuple(int(d) for d in self.shapes[OBS_LAYER][0])

  def observe_ego_layer(self, bank=None, rows=None, players=None, fingerprint: Optional[int] = None, out=None):
    """EGO_LAYER — the layer view in the avatar's own frame, cell for cell what "RGB" shows — of
    rows of `bank` (a contiguous uint8 device tensor [M, S], as observe_states' bank), or of the
    engine's worlds as they are now (`bank` None; `rows` are then world indices).  `rows`: the
    rows to draw, in order, repeats allowed (None: rows 0 .. count - 1; all of them without
    `players`).  `players` None: int32 [R, P, VH, VW, L]; else R ints, and the result is int32
    [R, VH, VW, L], the view of player players[i] of row rows[i].  The ids are OBS_LAYER's, with
    no facing encoded; for a viewer that faces north the view equals OBS_LAYER's.  Nothing of the
    engine's is written and no device memory of the engine's is allocated.  A row or player index
    out of range leaves its element as it was; the next synchronising call raises ValueError.
    `fingerprint`: the rows' (default: this engine's).  Enqueued on the current stream."""
    count, r, p, src = self._view_source("observe_ego_layer", "draw", bank, rows, players, fingerprint)
    shape = self.ego_layer_shape
    shape = (count,) + (shape[1:] if p is None else shape[2:])
    out = self._out("observe_ego_layer", out, shape, self._torch.int32)
    self.use_current_stream()
    ego_layer_request(self._L, self._h, MP_EGO_DRAW, dst=out.data_ptr(), dst_bytes=out.numel() * 4, **src)
    self._state_args = (bank, r, p, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def bind_ego_layer(self, out):
    """Registers `out`, a contiguous int32 device tensor of `ego_layer_shape`, as the EGO_LAYER
    leaf: from now on every submission (reset, step, step_many in every form, a load) is followed
    on the same stream by one launch that redraws every world's view into it.  None clears the
    registration; the engine's launches are then what they were.  Returns `out`."""
    t = self._torch
    if out is None:
      ego_layer_request(self._L, self._h, MP_EGO_REGISTER)
      self._ego_layer = None
      return None
    out = self._out("bind_ego_layer", out, self.ego_layer_shape, t.int32)
    ego_layer_request(self._L, self._h, MP_EGO_REGISTER, **self._view_ring(out, False, out.numel() * 4))
    self._ego_layer = out
    return out

  def bind_ego_layer_ring(self, tensor=None, slots: Optional[int] = None):
    """The EGO_LAYER leaf as a rollout ring: `tensor` int32 [T, *ego_layer_shape] (allocated when
    None, `slots` = T), T the engine's ring slots (`bind_ring` some kind first): the launch behind
    a submission writes the slot that submission wrote.  Returns the tensor."""
    t = self._torch
    shape = self.ego_layer_shape
    if tensor is None:
      if not slots or slots < 1:
        raise ValueError("bind_ego_layer_ring needs a tensor or a positive number of slots")
      tensor = t.empty((int(slots),) + shape, dtype=t.int32, device=self.device)
    if (not isinstance(tensor, t.Tensor) or tuple(tensor.shape[1:]) != shape or tensor.dtype != t.int32 or
        tensor.dim() != len(shape) + 1):
      raise ValueError(f"an EGO_LAYER ring is int32 [T, {', '.join(map(str, shape))}]")
    if slots is not None and int(slots) != tensor.shape[0]:
      raise ValueError(f"{tensor.shape[0]} slots in the tensor, {slots} asked for")
    if not tensor[0].is_contiguous() or tensor.device != self.device:
      raise ValueError("the slots of a ring must be contiguous and on the engine's device")
    ego_layer_request(self._L, self._h, MP_EGO_REGISTER, **self._view_ring(tensor, True, int(np.prod(shape)) * 4))
    self._ego_layer = tensor
    return tensor

  @property
  def num_layer_ids(self) -> int:
    """The number of ids OBS_LAYER and EGO_LAYER can hold, 1 + the largest: the length of a
    `classes` table of `hash_views`."""
    if getattr(self, "_num_layer_ids", None) is None:
      self._num_layer_ids = int(view_hash_request(self._L, self._h, MP_VIEWHASH_DRAW).num_ids)
    return self._num_layer_ids

  def _view_classes(self, classes):
    """`classes` of a hash_views call as a contiguous int32 [num_layer_ids] device tensor (a device
    tensor of that form is taken as it is), or None."""
    if classes is None:
      return None
    t = self._torch
    if (isinstance(classes, t.Tensor) and classes.dtype == t.int32 and classes.device == self.device and
        classes.is_contiguous() and tuple(classes.shape) == (self.num_layer_ids,)):
      return classes
    host = classes.cpu().numpy() if isinstance(classes, t.Tensor) else classes
    return t.from_numpy(_view_classes(host, self.num_layer_ids)).to(self.device)

  def hash_views(self, bank=None, rows=None, players=None, layers=None, classes=None, out=None,
                 fingerprint: Optional[int] = None):
    """int64 device tensor: the 64-bit hash (the u64's bits) of what each player sees — of its
    EGO_LAYER, `observe_ego_layer`'s view — in rows of `bank` (a contiguous uint8 device tensor
    [M, S]), or in the engine's worlds as they are now (`bank` None; `rows` are then world
    indices), worked out from the records by one launch without drawing a view.  `rows`: the rows
    to hash, in order, repeats allowed (None: rows 0 .. count - 1; all of them without `players`).
    `players` None: int64 [R, P]; else R ints, and the result is int64 [R], the hash of player
    players[i] of row rows[i].  `layers`: the layer indices that count (None: all).  `classes`:
    `num_layer_ids` ints mapping every id to its class — two ids of one class hash alike — (None:
    the ids themselves); a contiguous int32 device tensor is read where it lies.  Two views hash
    alike iff they agree in every included word (up to a 2^-64 collision); a cell outside the
    window and an excluded layer never count.  `torch.unique(h, return_counts=True)` is the
    per-agent novelty count.  Nothing of the engine's is written and no device memory of the
    engine's is allocated.  A row or player index out of range leaves its element as it was; the
    next synchronising call raises ValueError.  Hashes compare only within one fingerprint and
    one choice of layers and classes.  Enqueued on the current stream."""
    count, r, p, src = self._view_source("hash_views", "hash", bank, rows, players, fingerprint)
    mask = view_layer_mask(layers, int(self.info.num_layers))
    cls = self._view_classes(classes)
    out = self._out("hash_views", out, (count, self.P) if p is None else (count,), self._torch.int64)
    self.use_current_stream()
    view_hash_request(self._L, self._h, MP_VIEWHASH_DRAW, layer_mask=mask,
                      classes=None if cls is None else cls.data_ptr(),
                      classes_len=0 if cls is None else int(cls.numel()), dst=out.data_ptr(),
                      dst_bytes=out.numel() * 8, **src)
    self._view_hash_args = (bank, r, p, cls, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def bind_view_hash(self, out, layers=None, classes=None):
    """Registers `out` — a contiguous int64 device tensor [N, P], or [T, N, P] with T the engine's
    ring slots (`bind_ring` some kind first) — as the view hashes: from now on every submission
    (reset, step, step_many in every form, a load) is followed on the same stream by one launch
    that rewrites every viewer's `hash_views` value into it, or into the ring slot the submission
    wrote.  `layers`, `classes`: as `hash_views` takes them; the engine keeps the class table alive.
    None clears the registration; the engine's launches are then what they were.  Returns `out`."""
    t = self._torch
    if out is None:
      view_hash_request(self._L, self._h, MP_VIEWHASH_REGISTER)
      self._view_hash = None
      return None
    shape = (self.N, self.P)
    ring = isinstance(out, t.Tensor) and out.dim() == 3
    if (not isinstance(out, t.Tensor) or out.dtype != t.int64 or tuple(out.shape[-2:]) != shape or
        out.dim() not in (2, 3) or not (out[0] if ring else out).is_contiguous() or out.device != self.device):
      raise ValueError(f"bind_view_hash: out must be an int64 tensor of shape {shape} or [T, {self.N}, {self.P}] "
                       f"with contiguous slots on {self.device}")
    mask = view_layer_mask(layers, int(self.info.num_layers))
    cls = self._view_classes(classes)
    view_hash_request(self._L, self._h, MP_VIEWHASH_REGISTER, layer_mask=mask,
                      classes=None if cls is None else cls.data_ptr(),
                      classes_len=0 if cls is None else int(cls.numel()),
                      **self._view_ring(out, ring, self.N * self.P * 8))
    self._view_hash = (out, cls)
    return out

  @property
  def layer_id_names(self) -> Tuple[str, ...]:
    """What every id of OBS_LAYER and EGO_LAYER shows: `num_layer_ids` strings, "" for id 0
    (nothing) and the name of sprite i - 1 for id i ("OutOfBounds" is id 1) — what a `classes`
    table is written by."""
    if getattr(self, "_layer_id_names", None) is None:
      from . import pack as pack_lib
      names = bytes(pack_lib.loads(self.pack_bytes)["sprite_names"]).split(b"\0")[:-1]
      self._layer_id_names = ("",) + tuple(names[i].decode() if i < len(names) else ""
                                           for i in range(self.num_layer_ids - 1))
    return self._layer_id_names

  def _plane_classes(self, classes, num_classes):
    """(`classes` of an ego-planes call as a contiguous int32 [num_layer_ids] device tensor, C).  A
    device tensor of that form is read where it lies and is not checked here (the kernel takes an
    entry outside [-1, C) as -1 and reports it); anything else is checked on the host."""
    t = self._torch
    if classes is None:
      raise ValueError("ego_planes: classes is needed: one class (or -1) per layer id (num_layer_ids)")
    if (isinstance(classes, t.Tensor) and classes.dtype == t.int32 and classes.device == self.device and
        classes.is_contiguous() and tuple(classes.shape) == (self.num_layer_ids,)):
      C = int(classes.max()) + 1 if num_classes is None else int(num_classes)
      if not 1 <= C <= EGO_PLANES_MAX_CLASSES:
        raise ValueError(f"ego_planes: num_classes {C} is outside [1, {EGO_PLANES_MAX_CLASSES}]")
      return classes, C
    host = classes.cpu().numpy() if isinstance(classes, t.Tensor) else classes
    table, C = _plane_classes(host, self.num_layer_ids, num_classes)
    return t.from_numpy(table).to(self.device), C

  def ego_planes_shape(self, num_classes: int, facing: bool = False) -> Tuple[int, ...]:
    """(N, P, C', VH, VW) of the planes of every viewer: C' = num_classes, + 4 with `facing`."""
    N, P, VH, VW, _ = self.ego_layer_shape
    return (N, P, int(num_classes) + (4 if facing else 0), VH, VW)

  def observe_ego_planes(self, classes, bank=None, rows=None, players=None, layers=None, facing: bool = False,
                         num_classes: Optional[int] = None, out=None, fingerprint: Optional[int] = None):
    """uint8 device tensor [R, P, C', VH, VW] (or [R, C', VH, VW] with `players`, R ints: player
    players[i] of row rows[i]): what a conv net reads of each player's view — channels-first 0/1
    planes of its EGO_LAYER, written from the records by one launch without drawing the int32
    view — in rows of `bank` (a contiguous uint8 device tensor [M, S]), or in the engine's worlds as
    they are now (`bank` None; `rows` are then world indices).  `classes`: `num_layer_ids` ints in
    [-1, C) mapping every id to its class (`layer_id_names` says which id is which sprite); class
    plane c is 1 where some counted layer of the cell holds an id of class c, and -1 sets nothing.
    C = `num_classes` (at most 64), by default 1 + the largest entry.  `layers`: the layer indices
    that count (None: all).  `facing`: four more planes, C' = C + 4: plane C + d is 1 where a living
    avatar stands that faces (ORIENTATION[q] - ORIENTATION[p]) & 3 == d in the viewer's frame (the
    viewer itself: d = 0); a dead viewer's are 0.  `out`: a uint8 tensor of the result's shape that
    may start on any byte.  A contiguous int32 device `classes` is read where it lies; an entry of
    it outside [-1, C) counts as -1 and the next synchronising call raises ValueError.  A row or
    player index out of range leaves its element as it was and is reported the same way.  Nothing
    of the engine's is written.  Enqueued on the current stream."""
    count, r, p, src = self._view_source("observe_ego_planes", "draw", bank, rows, players, fingerprint)
    mask = view_layer_mask(layers, int(self.info.num_layers))
    cls, C = self._plane_classes(classes, num_classes)
    shape = self.ego_planes_shape(C, facing)
    shape = (count,) + (shape[1:] if p is None else shape[2:])
    out = self._out("observe_ego_planes", out, shape, self._torch.uint8)
    self.use_current_stream()
    ego_planes_request(self._L, self._h, MP_EGOPLANES_DRAW, layer_mask=mask, classes=cls.data_ptr(),
                       classes_len=int(cls.numel()), num_classes=C, facing=int(bool(facing)), dst=out.data_ptr(),
                       dst_bytes=out.numel(), **src)
    self._ego_planes_args = (bank, r, p, cls, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def bind_ego_planes(self, out, classes=None, layers=None, facing: bool = False, num_classes: Optional[int] = None):
    """Registers `out` — a uint8 device tensor [N, P, C', VH, VW], or [T, N, P, C', VH, VW] with T
    the engine's ring slots (`bind_ring` some kind first); it may start on any byte — as the planes
    of the worlds: from now on every submission (reset, step, step_many in every form, a load) is
    followed on the same stream by one launch that rewrites `observe_ego_planes(classes, ...)` of
    every world into it, or into the ring slot the submission wrote.  `classes`, `layers`,
    `facing`, `num_classes`: as `observe_ego_planes` takes them; the engine keeps the class table
    alive.  None clears the registration; the engine's launches are then what they were.  Returns
    `out`."""
    t = self._torch
    if out is None:
      ego_planes_request(self._L, self._h, MP_EGOPLANES_REGISTER)
      self._ego_planes = None
      return None
    mask = view_layer_mask(layers, int(self.info.num_layers))
    cls, C = self._plane_classes(classes, num_classes)
    shape = self.ego_planes_shape(C, facing)
    ring = isinstance(out, t.Tensor) and out.dim() == len(shape) + 1
    if (not isinstance(out, t.Tensor) or out.dtype != t.uint8 or tuple(out.shape[-len(shape):]) != shape or
        out.dim() not in (len(shape), len(shape) + 1) or not (out[0] if ring else out).is_contiguous() or
        out.device != self.device):
      raise ValueError(f"bind_ego_planes: out must be a uint8 tensor of shape {shape} or [T, {', '.join(map(str, shape))}] "
                       f"with contiguous slots on {self.device}")
    ego_planes_request(self._L, self._h, MP_EGOPLANES_REGISTER, layer_mask=mask, classes=cls.data_ptr(),
                       classes_len=int(cls.numel()), num_classes=C, facing=int(bool(facing)),
                       **self._view_ring(out, ring, int(np.prod(shape))))
    self._ego_planes = (out, cls)
    return out

  # ---- the world camera: WORLD.LAYER and the world planes (the world ops of MpEgoLayer, MpEgoPlanes)

  @property
  def world_layer_shape(self):
    """The shape of the WORLD.LAYER leaf, [N, H, W, L] (int32)."""
    info = self.info   # (MpInfo, read at creation: nothing is parsed or asked per call)
    return (self.N, int(info.map_h), int(info.map_w), int(info.num_layers))

  def observe_world_layer(self, bank=None, rows=None, out=None, fingerprint: Optional[int] = None):
    """WORLD.LAYER — the layer view of the whole map, what "WORLD.RGB" is rendered from: int32
    [R, H, W, L], north up — of rows of `bank` (a contiguous uint8 device tensor [M, S], as
    observe_states' bank), or of the engine's worlds as they are now (`bank` None; `rows` are then
    world indices).  `rows`: the rows to draw, in order, repeats allowed (None: all of them).  Id i
    is sprite i - 1 after the WORLD's sprite map (`world_layer_id_names`); no cell is off the map
    and a dead avatar shows nowhere.  `(layer == id).sum()` counts things on the map.  Nothing of
    the engine's is written.  A row index out of range leaves its element as it was; the next
    synchronising call raises ValueError.  Enqueued on the current stream."""
    count, r, _, src = self._view_source("observe_world_layer", "draw", bank, rows, None, fingerprint)
    out = self._out("observe_world_layer", out, (count,) + self.world_layer_shape[1:], self._torch.int32)
    self.use_current_stream()
    ego_layer_request(self._L, self._h, MP_EGO_WORLD_DRAW, dst=out.data_ptr(), dst_bytes=out.numel() * 4, **src)
    self._state_args = (bank, r, None, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def bind_world_layer(self, out):
    """Registers `out` — a contiguous int32 device tensor of `world_layer_shape`, or [T, N, H, W, L]
    with T the engine's ring slots (`bind_ring` some kind first) — as the WORLD.LAYER leaf: from now
    on every submission (reset, step, step_many in every form, a load) is followed on the same
    stream by one launch that redraws every world's map into it, or into the ring slot the
    submission wrote.  None clears the registration; the engine's launches are then what they
    were.  Returns `out`."""
    t = self._torch
    if out is None:
      ego_layer_request(self._L, self._h, MP_EGO_WORLD_REGISTER)
      self._world_layer = None
      return None
    shape = self.world_layer_shape
    ring = isinstance(out, t.Tensor) and out.dim() == len(shape) + 1
    if (not isinstance(out, t.Tensor) or out.dtype != t.int32 or tuple(out.shape[-len(shape):]) != shape or
        out.dim() not in (len(shape), len(shape) + 1) or not (out[0] if ring else out).is_contiguous() or
        out.device != self.device):
      raise ValueError(f"bind_world_layer: out must be an int32 tensor of shape {shape} or "
                       f"[T, {', '.join(map(str, shape))}] with contiguous slots on {self.device}")
    ego_layer_request(self._L, self._h, MP_EGO_WORLD_REGISTER, **self._view_ring(out, ring, int(np.prod(shape)) * 4))
    self._world_layer = out
    return out

  @property
  def num_world_layer_ids(self) -> int:
    """The number of ids WORLD.LAYER can hold, 1 + the largest: the length of a `classes` table of
    `observe_world_planes`."""
    if getattr(self, "_num_world_layer_ids", None) is None:
      self._num_world_layer_ids = int(ego_planes_request(self._L, self._h, MP_EGOPLANES_WORLD_DRAW).num_ids)
    return self._num_world_layer_ids

  @property
  def world_layer_id_names(self) -> Tuple[str, ...]:
    """What every id of WORLD.LAYER shows: `num_world_layer_ids` strings, "" for id 0 (nothing) and
    the name of sprite i - 1 for id i, after the WORLD's sprite map."""
    if getattr(self, "_world_layer_id_names", None) is None:
      from . import pack as pack_lib
      names = bytes(pack_lib.loads(self.pack_bytes)["sprite_names"]).split(b"\0")[:-1]
      self._world_layer_id_names = ("",) + tuple(names[i].decode() if i < len(names) else ""
                                                 for i in range(self.num_world_layer_ids - 1))
    return self._world_layer_id_names

  def _world_plane_classes(self, classes, num_classes):
    """`_plane_classes` over the world's ids."""
    t = self._torch
    n = self.num_world_layer_ids
    if classes is None:
      raise ValueError("world_planes: classes is needed: one class (or -1) per id of WORLD.LAYER "
                       "(num_world_layer_ids)")
    if (isinstance(classes, t.Tensor) and classes.dtype == t.int32 and classes.device == self.device and
        classes.is_contiguous() and tuple(classes.shape) == (n,)):
      C = int(classes.max()) + 1 if num_classes is None else int(num_classes)
      if not 1 <= C <= EGO_PLANES_MAX_CLASSES:
        raise ValueError(f"world_planes: num_classes {C} is outside [1, {EGO_PLANES_MAX_CLASSES}]")
      return classes, C
    host = classes.cpu().numpy() if isinstance(classes, t.Tensor) else classes
    table, C = _plane_classes(host, n, num_classes)
    return t.from_numpy(table).to(self.device), C

  def world_planes_shape(self, num_classes: int, facing: bool = False) -> Tuple[int, ...]:
    """(N, C', H, W) of the world planes: C' = num_classes, + 4 with `facing`."""
    N, H, W, _ = self.world_layer_shape
    return (N, int(num_classes) + (4 if facing else 0), H, W)

  def observe_world_planes(self, classes, bank=None, rows=None, layers=None, facing: bool = False,
                           num_classes: Optional[int] = None, out=None, fingerprint: Optional[int] = None):
    """uint8 device tensor [R, C', H, W]: the whole map as channels-first 0/1 planes — a centralised
    critic's input (`planes.half()`) — written from the records by one launch, in rows of `bank` (a
    contiguous uint8 device tensor [M, S]) or in the engine's worlds as they are now (`bank` None;
    `rows` are then world indices).  `classes`: `num_world_layer_ids` ints in [-1, C) mapping every
    id of WORLD.LAYER to its class (`world_layer_id_names` says which id is which sprite); class
    plane c is 1 where some counted layer of the cell holds an id of class c, -1 sets nothing.
    C = `num_classes` (at most 64), by default 1 + the largest entry.  `layers`: the layer indices
    that count (None: all).  `facing`: four more planes, C' = C + 4: plane C + d is 1 where a living
    avatar stands that faces d (absolute, 0 = N).  `out`: a uint8 tensor of the result's shape that
    may start on any byte.  A contiguous int32 device `classes` is read where it lies; an entry of
    it outside [-1, C) counts as -1 and the next synchronising call raises ValueError, as it does
    for a row index out of range, whose element is left as it was.  Enqueued on the current stream."""
    count, r, _, src = self._view_source("observe_world_planes", "draw", bank, rows, None, fingerprint)
    mask = view_layer_mask(layers, int(self.info.num_layers))
    cls, C = self._world_plane_classes(classes, num_classes)
    out = self._out("observe_world_planes", out, (count,) + self.world_planes_shape(C, facing)[1:], self._torch.uint8)
    self.use_current_stream()
    ego_planes_request(self._L, self._h, MP_EGOPLANES_WORLD_DRAW, layer_mask=mask, classes=cls.data_ptr(),
                       classes_len=int(cls.numel()), num_classes=C, facing=int(bool(facing)), dst=out.data_ptr(),
                       dst_bytes=out.numel(), **src)
    self._world_planes_args = (bank, r, cls, out)   # (kept until the next call: the launch may not have run yet)
    return out

  def bind_world_planes(self, out, classes=None, layers=None, facing: bool = False, num_classes: Optional[int] = None):
    """Registers `out` — a uint8 device tensor [N, C', H, W], or [T, N, C', H, W] with T the engine's
    ring slots (`bind_ring` some kind first); it may start on any byte — as the world planes: from
    now on every submission is followed on the same stream by one launch that rewrites
    `observe_world_planes(classes, ...)` of every world into it, or into the ring slot the
    submission wrote.  The engine keeps the class table alive.  None clears the registration; the
    engine's launches are then what they were.  Returns `out`."""
    t = self._torch
    if out is None:
      ego_planes_request(self._L, self._h, MP_EGOPLANES_WORLD_REGISTER)
      self._world_planes = None
      return None
    mask = view_layer_mask(layers, int(self.info.num_layers))
    cls, C = self._world_plane_classes(classes, num_classes)
    shape = self.world_planes_shape(C, facing)
    ring = isinstance(out, t.Tensor) and out.dim() == len(shape) + 1
    if (not isinstance(out, t.Tensor) or out.dtype != t.uint8 or tuple(out.shape[-len(shape):]) != shape or
        out.dim() not in (len(shape), len(shape) + 1) or not (out[0] if ring else out).is_contiguous() or
        out.device != self.device):
      raise ValueError(f"bind_world_planes: out must be a uint8 tensor of shape {shape} or "
                       f"[T, {', '.join(map(str, shape))}] with contiguous slots on {self.device}")
    ego_planes_request(self._L, self._h, MP_EGOPLANES_WORLD_REGISTER, layer_mask=mask, classes=cls.data_ptr(),
                       classes_len=int(cls.numel()), num_classes=C, facing=int(bool(facing)),
                       **self._view_ring(out, ring, int(np.prod(shape))))
    self._world_planes = (out, cls)
    return out

  @property
  def has_zapper(self) -> bool:
    """Whether the level carries a Zapper: without one there is no AVATAR_IDS_IN_RANGE_TO_ZAP."""
    if getattr(self, "_has_zapper", None) is None:
      self._has_zapper = has_zapper(self.pack_bytes)
    return self._has_zapper

  @property
  def avatar_ids_shape(self) -> Tuple[int, int, int]:
    """(N, P, P): the shape of AVATAR_IDS_IN_VIEW and of AVATAR_IDS_IN_RANGE_TO_ZAP (int32)."""
    return (self.N, self.P, self.P)

  def observe_avatar_ids(self, bank=None, rows=None, players=None, view: bool = True, zap: bool = True, out=None,
                         fingerprint: Optional[int] = None):
    """(AVATAR_IDS_IN_VIEW, AVATAR_IDS_IN_RANGE_TO_ZAP) — whom each player sees, and whom a zap it
    fired now could reach — of rows of `bank` (a contiguous uint8 device tensor [M, S]), or of the
    engine's worlds as they are now (`bank` None; `rows` are then world indices), written from the
    records by ONE launch.  int32 device tensors [R, P, P], row p the 0/1 vector of viewer p over
    the player slots; with `players` (R ints) [R, P], the vector of player players[i] of row
    rows[i].  `view`, `zap`: which of the two to work out; the other's place holds None.  `out`: a
    pair of tensors (or None) to write.  IN_VIEW: both alive and q's cell under p's window (1 at q
    == p).  IN_RANGE: the reference's rays on the avatars' own layer — blockers of other layers and
    the cooldown play no part; a level without a Zapper raises ValueError.  A dead player's row is
    0.  Nothing of the engine's is written.  A row or player index out of range leaves its element
    as it was; the next synchronising call raises ValueError.  Enqueued on the current stream."""
    if not view and not zap:
      raise ValueError("observe_avatar_ids: neither view nor zap is asked for")
    count, r, p, src = self._view_source("observe_avatar_ids", "draw", bank, rows, players, fingerprint)
    shape = (count, self.P, self.P) if p is None else (count, self.P)
    given = (None, None) if out is None else tuple(out)
    if len(given) != 2:
      raise ValueError("observe_avatar_ids: out is a pair (in_view, in_range); None where one is not asked for")
    t = self._torch
    out_v = self._out("observe_avatar_ids", given[0], shape, t.int32) if view else None
    out_z = self._out("observe_avatar_ids", given[1], shape, t.int32) if zap else None
    self.use_current_stream()
    avatar_ids_request(self._L, self._h, MP_AVATARIDS_DRAW,
                       dst=None if out_v is None else out_v.data_ptr(),
                       dst_bytes=0 if out_v is None else out_v.numel() * 4,
                       dst_zap=None if out_z is None else out_z.data_ptr(),
                       dst_zap_bytes=0 if out_z is None else out_z.numel() * 4, **src)
    self._avatar_ids_args = (bank, r, p, out_v, out_z)   # (kept until the next call: the launch may not have run yet)
    return out_v, out_z

  def bind_avatar_ids(self, view=None, zap=None):
    """Registers `view` (AVATAR_IDS_IN_VIEW) and `zap` (AVATAR_IDS_IN_RANGE_TO_ZAP) — contiguous
    int32 device tensors [N, P, P], or [T, N, P, P] with T the engine's ring slots (`bind_ring`
    some kind first); either may be None — : from now on every submission (reset, step, step_many
    in every form, a load) is followed on the same stream by ONE launch that rewrites
    `observe_avatar_ids()` of every world into them, or into the ring slot the submission wrote.
    Both None clears the registration; the engine's launches are then what they were.  Returns
    (view, zap)."""
    t = self._torch
    if view is None and zap is None:
      avatar_ids_request(self._L, self._h, MP_AVATARIDS_REGISTER)
      self._avatar_ids = None
      return None, None
    shape = self.avatar_ids_shape
    first = view if view is not None else zap
    ring = isinstance(first, t.Tensor) and first.dim() == 4
    for o in (view, zap):
      if o is None:
        continue
      if (not isinstance(o, t.Tensor) or o.dtype != t.int32 or tuple(o.shape[-3:]) != shape or
          o.dim() != (4 if ring else 3) or not (o[0] if ring else o).is_contiguous() or o.device != self.device or
          (ring and (o.shape[0] != first.shape[0] or (o.shape[0] > 1 and o.stride(0) != first.stride(0))))):
        raise ValueError(f"bind_avatar_ids: view and zap must be int32 tensors of shape {shape} or "
                         f"[T, {', '.join(map(str, shape))}] with contiguous slots (of one stride) on {self.device}")
    block = int(np.prod(shape)) * 4
    f = self._view_ring(first, ring, block)
    avatar_ids_request(self._L, self._h, MP_AVATARIDS_REGISTER,
                       dst=None if view is None else view.data_ptr(), dst_bytes=0 if view is None else f["dst_bytes"],
                       dst_zap=None if zap is None else zap.data_ptr(),
                       dst_zap_bytes=0 if zap is None else f["dst_bytes"], slot_stride=f["slot_stride"],
                       slots=f["slots"])
    self._avatar_ids = (view, zap)
    return view, zap

  def counters(self) -> Dict[str, int]:
    out = np.zeros(len(COUNTER_NAMES), np.uint64)
    _check(self._L, self._L.mp_counters(self._h, out.ctypes.data),
           "mp_counters")
    # (reward_sum_x1024 is a signed sum: coins pays negative rewards)
    return {k: int(v.astype(np.int64)) if k == "reward_sum_x1024" else int(v)
            for k, v in zip(COUNTER_NAMES, out)}

  def sync(self):
    _check(self._L, self._L.mp_sync(self._h), "mp_sync")

  def box_fill(self, kind: int, reps: int = 20):
    """mp_box_fill: what the box's memory system gives the buffer bound for pixel view
    `kind` — µs per launch of the runtime's memset, of a bare store loop in the frame
    launch's write order and of the same bytes as one chip-wide 4 KiB front.  OVERWRITES
    the view with junk (the next step redraws it)."""
    rep = MpBoxFill()
    _check(self._L, self._L.mp_box_fill(self._h, int(kind), int(reps), ctypes.byref(rep)), "mp_box_fill")
    return {"bytes": int(rep.bytes), "memset_us": round(rep.memset_us, 2),
            "product_order_us": round(rep.product_order_us, 2),
            "front_4k_us": round(rep.front_4k_us, 2), "workgroups": rep.groups,
            "storing_waves": rep.waves, "span_bytes": int(rep.span_bytes)}

  def fault_words(self) -> np.ndarray:
    """Diagnostics of the frame kernel's pipeline (include/mp_engine.h); host
    memory, never blocks."""
    out = np.zeros(64, np.uint32)
    _check(self._L, self._L.mp_fault_words(self._h, out.ctypes.data), "mp_fault_words")
    return out


def pack_agent_roles(pack_bytes: bytes):
  """The avatars' `agentRole` strings (gift_refinements: what the `gift` event reports as
  gifter_role / receipient_role, components.lua:174-181), () for a pack without them."""
  from meltingpot_amd import pack as pack_lib
  t = pack_lib.loads(pack_bytes)
  if "agent_roles" not in t:
    return ()
  return tuple(n.decode() for n in bytes(t["agent_roles"]).split(b"\0")[:-1])


def pack_role_names(pack_bytes: bytes):
  """Names of the roles a pack carries per-player constants for (sorted; the
  index is what MpConfig.roles takes), or None for a single-role substrate."""
  from meltingpot_amd import pack as pack_lib
  t = pack_lib.loads(pack_bytes)
  if "role_names" not in t:
    return None
  return tuple(n.decode() for n in bytes(t["role_names"]).split(b"\0")[:-1])


def load_pack(name: str) -> bytes:
  """Committed lowered-substrate pack (generated by tools/make_packs.py)."""
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets",
                      f"{name}.mpk")
  with open(path, "rb") as f:
    return f.read()
