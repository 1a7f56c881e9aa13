"""The C ABI of the requests, checked once over everything, without a GPU: every ctypes mirror of
meltingpot_amd/engine.py against include/mp_engine.h as a C99 and as a C++17 compiler lay it out;
the sizes and offsets the headers document, as literals; the prefix relations between the step
requests and between the view requests; engine.REQUESTS against the recorded answers of the two
carriers (tests/golden/request_dispatch.json); every `static inline` wrapper under include/ that
takes an engine, called from one program in both languages; the header's constants; and the kernels
in the code object.  (That the library exports exactly the declared symbols: tests/test_cabi_cpu.py.)"""
import ctypes
import json
import os
import re
import subprocess

import pytest

from meltingpot_amd import _build
from meltingpot_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
LANGUAGES = {"c99": ("gcc", "-std=c99", "c"), "c++17": ("g++", "-std=c++17", "cc")}
MIRRORS = {n: c for n, c in vars(E).items()
           if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}
CARRIERS = ("mp_snapshot", "mp_restore")
LEVELS = ("clean_up", "commons", "coins", "territory", "matrix", "coop", "gift", "cook", "mushroom")
INVALID = E.MP_ERR_INVALID

# The sizes csrc/engine_requests.hip asserts and include/mp_engine.h documents, and the four oldest
# requests' and MpStepRow's, by hand: a wrong edit of header and mirror together still fails here.
SIZES = {"MpAvatarIds": 144, "MpEgoPlanes": 160, "MpViewHash": 152, "MpEgoLayer": 128, "MpEpisodeStats": 224,
         "MpStatesObserve": 64, "MpStateLayout": 120, "MpStatesCheck": 88, "MpStatesHash": 104, "MpEpisodeStarts": 72,
         "MpStatesView": 80, "MpStepActive": 96, "MpStepUntil": 136, "MpStepListed": 176,
         "MpEventColumn": 32, "MpStatsBank": 32, "MpStateField": 32,
         "MpStepTrajectory": 40, "MpKernelVariant": 48, "MpWorldStates": 56, "MpStepMany": 112, "MpStepRow": 24}
OFFSETS = {
    "MpStepActive": {"struct_size": 0, "steps": 4, "fields": 8, "num_rows": 12, "actions": 16,
                     "actions_step_bytes": 24, "rows": 32, "active": 40, "active_step_bytes": 48, "reserved": 56},
    "MpStepUntil": {"struct_size": 0, "steps": 4, "fields": 8, "num_rows": 12, "actions": 16,
                    "actions_step_bytes": 24, "rows": 32, "active": 40, "active_step_bytes": 48, "stop": 56,
                    "pad": 60, "stopped": 64, "ran": 72, "returns": 80, "gamma": 88, "reserved": 96},
}

# Every call of a wrapper: (wrapper, C expression, the answer).  What earlier tests called keeps
# their arguments; the rest get NULLs and zeros.  No call has an engine, so none touches a device.
CALLS = [
    ("mp_step_many", "mp_step_many(NULL, NULL, 4, 0, 0, five_rows, five_bytes)", INVALID),
    ("mp_step_many", "mp_step_many(NULL, NULL, 0, 0, 0, NULL, NULL)", INVALID),
    ("mp_step_trajectory", "mp_step_trajectory(NULL, NULL, 4, 0, 0, two_rows, 2)", INVALID),
    ("mp_step_many_active", "mp_step_many_active(NULL, NULL, 4, 0, 0, NULL, 0, NULL, 0)", INVALID),
    ("mp_step_active", "mp_step_active(NULL, NULL, 0, NULL)", INVALID),
    ("mp_step_many_until", "mp_step_many_until(NULL, NULL, 4, 0, 0, NULL, 0, NULL, 0, MP_STOP_LAST | MP_STOP_REWARD, "
     "NULL, NULL, NULL, 0.97)", INVALID),
    ("mp_step_until", "mp_step_until(NULL, NULL, 0, MP_STOP_LAST, NULL)", INVALID),
    ("mp_step_many_listed", "mp_step_many_listed(NULL, NULL, 3, NULL, 4, 0, 0, NULL, 0, NULL, 0, MP_STOP_LAST, NULL, "
     "NULL, NULL, 0.97)", INVALID),
    ("mp_step_listed", "mp_step_listed(NULL, NULL, 3, NULL, 0)", INVALID),
    ("mp_set_episode_starts", "mp_set_episode_starts(NULL, NULL, 1, NULL, NULL, 0, 0)", INVALID),
    ("mp_clear_episode_starts", "mp_clear_episode_starts(NULL)", INVALID),
    ("mp_set_episode_stats", "mp_set_episode_stats(NULL, &stats)", INVALID),
    ("mp_clear_episode_stats", "mp_clear_episode_stats(NULL)", INVALID),
    ("mp_tally_events", "mp_tally_events(NULL, &column, 1, NULL, 0, NULL, 1, 1, NULL, NULL, NULL, NULL)", INVALID),
    ("mp_episode_stats_host", "mp_episode_stats_host(&stats)", INVALID),   # (steps 0: refused)
    ("mp_state_fingerprint", "(int)mp_state_fingerprint(NULL)", 0),
    ("mp_save_worlds", "mp_save_worlds(NULL, NULL, 4, NULL, 0)", INVALID),
    ("mp_load_worlds", "mp_load_worlds(NULL, NULL, 1, NULL, 0)", INVALID),
    ("mp_observe_states", "mp_observe_states(NULL, MP_OBS_LAYER, NULL, 1, NULL, 1, NULL, 0, 0)", INVALID),
    ("mp_observe_views", "mp_observe_views(NULL, MP_OBS_RGB, NULL, 0, NULL, NULL, 0, NULL, 0, 0)", INVALID),
    ("mp_ego_layer_draw", "mp_ego_layer_draw(NULL, NULL, 0, NULL, NULL, 0, NULL, 0, 0)", INVALID),
    ("mp_ego_layer_register", "mp_ego_layer_register(NULL, NULL, 0, 0, 0)", INVALID),
    ("mp_ego_layer_host", "mp_ego_layer_host(NULL, 0, NULL, NULL, 0, NULL, NULL, 0, NULL, 0, 0)", INVALID),
    ("mp_view_hash_draw", "mp_view_hash_draw(NULL, NULL, 0, NULL, NULL, 0, 0, NULL, 0, NULL, 0, 0)", INVALID),
    ("mp_view_hash_register", "mp_view_hash_register(NULL, NULL, 0, 0, 0, 0, NULL, 0)", INVALID),
    ("mp_view_hash_host", "mp_view_hash_host(NULL, 0, NULL, NULL, 0, NULL, NULL, 0, 0, NULL, 0, NULL, 0, 0)", INVALID),
    ("mp_view_hash_num_ids", "mp_view_hash_num_ids(NULL, NULL, 0, NULL, NULL)", INVALID),
    ("mp_ego_planes_draw", "mp_ego_planes_draw(NULL, NULL, 0, NULL, NULL, 0, 0, NULL, 0, 1, 0, NULL, 0, 0)", INVALID),
    ("mp_ego_planes_register", "mp_ego_planes_register(NULL, NULL, 0, 0, 0, 0, NULL, 0, 1, 0)", INVALID),
    ("mp_ego_planes_host", "mp_ego_planes_host(NULL, 0, NULL, NULL, 0, NULL, NULL, 0, 0, NULL, 0, 1, 0, NULL, 0, 0)",
     INVALID),
    ("mp_ego_planes_num_ids", "mp_ego_planes_num_ids(NULL, NULL, 0, NULL, NULL)", INVALID),
    ("mp_avatar_ids_draw", "mp_avatar_ids_draw(NULL, NULL, 0, NULL, NULL, 0, NULL, 0, NULL, 0, 0)", INVALID),
    ("mp_avatar_ids_register", "mp_avatar_ids_register(NULL, NULL, 0, NULL, 0, 0, 0)", INVALID),
    ("mp_avatar_ids_host", "mp_avatar_ids_host(NULL, 0, NULL, NULL, 0, NULL, NULL, 0, NULL, 0, NULL, 0, 0)", INVALID),
    # the wrappers no test called before: NULLs and zeros
    ("mp_kernel_variant", "mp_kernel_variant(NULL, NULL, 0, NULL, NULL, 0)", INVALID),
    ("mp_state_layout", "mp_state_layout(NULL, NULL, 0, NULL, NULL, 0, &layout)", INVALID),
    ("mp_check_states", "mp_check_states(NULL, NULL, 0, NULL, 0, NULL, 0)", INVALID),
    ("mp_check_states_host", "mp_check_states_host(NULL, 0, NULL, NULL, 0, NULL, 0, NULL, 0)", INVALID),
    ("mp_filter_states", "mp_filter_states(NULL, NULL, 0, NULL, 0, NULL, 0)", INVALID),
    ("mp_hash_states", "mp_hash_states(NULL, NULL, 0, NULL, 0, NULL, 0, NULL)", INVALID),
    ("mp_hash_worlds", "mp_hash_worlds(NULL, NULL, 0, NULL, NULL)", INVALID),
    ("mp_hash_states_host", "mp_hash_states_host(NULL, 0, NULL, NULL, 0, NULL, 0, NULL, 0, NULL)", INVALID),
    ("mp_state_hash_mask", "mp_state_hash_mask(NULL, NULL, 0, NULL, NULL, 0, NULL)", INVALID),
]
CONSTANTS = {"MP_ABI_VERSION": E.MP_ABI_VERSION, "MP_OBS_KINDS": 24, "MP_STEP_MANY_MAX": E.STEP_MANY_MAX,
             "MP_STEP_ROW_STATE": E.STEP_ROW_STATE, "MP_STEP_ROW_HASH": E.STEP_ROW_HASH,
             "MP_STOP_LAST": E.MP_STOP_LAST, "MP_STOP_REWARD": E.MP_STOP_REWARD, "MP_OBS_LAYER": E.OBS_LAYER}


def header_text(name="mp_engine.h"):
  return open(os.path.join(INCLUDE, name)).read()


def struct_typedefs():
  """{name: [field names]} of every `typedef struct { ... } MpX;` of mp_engine.h."""
  text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
  def names(body):   # (`int32_t a, b[3];` declares a and b)
    return [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", part).group(1)
            for decl in body.split(";") if decl.strip() for part in decl.split(",")]
  return {m.group(2): names(m.group(1)) for m in re.finditer(r"typedef struct\s*\{([^{}]*)\}\s*(Mp\w+);", text)}


def wrappers():
  """The names of the `static inline` functions under include/ that take an MpEngine*."""
  found = set()
  for name in HEADERS:
    for m in re.finditer(r"static inline\s+\w+\s+(mp_\w+)\(([^)]*)\)\s*\{", header_text(name)):
      if "MpEngine*" in m.group(2):
        found.add(m.group(1))
  return found


def program():
  """One program over every header: `Struct field offset` and `Struct sizeof size` for every mirror,
  `call index answer` for every entry of CALLS (index: its place there, then the message's first
  word), `constant name value` for CONSTANTS."""
  lines = ["#include <stddef.h>", "#include <stdio.h>"] + [f'#include "{h}"' for h in HEADERS]
  lines += ["int main(void) {",
            "  void* five_rows[5] = {0, 0, 0, 0, 0};",
            "  uint64_t five_bytes[5] = {0, 0, 0, 0, 0};",
            "  MpStepRow two_rows[2] = {{MP_OBS_LAYER, 0, NULL, 0}, {MP_OBS_POSITION, 0, NULL, 0}};",
            "  MpStepRow state_row = {MP_STEP_ROW_STATE, 0, NULL, 0};",
            "  MpEpisodeStats stats;",
            "  MpStateLayout layout;",
            "  MpEventColumn column = mp_event_column(MP_EVENT_ZAP, 1, 0, 0xffffffffu);",
            "  int rc;",
            "  memset(&stats, 0, sizeof stats);"]
  for name, mirror in MIRRORS.items():
    lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
    lines += [f'  printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in mirror._fields_]
  for i, (_, call, _) in enumerate(CALLS):
    lines += [f"  rc = {call};", f'  printf("call {i} %d %s\\n", rc, rc ? mp_last_error() : "");']
  lines += [f'  printf("constant {c} %d\\n", (int){c});' for c in CONSTANTS]
  lines += ['  printf("constant state_row.kind %d\\n", state_row.kind);', "  return 0;", "}"]
  return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=list(LANGUAGES))
def answers(request, tmp_path_factory):
  """What the program prints, compiled in one language with -Wall -Werror against the library:
  {"layout": {(struct, field): value}, "calls": [(code, message)], "constants": {name: value}}."""
  compiler, std, suffix = LANGUAGES[request.param]
  tmp = tmp_path_factory.mktemp("abi")
  src, exe = tmp / f"abi.{suffix}", tmp / "abi"
  src.write_text(program())
  lib = _build.build_engine()
  subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe), lib,
                  f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
  out = {"layout": {}, "calls": [], "constants": {}}
  for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
    a, b, c = line.split(None, 2)
    if a == "call":
      code, _, message = c.partition(" ")
      out["calls"].append((int(code), message))
    elif a == "constant":
      out["constants"][b] = int(c)
    else:
      out["layout"][a, b] = int(c)
  return out


@pytest.fixture(scope="module")
def dispatch():
  with open(os.path.join(ROOT, "tests", "golden", "request_dispatch.json")) as f:
    return json.load(f)


# ---- layout ------------------------------------------------------------------------------------
def test_the_mirrors_are_the_header_s_structs():
  """(MpObsKind and MpEventType are enums: no `typedef struct`.)"""
  structs = struct_typedefs()
  assert set(structs) == set(MIRRORS) and len(MIRRORS) == 27
  for name, mirror in MIRRORS.items():
    assert structs[name] == [f for f, _ in mirror._fields_], name


@pytest.mark.parametrize("name", list(MIRRORS))
def test_a_compiler_lays_the_struct_out_as_the_mirror(answers, name):
  mirror = MIRRORS[name]
  want = {(name, "sizeof"): ctypes.sizeof(mirror)}
  want.update({(name, f): getattr(mirror, f).offset for f, _ in mirror._fields_})
  got = {k: v for k, v in answers["layout"].items() if k[0] == name}
  assert got == want


def test_every_mirror_was_laid_out(answers):
  assert {n for n, _ in answers["layout"]} == set(MIRRORS)
  assert len(answers["layout"]) == sum(1 + len(m._fields_) for m in MIRRORS.values())


# ---- documented numbers ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SIZES))
def test_the_documented_size(name):
  assert ctypes.sizeof(MIRRORS[name]) == SIZES[name]


@pytest.mark.parametrize("name", list(OFFSETS))
def test_the_documented_offsets(name):
  M = MIRRORS[name]
  assert {f: getattr(M, f).offset for f, _ in M._fields_} == OFFSETS[name]


def test_the_documented_offsets_of_the_world_list():
  M, U = E.MpStepListed, E.MpStepUntil
  assert M.worlds.offset == ctypes.sizeof(U) == 136
  assert (M.count.offset, M.reserved2.offset, M.reserved3.offset) == (144, 148, 152)
  assert E.MpStepMany.per_step.size == 40 and E.MpStepMany.per_step_bytes.size == 40


# ---- prefix relations --------------------------------------------------------------------------
def test_the_step_requests_are_prefixes_of_each_other():
  T, A, U, M = E.MpStepTrajectory, E.MpStepActive, E.MpStepUntil, E.MpStepListed
  # the seven fields in front of MpStepActive are MpStepTrajectory's
  for name, _ in T._fields_:
    assert getattr(T, name).offset == getattr(A, name).offset and getattr(T, name).size == getattr(A, name).size, name
  # the fields in front of MpStepUntil are MpStepActive's, at its offsets; the new ones begin where its
  # reserved words do
  for name, _ in A._fields_:
    if name != "reserved":
      assert getattr(A, name).offset == getattr(U, name).offset and getattr(A, name).size == getattr(U, name).size, name
  assert A.reserved.offset == U.stop.offset
  # MpStepUntil's fields in front of MpStepListed, at its offsets; the list begins where that struct ends
  for name, _ in U._fields_:
    assert getattr(U, name).offset == getattr(M, name).offset and getattr(U, name).size == getattr(M, name).size, name
  assert M.worlds.offset == ctypes.sizeof(U)


def test_the_view_requests_share_their_head():
  """csrc/engine_views.hip's ViewRequest reads these fields of all four through one layout."""
  head = [f for f, _ in E.MpEgoLayer._fields_[:12]] + ["pack", "pack_len", "cfg"]
  assert head[:3] == ["struct_size", "op", "fingerprint"] and head[11] == "slots"
  for M in (E.MpViewHash, E.MpEgoPlanes, E.MpAvatarIds):
    for name in head:
      assert getattr(M, name).offset == getattr(E.MpEgoLayer, name).offset, (M.__name__, name)
      assert getattr(M, name).size == getattr(E.MpEgoLayer, name).size, (M.__name__, name)
    assert M.reserved2.size == 24 and M.reserved2.offset == ctypes.sizeof(M) - 24


# ---- the table ---------------------------------------------------------------------------------
def test_the_requests_sizes_tell_them_apart():
  sizes = [ctypes.sizeof(q.struct) for q in E.REQUESTS]
  assert len(set(sizes)) == len(sizes) == 18
  assert max(sizes) < 448   # (no engine's snapshot is that small)


def test_the_table_names_the_recorded_requests(dispatch):
  names = {n.split("/")[0] for n in dispatch} - {"odd_size", "null_buffer"}
  assert names == {q.struct.__name__ for q in E.REQUESTS}
  assert all(q.snapshot or q.restore for q in E.REQUESTS)
  assert [q.struct for q in E.REQUESTS if q.snapshot and q.restore] == [E.MpWorldStates]


@pytest.mark.parametrize("carrier", CARRIERS)
@pytest.mark.parametrize("q", E.REQUESTS, ids=lambda q: q.struct.__name__)
def test_the_table_s_flags_are_the_recorded_dispatch(dispatch, q, carrier):
  """Without an engine: through a carrier the request does not have, the carrier's "bad buffer";
  through one it has, the handler's own words where `null_engine` says it is reached."""
  code, text = dispatch[f"{q.struct.__name__}/{carrier}"]
  reached = (q.snapshot if carrier == "mp_snapshot" else q.restore) and q.null_engine
  assert code == INVALID
  assert (text != f"{carrier}: bad buffer") == reached, text


def test_send_takes_the_carrier_from_the_table():
  for q in E.REQUESTS:
    if q.snapshot != q.restore:
      assert E._CARRIER[q.struct] == ("mp_snapshot" if q.snapshot else "mp_restore")
  assert E.MpWorldStates not in E._CARRIER   # (world_states_request: by op)


# ---- wrappers ----------------------------------------------------------------------------------
def test_the_program_calls_every_wrapper():
  called = {name for name, _, _ in CALLS}
  assert wrappers() <= called, sorted(wrappers() - called)
  for name, call, _ in CALLS:
    assert name + "(" in call


def test_the_wrappers_answer(answers):
  assert len(answers["calls"]) == len(CALLS)
  for (name, call, want), (code, message) in zip(CALLS, answers["calls"]):
    assert code == want, (call, code, message)
  by_name = {name: message for (name, _, _), (_, message) in zip(CALLS, answers["calls"])}
  assert by_name["mp_step_trajectory"].startswith("MpStepTrajectory")


# ---- constants ---------------------------------------------------------------------------------
def test_the_constants_a_compiler_sees(answers):
  want = dict(CONSTANTS)
  want["state_row.kind"] = E.STEP_ROW_STATE
  assert answers["constants"] == want
  assert E.MP_ABI_VERSION == 8 and E.OBS_LAYER == 16 and E.OBS_RGB_POOL8 + 1 == 24
  assert (E.MP_STOP_LAST, E.MP_STOP_REWARD) == (1, 2)
  assert E.STEP_ROW_STATE >= 24 and E.STEP_ROW_STATE not in E.STEP_ROW_KINDS


def test_the_header_s_text():
  text = header_text()
  assert re.search(r"#define MP_ABI_VERSION 8\b", text) and re.search(r"MP_OBS_KINDS\s*=\s*24", text)
  assert re.search(r"MP_OBS_LAYER\s*=\s*16", text)
  assert re.search(rf"#define MP_STEP_MANY_MAX {E.STEP_MANY_MAX}\b", text)
  state = int(re.search(r"#define MP_STEP_ROW_STATE (0x[0-9a-fA-F]+|\d+)\b", text).group(1), 0)
  assert state == E.STEP_ROW_STATE
  assert re.search(r"enum\s*\{\s*MP_STATES_FINGERPRINT = 1, MP_STATES_SAVE = 2, MP_STATES_LOAD = 3\s*\}", text)
  for ops in ("MP_EGO_DRAW = 1, MP_EGO_REGISTER = 2, MP_EGO_HOST = 3",
              "MP_VIEWHASH_DRAW = 1, MP_VIEWHASH_REGISTER = 2, MP_VIEWHASH_HOST = 3",
              "MP_EGOPLANES_DRAW = 1, MP_EGOPLANES_REGISTER = 2, MP_EGOPLANES_HOST = 3",
              "MP_AVATARIDS_DRAW = 1, MP_AVATARIDS_REGISTER = 2, MP_AVATARIDS_HOST = 3"):
    assert ops in text, ops


def test_the_abi_version_and_the_symbol_count():
  assert E.load_library().mp_abi_version() == 8 == E.MP_ABI_VERSION
  assert len(E.ABI_SYMBOLS) == 30


# ---- kernels -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob():
  with open(_build.build_engine(), "rb") as f:
    return f.read()


@pytest.mark.parametrize("family", ["k_step_many", "k_step_rows", "k_step_states", "k_step_starts", "k_many_starts",
                                    "k_many_active", "k_many_until", "k_many_listed"])
def test_a_kernel_family_has_every_level(blob, family):
  for level in LEVELS:
    assert f"{family}_{level}".encode() in blob, level


@pytest.mark.parametrize("kernel", [
    "k_step_clean_up", "k_step_commons", "k_step_territory", "k_frame", "k_state_obs", "k_gather_rows",
    "k_state_view", "k_view_scalar", "k_episode_stats", "k_claim_listed", "k_ego_layer_rows", "k_ego_layer_views",
    "k_view_hash_rows", "k_view_hash_views", "k_ego_planes_rows", "k_ego_planes_views", "k_avatar_ids_rows",
    "k_avatar_ids_views"])
def test_a_kernel_is_in_the_code_object(blob, kernel):
  assert kernel.encode() in blob
