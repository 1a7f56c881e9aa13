// engine_views.hip — the requests about every viewer's window: MpEgoLayer, MpViewHash, MpEgoPlanes
// and MpAvatarIds (include/mp_engine.h), one front and four tails, and the world ops of the first
// and the third (WORLD.LAYER, the world planes: the whole map in place of the windows), two more
// tails on the same front.  engine_requests.hip's table carries them.
#include <string.h>

#include <vector>

#include "engine_state.h"
#include "ego_layer.h"
#include "view_hash.h"
#include "ego_planes.h"
#include "avatar_ids.h"
#include "world_view.h"

// The requests about every viewer's window — MpEgoLayer, MpViewHash, MpEgoPlanes, MpAvatarIds
// (include/mp_engine.h; carried by mp_snapshot; `e` is NULL for the host form) — are one front and four tails.  Each
// draws from bank rows or from the engine's worlds (one launch), registers or clears the tensor
// behind every submission (no launch), or applies its function to host rows; everything is
// checked first.  Their structs begin alike, and the front reads them through that beginning:
struct ViewRequest {
  uint32_t struct_size;
  int32_t op;              // 1: draw, 2: register, 3: host (MP_EGO_*, MP_VIEWHASH_*, MP_EGOPLANES_*)
  uint64_t fingerprint;
  const void* bank;
  const int32_t* rows;
  const int32_t* players;
  void* dst;
  uint64_t dst_bytes;
  int32_t bank_rows, count;
  uint64_t slot_stride;
  int32_t slots;
  int32_t word76;          // MpEgoLayer: reserved; the other two: classes_len
  const void* pack;
  uint64_t pack_len;
  const MpConfig* cfg;
};
enum { VIEW_DRAW = 1, VIEW_REGISTER = 2, VIEW_HOST = 3 };
#define MP_VIEW_FIELD(T, f) (offsetof(T, f) == offsetof(ViewRequest, f))
#define MP_VIEW_PREFIX(T)                                                                                      \
  (MP_VIEW_FIELD(T, op) && MP_VIEW_FIELD(T, fingerprint) && MP_VIEW_FIELD(T, bank) && MP_VIEW_FIELD(T, rows) && \
   MP_VIEW_FIELD(T, players) && MP_VIEW_FIELD(T, dst) && MP_VIEW_FIELD(T, dst_bytes) &&                        \
   MP_VIEW_FIELD(T, bank_rows) && MP_VIEW_FIELD(T, count) && MP_VIEW_FIELD(T, slot_stride) &&                  \
   MP_VIEW_FIELD(T, slots) && MP_VIEW_FIELD(T, pack) && MP_VIEW_FIELD(T, pack_len) && MP_VIEW_FIELD(T, cfg) && \
   sizeof(T) >= sizeof(ViewRequest))
static_assert(MP_VIEW_PREFIX(MpEgoLayer) && MP_VIEW_PREFIX(MpViewHash) && MP_VIEW_PREFIX(MpEgoPlanes) &&
                  MP_VIEW_PREFIX(MpAvatarIds),
              "MpEgoLayer, MpViewHash, MpEgoPlanes and MpAvatarIds share their leading fields");
static_assert(MP_AVATARIDS_DRAW == VIEW_DRAW && MP_AVATARIDS_REGISTER == VIEW_REGISTER && MP_AVATARIDS_HOST == VIEW_HOST,
              "and MpAvatarIds the numbers of their ops");
static_assert(MP_EGO_DRAW == VIEW_DRAW && MP_VIEWHASH_DRAW == VIEW_DRAW && MP_EGOPLANES_DRAW == VIEW_DRAW &&
                  MP_EGO_REGISTER == VIEW_REGISTER && MP_VIEWHASH_REGISTER == VIEW_REGISTER &&
                  MP_EGOPLANES_REGISTER == VIEW_REGISTER && MP_EGO_HOST == VIEW_HOST &&
                  MP_VIEWHASH_HOST == VIEW_HOST && MP_EGOPLANES_HOST == VIEW_HOST,
              "and the numbers of their ops");
static_assert(MP_EGO_WORLD_DRAW == VIEW_DRAW + 3 && MP_EGO_WORLD_REGISTER == VIEW_REGISTER + 3 &&
                  MP_EGO_WORLD_HOST == VIEW_HOST + 3 && MP_EGOPLANES_WORLD_DRAW == VIEW_DRAW + 3 &&
                  MP_EGOPLANES_WORLD_REGISTER == VIEW_REGISTER + 3 && MP_EGOPLANES_WORLD_HOST == VIEW_HOST + 3,
              "the world ops of MpEgoLayer and MpEgoPlanes are their ops + 3");
#undef MP_VIEW_PREFIX
#undef MP_VIEW_FIELD
static ViewRequest view_of(const void* request) {
  ViewRequest q;
  memcpy(&q, request, sizeof q);
  return q;
}

// The words that differ in the three requests' messages.
struct ViewWords {
  const char* who;       // "MpEgoLayer"
  const char* host_op;   // "MP_EGO_HOST"
  const char* thing;     // a registration: "the leaf" of N worlds
  const char* need;      // "needs" so many bytes
  const char* drawn;     // rows are "drawn"
  const char* draw;      // there is no state to "draw"
};

// The tables a request works with: the engine's, or the pack's by the host stage.
struct ViewTables {
  HostStage h;
  std::vector<int32_t> host_lut;   // (host form) the viewers' value tables
  const DevTables* t = nullptr;
  uint64_t fingerprint = 0;
  int32_t num_ids = 0;             // the length of a class table
};

// struct_size, op, engine, reserved words, pack: what is checked before the request is looked at.
static int view_prologue(const MpEngine* e, const ViewRequest& q, const ViewWords& w, size_t size, bool reserved_zero) {
  if (q.struct_size != size)
    return fail(MP_ERR_INVALID, "%s: struct_size %u, expected %zu", w.who, q.struct_size, size);
  if (q.op != VIEW_DRAW && q.op != VIEW_REGISTER && q.op != VIEW_HOST)
    return fail(MP_ERR_INVALID, "%s: unknown op %d", w.who, q.op);
  if (q.op == VIEW_HOST ? e != nullptr : e == nullptr) {
    if (e) return fail(MP_ERR_INVALID, "%s: %s takes no engine", w.who, w.host_op);
    return fail(MP_ERR_INVALID, "%s: NULL engine", w.who);
  }
  if (!reserved_zero) return fail(MP_ERR_INVALID, "%s: the reserved words must be 0", w.who);
  if (q.op == VIEW_HOST && (!q.pack || !q.cfg))
    return fail(MP_ERR_INVALID, "%s: %s needs the pack and its config (NULL pack or cfg)", w.who, w.host_op);
  return MP_OK;
}

// (`viewers` false: the world ops, which read none of the viewers' value tables)
static int view_tables(const MpEngine* e, const ViewRequest& q, ViewTables* v, bool viewers = true) {
  if (e) {
    v->t = &e->t;
    v->fingerprint = e->fingerprint;
    v->num_ids = e->num_layer_ids;
    return MP_OK;
  }
  if (int rc = host_stage(q.pack, q.pack_len, q.cfg, &v->h)) return rc;
  v->t = &v->h.d.t;
  v->fingerprint = state_fingerprint(v->h.pack, v->h.d.t);
  if (!viewers) return MP_OK;
  v->host_lut = layer_lut_rows(v->h.pack.data(), v->h.d.t);
  v->num_ids = view_hash::num_ids(v->host_lut.data(), v->t->P);
  return MP_OK;
}

// layer_mask as the kernels take it: 0 names every layer of the view.
static int view_layer_mask(const ViewWords& w, const ego_layer::Window& g, uint64_t asked, uint64_t* layer_mask) {
  if (g.L > 64) return fail(MP_ERR_UNSUPPORTED, "%s: %d layers; layer_mask names 64", w.who, g.L);
  const uint64_t every = g.L == 64 ? ~0ull : (1ull << g.L) - 1ull;
  if (asked & ~every)
    return fail(MP_ERR_INVALID, "%s: layer_mask %016llx has a bit that names no layer (the view has %d)", w.who,
                (unsigned long long)asked, g.L);
  *layer_mask = asked ? asked : every;
  return MP_OK;
}

static int view_record_lines(const ViewWords& w, const DevTables& t, const ego_layer::Window& g) {
  if ((t.grid_pad & 15) || (t.world_stride & 15) || (int64_t)g.L * g.HW > (int64_t)t.grid_pad)
    return fail(MP_ERR_UNSUPPORTED, "%s: a record of %d bytes with %d bytes of planes is not read in 16-byte lines",
                w.who, t.world_stride, t.grid_pad);
  return MP_OK;
}

// A registration's geometry: the ring, the bytes `dst` must hold (*need) with `world` bytes a world
// and slots `align`-byte aligned (1: anywhere), and `dst` itself.
static int view_register(MpEngine* e, const ViewRequest& q, const ViewWords& w, uint64_t world, unsigned align,
                         uint64_t* need) {
  const uint64_t block = (uint64_t)e->N * world;
  if (q.slots < 0) return fail(MP_ERR_INVALID, "%s: slots %d", w.who, q.slots);
  if (q.slots > 0 && q.slots != e->ring_slots)
    return fail(MP_ERR_INVALID, "%s: a ring of %d slots, the engine's ring has %d (mp_bind_output_ring; one "
                "position for all of them)", w.who, q.slots, e->ring_slots);
  if (q.slots > 0 && (q.slot_stride < block || (q.slot_stride & (align - 1)))) {
    char lie[48] = "";
    if (align > 1) snprintf(lie, sizeof lie, ", and slots lie %u-byte aligned", align);
    return fail(MP_ERR_INVALID, "%s: slot_stride %llu: a slot is %llu bytes%s", w.who,
                (unsigned long long)q.slot_stride, (unsigned long long)block, lie);
  }
  *need = q.slots > 0 ? (uint64_t)(q.slots - 1) * q.slot_stride + block : block;
  if (q.dst_bytes < *need)
    return fail(MP_ERR_INVALID, "%s: %s of %d worlds%s %s %llu bytes, dst has %llu", w.who, w.thing, e->N,
                q.slots > 0 ? " in every slot" : "", w.need, (unsigned long long)*need,
                (unsigned long long)q.dst_bytes);
  HIP_TRY(hipSetDevice(e->device));
  char name[48];
  snprintf(name, sizeof name, "%s (dst)", w.who);
  if (int rc = check_device_pointer(e, q.dst, name)) return rc;
  return check_bank(e, q.dst, *need, name);
}

static MpEngine::ViewRegistration registration_of(const ViewRequest& q) {
  MpEngine::ViewRegistration v;
  v.dst = q.dst;
  v.stride = q.slots > 0 ? q.slot_stride : 0;
  v.slots = q.slots;
  return v;
}

// What a draw or a host call reads and how much it writes: `view` bytes an element with players[],
// `world` without.
struct ViewSource {
  bool live;          // the engine's worlds
  int32_t src_rows;
  uint64_t need;      // bytes of dst
};
static int view_source(const MpEngine* e, const ViewRequest& q, const ViewWords& w, const ViewTables& v,
                       uint64_t view, uint64_t world, ViewSource* s) {
  s->live = q.op == VIEW_DRAW && !q.bank;
  if (q.op == VIEW_HOST && !q.bank) return fail(MP_ERR_INVALID, "%s: NULL bank", w.who);
  s->src_rows = s->live ? e->N : q.bank_rows;
  if (int rc = check_counts(w.who, q.count, s->src_rows)) return rc;
  if (int rc = check_row_list(w.who, q.rows, q.count, s->src_rows, w.drawn, false)) return rc;
  if (int rc = check_fingerprint(w.who, q.fingerprint, v.fingerprint, e ? "engine's" : "pack's")) return rc;
  if (int rc = check_dst_bytes(w.who, q.count, q.players ? view : world, q.dst_bytes, &s->need)) return rc;
  if (((uintptr_t)q.rows & 3) || ((uintptr_t)q.players & 3))
    return fail(MP_ERR_INVALID, "%s: rows %p and players %p must be 4-byte aligned", w.who, (const void*)q.rows,
                (const void*)q.players);
  return MP_OK;
}

// The fields every unit's Args has, of a draw or a host call.
template <class Args>
static void view_args(Args* a, const ego_layer::Window& g, const ViewRequest& q, const ViewTables& v,
                      const ViewSource& s) {
  a->g = g;
  a->rows = q.rows; a->players = q.players;
  a->src_rows = s.src_rows; a->count = q.count;
  a->stride = v.t->world_stride; a->grid_pad = v.t->grid_pad;
}

// The host twin met an index out of range at position `bad` (`row`: of rows[], else of players[]).
static int view_host_fault(const ViewRequest& q, const ViewWords& w, int bad, bool row) {
  return fail(MP_ERR_INVALID, "%s: %s[%d] = %d is %s; the elements from %d on were left as they were", w.who,
              row ? "rows" : "players", bad, row ? (q.rows ? q.rows[bad] : bad) : q.players[bad],
              row ? "not a row of the bank" : "not a player of this pack", bad);
}

// A draw's device memory: the state or the bank, rows, players, a class table, dst.
static int view_device_source(MpEngine* e, const ViewRequest& q, const ViewWords& w, const ViewSource& s,
                              const void* classes, uint64_t classes_bytes) {
  if (s.live && !e->has_state)
    return fail(MP_ERR_INVALID, "%s: the engine has never been reset; there is no state to %s", w.who, w.draw);
  const uint64_t count = (uint64_t)q.count, bank = (uint64_t)q.bank_rows * (uint64_t)e->t.world_stride;
  return check_extents(e, w.who, {{"bank", s.live ? nullptr : q.bank, bank, 16},   // (records are read in 16-byte lines)
                                  {"rows", q.rows, count * 4, 1},
                                  {"players", q.players, count * 4, 1},
                                  {"classes", classes, classes_bytes, 1},
                                  {"dst", q.dst, s.need, 1}});
}

// ---- the world ops: the whole map in place of the viewers' windows (world_view.h) ----------------
// The front reads a world op as the op it is the twin of (q.op - 3); `players` must be NULL.
constexpr int kWorldOps = 3;
static bool world_op(int32_t op) { return op > VIEW_HOST && op <= VIEW_HOST + kWorldOps; }

// The world's value table and the length of a class table: the engine's, or the pack's.
struct WorldTable {
  std::vector<int32_t> host;
  const int32_t* lut = nullptr;   // (an engine: device memory)
  int32_t num_ids = 0;
};
static void world_table(const MpEngine* e, const ViewTables& v, WorldTable* wt) {
  if (e) { wt->lut = e->d_world_lut; wt->num_ids = e->num_world_ids; return; }
  wt->host = world_lut_row(v.h.pack.data(), *v.t);
  wt->lut = wt->host.data();
  wt->num_ids = world_view::num_ids(wt->lut);
}

static int world_geometry(const ViewWords& w, const DevTables& t, const ego_layer::Window& g) {
  if (int rc = view_record_lines(w, t, g)) return rc;
  if ((uint64_t)g.HW * (uint64_t)g.L * (uint64_t)g.L >= (1ull << 32))   // (a word's cell is found with one multiply)
    return fail(MP_ERR_UNSUPPORTED, "%s: a map of %d cells and %d layers", w.who, g.HW, g.L);
  return MP_OK;
}

static int world_layer_request(MpEngine* e, const MpEgoLayer& r) {
  static const ViewWords w = {"MpEgoLayer", "MP_EGO_WORLD_HOST", "the WORLD.LAYER leaf", "needs", "drawn", "draw"};
  const char* const kWho = w.who;
  ViewRequest q = view_of(&r);
  q.op -= kWorldOps;
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.players) return fail(MP_ERR_INVALID, "%s: the world ops take no players (players must be NULL)", kWho);
  if (q.op == VIEW_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->wl = MpEngine::ViewRegistration{};
    return MP_OK;
  }
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  if ((uintptr_t)r.dst & 3) return fail(MP_ERR_INVALID, "%s: dst %p is not 4-byte aligned", kWho, r.dst);
  ViewTables v;
  if (int rc = view_tables(e, q, &v, false)) return rc;
  WorldTable wt;
  world_table(e, v, &wt);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  const uint64_t world = (uint64_t)g.HW * (uint64_t)g.L * 4u;
  if (g.L > 64) return fail(MP_ERR_UNSUPPORTED, "%s: %d layers; the world ops take 64", kWho, g.L);
  if (int rc = world_geometry(w, *v.t, g)) return rc;
  if (q.op == VIEW_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 4, &need)) return rc;
    if (world_view::layer_plan(g, e->N, e->num_cus).waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes need %d B of LDS", kWho,
                  world_view::layer_plan(g, e->N, e->num_cus).lds);
    e->wl = registration_of(q);
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, world, world, &s)) return rc;
  world_view::LayerArgs a = {};
  view_args(&a, g, q, v, s);
  a.dst = (int32_t*)r.dst;
  a.lut = wt.lut;
  if (q.op == VIEW_HOST) {
    a.src = (const uint8_t*)r.bank;
    const int bad = world_view::host(a);
    return bad >= 0 ? view_host_fault(q, w, bad, true) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, nullptr, 0)) return rc;
  const world_view::Plan p = world_view::layer_plan(g, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes need %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.fault = e->t.fault;
  world_view::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// (`out` is the caller's struct: num_ids — the world's — is written back)
static int world_planes_request(MpEngine* e, MpEgoPlanes* out) {
  static const ViewWords w = {"MpEgoPlanes", "MP_EGOPLANES_WORLD_HOST", "the world planes", "need", "drawn", "draw"};
  const char* const kWho = w.who;
  MpEgoPlanes r;
  memcpy(&r, out, sizeof r);
  ViewRequest q = view_of(&r);
  q.op -= kWorldOps;
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.players) return fail(MP_ERR_INVALID, "%s: the world ops take no players (players must be NULL)", kWho);
  if (q.op == VIEW_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->wp = MpEngine::ViewRegistration{};
    out->num_ids = e->num_world_ids;
    return MP_OK;
  }
  ViewTables v;
  if (int rc = view_tables(e, q, &v, false)) return rc;
  WorldTable wt;
  world_table(e, v, &wt);
  const int32_t num_ids = wt.num_ids;
  out->num_ids = num_ids;
  if (q.op != VIEW_REGISTER && r.count == 0 && !r.dst) return MP_OK;   // the question alone
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  uint64_t layer_mask;
  if (int rc = view_layer_mask(w, g, r.layer_mask, &layer_mask)) return rc;
  if (!r.classes) return fail(MP_ERR_INVALID, "%s: NULL classes: the planes are those of a class table", kWho);
  if (r.classes_len != num_ids)
    return fail(MP_ERR_INVALID, "%s: classes_len %d: a class table of the world has one entry per id of the world's "
                "sprite map, %d of them", kWho, r.classes_len, num_ids);
  if ((uintptr_t)r.classes & 3)
    return fail(MP_ERR_INVALID, "%s: classes %p is not 4-byte aligned", kWho, (const void*)r.classes);
  if (r.num_classes < 1 || r.num_classes > ego_planes::kMaxClasses)
    return fail(MP_ERR_INVALID, "%s: num_classes %d is outside [1, %d]", kWho, r.num_classes, ego_planes::kMaxClasses);
  if (r.facing != 0 && r.facing != 1) return fail(MP_ERR_INVALID, "%s: facing %d is neither 0 nor 1", kWho, r.facing);
  if (int rc = world_geometry(w, *v.t, g)) return rc;
  const int num_planes = r.num_classes + (r.facing ? 4 : 0);
  const uint64_t world = (uint64_t)num_planes * (uint64_t)g.HW;
  if (q.op == VIEW_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 1, &need)) return rc;
    if (int rc = check_bank(e, r.classes, (uint64_t)num_ids * 4, "MpEgoPlanes (classes)")) return rc;
    const world_view::Plan p = world_view::planes_plan(g, r.num_classes, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes and class masks need %d B of LDS", kWho, p.lds);
    e->wp = registration_of(q);
    e->wp.mask = layer_mask;
    e->wp.classes = r.classes;
    e->wp.num_classes = r.num_classes;
    e->wp.facing = r.facing;
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, world, world, &s)) return rc;
  world_view::PlanesArgs a = {};
  view_args(&a, g, q, v, s);
  a.dst = (uint8_t*)r.dst;
  a.lut = wt.lut;
  a.layer_mask = layer_mask;
  a.classes = r.classes; a.num_ids = num_ids;
  a.num_classes = r.num_classes; a.facing = r.facing;
  if (q.op == VIEW_HOST) {
    for (int32_t id = 0; id < num_ids; ++id)
      if (r.classes[id] < -1 || r.classes[id] >= r.num_classes)
        return fail(MP_ERR_INVALID, "%s: classes[%d] = %d is outside [-1, num_classes = %d)", kWho, id,
                    r.classes[id], r.num_classes);
    a.src = (const uint8_t*)r.bank;
    const int bad = world_view::host(a);
    return bad >= 0 ? view_host_fault(q, w, bad, true) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, r.classes, (uint64_t)num_ids * 4)) return rc;
  const world_view::Plan p = world_view::planes_plan(g, r.num_classes, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes and class masks need %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.fault = e->t.fault;
  world_view::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

int ego_layer_request(MpEngine* e, const MpEgoLayer& r) {
  if (world_op(r.op)) return world_layer_request(e, r);
  static const ViewWords w = {"MpEgoLayer", "MP_EGO_HOST", "the leaf", "needs", "drawn", "draw"};
  const char* const kWho = w.who;
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_EGO_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->ego = MpEngine::ViewRegistration{};
    return MP_OK;
  }
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  if ((uintptr_t)r.dst & 3) return fail(MP_ERR_INVALID, "%s: dst %p is not 4-byte aligned", kWho, r.dst);
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  const uint64_t view = (uint64_t)g.VH * (uint64_t)g.VW * (uint64_t)g.L * 4u, world = view * (uint64_t)g.P;
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  if (r.op == MP_EGO_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 4, &need)) return rc;
    const ego_layer::Plan p = ego_layer::plan_of(g, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes need %d B of LDS", kWho, p.lds);
    e->ego = registration_of(q);
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, view, world, &s)) return rc;
  ego_layer::Args a = {};
  view_args(&a, g, q, v, s);
  a.dst = (int32_t*)r.dst;
  if (r.op == MP_EGO_HOST) {
    a.src = (const uint8_t*)r.bank;
    a.lut = v.host_lut.data();
    uint32_t what = 0;
    const int bad = ego_layer::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultEgoRow) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, nullptr, 0)) return rc;
  const ego_layer::Plan p = ego_layer::plan_of(g, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's render planes need %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.lut = e->d_layer_lut; a.fault = e->t.fault;
  ego_layer::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// (`out` is the caller's struct: num_ids is written back)
int view_hash_request(MpEngine* e, MpViewHash* out) {
  static const ViewWords w = {"MpViewHash", "MP_VIEWHASH_HOST", "the hashes", "need", "hashed", "hash"};
  const char* const kWho = w.who;
  MpViewHash r;
  memcpy(&r, out, sizeof r);
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_VIEWHASH_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->vh = MpEngine::ViewRegistration{};
    out->num_ids = e->num_layer_ids;
    return MP_OK;
  }
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const int32_t num_ids = v.num_ids;
  if (num_ids < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the pack's view tables hold a negative id", kWho);
  out->num_ids = num_ids;
  if (r.op != MP_VIEWHASH_REGISTER && r.count == 0 && !r.dst) return MP_OK;   // the question alone
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  if ((uintptr_t)r.dst & 7) return fail(MP_ERR_INVALID, "%s: dst %p is not 8-byte aligned", kWho, r.dst);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  uint64_t layer_mask;
  if (int rc = view_layer_mask(w, g, r.layer_mask, &layer_mask)) return rc;
  if (r.classes ? r.classes_len != num_ids : r.classes_len != 0)
    return fail(MP_ERR_INVALID, "%s: classes_len %d: a class table has one entry per id, %d of them (0 without "
                "a table)", kWho, r.classes_len, num_ids);
  if ((uintptr_t)r.classes & 3)
    return fail(MP_ERR_INVALID, "%s: classes %p is not 4-byte aligned", kWho, (const void*)r.classes);
  const uint64_t world = (uint64_t)g.P * 8u;
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  const int num_classes = r.classes ? num_ids : 0;
  if (r.op == MP_VIEWHASH_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 8, &need)) return rc;
    if (r.classes)
      if (int rc = check_bank(e, r.classes, (uint64_t)num_classes * 4, "MpViewHash (classes)")) return rc;
    const view_hash::Plan p = view_hash::plan_of(g, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render planes need %d B of LDS", kWho, p.lds);
    e->vh = registration_of(q);
    e->vh.mask = layer_mask;
    e->vh.classes = r.classes;
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, 8u, world, &s)) return rc;
  view_hash::Args a = {};
  view_args(&a, g, q, v, s);
  a.dst = (uint64_t*)r.dst;
  a.layer_mask = layer_mask;
  a.classes = r.classes; a.num_classes = num_classes;
  if (r.op == MP_VIEWHASH_HOST) {
    a.src = (const uint8_t*)r.bank;
    a.lut = v.host_lut.data();
    uint32_t what = 0;
    const int bad = view_hash::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultViewHashRow) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, r.classes, (uint64_t)num_classes * 4)) return rc;
  const view_hash::Plan p = view_hash::plan_of(g, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render planes need %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.lut = e->d_layer_lut; a.fault = e->t.fault;
  view_hash::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// (`out` is the caller's struct: num_ids is written back)
int ego_planes_request(MpEngine* e, MpEgoPlanes* out) {
  if (world_op(out->op)) return world_planes_request(e, out);
  static const ViewWords w = {"MpEgoPlanes", "MP_EGOPLANES_HOST", "the planes", "need", "drawn", "draw"};
  const char* const kWho = w.who;
  MpEgoPlanes r;
  memcpy(&r, out, sizeof r);
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_EGOPLANES_REGISTER && !r.dst) {   // clears the registration: the engine's launches are what they were
    e->ep = MpEngine::ViewRegistration{};
    out->num_ids = e->num_layer_ids;
    return MP_OK;
  }
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const int32_t num_ids = v.num_ids;
  if (num_ids < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the pack's view tables hold a negative id", kWho);
  out->num_ids = num_ids;
  if (r.op != MP_EGOPLANES_REGISTER && r.count == 0 && !r.dst) return MP_OK;   // the question alone
  if (!r.dst) return fail(MP_ERR_INVALID, "%s: NULL dst", kWho);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  uint64_t layer_mask;
  if (int rc = view_layer_mask(w, g, r.layer_mask, &layer_mask)) return rc;
  if (!r.classes) return fail(MP_ERR_INVALID, "%s: NULL classes: the planes are those of a class table", kWho);
  if (r.classes_len != num_ids)
    return fail(MP_ERR_INVALID, "%s: classes_len %d: a class table has one entry per id, %d of them", kWho,
                r.classes_len, num_ids);
  if ((uintptr_t)r.classes & 3)
    return fail(MP_ERR_INVALID, "%s: classes %p is not 4-byte aligned", kWho, (const void*)r.classes);
  if (r.num_classes < 1 || r.num_classes > ego_planes::kMaxClasses)
    return fail(MP_ERR_INVALID, "%s: num_classes %d is outside [1, %d]", kWho, r.num_classes, ego_planes::kMaxClasses);
  if (r.facing != 0 && r.facing != 1) return fail(MP_ERR_INVALID, "%s: facing %d is neither 0 nor 1", kWho, r.facing);
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  const int num_planes = r.num_classes + (r.facing ? 4 : 0);
  const uint64_t view = (uint64_t)num_planes * (uint64_t)g.VH * (uint64_t)g.VW, world = (uint64_t)g.P * view;
  if (view * (uint64_t)g.VH * (uint64_t)g.VW >= (1ull << 32))   // (a byte's plane is found with one multiply)
    return fail(MP_ERR_UNSUPPORTED, "%s: a viewer's planes are %llu bytes", kWho, (unsigned long long)view);
  if (r.op == MP_EGOPLANES_REGISTER) {
    uint64_t need;
    if (int rc = view_register(e, q, w, world, 1, &need)) return rc;
    if (int rc = check_bank(e, r.classes, (uint64_t)num_ids * 4, "MpEgoPlanes (classes)")) return rc;
    const ego_planes::Plan p = ego_planes::plan_of(g, num_planes, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render and bit planes need %d B of LDS",
                  kWho, p.lds);
    e->ep = registration_of(q);
    e->ep.mask = layer_mask;
    e->ep.classes = r.classes;
    e->ep.num_classes = r.num_classes;
    e->ep.facing = r.facing;
    return MP_OK;
  }
  ViewSource s;
  if (int rc = view_source(e, q, w, v, view, world, &s)) return rc;
  ego_planes::Args a = {};
  view_args(&a, g, q, v, s);
  a.dst = (uint8_t*)r.dst;
  a.layer_mask = layer_mask;
  a.classes = r.classes; a.num_ids = num_ids;
  a.num_classes = r.num_classes; a.facing = r.facing;
  if (r.op == MP_EGOPLANES_HOST) {
    for (int32_t id = 0; id < num_ids; ++id)
      if (r.classes[id] < -1 || r.classes[id] >= r.num_classes)
        return fail(MP_ERR_INVALID, "%s: classes[%d] = %d is outside [-1, num_classes = %d)", kWho, id,
                    r.classes[id], r.num_classes);
    a.src = (const uint8_t*)r.bank;
    a.lut = v.host_lut.data();
    uint32_t what = 0;
    const int bad = ego_planes::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultEgoPlanesRow) : MP_OK;
  }
  if (int rc = view_device_source(e, q, w, s, r.classes, (uint64_t)num_ids * 4)) return rc;
  const ego_planes::Plan p = ego_planes::plan_of(g, num_planes, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: the value tables and one wave's render and bit planes need %d B of LDS",
                kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.lut = e->d_layer_lut; a.fault = e->t.fault;
  ego_planes::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}

// Two destinations of one shape, either may be absent: the front's checks run once for each that
// is there, on a copy of the request's beginning that names it as `dst`.
int avatar_ids_request(MpEngine* e, const MpAvatarIds& r) {
  static const ViewWords w = {"MpAvatarIds", "MP_AVATARIDS_HOST", "a leaf", "needs", "drawn", "draw"};
  const char* const kWho = w.who;
  const ViewRequest q = view_of(&r);
  if (int rc = view_prologue(e, q, w, sizeof r,
                             r.reserved == 0 && r.reserved2[0] == 0 && r.reserved2[1] == 0 && r.reserved2[2] == 0))
    return rc;
  if (r.op == MP_AVATARIDS_REGISTER && !r.dst && !r.dst_zap) {   // clears the registration: the engine's launches are what they were
    e->av = e->avz = MpEngine::ViewRegistration{};
    return MP_OK;
  }
  if (!r.dst && !r.dst_zap) return fail(MP_ERR_INVALID, "%s: NULL dst and NULL dst_zap", kWho);
  if (((uintptr_t)r.dst | (uintptr_t)r.dst_zap) & 3)
    return fail(MP_ERR_INVALID, "%s: dst %p and dst_zap %p must be 4-byte aligned", kWho, r.dst, r.dst_zap);
  ViewTables v;
  if (int rc = view_tables(e, q, &v)) return rc;
  const SubstrateTables& sub = e ? e->sub : v.h.d.sub;
  const ZapRules* zap = zap_rules_of(sub);
  if (r.dst_zap && !zap)
    return fail(MP_ERR_INVALID, "%s: %s has no Zapper: there is no AVATAR_IDS_IN_RANGE_TO_ZAP on this level "
                "(AVATAR_IDS_IN_VIEW works on every level)", kWho, family_name(sub));
  if (r.dst_zap && (zap->shape.n < 1 || zap->shape.n > 16))
    return fail(MP_ERR_UNSUPPORTED, "%s: a zap footprint of %d cells", kWho, zap->shape.n);
  const ego_layer::Window g = ego_layer::window_of(*v.t);
  const uint64_t view = (uint64_t)g.P * 4u, world = view * (uint64_t)g.P;
  if (int rc = view_record_lines(w, *v.t, g)) return rc;
  if (v.t->avatar_layer < 0 || v.t->avatar_layer >= g.L)
    return fail(MP_ERR_UNSUPPORTED, "%s: avatar_layer %d is no render plane", kWho, v.t->avatar_layer);
  ViewRequest qv = q, qz = q;   // the request as IN_VIEW's alone, as IN_RANGE's alone
  qz.dst = r.dst_zap; qz.dst_bytes = r.dst_zap_bytes;
  avatar_ids::Args a = {};
  avatar_ids_tables(&a, *v.t, r.dst_zap ? zap : nullptr,
                    e ? (const uint32_t*)e->t.step_blob : (const uint32_t*)v.h.d.step_blob.data());
  if (r.op == MP_AVATARIDS_REGISTER) {
    uint64_t need;
    if (r.dst) if (int rc = view_register(e, qv, w, world, 4, &need)) return rc;
    if (r.dst_zap) if (int rc = view_register(e, qz, w, world, 4, &need)) return rc;
    const avatar_ids::Plan p = avatar_ids::plan_of(g, a.plane_at, e->N, e->num_cus);
    if (p.waves < 1)
      return fail(MP_ERR_UNSUPPORTED, "%s: one wave's avatar plane needs %d B of LDS", kWho, p.lds);
    e->av = r.dst ? registration_of(qv) : MpEngine::ViewRegistration{};
    e->avz = r.dst_zap ? registration_of(qz) : MpEngine::ViewRegistration{};
    return MP_OK;
  }
  ViewSource s, sz;
  if (r.dst) if (int rc = view_source(e, qv, w, v, view, world, &s)) return rc;
  if (r.dst_zap) if (int rc = view_source(e, qz, w, v, view, world, &sz)) return rc;
  if (!r.dst) s = sz;
  view_args(&a, g, q, v, s);
  a.dst = (int32_t*)r.dst;
  a.dst_zap = (int32_t*)r.dst_zap;
  if (r.op == MP_AVATARIDS_HOST) {
    a.src = (const uint8_t*)r.bank;
    uint32_t what = 0;
    const int bad = avatar_ids::host(a, &what);
    return bad >= 0 ? view_host_fault(q, w, bad, what == kFaultAvatarIdsRow) : MP_OK;
  }
  if (r.dst) if (int rc = view_device_source(e, qv, w, s, nullptr, 0)) return rc;
  if (r.dst_zap) if (int rc = view_device_source(e, qz, w, s, nullptr, 0)) return rc;
  const avatar_ids::Plan p = avatar_ids::plan_of(g, a.plane_at, r.count, e->num_cus);
  if (p.waves < 1)
    return fail(MP_ERR_UNSUPPORTED, "%s: one wave's avatar plane needs %d B of LDS", kWho, p.lds);
  a.src = s.live ? e->d_state : (const uint8_t*)r.bank;
  a.fault = e->t.fault;
  avatar_ids::launch(a, p, e->stream);
  HIP_TRY(hipGetLastError());
  return MP_OK;
}
