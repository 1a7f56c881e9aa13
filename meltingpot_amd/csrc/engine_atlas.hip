// engine_atlas.hip — the sprite atlas and the composite cache of an engine, built on the host by
// mp_create (build_atlas) and uploaded once.  No kernel here.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "engine_state.h"

namespace {

// The renderer's images: the de-duplicated sprite atlas (noRotate sprites and solid colours
// have four identical facings), then the composite cache's and its (base, overlay) table.
struct Atlas {
  std::vector<uint8_t> images = std::vector<uint8_t>(256, 0);   // image 0: unused padding
  std::vector<uint16_t> slots;                                  // (sprite, facing) -> image
  std::vector<uint32_t> pair_table = std::vector<uint32_t>(kPairSlots, 0xffffffffu);
  int count = 1, pair_probe = 0, n_composites = 0, used_slots = 0;

  int add_image(const uint8_t* img, int from) {
    for (int k = from; k < count; ++k)
      if (memcmp(images.data() + (size_t)k * 256, img, 256) == 0) return k;
    images.insert(images.end(), img, img + 256);
    return count++;
  }
  void add_sprites(const uint8_t* rgba, const int32_t* flags, int nimg) {
    slots.assign((size_t)nimg, 0);
    for (int i = 0; i < nimg; ++i) {
      uint8_t img[256];
      memcpy(img, rgba + (size_t)i * 256, 256);
      if (flags[i >> 2] & MPK_SPRITE_OPAQUE) {
        // opaque images are only ever copied: store them pre-packed, 8 rows of
        // 24 B RGB followed by 8 B of padding
        uint8_t packed[256] = {0};
        for (int py = 0; py < 8; ++py)
          for (int px = 0; px < 8; ++px)
            for (int ch = 0; ch < 3; ++ch)
              packed[py * 32 + px * 3 + ch] = img[(py * 8 + px) * 4 + ch];
        memcpy(img, packed, 256);
      }
      slots[(size_t)i] = (uint16_t)add_image(img, 1);
    }
  }
  int lookup(uint32_t a, uint32_t b) const {
    for (uint32_t h = pair_hash(a, b), k = 0; k < (uint32_t)kPairSlots; ++k) {
      const uint32_t ent = pair_table[(h + k) & (kPairSlots - 1)];
      if (ent == 0xffffffffu) return -1;
      if ((ent >> 10) == ((a << 10) | b)) return (int)(ent & 1023u);
    }
    return -1;
  }
  void insert(uint32_t a, uint32_t b, uint32_t c) {
    for (uint32_t h = pair_hash(a, b), k = 0; k < (uint32_t)kPairSlots; ++k) {
      uint32_t& ent = pair_table[(h + k) & (kPairSlots - 1)];
      if (ent == 0xffffffffu) {
        ent = (a << 20) | (b << 10) | c;
        if ((int)k + 1 > pair_probe) pair_probe = (int)k + 1;
        return;
      }
    }
  }
  // one overlay image blended onto a packed opaque image, exactly as
  // render.hip does it (A7: (s*a + d*(255-a) + 127) / 255; binary sprites
  // replace where alpha > 0)
  void blend(int base_img, int ov_img, bool partial, uint8_t* out) const {
    memcpy(out, images.data() + (size_t)base_img * 256, 256);
    const uint8_t* ov = images.data() + (size_t)ov_img * 256;
    for (int py = 0; py < 8; ++py)
      for (int px = 0; px < 8; ++px) {
        const uint8_t* s = ov + (py * 8 + px) * 4;
        uint8_t* d = out + py * 32 + px * 3;
        const unsigned a = s[3];
        for (int ch = 0; ch < 3; ++ch) {
          if (partial) d[ch] = (uint8_t)((s[ch] * a + d[ch] * (255u - a) + 127u) / 255u);
          else if (a) d[ch] = s[ch];
        }
      }
  }
};

// An opaque look, then up to two non-opaque looks on higher layers; `cells` that can show it.
struct Look { int layer, sprite, orient; };
struct Stack { int n; Look l[3]; long cells; };

Stack& count_stack(std::vector<Stack>& stacks, const Look* l, int n) {
  for (auto& sk : stacks) {
    bool eq = sk.n == n;
    for (int k = 0; eq && k < n; ++k) eq = sk.l[k].sprite == l[k].sprite && sk.l[k].orient == l[k].orient;
    if (eq) { sk.cells++; return sk; }
  }
  Stack sk; sk.n = n; sk.cells = 1;
  for (int k = 0; k < n; ++k) sk.l[k] = l[k];
  stacks.push_back(sk);
  return stacks.back();
}

// Composite cache (render.hip phase 1): the (opaque base, overlay) stacks that the
// map's static pieces can form — dirt on water, shadows on sand, claimed-resource
// paint on its texture ... — so such cells become plain copies.  A piece's possible
// looks are all sprite-bearing states of its prefab ("prefab.state" names); avatars,
// their markings and beams move, so they are never part of a cached stack.
std::vector<Stack> collect_stacks(const MpEngine* e, const int32_t* flags) {
  const DevTables& t = e->t;
  const void* hp = e->pack.data();
  uint64_t names_len = 0;
  const char* names = table<char>(hp, "state_names", &names_len);
  const int32_t* objs = table<int32_t>(hp, "objects");
  const int32_t* st_layer = table<int32_t>(hp, "state_layer");
  const int32_t* st_sprite = table<int32_t>(hp, "state_sprite");
  const int32_t* st_orient = table<int32_t>(hp, "state_orient");
  const int nobj = table<int32_t>(hp, "hdr")[MPK_HDR_NOBJ];
  std::vector<std::string> prefab((size_t)t.nstates);
  for (uint64_t s = 0, off = 0; s < (uint64_t)t.nstates && off < names_len; ++s) {
    const std::string nm(names + off);
    off += nm.size() + 1;
    prefab[s] = nm.substr(0, nm.find('.'));
  }
  std::vector<std::vector<Look>> cell_looks((size_t)t.H * t.W);
  for (int i = 0; i < nobj; ++i) {
    const int32_t* ob = objs + 4 * i;
    if (ob[0] == MPK_KIND_SCENE || ob[0] == MPK_KIND_AVATAR || ob[0] == MPK_KIND_MARKING) continue;
    for (int s = 1; s < t.nstates; ++s)
      if (prefab[(size_t)s] == prefab[(size_t)ob[3]] && st_sprite[s] >= 0 && st_layer[s] >= 0)
        cell_looks[(size_t)ob[2] * t.W + ob[1]].push_back({st_layer[s], st_sprite[s], st_orient[s]});
  }
  std::vector<Stack> stacks;
  auto overlay = [&](const Look& l) { return !(flags[l.sprite] & (MPK_SPRITE_OPAQUE | MPK_SPRITE_EMPTY)); };
  for (const auto& looks : cell_looks) {
    // (sprite -1: no opaque piece below — the renderer starts from image 0,
    // black; the *_in_the_matrix maps have no floor under their resources)
    std::vector<Look> bases;
    for (const Look& a : looks)
      if (flags[a.sprite] & MPK_SPRITE_OPAQUE) bases.push_back(a);
    if (bases.empty()) bases.push_back({-1, -1, 0});   // a cell no piece can cover
    for (const Look& a : bases)
      for (const Look& b : looks) {
        if (b.layer <= a.layer || !overlay(b)) continue;
        const Look ab[3] = {a, b, b};
        count_stack(stacks, ab, 2);
        for (const Look& c : looks) {
          if (c.layer <= b.layer || !overlay(c)) continue;
          const Look abc[3] = {a, b, c};
          count_stack(stacks, abc, 3);
        }
      }
  }
  // stacks the lowering knows to be the common ones (territory: texture + wet +
  // dry paint of the SAME player, 9 of 81 combinations): first in their class
  uint64_t nh = 0;
  const int32_t* hints = table<int32_t>(hp, "composite_hints", &nh);
  for (uint64_t i = 0; hints && i + 2 < nh; i += 3) {
    Look l[3]; int n = 0; bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const int st = hints[i + k];
      if (st == 0 && k > 0) break;
      if (st <= 0 || st >= t.nstates || st_sprite[st] < 0 || st_layer[st] < 0) { ok = false; break; }
      l[n++] = {st_layer[st], st_sprite[st], st_orient[st]};
    }
    if (!ok || n < 2 || !(flags[l[0].sprite] & MPK_SPRITE_OPAQUE)) continue;
    for (int m = 2; m <= n; ++m) count_stack(stacks, l, m).cells = 1L << 40;
  }
  std::sort(stacks.begin(), stacks.end(), [](const Stack& x, const Stack& y) {
    return x.n != y.n ? x.n < y.n : x.cells > y.cells;   // all pairs before triples
  });
  return stacks;
}

// The composite cache's images, most common stacks first, in the LDS the renderer's preferred
// geometry leaves (more images must not cost worlds per workgroup: tools/sweep_env.sh).
void fill_composites(MpEngine* e, const MpDevOptions* dev, const int32_t* flags,
                     const std::vector<Stack>& stacks, Atlas& a) {
  DevTables& t = e->t;
  t.n_images = a.count;
  int max_composites = kPairSlots;
  for (int v = 0; v < 6; ++v) {
    const FramePlan p0 = plan_frame(t, e->sub, e->N, (v & 1) != 0, v >> 1, e->num_cus, dev, 1, e->world_pool);
    max_composites = std::min(max_composites,
                              (160 * 1024 - frame_lds_bytes(t, p0, 1, e->world_pool, v >> 1)) / 272);
  }
  max_composites = std::max(0, std::min(max_composites, kPairSlots / 2));
  if (dev && dev->max_composites >= 0) max_composites = std::min(max_composites, (int)dev->max_composites);
  for (const Stack& sk : stacks)
    for (int f = 0; f < 4; ++f) {
      int base = sk.l[0].sprite < 0 ? 0 : a.slots[(size_t)sk.l[0].sprite * 4 + ((f + sk.l[0].orient) & 3)];
      for (int k = 1; k < sk.n; ++k) {
        const int ov = a.slots[(size_t)sk.l[k].sprite * 4 + ((f + sk.l[k].orient) & 3)];
        int comp = a.lookup((uint32_t)base, (uint32_t)ov);
        if (comp < 0) {
          // (a triple extends a cached pair; it is skipped if its pair was)
          if (k < sk.n - 1 || a.n_composites >= max_composites || a.used_slots >= kPairSlots / 2 ||
              a.count >= 1023)
            break;
          uint8_t img[256];
          a.blend(base, ov, (flags[sk.l[k].sprite] & MPK_SPRITE_PARTIAL) != 0, img);
          const int before = a.count;
          comp = a.add_image(img, 0);
          a.n_composites += a.count - before;
          a.insert((uint32_t)base, (uint32_t)ov, (uint32_t)comp);
          ++a.used_slots;
        }
        base = comp;
      }
    }
}

}  // namespace

// The renderer's atlas, composite cache and render blob.  (On the device side only
// because the composite budget comes from plan_frame, which needs the CU count.)
int build_atlas(MpEngine* e, const MpDevOptions* dev, const DecodedPack& d) {
  DevTables& t = e->t;
  const int32_t* flags = table<int32_t>(e->pack.data(), "sprite_flags");
  Atlas a;
  a.add_sprites(table<uint8_t>(e->pack.data(), "sprite_rgba"), flags, t.nsprites * 4);
  t.scratch_cells = (dev && dev->scratch_cells > 0) ? dev->scratch_cells : 8;
  if (!(dev && dev->no_composite_cache)) fill_composites(e, dev, flags, collect_stacks(e, flags), a);
  if (a.count > 1023) return fail(MP_ERR_PACK, "mp_create: %d distinct sprite images", a.count);
  t.n_images = a.count;
  t.pair_probe = a.pair_probe;
  // the atlas and the render blob (what every render workgroup stages besides its worlds,
  // already in LDS layout), uploaded in one buffer
  const void* hp = e->pack.data();
  const int nimg = t.nsprites * 4;
  const size_t img_bytes = (size_t)a.count * 256, slot_bytes = ((size_t)nimg * 2 + 15) & ~(size_t)15,
               pair_bytes = (size_t)kPairSlots * 4, blob_bytes = (size_t)render_blob_bytes(t);
  std::vector<uint8_t> flags8((size_t)t.nsprites);
  for (int s = 0; s < t.nsprites; ++s)
    flags8[(size_t)s] = (uint8_t)(((flags[s] & MPK_SPRITE_OPAQUE) ? 1 : 0) |
                                  ((flags[s] & MPK_SPRITE_PARTIAL) ? 2 : 0) |
                                  ((flags[s] & MPK_SPRITE_EMPTY) ? 4 : 0));
  const int8_t* splayer = reinterpret_cast<const int8_t*>(d.extra.data() + 256);   // state -> player
  // viewers 0 .. P-1, then the world view (row P_pack of the pack's table)
  const int32_t* vmap = table<int32_t>(hp, "view_sprite_map");
  std::vector<int32_t> vmap_p((size_t)(t.P + 1) * t.nsprites);
  for (int v = 0; v <= t.P; ++v)
    memcpy(vmap_p.data() + (size_t)v * t.nsprites,
           vmap + (size_t)(v < t.P ? v : t.P_pack) * t.nsprites, (size_t)t.nsprites * 4);
  std::vector<uint8_t> buf(img_bytes + slot_bytes + pair_bytes + blob_bytes, 0);
  memcpy(buf.data(), a.images.data(), img_bytes);
  memcpy(buf.data() + img_bytes, a.slots.data(), (size_t)nimg * 2);
  memcpy(buf.data() + img_bytes + slot_bytes, a.pair_table.data(), pair_bytes);
  uint8_t* blob = buf.data() + img_bytes + slot_bytes + pair_bytes;
  build_render_blob(t, a.images.data(), a.slots.data(), a.pair_table.data(),
                    table<int32_t>(hp, "state_sprite"), splayer, vmap_p.data(), flags8.data(),
                    table<int32_t>(hp, "state_orient"), blob);
  t.vis_layers = render_visible_layers(t, blob, table<int32_t>(hp, "state_layer"));
  HIP_TRY(hipMalloc((void**)&e->d_atlas, buf.size()));
  HIP_TRY(hipMemcpy(e->d_atlas, buf.data(), buf.size(), hipMemcpyHostToDevice));
  t.atlas_compact = e->d_atlas;
  t.img_slot = reinterpret_cast<const uint16_t*>(e->d_atlas + img_bytes);
  t.pair_table = reinterpret_cast<const uint32_t*>(e->d_atlas + img_bytes + slot_bytes);
  t.render_blob = e->d_atlas + img_bytes + slot_bytes + pair_bytes;
  if (dev && dev->verbose)
    fprintf(stderr, "mp_engine: composite cache: %d images, %d table entries, probe %d\n",
            a.n_composites, a.used_slots, a.pair_probe);
  return MP_OK;
}
