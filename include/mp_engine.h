/* mp_engine.h — C ABI of the MI355X batched substrate engine (libmp_engine.so).
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json: the
 * DMLab2D/Lua step + render path of Melting Pot.  In the reference that path
 * sits behind the `dmlab2d.Environment` object built at
 * meltingpot/utils/substrates/builder.py:179-187 and driven through
 * meltingpot/utils/substrates/wrappers/base.py:38-84
 * (reset / step / observation / events / *_spec / close).  Underneath, dmlab2d
 * drives the Lua API object of lua/modules/api_factory.lua:26-115
 * (init / start / discreteActions / advance / observation).  Each entry point
 * below names the reference interface it replaces.  INTEGRATION.md shows the
 * ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - Plain C, no torch / HIP types in the signatures (a stream is a void*
 *     holding a hipStream_t; device buffers are raw device pointers).
 *   - An engine owns N independent worlds of one substrate on one GPU.  The
 *     caller owns every action / observation buffer it passes in
 *     (`tensor.data_ptr()`); the engine never frees or retains caller memory
 *     beyond what mp_bind_output documents.
 *   - Every function returns MP_OK (0) or a negative MP_ERR_* code;
 *     mp_last_error() returns a message for the calling thread.
 *   - Like a Lab2d instance an engine is not re-entrant: one host thread per
 *     engine.  All work is enqueued on the engine's stream (mp_set_stream);
 *     mp_step / mp_observe never synchronise the host.
 *   - There is NO CPU fallback: every entry point that needs a GPU fails with
 *     MP_ERR_NO_DEVICE when none is present.
 */
#ifndef MP_ENGINE_H_
#define MP_ENGINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden and linked against an export map
 * (meltingpot_amd/csrc/exports.map): what this header declares is ALL it exports. */
#pragma GCC visibility push(default)

/* 8: mp_place_output_ring and mp_alloc_output_scattered are gone (measured: they did not pay);
 * mp_box_fill — what the box's memory system gives the bound view — is new; MpInfo.plan_pace /
 * visible_layers / plan_team / plan_late_priority */
#define MP_ABI_VERSION 8

enum {
  MP_OK = 0,
  MP_ERR_INVALID = -1,    /* bad argument (the reference raises ValueError) */
  MP_ERR_PACK = -2,       /* malformed / unsupported substrate pack */
  MP_ERR_NO_DEVICE = -3,  /* no HIP device: the engine has no CPU path */
  MP_ERR_HIP = -4,        /* a HIP runtime call failed */
  MP_ERR_UNSUPPORTED = -5 /* observation not provided by this substrate */
};

/* Observation kinds (reference names: clean_up.py:813-832, specs.py:26-43,
 * avatar_library.lua:225-277,869-881, component_library.lua:786-803). */
/* The events the three levels emit on the hot path (Lua `events:add(name,
 * 'dict', key, value, ...)`), payload ints a, b; player indices are 1-based as
 * in Lua.  Rows of one step are in no particular order: sort them. */
typedef enum {
  MP_EVENT_ZAP = 1,                /* avatar_library.lua:661  a=source b=target */
  MP_EVENT_EDIBLE_CONSUMED = 2,    /* component_library.lua:996, clean_up/components.lua:402  a=player_index */
  MP_EVENT_PLAYER_CLEANED = 3,     /* clean_up/components.lua:152  a=player_index */
  MP_EVENT_CLAIMED_RESOURCE = 4,   /* territory/components.lua:133  a=player_index */
  MP_EVENT_DESTROYED_RESOURCE = 5, /* territory/components.lua:168  a=player_index */
  MP_EVENT_SANCTIONING = 6,        /* avatar_library.lua:1088  a=source b=target */
  MP_EVENT_REMOVAL_DUE_TO_SANCTIONING = 7, /* avatar_library.lua:1070  a=source b=target */
  MP_EVENT_SET_SANCTIONING_LEVEL = 8,      /* avatar_library.lua:1118  a=player_index b=level */
  MP_EVENT_AVATAR_STARTED = 9,     /* avatar_library.lua:317 ('str', 'success'), once per avatar at reset */
  MP_EVENT_COIN_CONSUMED = 10,     /* coins/components.lua:151-154  a=player_index b=player_coin_type << 1 | coin_type
                                      (indices of the level's two coin colours instead of their names) */
  MP_EVENT_INTERACTION = 11,       /* the_matrix/components.lua:790  a=row_player_idx b=col_player_idx
                                      (rewards and inventories: MP_OBS_INTERACTION_INVENTORIES, MP_OBS_REWARD) */
  MP_EVENT_COLLECTED_RESOURCE = 12,/* the_matrix/components.lua:117  a=player_index b=class
                                      (the_matrix's destroyed_resource, :178, is MP_EVENT_DESTROYED_RESOURCE
                                      with b=class) */
  MP_EVENT_MINING = 13,            /* coop_mining/components.lua:196  a=player b=ore_type (1 iron, 2 gold) */
  MP_EVENT_EXTRACTION = 14,        /* coop_mining/components.lua:210  a=player b=ore_type */
  MP_EVENT_EXTRACTION_PAIR = 15,   /* coop_mining/components.lua:220  a=player_a b=player_b << 2 | ore_type */
  MP_EVENT_RECEIVER_ACCEPTED_ITEM = 17,   /* collaborative_cooking/components.lua:325-328  a=player_index
                                             b=item (1 tomato, 2 dish, 3 soup); 'receiver' is the
                                             component's name, "Receiver" */
  MP_EVENT_ITEM_DROPPED_INTO_POT = 18,    /* :397-400  a=player_index b=item; 'pot' = "CookingPot" */
  MP_EVENT_COOKED_FOOD_COLLECTED = 19,    /* :412-415  a=player_index b=cooked_item (3 soup) */
  MP_EVENT_EATING_MUSHROOM = 20,   /* externality_mushrooms/components.lua:72-74  a=player_index b=mushroom_type
                                      (1 fullInternalityZeroExternality, 2 halfInternalityHalfExternality,
                                      3 zeroInternalityFullExternality, 4 negativeInternalityNegativeExternality) */
  MP_EVENT_GIFT = 16               /* gift_refinements/components.lua:176-182  a=gifter_index | source_type << 4
                                      b=receipient_index | received_amount << 4 (the count the recipient
                                      then holds: what Inventory:addTokens returns); the two roles are the
                                      avatars' agentRole kwargs, known to the host */
} MpEventType;
#define MP_EVENT_ROWS 128  /* 1 header row + up to 127 events per world-step; more are counted
                              in the header's `dropped` (never seen: 16 commons_harvest players
                              half of whose actions are beams peak at 16 events in a step over 400 steps,
                              tests/test_gpu_surface.py::test_event_rows_hold_a_zap_storm) */

typedef enum {
  MP_OBS_RGB = 0,            /* "N.RGB"        u8  [N][P][VH*S][VW*S][3] */
  MP_OBS_WORLD_RGB = 1,      /* "WORLD.RGB"    u8  [N][H*S][W*S][3]; with MpConfig.world_pool
                                k = 2, 4, 8: u8 [N][H*S/k][W*S/k][3], byte (y, x, c) the k x k
                                block average of the full image, rounded half up (the rule of
                                MP_OBS_RGB_POOL*), drawn straight from the cells' images in every
                                launch that draws this kind; its buffers (and mp_observe's `dst`)
                                must then be 16-byte aligned, and mp_box_fill does not take it */
  MP_OBS_REWARD = 2,         /* "N.REWARD"     f64 [N][P] */
  MP_OBS_READY_TO_SHOOT = 3, /* "N.READY_TO_SHOOT" f64 [N][P] */
  MP_OBS_AUX0 = 4,           /* substrate metric 0, f64 [N][P]
                                clean_up: NUM_OTHERS_WHO_CLEANED_THIS_STEP */
  MP_OBS_STEP_TYPE = 5,      /* dm_env.StepType i32 [N]: 0 FIRST 1 MID 2 LAST */
  MP_OBS_DISCOUNT = 6,       /* f64 [N]  (0 on FIRST/LAST, 1 on MID) */
  MP_OBS_COLLECTIVE_REWARD = 7, /* f64 [N] = sum_p REWARD
                                (collective_reward_wrapper.py:49) */
  MP_OBS_POSITION = 8,       /* "N.POSITION" i32 [N][P][2] (x, y); debug obs
                                (avatar_library.lua:806-855) */
  MP_OBS_ORIENTATION = 9,    /* "N.ORIENTATION" i32 [N][P] */
  MP_OBS_EVENTS = 10,        /* env.events() of the last step / reset, i32
                                [N][MP_EVENT_ROWS][4]: row 0 = {count, dropped,
                                0, 0}, rows 1..count = {MpEventType, a, b, 0}
                                (wrappers/base.py:72-74, `events:add` sites
                                listed at MpEventType) */
  /* Debug observations (the reference builds them when a config sets
   * _ENABLE_DEBUG_OBSERVATIONS, clean_up.py:751-784).  They are produced only
   * while a buffer is bound (mp_bind_output) or MpConfig.debug_observations is
   * set; otherwise mp_observe returns MP_ERR_UNSUPPORTED for them. */
  MP_OBS_AUX1 = 11,          /* f64 [N][P]  clean_up: PLAYER_CLEANED
                                (clean_up/components.lua:227,249) */
  MP_OBS_AUX2 = 12,          /* f64 [N][P]  clean_up: PLAYER_ATE_APPLE (:429,458) */
  MP_OBS_AUX3 = 13,          /* f64 [N][P]  clean_up: NUM_OTHERS_PLAYER_ZAPPED_THIS_STEP
                                (avatar_library.lua:672-677) */
  MP_OBS_AUX4 = 14,          /* f64 [N][P]  clean_up: NUM_OTHERS_WHO_ATE_THIS_STEP
                                (clean_up/components.lua:538) */
  MP_OBS_ZAP_MATRIX = 15,    /* f64 [N][P][P]  playerZapMatrix(zapped, zapper) of the
                                step (avatar_library.lua:657-659; GlobalMetricHolder
                                clears it every step, component_library.lua:717-722) */
  MP_OBS_LAYER = 16,         /* "N.LAYER" i32 [N][P][VH][VW][L]: the player's layer
                                view with orientation 'N' (the window is not turned
                                with the avatar, avatar_library.lua:246-257): 1 +
                                sprite index (after the viewer's spriteMap) of the
                                piece or beam in each cell-layer, 0 = nothing;
                                cells outside the map hold OutOfBounds in every
                                layer.  Bound (mp_bind_output or
                                mp_bind_output_ring), it is written by the launch
                                that resets or steps the worlds, from each record
                                while it is in LDS: no launch of its own.
                                mp_observe reads it from the records in HBM.
                                mp_place_output does not take this kind. */
  MP_OBS_INVENTORY = 17,     /* "N.INVENTORY" f64 [N][P][R]: TheMatrix.playerResources
                                (the_matrix/components.lua:942-963); gift_refinements:
                                Inventory.inventory (gift_refinements/components.lua:239-353);
                                R = MpInfo.num_resources */
  MP_OBS_INTERACTION_INVENTORIES = 18, /* "N.INTERACTION_INVENTORIES" f64 [N][P][2][R]:
                                (own, partner's) inventory of the interaction resolved
                                this step, -1 otherwise (the_matrix/components.lua:761-783,
                                899-903) */
  MP_OBS_MATRIX_CUMULANTS = 19, /* *_in_the_matrix debug observations (the_matrix.py:22-60;
                                GameInteractionZapper's binary cumulants, components.lua:
                                808-853), f64 [N][P][1 + 3 R], 0 / 1, columns
                                  0           "N.INTERACTED_THIS_STEP"
                                  1 + 3 k     "N.COLLECTED_RESOURCE_<k+1>"
                                  2 + 3 k     "N.DESTROYED_RESOURCE_<k+1>"
                                  3 + 3 k     "N.ARGMAX_INTERACTION_INVENTORY_WAS_<k+1>"
                                produced while bound or with MpConfig.debug_observations */
  MP_OBS_INTERACTION_REWARDS = 20, /* *_in_the_matrix: f64 [N][P][2], (row_reward,
                                col_reward) of the latest interaction player p took part
                                in — with MP_OBS_INTERACTION_INVENTORIES the rest of the
                                reference's 'interaction' event payload (the_matrix/
                                components.lua:789-797: row_reward, col_reward,
                                row_inventory, col_inventory), exact f64: an event row
                                {MP_EVENT_INTERACTION, row, col} of a step says which
                                players' entries are this step's */
  /* Pooled per-agent RGB: "N.RGB" cut down by an area filter, u8 [N][P][VH*S/k][VW*S/k][3] for
   * k = 2, 4, 8 — byte (y, x, c) is the k x k block average of the full image I of MP_OBS_RGB,
   * rounded half up: (sum_{i,j<k} I[y*k+i][x*k+j][c] + k*k/2) / (k*k).  Everything the full image
   * shows is pooled as it is (OutOfBounds, the black view of a dead avatar, beams, facings,
   * per-viewer sprite maps).  The frame launch draws it straight from the cells' images: the full
   * image is never written.  Bound (mp_bind_output / _ring / mp_place_output) it is drawn by the
   * launch that steps the worlds, alone or together with MP_OBS_WORLD_RGB; at most ONE per-agent
   * view can be bound at a time — binding a pooled kind while MP_OBS_RGB or another pooled kind is
   * bound (or MP_OBS_RGB while a pooled kind is) is MP_ERR_INVALID.  Buffers of these kinds (and
   * mp_observe's `dst`) must be 16-byte aligned.  mp_box_fill does not take them. */
  MP_OBS_RGB_POOL2 = 21,     /* u8 [N][P][VH*S/2][VW*S/2][3]  (clean_up: 44 x 44) */
  MP_OBS_RGB_POOL4 = 22,     /* u8 [N][P][VH*S/4][VW*S/4][3]  (22 x 22) */
  MP_OBS_RGB_POOL8 = 23,     /* u8 [N][P][VH*S/8][VW*S/8][3]  (11 x 11: one pixel a cell) */
  MP_OBS_KINDS = 24
} MpObsKind;

typedef struct MpEngine MpEngine;

/* Test / development overrides of the launch plan (MpConfig.dev; NULL in every
 * product path: meltingpot_amd.substrate / lab2d_env never set it).  They change
 * how the work is laid out over workgroups and LDS, never a result: the tests
 * use them to drive the frame kernel through its corner geometries (tiny and
 * ragged batches, many batches per workgroup, the direct-store path) and
 * tools/ to sweep the plan.  The library reads NO environment variable.
 * 0 (or -1 for max_composites) = the engine's own choice. */
typedef struct {
  uint32_t struct_size;     /* = sizeof(MpDevOptions) */
  int32_t batch_worlds;     /* worlds per LDS batch of the frame kernel */
  int32_t waves;            /* waves per workgroup */
  int32_t feeders;          /* feeder waves among them */
  int32_t max_groups;       /* cap on workgroups (more batches per workgroup) */
  int32_t scratch_cells;    /* composited cells a wave stages per pass */
  int32_t no_composite_cache; /* 1: every overlay is composited on the fly */
  int32_t max_composites;   /* cap on composite-cache images, -1 = none */
  int32_t verbose;          /* 1: print the plans to stderr */
  int32_t late_feeder_prio; /* 1 + wave priority (0..3) of the feeders after their first batch */
  int32_t ring_batches;     /* batches resident in LDS (the ring's depth), >= 2 */
  int32_t static_pct;       /* 1..100: share of a workgroup's even split it owns as a
                               contiguous range; the rest of the launch's batches are
                               claimed from a device-wide pool (100: no pool) */
  int32_t world_waves;      /* two views in one launch: renderer waves that draw WORLD.RGB */
  int32_t store_sc1;        /* 1: the pixels leave as sc1 stores */
  int32_t head;             /* 1 + FramePlan::head (how a stepping launch starts: 2 = the DMA
                               head, 1 = the older road) */
  int32_t no_next_orders;   /* 1: a step does not leave the NEXT step's shuffled visiting orders
                               in the world's record (it draws them at its own start instead) */
  int32_t record_pad;       /* unused 64-byte blocks behind every world's record (another stride) */
  int32_t pace;             /* 1 + FramePlan::pace: what a renderer wave sleeps between two passes,
                               in units of 512 cycles (mp_tune's throttle for a view the memory side
                               serves unevenly) */
  int32_t team;             /* 1: with single-world batches (batch_worlds = 1, nothing pooled), the workgroups
                               of an XCD share one contiguous range of worlds and deal it among themselves */
  int32_t generic_kernel;   /* 1: the generic frame kernels even for a committed pack that has kernels with its
                               constants compiled in (MpKernelVariant).  Appended: mp_create also takes
                               struct_size = offsetof(MpDevOptions, generic_kernel), which reads as 0 */
} MpDevOptions;

typedef struct {
  uint32_t struct_size;  /* = sizeof(MpConfig) */
  int32_t device;        /* HIP device ordinal */
  int32_t num_worlds;    /* N worlds owned by this engine */
  int32_t auto_reset;    /* 1: a world whose episode ended restarts on the next
                            mp_step (dm_env: step after LAST == reset) */
  uint64_t world_offset; /* global index of this engine's world 0; world w is
                            seeded from (world_offset + w) so results do not
                            depend on how worlds are sharded over GPUs */
  uint64_t base_seed;    /* 0: seed_w = 0x9E3779B97F4A7C15 * (w+1) (BASELINE.md
                            §4); else seed_w = base_seed + w (builder.py:174-181
                            with one env_seed per world) */
  void* stream;          /* hipStream_t, or NULL for the legacy default stream */
  int32_t num_players;   /* 0: the pack's default (MPK_HDR_DEFAULT_P, else all the
                            avatars it was lowered for); else 1 <= num_players <=
                            the pack's count: the first num_players avatars play
                            (the reference: num_players = len(roles),
                            configs/substrates/clean_up.py:847) */
  int32_t debug_observations; /* 1: the engine keeps buffers for the debug
                            observation kinds (MP_OBS_AUX1..) and fills them every step */
  int32_t unfused;       /* launches of a step with a bound RGB view — same results
                            either way.  2: ONE launch (rules and pixels fused);
                            1: one launch for the rules and one per view;
                            0: the engine's choice (the fused launch; DESIGN.md
                            section 3).  MpInfo.fused reports the launch form */
  int32_t literal_base_seed; /* 1: seed_w = base_seed + w even for base_seed 0 (an
                            env_seed of 0 is a seed like any other, builder.py:174-181) */
  const MpDevOptions* dev; /* NULL (product); tests / tools: see MpDevOptions */
  const int32_t* roles;  /* NULL: the assignment the pack was lowered for (the config's
                            default_player_roles).  Else HOST int32[num_players]:
                            the role of each player as an index into the pack's
                            "role_names" (sorted names, NUL-separated) — for
                            substrates whose config builds per-player constants from
                            the roles (bach_or_stravinsky_in_the_matrix__*: row /
                            column player and avatar colour, configs/substrates/
                            bach_or_stravinsky_in_the_matrix__repeated.py:473-497);
                            MP_ERR_INVALID for a pack without per-role tables */
  int32_t world_pool;    /* 0 or 1: MP_OBS_WORLD_RGB is the full image; 2, 4, 8: it is that image
                            pooled by this factor, for this engine everywhere the kind is used
                            (mp_obs_bytes, mp_bind_output / _ring, mp_observe, mp_tune,
                            mp_place_output); other values are MP_ERR_INVALID.  Appended to the
                            ABI-8 layout: mp_create also takes struct_size =
                            offsetof(MpConfig, world_pool) (72 bytes), which reads as 1 */
} MpConfig;

typedef struct {
  int32_t abi_version;
  int32_t substrate;     /* MPK_SUBSTRATE_* */
  int32_t num_worlds, num_players, num_actions;
  int32_t map_h, map_w, num_layers, sprite_size;
  int32_t view_h, view_w; /* egocentric window in cells */
  int32_t max_frames;
  int32_t world_state_bytes; /* bytes of HBM-resident state per world */
  int32_t fused;         /* 1: a step with a bound view is one launch (MpConfig.unfused) */
  int32_t num_resources; /* *_in_the_matrix: resource classes R; gift_refinements: token types
                            (0 elsewhere) */
  int32_t num_action_fields; /* A = len(actionOrder): the raw fields of mp_step_fields */
  /* the launch plan of a step with the pixel views bound right now (mp_tune may have
   * replaced the stock one): worlds per LDS batch, batches resident, batches a
   * workgroup owns, batches pooled behind the claim counter, workgroups */
  int32_t plan_batch_worlds, plan_ring_batches, plan_owned_batches, plan_pooled_batches,
          plan_groups, plan_store_sc1 /* 1: sc1 pixel stores */;
  int32_t plan_feeders, plan_waves; /* (ABI 5) feeder waves among the waves of a workgroup */
  /* (ABI 6) the rollout ring (mp_bind_output_ring): its slots (0: none) and the slot the
   * NEXT mp_reset / mp_step writes; the last one written is (ring_next + ring_slots - 1)
   * % ring_slots once anything has been submitted */
  int32_t ring_slots, ring_next;
  /* (ABI 8) what a renderer wave sleeps between two passes under the plan above, in units of 512
   * cycles (mp_tune: 0 on a view the memory side takes evenly), and the render planes that can show
   * anything (bit l: some state of layer l has a sprite with a visible pixel — the only planes the
   * renderers read) */
  int32_t plan_pace, visible_layers;
  /* (ABI 8) 1: the plan deals its single-world batches to XCD teams (each XCD writes one compact
   * front); the feeders' wave priority (0 - 3) after their first world */
  int32_t plan_team, plan_late_priority;
  /* (ABI 6) virtual address space this PROCESS has retired with mapped views
   * (mp_free_output / mp_place_output keep a released view's range reserved), and the
   * bound beyond which mp_alloc_output / mp_place_output refuse to map more */
  int64_t retired_va_bytes, retired_va_limit;
} MpInfo;

/* ABI version of the loaded library. */
int mp_abi_version(void);

/* Message for the last error on this thread ("" if none). */
const char* mp_last_error(void);

/* Construction.  Replaces dmlab2d.Lab2d(root, settings) +
 * dmlab2d.Environment(env, names, seed) (builder.py:182-187) and Lua api:init
 * (api_factory.lua:53-67).  `pack` is an MPK1 blob (include/mp_pack.h): the
 * lowered form of the settings dict the reference passes to builder.builder().
 * A malformed pack is refused with MP_ERR_PACK before any device call.
 * Geometry limits, also checked before any device call: H * W <= 4096 cells and a
 * view window of at most 64 x 64 cells (MP_ERR_PACK); a map at most 64 cells wide,
 * since a row of WORLD.RGB cells is drawn in one 64-lane wave pass, and at most 255
 * cells tall, since avatar coordinates are kept in 8-bit fields (MP_ERR_UNSUPPORTED).
 * A TORUS map must be at least as wide and as tall as the view's reach.
 * All worlds start un-reset; call mp_reset before the first mp_step. */
int mp_create(const void* pack, uint64_t pack_len, const MpConfig* cfg,
              MpEngine** out);

/* dmlab2d.Environment.close() (wrappers/base.py:76-78). */
void mp_destroy(MpEngine* eng);

int mp_info(const MpEngine* eng, MpInfo* out);

/* Which frame kernels step and draw an engine's worlds (same results either way).  The packs
 * committed with the package whose scalars — map, view and record geometry, layer and state ids,
 * beam shapes, cooldowns, thresholds — are compiled into kernels of their own (clean_up with its
 * default player count) run those; every other pack, and such a pack edited in any byte, created
 * with another player count or with MpDevOptions.record_pad / generic_kernel, runs the generic
 * kernels, which take the same values as arguments.
 *
 * The question travels as a request struct through mp_snapshot, like MpWorldStates: call
 * mp_snapshot(eng, &req, sizeof(MpKernelVariant)) with struct_size = sizeof(MpKernelVariant);
 * include/mp_kernel_variant.h wraps it as an inline C function.  MP_OK and `variant` set, or a
 * negative MP_ERR_*.
 *   eng != NULL: what `eng` runs (the other members are ignored).
 *   eng == NULL: what mp_create on `pack` / `pack_len` / `cfg` WOULD select, decided on the host
 *     alone (no device is touched; errors as mp_create's for a bad pack or config).  With `fields`
 *     != NULL also writes, NUL-terminated, the pack's value of every scalar a stock kernel folds,
 *     one "<group> <member> <C literal>" line each plus "hash <FNV-1a of the pack>" — what
 *     tools/make_stock_header.py turns into csrc/stock_<level>.h; MP_ERR_UNSUPPORTED for a level
 *     without stock kernels, MP_ERR_INVALID if `fields_cap` bytes do not hold it. */
enum { MP_KERNEL_GENERIC = 0, MP_KERNEL_STOCK = 1 };
typedef struct {
  uint32_t struct_size;   /* = sizeof(MpKernelVariant) */
  int32_t variant;        /* out: MP_KERNEL_* */
  const void* pack;       /* the host-only question (eng == NULL) */
  uint64_t pack_len;
  const MpConfig* cfg;
  char* fields;           /* NULL, or where the folded fields' text goes */
  uint64_t fields_cap;
} MpKernelVariant;

/* Work submitted after this call is enqueued on `stream` (a hipStream_t); it is
 * ordered after everything the engine has enqueued on its previous stream. */
int mp_set_stream(MpEngine* eng, void* stream);

/* Register a caller-owned DEVICE buffer for an observation kind (NULL
 * unbinds).  While bound, every mp_reset / mp_step refreshes the buffer as
 * part of the same submission (RGB kinds are rendered straight into it; the
 * scalar kinds are written by the step kernel).  The buffer must stay valid
 * until unbound or mp_destroy.  Replaces the per-name api:observation(idx)
 * reads after each step (api_factory.lua:73-75). */
int mp_bind_output(MpEngine* eng, MpObsKind kind, void* device_ptr);
/* (MP_ERR_INVALID for a pointer the device cannot write — plain host memory, memory of
 * another device: a launch writing through it would fault the GPU in the middle of a step) */

/* A rollout ring: observations a learner keeps without copying them.  The reference
 * hands back FRESH arrays every step (wrappers/multiplayer_wrapper.py:108-118,
 * utils/substrates/substrate.py:74-81) and a rollout simply stores them; a bound
 * buffer (mp_bind_output) is overwritten in place.  With a ring bound for `kind`,
 * submission number t since the ring was bound (every mp_reset and every mp_step* is one
 * submission; binding the first kind of a ring restarts the count) writes the kind
 * into slot t % slots: DEVICE memory `base` + slot * slot_stride_bytes,
 * slot_stride_bytes >= mp_obs_bytes(kind) and a multiple of 256.  All kinds bound as
 * rings share one slot count and one position, so slot s of every kind holds the same
 * step; kinds bound with mp_bind_output keep being overwritten in place.  Rebinding is
 * a pointer store per kind; no call synchronises or re-tunes between steps: mp_tune
 * (once, after binding) times the candidate launch plans on EVERY slot of the bound
 * pixel views and remembers a plan per slot.  mp_observe of a ring-bound scalar kind
 * reads the slot written last.  base == NULL unbinds the kind (like mp_bind_output
 * with NULL; so does mp_bind_output on the kind).  MpInfo.ring_slots / ring_next
 * report the position.  MP_OBS_LAYER may be a ring kind like any other; mp_tune's
 * probe launches do not write it, so every LAYER slot keeps the step that wrote it. */
int mp_bind_output_ring(MpEngine* eng, MpObsKind kind, void* base,
                        uint64_t slot_stride_bytes, int32_t slots);

/* Episode start for the worlds selected by `mask` (HOST u8[N], NULL = all).
 * `seeds` (HOST u64[N], NULL = keep) overrides the per-world seed and restarts
 * the world's episode count.  Episode e of a world draws from the counter-based
 * generator keyed by the world's seed with e in the counter:
 * like the reference's rebuild-with-seed+1 convention (builder.py:177-181,
 * reset_wrapper.py:37-45) every episode has its own stream, and — unlike
 * seed + e — worlds with adjacent seeds never share one.  Replaces
 * api:start(episode, seed) (api_factory.lua:85-102). */
int mp_reset(MpEngine* eng, const uint64_t* seeds, const uint8_t* mask);

/* One environment step for all N worlds.  `actions` is a DEVICE int32[N][P]
 * of discrete action ids into the substrate's ACTION_SET (clean_up.py:473-483;
 * the table lookup of discrete_action_wrapper.py:97-109 happens on device).
 * Out-of-range ids are treated as NOOP and counted in mp_counters[MP_CTR_BAD_ACTIONS].
 * Replaces api:discreteActions + api:advance (api_factory.lua:81,104-111). */
int mp_step(MpEngine* eng, const int32_t* actions_device);

/* Same with a HOST int32[N][P]; validates ids (MP_ERR_INVALID, like
 * discrete_action_wrapper.py:28-49).  The array is copied into a ring of
 * pinned, device-mapped buffers that the step kernel reads directly, so the
 * caller may reuse `actions_host` as soon as the call returns and nothing
 * synchronises the stream (the 4th later call waits for this one's step). */
int mp_step_host(MpEngine* eng, const int32_t* actions_host);

/* The raw action surface of dmlab2d.Environment.step: one int per field of the
 * avatar's actionOrder ("<player>.move", ".turn", ".fireZap" ...;
 * avatar_library.lua:205-223, wrappers/base.py:38-44), DEVICE int32 [N][P][A],
 * A = MpInfo.num_action_fields, any combination inside the actionSpec ranges of
 * the pack's "action_spec" table (move + turn + zap in one step: a scenario's or
 * a human player's action, human_players/level_playing_utils.py:283,333-334;
 * or the rows of a custom `action_table`, discrete_action_wrapper.py:77-109).
 * An avatar with a field outside its range does NOOP and is counted in
 * MP_CTR_BAD_ACTIONS.  mp_step(ids) == mp_step_fields(ACTION_SET[ids]). */
int mp_step_fields(MpEngine* eng, const int32_t* fields_device);

/* Same with a HOST int32 [N][P][A]; validates the ranges (MP_ERR_INVALID). */
int mp_step_fields_host(MpEngine* eng, const int32_t* fields_host);

/* Write observation `kind` for all worlds into the caller-owned DEVICE buffer
 * `dst` (layouts in MpObsKind).  Replaces api:observation(idx). */
int mp_observe(MpEngine* eng, MpObsKind kind, void* dst_device);

/* Bytes of observation `kind` for all N worlds (0 if unsupported). */
uint64_t mp_obs_bytes(const MpEngine* eng, MpObsKind kind);

/* Canonical state dump to HOST buffers (synchronises): the layout the parity
 * tests compare bit-for-bit with the oracle's:
 *   grid u8 [N][L][H][W]   state id of the piece (or beam pseudo-state)
 *   avat i32[N][P][8]      x, y, orient, alive, zap_timer, aux_timer,
 *                          frames_in_state, 0
 *   glob i32[N][8]         step, done, frame, aux_count, episode, 0, 0, 0 */
int mp_dump(MpEngine* eng, uint8_t* grid, int32_t* avat, int32_t* glob);

/* Checkpoint / restore of the raw HBM state of all worlds (synchronises).
 * `bytes` must equal mp_snapshot_bytes().  (The reference has no equivalent:
 * SURVEY.md §5 "checkpoint / resume".) */
uint64_t mp_snapshot_bytes(const MpEngine* eng);
int mp_snapshot(MpEngine* eng, void* host_buf, uint64_t bytes);
int mp_restore(MpEngine* eng, const void* host_buf, uint64_t bytes);

/* World states as device data: save chosen worlds' records into rows of a caller-owned device
 * buffer, and start any worlds from such rows — forks, rewinds, restarts from states of
 * interest, the same world replayed many times.  A row is a world's whole record
 * (MpInfo.world_state_bytes = S bytes): its grid, avatars, timers, seed, episode and step.  Every
 * random draw is keyed by the record's own seed and counted by its episode and step, so a loaded
 * world continues exactly as the world it was saved from would under the same actions —
 * auto-resets included (episode e + 1 of the source's seed).
 *
 * The library's exported entry points do not grow: these operations go through the two state
 * entry points above, as a request.  A call of mp_snapshot or mp_restore whose `bytes` is
 * sizeof(MpWorldStates) (no engine's snapshot is that small) takes `host_buf` as a HOST
 * MpWorldStates with struct_size = sizeof(MpWorldStates); every other call is what it always
 * was.  A request is enqueued on the engine's stream and does not synchronise.
 * include/mp_world_states.h wraps the three operations as inline C functions
 * (state fingerprint, save worlds, load worlds).
 *
 * MP_STATES_FINGERPRINT (mp_snapshot): `fingerprint` := a 64-bit hash of everything that decides a
 * record's layout and meaning (the pack with its roles applied, the player count, the record's
 * geometry with MpDevOptions.record_pad, the library's record layout).  Rows load only into an
 * engine with the same fingerprint — any N, any world_offset, another instance.
 *
 * MP_STATES_SAVE (mp_snapshot): row i of `bank` (device uint8 [count][S], bank_bytes >= count * S)
 * = the record of world worlds[i] (device int32 [count]; NULL = every world, count = N);
 * `fingerprint` := the engine's.  MP_ERR_INVALID, before any launch: NULL / non-positive
 * arguments, bank_bytes < count * S, a buffer that is not device memory of the engine's device
 * or whose [ptr, ptr + count * S) is not inside one allocation, an engine that has never been
 * reset (mp_reset, mp_restore or a load).  A world index outside [0, N) is never read: its row is
 * left as it was and the next synchronising call returns MP_ERR_INVALID.
 *
 * MP_STATES_LOAD (mp_restore): ONE launch shaped like a masked mp_reset.  src (device int32 [N]):
 * src[w] = r >= 0 starts world w from row r of `bank` (device uint8 [bank_rows][S]); -1 leaves
 * world w as a masked reset leaves a world outside its mask.  Several worlds may take one row.
 * `fingerprint`: the rows' (MP_STATES_SAVE's).  Every bound view (RGB, RGB_POOL*, WORLD.RGB,
 * LAYER) is drawn by the launch, and it writes the rollout ring's next slot like any
 * submission.  A loaded world keeps its OWN cumulative counters (WorldTail::ctr and reward_fx,
 * which only feed mp_counters): mp_counters goes on counting the work this engine did.  What
 * the launch writes for a loaded world:
 *   (A) functions of the record, equal to what the source's last launch wrote:
 *       MP_OBS_RGB, MP_OBS_RGB_POOL2/4/8, MP_OBS_WORLD_RGB, MP_OBS_LAYER, MP_OBS_READY_TO_SHOOT,
 *       MP_OBS_POSITION, MP_OBS_ORIENTATION, MP_OBS_INVENTORY;
 *   (B) transition kinds, as a reset writes them (STEP_TYPE = FIRST): MP_OBS_REWARD,
 *       MP_OBS_COLLECTIVE_REWARD, MP_OBS_STEP_TYPE, MP_OBS_DISCOUNT, MP_OBS_EVENTS, MP_OBS_AUX0,
 *       MP_OBS_AUX1..4, MP_OBS_ZAP_MATRIX, MP_OBS_INTERACTION_INVENTORIES,
 *       MP_OBS_MATRIX_CUMULANTS, MP_OBS_INTERACTION_REWARDS (which a reset leaves as it was).
 *   A row saved from a finished world loads finished: STEP_TYPE LAST, discount 0, reward 0,
 *   no events (what a frozen world reports); its next mp_step auto-resets it or leaves it
 *   frozen.  MP_ERR_INVALID, before any launch: NULL arguments, bank_rows <= 0, a fingerprint
 *   that is not this engine's, a bank or src that is not device memory of the engine's device
 *   or that does not lie inside one allocation.  An src[w] that is neither -1 nor a row is never
 *   read: world w is left as it was and the next synchronising call returns MP_ERR_INVALID.
 *   (The reference has no equivalent: SURVEY.md §5 "checkpoint / resume".) */
enum { MP_STATES_FINGERPRINT = 1, MP_STATES_SAVE = 2, MP_STATES_LOAD = 3 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpWorldStates) */
  int32_t op;              /* MP_STATES_* */
  uint64_t fingerprint;    /* LOAD: the rows' (in); FINGERPRINT, SAVE: the engine's (out) */
  const int32_t* worlds;   /* SAVE: device int32 [count], NULL = every world */
  const int32_t* src;      /* LOAD: device int32 [N] */
  void* bank;              /* SAVE: written; LOAD: read — device uint8 [rows][S] */
  uint64_t bank_bytes;     /* SAVE: bytes of `bank` */
  int32_t count;           /* SAVE: rows to write */
  int32_t bank_rows;       /* LOAD: rows of `bank` */
} MpWorldStates;

/* Observations of bank rows: the views of saved world states, drawn without loading them into a
 * world.  For a replay buffer that keeps states and draws the minibatch it samples, a planner that
 * wants the pixels of a few leaves, a video of one world of a rollout kept as states.  Like the
 * requests above it rides mp_snapshot and is recognised by its size: `bytes` =
 * sizeof(MpStatesObserve), `host_buf` a HOST MpStatesObserve with struct_size set to it.
 * include/mp_states_observe.h wraps it as an inline C function.
 *
 * `dst` is laid out as the kind's [N]... layout (MpObsKind) with `count` in place of N.  Element i
 * is a function of row rows[i] of `bank` (rows == NULL: row i) alone:
 *   the pixel kinds (MP_OBS_RGB, MP_OBS_RGB_POOL2/4/8, MP_OBS_WORLD_RGB at the engine's
 *   MpConfig.world_pool) and MP_OBS_LAYER: byte for byte what mp_observe(kind) writes for a world
 *   whose record is that row;
 *   MP_OBS_READY_TO_SHOOT, MP_OBS_POSITION, MP_OBS_ORIENTATION, MP_OBS_INVENTORY: what
 *   MP_STATES_LOAD writes for a world loaded from that row.
 * These are the kinds of MP_STATES_LOAD's group of record functions; a transition kind (its other
 * group) is not a function of the record and is refused.  Rows saved from finished episodes and
 * rows with dead avatars are drawn like any other; `count` may be smaller or larger than the
 * engine's N and rows may repeat.
 *
 * The request is enqueued on the engine's stream and does not synchronise.  It writes nothing of
 * the engine's: not its records or counters, not an in-place or bound output, not a ring slot or
 * the ring's position, not the kept plans, and mp_tune still regards an engine nothing else has
 * been done with as such.  It is legal on an engine that has never been reset: the rows may come
 * from another engine with the same fingerprint.  With `rows` the pixel kinds and LAYER copy the
 * rows next to each other into a scratch the engine owns and draw from it.  The scratch grows on
 * demand and lives until mp_destroy; a request that has to grow it (the first one with `rows`,
 * and every one that needs more than any before it) frees and allocates device memory, which
 * waits for the device — every other request only enqueues.
 *
 * Refused before any launch, the engine left as it was — MP_ERR_INVALID: NULL bank or dst;
 * count < 1 or bank_rows < 1; rows == NULL with count > bank_rows; a bank that is not 16-byte
 * aligned; a wrong struct_size; a fingerprint that is not the engine's;
 * dst_bytes < count x the kind's bytes per world; a pooled view (MP_OBS_RGB_POOL*, a pooled
 * MP_OBS_WORLD_RGB) whose dst is not 16-byte aligned, any other dst not aligned to the kind's
 * element size; a bank, rows or dst that is not device memory of the engine's device or does not
 * lie inside one allocation; a kind outside [0, MP_OBS_KINDS); a transition kind.
 * MP_ERR_UNSUPPORTED: a kind the level does not have (mp_obs_bytes == 0); a pixel kind whose draw
 * plan for `count` worlds does not fit the LDS beside the engine's composite cache.
 * A rows[i] outside [0, bank_rows) is never read: element i of dst is left as it was and the next
 * synchronising call returns MP_ERR_INVALID.  Two limits of that: the pixel kinds and LAYER, which
 * draw every element of dst from the gathered rows, keep eight such elements of a request as they
 * were (any eight; a further one holds what an empty record shows); and of several such indices
 * one is reported, with a position and a value that may belong to two different ones. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpStatesObserve) */
  int32_t kind;            /* MpObsKind */
  uint64_t fingerprint;    /* in: the rows' (MP_STATES_SAVE's) */
  const void* bank;        /* device uint8 [bank_rows][S] */
  const int32_t* rows;     /* device int32 [count], NULL = rows 0 .. count - 1 */
  void* dst;               /* device: the kind's layout with count in place of N */
  uint64_t dst_bytes;
  int32_t bank_rows;
  int32_t count;
  uint64_t reserved;       /* 0 */
} MpStatesObserve;

/* Sampled views of bank rows: ONE player's view of each sampled row — the (step, world, player)
 * triples a multi-agent learner draws from a replay buffer that keeps states.  Where
 * MpStatesObserve draws every player of a row, this request writes the sampled views alone: P x
 * fewer bytes, and no [count][P]... intermediate to index afterwards.  It rides mp_snapshot and is
 * recognised by its size: `bytes` = sizeof(MpStatesView), `host_buf` a HOST MpStatesView with
 * struct_size set to it.  include/mp_states_view.h wraps it as an inline C function.
 *
 * Element i of `dst` is the view of player players[i] of row rows[i] of `bank` (rows == NULL: row
 * i).  `dst` has the kind's per-player layout with the [N][P] axes replaced by [count]:
 *   MP_OBS_RGB             u8  [count][VH*S][VW*S][3]
 *   MP_OBS_RGB_POOLk       u8  [count][VH*S/k][VW*S/k][3]
 *   MP_OBS_LAYER           i32 [count][VH][VW][L]
 *   MP_OBS_READY_TO_SHOOT  f64 [count]
 *   MP_OBS_POSITION        i32 [count][2]
 *   MP_OBS_ORIENTATION     i32 [count]
 *   MP_OBS_INVENTORY       f64 [count][R]
 * and element i is, byte for byte, element [i][players[i]] of what an MpStatesObserve request
 * with the same `rows` writes.  Rows may repeat, (row, player) pairs may repeat, and `count` has no
 * relation to the engine's N.  `dst` needs the alignment of the kind's element size only: 1 for
 * every pixel kind, the pooled ones included (a pooled view of clean_up is 363 bytes: views start
 * on any byte), 4 for LAYER, POSITION and ORIENTATION, 8 for the f64 kinds.
 *
 * The request is enqueued on the engine's stream and does not synchronise; no path of it
 * allocates or frees device memory.  Every record is read from the bank row where it lies.  It
 * writes nothing of the engine's: not its records or counters, not an in-place or bound output, not
 * a ring slot or the ring's position, not the kept plans, not the scratch or the stash of
 * MpStatesObserve, and mp_tune still regards an engine nothing else has been done with as such.
 * It is legal on an engine that has never been reset.
 *
 * Refused before any launch, the engine left as it was — MP_ERR_INVALID: everything
 * MpStatesObserve refuses (NULL bank or dst; count < 1 or bank_rows < 1; rows == NULL with count >
 * bank_rows; a bank that is not 16-byte aligned; a wrong struct_size; a fingerprint that is not
 * the engine's; dst_bytes < count x the kind's bytes per view; a dst not aligned to the kind's
 * element size; a bank, rows, players or dst that is not device memory of the engine's device or
 * does not lie inside one allocation; a kind outside [0, MP_OBS_KINDS); a transition kind); NULL
 * players; MP_OBS_WORLD_RGB, which is not a per-player kind; nonzero reserved words.
 * MP_ERR_UNSUPPORTED: a kind the level does not have (mp_obs_bytes == 0); a record and a row of
 * view cells that do not fit the LDS beside the renderer's tables.
 * A rows[i] outside [0, bank_rows) or a players[i] outside [0, P) is never used as an index:
 * element i of dst is left as it was — every such element of a request, however many — and the
 * next synchronising call returns MP_ERR_INVALID once, naming MpStatesView, rows[i] or players[i]
 * and the value (of several such indices one is reported); the engine stays usable. */
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpStatesView) */
  int32_t kind;            /* MpObsKind: a per-player kind that is a function of the record */
  uint64_t fingerprint;    /* in: the rows' (MP_STATES_SAVE's) */
  const void* bank;        /* device uint8 [bank_rows][S] */
  const int32_t* rows;     /* device int32 [count], NULL = rows 0 .. count - 1 */
  const int32_t* players;  /* device int32 [count] */
  void* dst;               /* device: the kind's per-player layout, [count] elements */
  uint64_t dst_bytes;
  int32_t bank_rows;
  int32_t count;
  uint64_t reserved[2];    /* 0 */
} MpStatesView;

/* EGO_LAYER: the layer view in the avatar's OWN frame, as "RGB" shows it.  MP_OBS_LAYER is the
 * reference's "N.LAYER" (avatar_library.lua:247-257, orientation = 'N'): its window is not turned
 * with the avatar, so an avatar that faces east gets the cells to its north while its "RGB" shows
 * the cells to its east.  EGO_LAYER is the layer observation the reference renders "RGB" from
 * (avatar_library.lua:264-275, no orientation = 'N') and throws away: cell (i, j) of it names
 * the sprites under cell (i, j) of "RGB".  It is no MpObsKind: it rides mp_snapshot as a request of
 * its own and is recognised by its size: `bytes` = sizeof(MpEgoLayer), `host_buf` a HOST
 * MpEgoLayer with struct_size set to it.  include/mp_ego_layer.h wraps it as inline C functions.
 *
 * Definition.  For a record (a bank row or a live world) and a viewer p, EGO_LAYER is int32
 * [VH][VW][L], MP_OBS_LAYER's shape (VH = forward + backward + 1, VW = left + right + 1).  With
 * vo = orientation[p], dx = vx - left, dy = vy - forward, the world offset (ax, ay) of window cell
 * (vx, vy) follows the renderer's table: vo 0: (dx, dy); 1: (-dy, dx); 2: (-dx, -dy); 3: (dy, -dx).
 * The world cell is (avatar_x[p] + ax, avatar_y[p] + ay); TORUS wraps both coordinates, otherwise
 * a cell off the map is out of bounds.  The value at layer l is the one N.LAYER gives for that
 * world cell: 1 + the viewer's remapped sprite of the state in plane l (0 for nothing), the
 * OutOfBounds id on every layer of a cell off the map, and on every layer of every cell when the
 * viewer is dead or off the grid (A6).  For a viewer that faces north EGO_LAYER equals
 * MP_OBS_LAYER element for element.
 * The ids are N.LAYER's (A17): the registration index behind the viewer's sprite map, with NO
 * facing encoded.  The window is turned, the ids are not: an avatar q's facing in viewer p's frame
 * is (ORIENTATION[q] - ORIENTATION[p]) & 3, and the pseudo-states of oriented beams and of kitchen
 * inventories keep their absolute ids.
 *
 * MP_EGO_DRAW: element i of `dst` is the view of row rows[i] (NULL: row i) of `bank` (device
 *   uint8 [bank_rows][S], 16-byte aligned); a NULL bank means the engine's own worlds as they are
 *   now (rows[] are then world indices, bank_rows is ignored, the engine must have been reset).
 *   players == NULL: dst is int32 [count][P][VH][VW][L], every viewer of each row; otherwise
 *   players is device int32 [count] and dst is [count][VH][VW][L], the view of player players[i]
 *   of row rows[i].  Rows and (row, player) pairs may repeat and `count` has no relation to the
 *   engine's N.  `dst` is 4-byte aligned.  Stream-ordered, no synchronisation, no allocation;
 *   nothing of the engine's is written.  `fingerprint`: the rows' (with a NULL bank: the engine's).
 *   A rows[i] that is no row (no world) or a players[i] outside [0, P) is never used as an index:
 *   element i of dst is left as it was — every such element — and the next synchronising call
 *   returns MP_ERR_INVALID once, naming MpEgoLayer, rows[i] or players[i] and the value (of several
 *   such indices one is reported); the engine stays usable.
 * MP_EGO_REGISTER: `dst` names a device int32 [N][P][VH][VW][L] (slots == 0), or a ring: slot s
 *   is at dst + s * slot_stride bytes, and `slots` must equal the engine's ring slots
 *   (mp_bind_output_ring).  While registered, every submission (reset, step, step_fields, every
 *   K-step request, a load) is followed on the same stream by ONE launch that redraws all N
 *   worlds from their records into dst, or into the ring slot that submission wrote.  The value
 *   is a function of the record, so a masked, stopped or listed call needs no special case: a
 *   world that did not run is redrawn to the bytes it had.  dst_bytes covers the tensor (the last
 *   slot's end for a ring); the pointer is validated like a bound buffer.  mp_tune's probe
 *   submissions do not write it.  A NULL dst clears the registration: the engine's launches are
 *   then what they were.  An engine without a registration issues the launches it issued before.
 * MP_EGO_HOST (eng == NULL; pack, pack_len, cfg as for mp_create): MP_EGO_DRAW of HOST rows into
 *   a HOST dst, computed by the library without a device (bank must not be NULL).  A bad index
 *   returns MP_ERR_INVALID at once, naming it; the elements before it are written.
 *
 * Refused before any launch, the engine left as it was — MP_ERR_INVALID: a wrong struct_size or
 * op; an engine with MP_EGO_HOST, none with the others; MP_EGO_HOST without a pack; NULL dst (draw,
 * host); count < 1, or bank_rows < 1 with a bank; rows == NULL with count above the rows there
 * are; a fingerprint that is not the engine's (the pack's); dst_bytes short of what is written; a
 * dst, rows or players that is not 4-byte aligned, a bank that is not 16-byte aligned; memory
 * that is not the engine's device's or leaves its allocation; a ring whose slots are not the
 * engine's or whose stride is short of a slot or no multiple of 4; nonzero reserved words.
 * MP_ERR_UNSUPPORTED: a record whose render planes do not fit one wave's share of the LDS. */
enum { MP_EGO_DRAW = 1, MP_EGO_REGISTER = 2, MP_EGO_HOST = 3 };
/* WORLD.LAYER: the same request with the WORLD in place of the viewers — the layer view of the whole
 * map, which the reference builds on every step to render "WORLD.RGB" from and throws away
 * (base_simulation.lua:348-360, worldLayerView through worldSpriteMap).
 *
 * The world's value table.  Wt[s] = 1 + view_sprite_map[P][state_sprite[s]] for 1 <= s <
 * min(nstates, 256) with state_sprite[s] >= 0, else 0: row P of the pack's view_sprite_map is the
 * world's.  num_world_ids = 1 + max(Wt).  The ids are numbered like "LAYER"'s: id i is sprite
 * i - 1, after the WORLD's sprite map and no viewer's.
 * Definition.  For a record (a bank row or a live world) WORLD.LAYER is int32 [H][W][L], north up:
 * out[y][x][l] = Wt[planes[l][y][x]].  No cell is off the map, so OutOfBounds never occurs.  A
 * dead avatar is on no plane and shows nowhere.
 *
 * The ops are those of MP_EGO_DRAW, MP_EGO_REGISTER and MP_EGO_HOST in every word above, with these
 * differences: `players` must be NULL (MP_ERR_INVALID otherwise); an element of dst is one record's
 * [H][W][L] (4-byte aligned), a registration's tensor int32 [N][H][W][L]; the registration is one
 * of its own beside EGO_LAYER's, its launch follows those of the viewers' registrations behind
 * every submission, and a NULL dst clears it alone.  A bad rows[i] is reported as above, naming
 * MpEgoLayer (MP_EGO_WORLD_DRAW).  MP_ERR_UNSUPPORTED also for more than 64 layers.  There is no
 * inline wrapper for these ops: a C caller fills the struct itself and hands it to mp_snapshot. */
enum { MP_EGO_WORLD_DRAW = 4, MP_EGO_WORLD_REGISTER = 5, MP_EGO_WORLD_HOST = 6 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpEgoLayer) */
  int32_t op;              /* MP_EGO_* */
  uint64_t fingerprint;    /* in (draw, host): the rows' */
  const void* bank;        /* uint8 [bank_rows][S]; NULL (draw): the engine's worlds */
  const int32_t* rows;     /* int32 [count], NULL = rows 0 .. count - 1 */
  const int32_t* players;  /* int32 [count], NULL = every viewer of each row */
  void* dst;               /* int32: see the op */
  uint64_t dst_bytes;
  int32_t bank_rows;
  int32_t count;
  uint64_t slot_stride;    /* MP_EGO_REGISTER with a ring: bytes between two slots */
  int32_t slots;           /* MP_EGO_REGISTER: 0, or the ring's slots */
  int32_t reserved;        /* 0 */
  const void* pack;        /* MP_EGO_HOST */
  uint64_t pack_len;
  const MpConfig* cfg;
  uint64_t reserved2[3];   /* 0 */
} MpEgoLayer;

/* The layout of a record, told by the library: what the bytes of a saved row are, so that a
 * caller can read and edit world states by field.  Rides mp_snapshot, recognised by its size:
 * `bytes` = sizeof(MpStateLayout), `host_buf` a HOST MpStateLayout with struct_size set to it.
 * include/mp_state_check.h wraps it as an inline C function.
 *   eng != NULL: the engine's layout (pack / pack_len / cfg are ignored).
 *   eng == NULL: the layout an engine created with mp_create(pack, pack_len, cfg) would have,
 *     worked out on the host alone (no device is touched; errors as mp_create's).
 * A row is uint8 [world_stride]: grid_planes planes of H x W bytes, layer-major — the L render
 * planes (a byte is a state id of the pack, 0 = nothing) and behind them the level's hidden planes
 * — then whatever the level keeps up to grid_bytes (the matrix games' player block, at
 * player_block, else -1), padding up to grid_pad, and at grid_pad the tail: tail_bytes bytes whose
 * named fields `fields[0 .. num_fields)` lists with offset (from grid_pad), element size and
 * element count.  The names and offsets come from the one list of the tail's members the library
 * itself is compiled from.  `fields` may be NULL (num_fields is still set); fields_cap smaller than
 * num_fields is MP_ERR_INVALID. */
typedef struct {
  char name[16];
  int32_t offset;          /* bytes from grid_pad */
  int32_t elem_bytes;      /* 1, 2, 4 or 8 */
  int32_t count;           /* elements: 16 for a per-avatar array, 1 for a scalar */
  int32_t reserved;
} MpStateField;
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpStateLayout) */
  uint32_t layout_version; /* out: MP_RECORD_LAYOUT_VERSION of the library */
  const void* pack;        /* the host-only question (eng == NULL) */
  uint64_t pack_len;
  const MpConfig* cfg;
  /* out */
  int32_t map_h, map_w, num_layers, num_players, num_states;
  int32_t grid_planes, grid_bytes, grid_pad, world_stride, tail_bytes;
  int32_t max_frames, avatar_layer, substrate, player_block;
  int32_t reserved[2];
  uint64_t fingerprint;    /* out: MP_STATES_FINGERPRINT's value */
  MpStateField* fields;    /* HOST array [fields_cap], or NULL */
  int32_t fields_cap;
  int32_t num_fields;      /* out */
} MpStateLayout;

/* Is a record well-formed?  Rows that came from MP_STATES_SAVE or MP_STEP_ROW_STATE always are;
 * rows a caller edited, or built, may not be, and a step uses a record's bytes as cell
 * coordinates, state ids and table indices.  The check judges a row against the rules below
 * WITHOUT loading it; nothing of the engine's is written.  Rides mp_snapshot, recognised by its
 * size: `bytes` = sizeof(MpStatesCheck), `host_buf` a HOST MpStatesCheck with struct_size set to
 * it.  include/mp_state_check.h wraps the three forms as inline C functions.
 *
 * A verdict is two int32: (rule, offset word).  (0, 0): well-formed.  Otherwise the
 * lexicographically smallest pair among the row's violations; the offset word is the byte offset
 * in the row of the offending byte (for rule 7: sub-code << 24 | byte offset):
 *   1  a byte of a render plane is >= the pack's state count
 *   2  a non-zero byte of render plane l is a state of another layer
 *   3  a tail value out of range: aori >= 4, aalive > 1 (avatars < num_players only), done, cont
 *      or started not 0 or 1, step outside [0, max_frames]
 *   4  a living avatar with ax >= W or ay >= H, or whose cell of the avatar plane does not hold
 *      one of its own avatar states
 *   5  an avatar state of avatar p in a cell other than (ax[p], ay[p]), or anywhere while p is
 *      not alive
 *   6  orders_step neither 0 nor step + 1; or, with orders_step != 0, a stream of next_orders
 *      whose nibbles over the positions < num_players are not a permutation of the avatars
 *   7  a level's own rule (DESIGN.md section 3.9 lists them with the source lines they protect)
 * Never judged: the padding, the bytes of avatars >= num_players, ctr[], reward_fx.
 *
 * MP_CHECK_ROWS (eng != NULL): out (device int32 [count][2]) element i := the verdict of row
 *   rows[i] (device int32 [count]; NULL: row i, count <= bank_rows) of `bank` (device uint8
 *   [bank_rows][S]).  Enqueued on the engine's stream, no synchronisation.  A rows[i] outside the
 *   bank is never read: element i is (-1, rows[i]) and the next synchronising call returns
 *   MP_ERR_INVALID.
 * MP_CHECK_HOST (eng == NULL; pack, pack_len, cfg as for mp_create): the same verdicts of HOST
 *   rows into a HOST out, by the same rule functions compiled for the host; no device is touched.
 *   A rows[i] outside the bank gives (-1, rows[i]).
 * MP_CHECK_FILTER (eng != NULL): for a checked load.  rows = src (device int32 [N], as
 *   MP_STATES_LOAD takes it), count = N, out = checked (device int32 [N]): checked[w] := src[w]
 *   when row src[w] is well-formed, and also when src[w] is -1 or no row of the bank (the load
 *   handles both); -1 otherwise — the world is then left alone by a load from `checked`, and the
 *   next synchronising call returns MP_ERR_INVALID naming the world, the row and the rule (of
 *   several refused worlds one is named).  The engine stays usable.
 * Refused before any launch, MP_ERR_INVALID: NULL bank or out, count < 1 or bank_rows < 1, an
 * unknown op, a fingerprint that is not the engine's (host form: the pack's), out_bytes too
 * small, a bank that is not 16-byte aligned, rows or out not 4-byte aligned, device memory that
 * is not the engine's device's or not inside one allocation, count != N for a filter. */
enum { MP_CHECK_ROWS = 1, MP_CHECK_HOST = 2, MP_CHECK_FILTER = 3 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpStatesCheck) */
  int32_t op;              /* MP_CHECK_* */
  uint64_t fingerprint;    /* in: the rows' */
  const void* pack;        /* MP_CHECK_HOST */
  uint64_t pack_len;
  const MpConfig* cfg;
  const void* bank;        /* uint8 [bank_rows][S] */
  int32_t bank_rows;
  int32_t count;
  const int32_t* rows;     /* int32 [count] or NULL (FILTER: src[N]) */
  void* out;               /* int32 [count][2] (FILTER: int32 [N]) */
  uint64_t out_bytes;
  uint64_t reserved;       /* 0 */
} MpStatesCheck;

/* Are two records the same state?  Comparing rows byte for byte says "different" of equal states:
 * ctr[] and reward_fx are the bookkeeping of the engine a row was loaded into, the cached visiting
 * orders (orders_step, next_orders) may be present or absent, and the padding and the bytes of
 * avatars >= num_players hold whatever an edit left.  The hash is a 64-bit function of exactly the
 * bytes a state's future and its observations depend on, computed on the device where the rows
 * lie, 8 bytes a row: transposition tables and duplicate pruning in tree search, proof that a
 * regenerated rollout is the recorded one, exploration cells from a chosen subset of planes and
 * fields.  Rides mp_snapshot, recognised by its size: `bytes` = sizeof(MpStatesHash), `host_buf` a
 * HOST MpStatesHash with struct_size set to it.  include/mp_state_hash.h wraps the forms as
 * inline C functions.
 *
 * The function.  A row is S = world_stride bytes (a multiple of 16).  With w_j the little-endian
 * u32 at byte 4 j, m_j the u32 with 0xFF in every INCLUDED byte of that word, and
 *   fmix64(h): h ^= h >> 33; h *= 0xff51afd7ed558ccd; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53;
 *              h ^= h >> 33   (u64),
 *   c_j = fmix64((u64)(j + 1) << 32 | (w_j & m_j))   for every j with m_j != 0,
 *   H   = fmix64(sum_j c_j mod 2^64).
 * fmix64 is a bijection: changing one included byte always changes H, changing an excluded byte
 * never does.  Hashes compare only between rows of one fingerprint, hashed with one spec.
 *
 * Included bytes.  flags == 0, the default spec, "the state": every byte of the grid_planes planes;
 * the level's block [player_block, grid_bytes) where the level has one; every field of the tail
 * but ctr, reward_fx, orders_step and next_orders — of the 16-element (per-avatar) fields only the
 * elements < num_players.  flags & MP_HASH_CUSTOM: the planes whose bit is set in plane_mask (bit l
 * = grid plane l; a pack with more than 64 planes is refused), the fields whose bit is set in
 * field_mask (bit i = fields[i] of MpStateLayout; ctr and next_orders may be named), per-avatar
 * fields still cut to < num_players, and the level's block with MP_HASH_PLAYER_BLOCK.  Never
 * included: what lies between the planes and the level's block, the padding up to grid_pad, what
 * follows the tail's last field.
 *
 * MP_HASH_ROWS (eng != NULL): out (device u64 [count]) element i := H of row rows[i] (device int32
 *   [count]; NULL: row i, count <= bank_rows) of `bank` (device uint8 [bank_rows][S]).  Enqueued on
 *   the engine's stream, no synchronisation.  A rows[i] outside the bank is never read: element i
 *   of out keeps what it held, and the next synchronising call returns MP_ERR_INVALID.
 * MP_HASH_WORLDS (eng != NULL): the same over the engine's own records where they lie (bank and
 *   bank_rows are ignored): rows is a list of worlds (NULL: every world, count = N).  Refused on
 *   an engine that has never been reset, like MP_STATES_SAVE.  fingerprint is ignored.
 * MP_HASH_HOST (eng == NULL; pack, pack_len, cfg as for mp_create): H of HOST rows into a HOST
 *   out, by the same function compiled for the host; no device is touched.  Every rows[i] inside
 *   the bank is hashed; if one lies outside, its element keeps what it held and the call returns
 *   MP_ERR_INVALID naming the first.
 * MP_HASH_MASK (eng != NULL, or NULL with pack, pack_len, cfg): out (HOST uint8 [S], out_bytes >=
 *   S) := the spec's byte mask, 0xFF where a byte counts.  Nothing else is read.
 * The engine keeps the default spec's mask on the device from mp_create on, and the mask of the
 * most recent custom spec: a request with the default spec or with the custom spec of the request
 * before only enqueues.  A request with a NEW custom spec waits for the engine's stream once, to
 * replace that mask (as an MpStatesObserve request that has to grow its scratch does).
 * Refused before any launch, MP_ERR_INVALID, the engine left as it was: NULL bank or out, count <
 * 1 or bank_rows < 1, rows == NULL with count > bank_rows (WORLDS: count != N), an unknown op or
 * flag, a fingerprint that is not the engine's (host form: the pack's), out_bytes too small, a
 * bank that is not 16-byte aligned, an out that is not 8-byte aligned, rows not 4-byte aligned,
 * device memory that is not the engine's device's or not inside one allocation, a plane_mask or
 * field_mask bit that names no plane or no field, MP_HASH_PLAYER_BLOCK on a level without one, a
 * custom spec that includes no byte.  The request writes `out` and, for a bad index, the fault
 * words — nothing else of the engine's; an engine nothing else has touched is still untouched to
 * mp_tune. */
enum { MP_HASH_ROWS = 1, MP_HASH_WORLDS = 2, MP_HASH_HOST = 3, MP_HASH_MASK = 4 };
enum { MP_HASH_CUSTOM = 1, MP_HASH_PLAYER_BLOCK = 2 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpStatesHash) */
  int32_t op;              /* MP_HASH_* */
  uint64_t fingerprint;    /* in: the rows' (ROWS, HOST) */
  const void* pack;        /* MP_HASH_HOST, MP_HASH_MASK without an engine */
  uint64_t pack_len;
  const MpConfig* cfg;
  const void* bank;        /* uint8 [bank_rows][S] (ROWS, HOST) */
  int32_t bank_rows;
  int32_t count;
  const int32_t* rows;     /* int32 [count] or NULL (WORLDS: a world list) */
  void* out;               /* u64 [count] (MASK: uint8 [S]) */
  uint64_t out_bytes;
  uint64_t plane_mask;     /* MP_HASH_CUSTOM: bit l = grid plane l */
  uint32_t field_mask;     /* MP_HASH_CUSTOM: bit i = tail field i of MpStateLayout */
  int32_t flags;           /* 0: the default spec; MP_HASH_CUSTOM [| MP_HASH_PLAYER_BLOCK] */
  uint64_t reserved;       /* 0 */
} MpStatesHash;

/* Do two PLAYERS see the same thing?  MpStatesHash says whether two worlds are one state; it hashes
 * absolute map bytes, so it is neither egocentric nor limited to a viewer's window.  MpViewHash is
 * the hash of what one player observes — its EGO_LAYER (MpEgoLayer) — worked out on the device
 * from the record, without drawing the view: 8 bytes a viewer.  Per-agent novelty counts
 * (torch.unique(h, return_counts=True)), information-set keys of the acting player, dropping
 * duplicate (step, world, player) views from a replay buffer, "did my view change?" for frame
 * skip.  Rides mp_snapshot, recognised by its size: `bytes` = sizeof(MpViewHash), `host_buf` a
 * HOST MpViewHash with struct_size set to it.  include/mp_view_hash.h wraps it as inline C
 * functions.
 *
 * The function.  For a record (a bank row or a live world) and a viewer p let E be the viewer's
 * EGO_LAYER, int32 [VH][VW][L], exactly as MpEgoLayer defines it (a dead or off-grid viewer: every
 * word OutOfBounds), and e = (vy * VW + vx) * L + l.  With fmix64 the one MpStatesHash spells out:
 *   v_e = classes ? classes[E_e] : E_e,
 *   c_e = fmix64((u64)(e + 1) << 32 | (u32)v_e)   for every e whose layer l is included,
 *   V   = fmix64(sum_e c_e mod 2^64).
 * Layer l is included iff bit l of layer_mask is set; layer_mask == 0 means every layer.  Words
 * that are 0 are included like any other.  `classes` is an optional int32 table with one entry
 * per possible id, 0 .. the largest id the viewers' value tables hold: classes_len must equal
 * num_ids, which every request that gets as far as the tables writes back into the caller's
 * struct (count == 0 with a NULL dst, MP_VIEWHASH_DRAW or MP_VIEWHASH_HOST, asks for nothing
 * else).  fmix64 is a bijection, so the properties of the state hash hold:
 *   - changing one included word always changes V;
 *   - changing an excluded layer, or a cell outside the viewer's window, never changes V;
 *   - with `classes`, two ids of one class are indistinguishable by construction.
 * Hashes compare only within one fingerprint and one (layer_mask, classes) choice.
 *
 * MP_VIEWHASH_DRAW: element i of `dst` belongs to row rows[i] (NULL: row i) of `bank` (device
 *   uint8 [bank_rows][S], 16-byte aligned); a NULL bank means the engine's own worlds as they are
 *   now (rows[] are then world indices, bank_rows is ignored, the engine must have been reset).
 *   players == NULL: dst is u64 [count][P], V of every viewer of each row; otherwise players is
 *   device int32 [count] and dst is u64 [count], V of player players[i] of row rows[i].  Rows and
 *   (row, player) pairs may repeat and `count` has no relation to the engine's N.  `dst` is
 *   8-byte aligned; `classes` is a DEVICE int32 [classes_len] or NULL.  Stream-ordered, no
 *   synchronisation, no allocation; nothing of the engine's is written.  A rows[i] that is no
 *   row (no world) or a players[i] outside [0, P) is never used as an index: element i of dst is
 *   left as it was — every such element — and the next synchronising call returns MP_ERR_INVALID
 *   once, naming MpViewHash, rows[i] or players[i] and the value (of several such indices one is
 *   reported); the engine stays usable.
 * MP_VIEWHASH_REGISTER: `dst` names a device u64 [N][P] (slots == 0), or a ring: slot s is at dst
 *   + s * slot_stride bytes, and `slots` must equal the engine's ring slots (mp_bind_output_ring),
 *   as MP_EGO_REGISTER.  While registered, every submission (reset, step, step_fields, every
 *   K-step request, a load) is followed on the same stream by ONE launch that rewrites all N * P
 *   hashes from the records, into dst or into the ring slot that submission wrote; `classes` (a
 *   DEVICE table the caller keeps alive and may rewrite between submissions) and layer_mask are
 *   the registration's.  mp_tune's probe submissions do not write it.  A NULL dst clears the
 *   registration: the engine's launches are then what they were.  An engine without a
 *   registration issues exactly the launches it issued before.
 * MP_VIEWHASH_HOST (eng == NULL; pack, pack_len, cfg as for mp_create): MP_VIEWHASH_DRAW of HOST
 *   rows into a HOST dst with a HOST `classes`, computed by the library without a device (bank
 *   must not be NULL).  A bad index returns MP_ERR_INVALID at once, naming it; the elements before
 *   it are written.
 *
 * Refused before any launch, the engine left as it was — MP_ERR_INVALID: what MpEgoLayer refuses
 * (with 8-byte alignment of dst and of a ring's stride); a layer_mask bit that names no layer;
 * classes_len != num_ids with a table, != 0 without one; a class table that is not 4-byte aligned
 * or not the engine's device's.  MP_ERR_UNSUPPORTED: where MpEgoLayer returns it (a record whose
 * render planes, beside the viewers' value tables, do not fit one wave's share of the LDS); more
 * than 64 layers. */
enum { MP_VIEWHASH_DRAW = 1, MP_VIEWHASH_REGISTER = 2, MP_VIEWHASH_HOST = 3 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpViewHash) */
  int32_t op;              /* MP_VIEWHASH_* */
  uint64_t fingerprint;    /* in (draw, host): the rows' */
  const void* bank;        /* uint8 [bank_rows][S]; NULL (draw): the engine's worlds */
  const int32_t* rows;     /* int32 [count], NULL = rows 0 .. count - 1 */
  const int32_t* players;  /* int32 [count], NULL = every viewer of each row */
  void* dst;               /* u64: see the op */
  uint64_t dst_bytes;
  int32_t bank_rows;
  int32_t count;
  uint64_t slot_stride;    /* MP_VIEWHASH_REGISTER with a ring: bytes between two slots */
  int32_t slots;           /* MP_VIEWHASH_REGISTER: 0, or the ring's slots */
  int32_t classes_len;     /* 0 without classes, else num_ids */
  const void* pack;        /* MP_VIEWHASH_HOST */
  uint64_t pack_len;
  const MpConfig* cfg;
  uint64_t layer_mask;     /* bit l = layer l; 0 = every layer */
  const int32_t* classes;  /* int32 [classes_len] or NULL (host form: a HOST table) */
  int32_t num_ids;         /* out: the length a class table must have */
  int32_t reserved;        /* 0 */
  uint64_t reserved2[3];   /* 0 */
} MpViewHash;

/* What a conv net reads of a player's view.  EGO_LAYER (MpEgoLayer) is int32 sprite ids, and every
 * learner turns it into a channels-first stack of 0/1 planes ("wall here", "apple here", "another
 * avatar here") before its first convolution: a gather through an id -> class table, a one-hot, a
 * reduction over the layers and a permute.  MpEgoPlanes writes those planes themselves, uint8,
 * from the record, without drawing the int32 view, and adds what the ids do not carry: where the
 * others face.  Rides mp_snapshot, recognised by its size: `bytes` = sizeof(MpEgoPlanes),
 * `host_buf` a HOST MpEgoPlanes with struct_size set to it.  include/mp_ego_planes.h wraps it as
 * inline C functions.
 *
 * The class table.  `classes` is int32 [classes_len], one entry per possible id, 0 .. the largest
 * id the viewers' value tables hold: classes_len must equal num_ids, which every request that gets
 * as far as the tables writes back into the caller's struct (count == 0 with a NULL dst,
 * MP_EGOPLANES_DRAW or MP_EGOPLANES_HOST, asks for nothing else).  Every entry lies in
 * [-1, num_classes), and 1 <= num_classes = C <= 64.
 *
 * The planes.  For a record (a bank row or a live world) and a viewer p let E be the viewer's
 * EGO_LAYER, int32 [VH][VW][L], exactly as MpEgoLayer defines it (a cell off the map, and every
 * cell of a dead viewer: OutOfBounds).  The viewer's block is uint8 [C'][VH][VW], C' = C, or C + 4
 * with `facing`; every byte is 0 or 1:
 *   class plane c < C:   out[c][i][j] = 1 iff some layer l with bit l of layer_mask set (0: every
 *     layer) has classes[E[i][j][l]] == c.  Class -1 sets nothing.
 *   facing plane C + d, d in 0 .. 3:   out[C + d][i][j] = 1 iff the viewer is alive, window cell
 *     (i, j) maps to a cell (x, y) ON the map — by the turned offset and the torus wrap of
 *     EGO_LAYER — and some living avatar q < P has (ax[q], ay[q]) == (x, y) and
 *     ((aori[q] - aori[p]) & 3) == d.  The viewer sees itself at (vf, vl) with d = 0.  On a torus
 *     whose window is larger than the map an avatar appears in every window cell that maps to its
 *     cell.  A dead viewer's facing planes are 0.  layer_mask and classes have no influence here.
 *
 * MP_EGOPLANES_DRAW: element i of `dst` belongs to row rows[i] (NULL: row i) of `bank` (device
 *   uint8 [bank_rows][S], 16-byte aligned); a NULL bank means the engine's own worlds as they are
 *   now (rows[] are then world indices, bank_rows is ignored, the engine must have been reset).
 *   players == NULL: dst is uint8 [count][P][C'][VH][VW]; otherwise players is device int32 [count]
 *   and dst is uint8 [count][C'][VH][VW], the planes of player players[i] of row rows[i].  Rows and
 *   (row, player) pairs may repeat and `count` has no relation to the engine's N.  `dst` may start
 *   on ANY byte (C' * VH * VW is odd for most packs, and a mixture hands each member a slice of
 *   one tensor); no byte outside the count blocks is written.  `classes` is a DEVICE table.
 *   Stream-ordered, no synchronisation, no allocation; nothing of the engine's is written.  A
 *   rows[i] that is no row (no world) or a players[i] outside [0, P) is never used as an index:
 *   element i of dst is left as it was — every such element — and the next synchronising call
 *   returns MP_ERR_INVALID once, naming MpEgoPlanes, rows[i] or players[i] and the value (of
 *   several such indices one is reported); the engine stays usable.  An entry of the device table
 *   outside [-1, num_classes) counts as -1 and is reported the same way, naming classes[id].
 * MP_EGOPLANES_REGISTER: `dst` names a device uint8 [N][P][C'][VH][VW] (slots == 0), or a ring:
 *   slot s is at dst + s * slot_stride bytes, and `slots` must equal the engine's ring slots
 *   (mp_bind_output_ring), as MP_EGO_REGISTER.  While registered, every submission (reset, step,
 *   step_fields, every K-step request, a load) is followed on the same stream by ONE launch that
 *   rewrites all N blocks from the records, into dst or into the ring slot that submission wrote
 *   (behind the view-hash launch); `classes` (a DEVICE table the caller keeps alive and may rewrite
 *   between submissions), layer_mask, num_classes and facing are the registration's.  mp_tune's
 *   probe submissions do not write it.  A NULL dst clears the registration: the engine's launches
 *   are then what they were.  An engine without a registration issues exactly the launches it
 *   issued before.
 * MP_EGOPLANES_HOST (eng == NULL; pack, pack_len, cfg as for mp_create): MP_EGOPLANES_DRAW of HOST
 *   rows into a HOST dst with a HOST `classes`, computed by the library without a device (bank
 *   must not be NULL).  A bad index returns MP_ERR_INVALID at once, naming it; the elements before
 *   it are written.  An entry outside [-1, num_classes) is refused before anything is written.
 *
 * Refused before any launch, the engine left as it was — MP_ERR_INVALID: a NULL classes;
 * classes_len != num_ids; num_classes outside [1, 64]; facing other than 0 or 1; a short
 * dst_bytes or slot_stride; a host pointer where a device one is needed; a fingerprint that is
 * not the engine's (the pack's); an engine never reset (a NULL bank); a layer_mask bit that names
 * no layer; misaligned bank, rows, players or classes.  MP_ERR_UNSUPPORTED: a record whose render
 * planes, beside the viewers' value tables and the bit planes of one viewer, do not fit one wave's
 * share of the LDS; more than 64 layers. */
enum { MP_EGOPLANES_DRAW = 1, MP_EGOPLANES_REGISTER = 2, MP_EGOPLANES_HOST = 3 };
/* The world planes: the same request with the WORLD in place of the viewers — the critic's input of
 * a centralised-critic method, a world model's global state.
 *
 * The class table.  `classes` is int32 [num_world_ids] (see MP_EGO_WORLD_DRAW: the ids of the
 * world's value table), entries in [-1, C), 1 <= C <= 64.  classes_len must equal num_world_ids,
 * which these ops write back into num_ids (count == 0 with a NULL dst asks for nothing else).
 * The planes.  With WL the record's WORLD.LAYER, an element is uint8 [C'][H][W], C' = C, or C + 4
 * with `facing`; every byte is 0 or 1:
 *   class plane c < C:   out[c][y][x] = 1 iff some layer l with bit l of layer_mask set (0: every
 *     layer) has classes[WL[y][x][l]] == c.  Class -1 sets nothing.
 *   facing plane C + d:  out[C + d][y][x] = 1 iff some living avatar q < P stands on (x, y) with
 *     aori[q] == d.  This is ABSOLUTE facing, 0 = N: there is no viewer.
 *
 * The ops are those of MP_EGOPLANES_DRAW, MP_EGOPLANES_REGISTER and MP_EGOPLANES_HOST in every word
 * above, with these differences: `players` must be NULL (MP_ERR_INVALID otherwise); an element of
 * dst is one record's [C'][H][W] and may start on any byte, a registration's tensor uint8
 * [N][C'][H][W]; the registration is one of its own beside the viewers' planes, its launch is the
 * last behind every submission, and a NULL dst clears it alone.  A bad rows[i] and an entry of the
 * device class table outside [-1, C) (it counts as -1) are reported as above, naming MpEgoPlanes
 * (MP_EGOPLANES_WORLD_DRAW).  MP_ERR_UNSUPPORTED: a record whose render planes and one u64 a cell
 * do not fit one wave's share of the LDS; more than 64 layers.  There is no inline wrapper for these
 * ops: a C caller fills the struct itself and hands it to mp_snapshot. */
enum { MP_EGOPLANES_WORLD_DRAW = 4, MP_EGOPLANES_WORLD_REGISTER = 5, MP_EGOPLANES_WORLD_HOST = 6 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpEgoPlanes) */
  int32_t op;              /* MP_EGOPLANES_* */
  uint64_t fingerprint;    /* in (draw, host): the rows' */
  const void* bank;        /* uint8 [bank_rows][S]; NULL (draw): the engine's worlds */
  const int32_t* rows;     /* int32 [count], NULL = rows 0 .. count - 1 */
  const int32_t* players;  /* int32 [count], NULL = every viewer of each row */
  void* dst;               /* uint8: see the op */
  uint64_t dst_bytes;
  int32_t bank_rows;
  int32_t count;
  uint64_t slot_stride;    /* MP_EGOPLANES_REGISTER with a ring: bytes between two slots */
  int32_t slots;           /* MP_EGOPLANES_REGISTER: 0, or the ring's slots */
  int32_t classes_len;     /* num_ids */
  const void* pack;        /* MP_EGOPLANES_HOST */
  uint64_t pack_len;
  const MpConfig* cfg;
  uint64_t layer_mask;     /* bit l = layer l; 0 = every layer */
  const int32_t* classes;  /* int32 [classes_len] (host form: a HOST table) */
  int32_t num_ids;         /* out: the length a class table must have */
  int32_t num_classes;     /* C, 1 .. 64 */
  int32_t facing;          /* 1: the four facing planes behind the class planes */
  int32_t reserved;        /* 0 */
  uint64_t reserved2[3];   /* 0 */
} MpEgoPlanes;

/* Whom does a player see, and whom could it zap?  EGO_LAYER, the view hashes and the planes
 * describe CELLS; MpAvatarIds describes PLAYERS: the reference's per-avatar observations
 * AVATAR_IDS_IN_VIEW (AvatarIdsInViewObservation, avatar_library.lua:1204-1264) and
 * AVATAR_IDS_IN_RANGE_TO_ZAP (AvatarIdsInRangeToZapObservation, :1267-1315, on
 * Zapper:getWhoZappable, :780-824), two int32 0/1 vectors over the player slots, worked out from
 * the record alone.  Attention and communication masks, opponent-model targets, "is a zap worth its
 * cooldown", and counting who could have zapped whom and did not.  Rides mp_snapshot, recognised by
 * its size: `bytes` = sizeof(MpAvatarIds), `host_buf` a HOST MpAvatarIds with struct_size set to
 * it.  include/mp_avatar_ids.h wraps it as inline C functions.
 *
 * The definition.  P is the player count; a record's head is ax, ay, aori, aalive.
 *   IN_VIEW[p][q] = 1 iff viewer p is alive, avatar q is alive, and some cell (vx, vy) of p's
 *     window lies over q's cell: the cell EGO_LAYER (MpEgoLayer) shows there, by the turned offset
 *     and the torus wrap.  It is 1 at q == p for a living viewer (the reference's rectangle holds
 *     the avatar's own cell), and 0 or 1 even where a torus smaller than the window shows q more
 *     than once.  A dead viewer's row is all 0 (the reference leaves that case undefined; the
 *     facing planes of MpEgoPlanes do the same).  Only the avatar layer counts: in every committed
 *     pack avatars live on avatar_layer alone, so the reference's `layers` argument has no
 *     counterpart.
 *   IN_RANGE[p][q] is the reference's rays, literally, on the avatar's own layer.  The pack's zap
 *     footprint (the Zapper's beamLength and beamRadius) is a list of cells (lat, fw, pred): cell j
 *     of living p lies at pos + lat * right(ori) + fw * forward(ori), under the map's topology as a
 *     step's beam applies it.  A cell STOPS its ray when it lies off the map or when its byte of
 *     the avatar_layer plane is not 0.  Cell j is REACHED when it is on the map and no cell of
 *     pred(j) stops.  IN_RANGE[p][q] = 1 iff some reached cell holds q's avatar state.  Readiness
 *     plays no part: a cooldown does not enter.  BLOCKERS ON OTHER LAYERS PLAY NO PART either:
 *     getWhoZappable casts on self.gameObject:getLayer() only.  This is the reference's
 *     observation, not a prediction of the next beam on levels whose beam blockers lie elsewhere.
 *     A dead p's row is all 0 (:1289-1291).  A level without a Zapper (coins, the kitchens, the
 *     matrix games, coop_mining, gift_refinements) refuses dst_zap with MP_ERR_INVALID, naming the
 *     level's family; IN_VIEW works on every level.
 *
 * `dst` takes IN_VIEW and `dst_zap` IN_RANGE; either may be NULL, not both.  One launch writes
 * both.
 * MP_AVATARIDS_DRAW: element i belongs to row rows[i] (NULL: row i) of `bank` (device uint8
 *   [bank_rows][S], 16-byte aligned); a NULL bank means the engine's own worlds as they are now
 *   (rows[] are then world indices, bank_rows is ignored, the engine must have been reset).
 *   players == NULL: each destination is int32 [count][P][P], row p the vector of viewer p;
 *   otherwise players is device int32 [count] and each is int32 [count][P], the vector of player
 *   players[i] of row rows[i].  Rows and (row, player) pairs may repeat and `count` has no
 *   relation to the engine's N.  Destinations are 4-byte aligned.  Stream-ordered, no
 *   synchronisation, no allocation; nothing of the engine's is written.  A rows[i] that is no row
 *   (no world) or a players[i] outside [0, P) is never used as an index: element i of both
 *   destinations is left as it was — every such element — and the next synchronising call returns
 *   MP_ERR_INVALID once, naming MpAvatarIds, rows[i] or players[i] and the value (of several such
 *   indices one is reported); the engine stays usable.
 * MP_AVATARIDS_REGISTER: `dst` and `dst_zap` name device int32 [N][P][P] tensors (slots == 0), or
 *   rings: slot s is at + s * slot_stride bytes of each, and `slots` must equal the engine's ring
 *   slots (mp_bind_output_ring), as MP_EGO_REGISTER.  While registered, every submission (reset,
 *   step, step_fields, every K-step request, a load) is followed on the same stream by ONE launch
 *   that rewrites them from the records, into the tensors or into the ring slot that submission
 *   wrote (behind the planes' launch).  mp_tune's probe submissions do not write them.  Both NULL
 *   clears the registration: the engine's launches are then what they were.  An engine without a
 *   registration issues exactly the launches it issued before.
 * MP_AVATARIDS_HOST (eng == NULL; pack, pack_len, cfg as for mp_create): MP_AVATARIDS_DRAW of HOST
 *   rows into HOST destinations, computed by the library without a device (bank must not be
 *   NULL).  A bad index returns MP_ERR_INVALID at once, naming it; the elements before it are
 *   written.
 *
 * Refused before any launch, the engine left as it was — MP_ERR_INVALID: what MpEgoLayer refuses,
 * for either destination (dst_zap_bytes is dst_zap's size); dst_zap on a level without a Zapper.
 * MP_ERR_UNSUPPORTED: a record whose avatar_layer plane does not fit one wave's share of the LDS. */
enum { MP_AVATARIDS_DRAW = 1, MP_AVATARIDS_REGISTER = 2, MP_AVATARIDS_HOST = 3 };
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpAvatarIds) */
  int32_t op;              /* MP_AVATARIDS_* */
  uint64_t fingerprint;    /* in (draw, host): the rows' */
  const void* bank;        /* uint8 [bank_rows][S]; NULL (draw): the engine's worlds */
  const int32_t* rows;     /* int32 [count], NULL = rows 0 .. count - 1 */
  const int32_t* players;  /* int32 [count], NULL = every viewer of each row */
  void* dst;               /* IN_VIEW, int32: see the op; NULL: not asked for */
  uint64_t dst_bytes;
  int32_t bank_rows;
  int32_t count;
  uint64_t slot_stride;    /* MP_AVATARIDS_REGISTER with a ring: bytes between two slots (of both) */
  int32_t slots;           /* MP_AVATARIDS_REGISTER: 0, or the ring's slots */
  int32_t reserved;        /* 0 */
  const void* pack;        /* MP_AVATARIDS_HOST */
  uint64_t pack_len;
  const MpConfig* cfg;
  void* dst_zap;           /* IN_RANGE, int32, the shape of dst; NULL: not asked for */
  uint64_t dst_zap_bytes;
  uint64_t reserved2[3];   /* 0 */
} MpAvatarIds;

/* Action sequences: K steps of every world in ONE submission, bit-identical to K calls of the
 * single-step entry points (mp_step, or mp_step_fields with fields = 1) with the same actions,
 * which also hands back the transition of every one of the K steps.  For planners that fork a
 * state into many worlds and run a K-step action sequence in each, action repeat, replaying a
 * recorded trace, fast-forwarding.  Like the world states it rides an existing entry point as a
 * request: a call of mp_restore whose `bytes` is sizeof(MpStepMany) (neither sizeof(MpWorldStates)
 * nor any engine's snapshot size: a record is >= 448 bytes) takes `host_buf` as a HOST MpStepMany
 * with struct_size = sizeof(MpStepMany).  The request is enqueued on the engine's stream like a
 * step and does not synchronise; it marks the engine as in use, as a step does.
 * include/mp_step_many.h wraps it as an inline C function.
 *
 * After the request (A = the actions of the K steps):
 *  1. every world's record, the counters, every in-place or bound scalar output, the events of the
 *     last step, a bound MP_OBS_LAYER and every bound pixel view hold exactly the bytes they hold
 *     after K single steps with A[0] .. A[K - 1].  Auto-reset included: a world whose episode ends
 *     at step k uses step k + 1 as its reset (that step's actions are ignored) and goes on in the
 *     new episode; with auto_reset = 0 it stays frozen and reports what a frozen world reports to
 *     the end of the sequence.  Out-of-range action ids are NOOPs counted in MP_CTR_BAD_ACTIONS.
 *  2. per_step[i], each optional (NULL: not asked for), stacked along a leading K:
 *       [0] MP_OBS_REWARD f64 [K][N][P]      [1] MP_OBS_COLLECTIVE_REWARD f64 [K][N]
 *       [2] MP_OBS_STEP_TYPE i32 [K][N]      [3] MP_OBS_DISCOUNT f64 [K][N]
 *       [4] MP_OBS_EVENTS i32 [K][N][MP_EVENT_ROWS][4]
 *     Row k is what the in-place buffer of that kind holds after step k of the sequential loop
 *     (EVENTS: the header row and the rows it counts; rows beyond the count are not written).
 *     These are the kinds every path of a step (step, reset, frozen) writes for a started world;
 *     no other kind has per-step rows.  A world that has never been reset writes nothing.  The
 *     in-place (or bound) buffers of the five kinds hold step K's values either way.
 *  3. it is one submission: with a rollout ring bound it writes ONE slot, the state after step K.
 *     Pixel views and LAYER are drawn once, from the final records (the K-step kernel, then the
 *     draw-only launches).
 *  4. `actions` is device memory: discrete ids int32 [K][N][P] (fields = 0) or raw fields int32
 *     [K][N][P][A] (fields = 1).  actions_step_bytes is the distance between two steps' blocks
 *     (0: the same [N][P] block every step, which is action repeat); per_step_bytes[i] the
 *     distance between two steps' rows of per_step[i].  Distances larger than a block let several
 *     engines read and write their own columns of shared [K][N total] tensors.
 *  5. 1 <= steps <= MP_STEP_MANY_MAX.
 *  6. MP_ERR_INVALID before any launch, the engine left as it was: NULL engine or actions; a wrong
 *     struct_size; steps out of range; fields neither 0 nor 1; an engine that has never been reset
 *     (mp_reset, mp_restore or a load); an actions_step_bytes that is neither 0 nor a multiple of
 *     4 >= one step's block; a per_step_bytes[i] smaller than one step's rows or not a multiple of
 *     the element size (8, 8, 4, 8; 16 for EVENTS, whose rows are stored as int4); a buffer not
 *     aligned to its element size (EVENTS: 16 bytes); any buffer that is not device memory of the
 *     engine's device or whose extent [ptr, ptr + (steps - 1) * distance + block) does not lie
 *     inside one allocation. */
#define MP_STEP_MANY_MAX 4096
typedef struct {
  uint32_t struct_size;        /* = sizeof(MpStepMany) */
  int32_t steps;               /* K */
  int32_t fields;              /* 0: discrete ids [K][N][P]; 1: raw fields [K][N][P][A] */
  int32_t reserved;
  const int32_t* actions;      /* device */
  uint64_t actions_step_bytes; /* 0: the same block every step */
  void* per_step[5];           /* device or NULL: REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT, EVENTS */
  uint64_t per_step_bytes[5];  /* distance between two steps' rows of each */
} MpStepMany;

/* Action sequences with per-step rows of the observations: an MpStepMany request that may ask for
 * rows of ANY non-pixel kind.  It rides mp_restore in the same way, by its own size: `bytes` =
 * sizeof(MpStepTrajectory), `host_buf` a HOST MpStepTrajectory with struct_size set to it.
 * include/mp_step_trajectory.h wraps it as an inline C function.  An MpStepMany request keeps
 * doing exactly what it does.
 *
 * Everything MpStepMany promises holds (its points 1, 3, 4 and 5: records, counters, in-place and
 * bound buffers, a bound LAYER, bound pixel views and the one ring slot hold what they hold after
 * K single steps; a world never reset writes nothing; one submission).  rows[0 .. num_rows) is a
 * HOST array naming each wanted kind once, among
 *   MP_OBS_REWARD, READY_TO_SHOOT, AUX0, STEP_TYPE, DISCOUNT, COLLECTIVE_REWARD, POSITION,
 *   ORIENTATION, EVENTS, AUX1..AUX4, ZAP_MATRIX, LAYER, INVENTORY, INTERACTION_INVENTORIES,
 *   MATRIX_CUMULANTS, INTERACTION_REWARDS,
 * with `rows` the device buffer of row 0, laid out as the kind's [N]... behind a leading K, and
 * `step_bytes` the distance between two rows: at least one step's block (mp_obs_bytes) and a
 * multiple of the element size (4 for STEP_TYPE, POSITION, ORIENTATION and LAYER, 16 for EVENTS,
 * 8 otherwise), to which the buffer is aligned too; larger distances are the columns of a shared
 * [K][N total] tensor.  Row k of kind X is, byte for byte, what the in-place (or bound) buffer of
 * X holds after the k-th call of the loop of single steps started from the same engine state
 * (EVENTS: the header row and the rows it counts).  For LAYER it is what a bound LAYER buffer
 * would hold after step k; LAYER need not be bound, and a bound one gets the final state as ever.
 *
 * The carry rule.  A single step leaves a kind's buffer as it was wherever it does not write it,
 * and the rows show exactly that: where step k writes nothing row k equals row k - 1, and row 0
 * equals the buffer as it was before the request.  A frozen world (done, auto_reset = 0) writes
 * REWARD, COLLECTIVE_REWARD, STEP_TYPE, DISCOUNT and the EVENTS header only, so its
 * READY_TO_SHOOT, AUX0, POSITION, ORIENTATION, inventories and debug kinds repeat what the
 * episode's last step left; MP_OBS_INTERACTION_REWARDS and MP_OBS_INTERACTION_INVENTORIES change
 * at an interaction and are carried from step to step (and over a reset, as far as a reset leaves
 * them) until the next one.  LAYER is a function of the record and is written at every step of a
 * started world.
 *
 * Refused before any launch, the engine left as it was: everything MpStepMany refuses (its point
 * 6, with this request's name); num_rows < 0, or > 0 with rows NULL; a kind outside
 * [0, MP_OBS_KINDS) or named twice, or a NULL buffer: MP_ERR_INVALID; a pixel kind (MP_OBS_RGB,
 * MP_OBS_RGB_POOL*, MP_OBS_WORLD_RGB): MP_ERR_INVALID — intermediate frames are what mp_step with
 * a rollout ring (mp_bind_output_ring) draws; a kind the substrate does not produce
 * (mp_obs_bytes == 0), or a debug kind (AUX1..4, ZAP_MATRIX, MATRIX_CUMULANTS) that is not being
 * produced (neither bound nor MpConfig.debug_observations; mp_observe's rule): MP_ERR_UNSUPPORTED;
 * a step_bytes or an alignment as above, a buffer that is not device memory of the engine's
 * device or whose extent [rows, rows + (steps - 1) * step_bytes + block) does not lie inside one
 * allocation: MP_ERR_INVALID.
 *
 * Per-step world states.  A row may also name MP_STEP_ROW_STATE, which is no observation kind:
 * row k is uint8 [N][S] (S = MpInfo.world_state_bytes), for a started world byte for byte what
 * MP_STATES_SAVE of that world gives after the k-th call of the loop of single steps — counters
 * and the cached visiting orders included, over auto-reset steps and frozen steps alike; a world
 * never reset writes nothing.  Beam search, branching from the middle of a sequence, a rollout
 * kept as states whose observations an MpStatesObserve request draws later.  Checked like every
 * row, with element size 16: step_bytes >= N * S and a multiple of 16, the buffer 16-byte
 * aligned.  num_rows may therefore reach MP_OBS_KINDS + 1.
 *
 * Per-step state hashes.  A row may name MP_STEP_ROW_HASH, no observation kind either: row k is
 * u64 [N], for a started world H (MpStatesHash, the default spec) of what MP_STEP_ROW_STATE's row
 * k holds — 8 bytes a world-step where the state row costs S, and the same for every level, so
 * that engines of different levels can share one [K][N total] tensor.  Written over auto-reset
 * steps and frozen steps alike; a world never reset writes nothing.  Checked like every row, with
 * element size 8: step_bytes >= N * 8 and a multiple of 8, the buffer 8-byte aligned.  The row
 * always has the default spec (MpStepRow has no room for one).  (The row's value is not 0x101:
 * requests that named 0x101 were refused before there was this row, and still are.)  The limit on
 * num_rows stays MP_OBS_KINDS + 1: the pixel kinds can never be named, so no valid request comes
 * near it. */
#define MP_STEP_ROW_STATE 0x100
#define MP_STEP_ROW_HASH 0x102
typedef struct {
  int32_t kind;                /* MpObsKind, MP_STEP_ROW_STATE or MP_STEP_ROW_HASH */
  int32_t reserved;
  void* rows;                  /* device: row 0 */
  uint64_t step_bytes;         /* distance between two rows */
} MpStepRow;
typedef struct {
  uint32_t struct_size;        /* = sizeof(MpStepTrajectory) */
  int32_t steps;               /* K */
  int32_t fields;              /* 0: discrete ids [K][N][P]; 1: raw fields [K][N][P][A] */
  int32_t num_rows;
  const int32_t* actions;      /* device */
  uint64_t actions_step_bytes; /* 0: the same block every step */
  const MpStepRow* rows;       /* HOST array [num_rows] */
} MpStepTrajectory;

/* Episode starts: where an auto-reset episode begins.  An engine with auto_reset = 1 restarts a
 * finished world from the pack's map; with a registration it restarts it from a row of a bank of
 * saved states instead, chosen by a device tensor the caller may rewrite at any time — curricula
 * and prioritised level replay, Go-Explore restarts, training on the middle of long episodes,
 * evaluation from a fixed set of situations, also in the middle of a K-step launch.  Rides
 * mp_restore, recognised by its size: `bytes` = sizeof(MpEpisodeStarts), `host_buf` a HOST
 * MpEpisodeStarts with struct_size set to it.  include/mp_episode_starts.h wraps it as inline C
 * functions.  A request with bank == NULL clears the registration.
 *
 * The registration names `bank` (device uint8 [bank_rows][S]), `rows` (device int32 [N]) and,
 * optionally, `verdicts` (device int32 [bank_rows][2], as MP_CHECK_ROWS writes them for the whole
 * bank).  The engine reads all three in place, in stream order, in every later stepping
 * submission: the caller keeps them alive and may rewrite `rows` (and the bank, and the verdicts)
 * whenever it likes.  The bank is never written.
 *
 * In any step (mp_step, mp_step_fields, their host forms, each of the K steps of an MpStepMany /
 * MpStepTrajectory request), for a world w that auto-resets in that step (started, done), with
 * r = rows[w] read at that moment:
 *   r == -1: the level's own reset, byte for byte what happens without a registration.
 *   0 <= r < bank_rows, and verdicts NULL or verdicts[r] == (0, 0): the world starts from row r.
 *     Its record and every output are what MP_STATES_LOAD writes for a world loaded from that row
 *     (the kinds that are functions of the record; the transition kinds as a reset writes them,
 *     STEP_TYPE FIRST; a row saved from a finished episode reports LAST, as a load does), on top of
 *     what the replaced auto-reset step left.
 *   anything else (an index outside [-1, bank_rows), or a row whose verdict is not (0, 0)): the
 *     row is never read, the world takes the level's own reset, and the next synchronising call
 *     returns MP_ERR_INVALID naming the world, the index and the rule; the engine stays usable.
 * The defining identity (fresh = 0): a step with a registration leaves every record, counter,
 * in-place or bound output and event row exactly as a step without one followed by
 * MP_STATES_LOAD with src[w] = rows[w] for the worlds that were done before the step and -1
 * elsewhere.  So the destination keeps its own ctr[] and reward_fx, and the start counts as the
 * episode start it replaces (MP_CTR_EPISODES + 1).  In a K-step request, row k of a step that
 * starts a world holds the start's values; rows of kinds a start does not write carry from row
 * k - 1 by the carry rule above.
 * fresh = 1: the started record is the row except that `seed` is the destination world's own,
 * `episode` is the destination's episode + 1 (what its own reset would have set) and
 * `orders_step` is 0 — as gathering the rows, editing those three fields and loading.  Worlds that
 * start from one row then draw differently; with fresh = 0 they share every environment draw.
 * Not affected: mp_reset (masked or not), MP_STATES_LOAD, MP_STATES_SAVE, MpStatesObserve,
 * MpStatesHash, MpStatesCheck, frozen worlds, mp_tune, mp_place_output and mp_box_fill.  The
 * registration is engine configuration, not part of a record: mp_snapshot does not carry it and
 * mp_restore of a snapshot leaves it in place.
 * While a registration is set a step with a bound pixel view is two launches (the step kernels,
 * then the draw-only launch per view) and MpInfo.fused reports 0; clearing it returns the engine
 * to the launches it had.  Ring slots are pointed and advanced as ever.
 * Refused, MP_ERR_INVALID, nothing changed: a wrong struct_size; an engine with auto_reset = 0;
 * bank_rows <= 0; NULL rows; fresh neither 0 nor 1; a fingerprint that is not the engine's; a bank
 * that is not 16-byte aligned, rows or verdicts not 4-byte aligned; bank, rows or verdicts that
 * are not device memory of the engine's device inside one allocation.  MP_ERR_UNSUPPORTED: an
 * engine created with MpConfig.unfused = 2 (it promised one launch a step). */
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpEpisodeStarts) */
  int32_t fresh;           /* 0: a started world is the world the row was saved from; 1: see above */
  uint64_t fingerprint;    /* the rows' */
  const void* bank;        /* device uint8 [bank_rows][S]; NULL clears the registration */
  const int32_t* rows;     /* device int32 [N] */
  const int32_t* verdicts; /* device int32 [bank_rows][2], or NULL */
  int32_t bank_rows;
  int32_t reserved;        /* 0 */
  uint64_t reserved2[3];   /* 0 */
} MpEpisodeStarts;

/* Stepping some of the worlds: an MpStepTrajectory request under a device mask that says, per step
 * and per world, whether the world runs — rollouts of different depths, a tree search that expands
 * only the leaves picked this round, worlds that stop after their first episode while the engine
 * keeps auto_reset = 1.  Rides mp_restore, recognised by its size: `bytes` = sizeof(MpStepActive),
 * `host_buf` a HOST MpStepActive with struct_size set to it.  include/mp_step_active.h wraps it as
 * inline C functions.  Every other request and entry point keeps doing exactly what it does.
 *
 * `active` is device memory, uint8 [K][N]; any non-zero byte means "active".  active_step_bytes is
 * the distance between two steps' rows: 0 means the same [N] row is read at every step, otherwise
 * it is >= N; larger distances let several engines read their own columns of one [K][N total]
 * tensor, as actions_step_bytes does.  steps = 1 is the masked single step; num_rows = 0 is
 * allowed; the five kinds of MpStepMany are named as rows of their MpObsKind.
 *
 * In step k:
 *   an active world (active[k][w] != 0) does exactly what it does in an MpStepTrajectory request:
 *     step, auto-reset, registered episode start (rows[w] read at that moment), frozen step, or
 *     nothing for a world never reset.  The action of an auto-reset step is ignored as ever.
 *   a skipped world is not touched: no byte of its record (the cached visiting orders, ctr[],
 *     reward_fx and done included), none of its elements of any in-place or bound non-pixel
 *     output, none of its event rows.  It adds nothing to mp_counters.  A world paused on LAST
 *     stays on LAST and takes its reset, or its registered start, in the first later step in which
 *     it is active.
 * The defining identity: a K-step request with a mask leaves every record, counter, in-place or
 * bound output, event row and per-step row exactly as the loop of K one-step requests with the
 * rows active[0] .. active[K - 1] leaves them.
 * Per-step rows (every kind of MpStepTrajectory, MP_STEP_ROW_STATE and MP_STEP_ROW_HASH) follow
 * the carry rule above: row k of a skipped step equals row k - 1, and row 0 equals the buffer as
 * it was before the request.  The rewards of a skipped step therefore REPEAT: a caller that sums
 * them multiplies by the mask.  A state row or hash row of a skipped step holds the unchanged
 * record or its hash.
 * Bound pixel views are drawn once after the request by the draw-only launches, for all worlds: a
 * skipped world's pixels are redrawn from its unchanged record and hold the same bytes.  The call
 * is therefore the step kernels plus one draw per view, whatever MpInfo.fused says, and it does
 * not change MpInfo.fused: the mask is per call, not a registration, and the engine's next
 * unmasked step is the launch it was.
 *
 * Refused before any launch, the engine left as it was.  MP_ERR_INVALID: everything
 * MpStepTrajectory refuses, with this request's name; NULL active; an active_step_bytes that is
 * neither 0 nor >= N; an `active` that is not device memory of the engine's device or whose extent
 * [active, active + (steps - 1) * active_step_bytes + N) does not lie inside one allocation;
 * non-zero reserved words.  MP_ERR_UNSUPPORTED: a rollout ring is bound (mp_bind_output_ring: a
 * slot row of a skipped world has no defined content); an engine created with MpConfig.unfused = 2
 * that has a pixel view bound (it promised one launch a step). */
typedef struct {
  uint32_t struct_size;        /* = sizeof(MpStepActive) */
  int32_t steps;               /* K */
  int32_t fields;              /* 0: discrete ids [K][N][P]; 1: raw fields [K][N][P][A] */
  int32_t num_rows;
  const int32_t* actions;      /* device */
  uint64_t actions_step_bytes; /* 0: the same block every step */
  const MpStepRow* rows;       /* HOST array [num_rows] */
  const uint8_t* active;       /* device uint8 [K][N]: non-zero = world w runs step k */
  uint64_t active_step_bytes;  /* 0: the same row every step; otherwise >= N */
  uint64_t reserved[5];        /* 0 */
} MpStepActive;

/* Stopping worlds inside a K-step request: an MpStepActive request in which a world that ends its
 * episode, or is paid, stops THERE for the rest of the request — returns that end with the
 * episode, "repeat this action until something happens", closed-loop evaluation without a host
 * synchronisation per step.  Rides mp_restore, recognised by its size: `bytes` =
 * sizeof(MpStepUntil), `host_buf` a HOST MpStepUntil with struct_size set to it.
 * include/mp_step_until.h wraps it as inline C functions.  Every other request and entry point
 * keeps doing exactly what it does; an MpStepActive request runs the kernels it ran.
 *
 * The ten leading fields are MpStepActive's, at its offsets, with one difference: `active` may be
 * NULL, which is a mask of all ones (active_step_bytes is then ignored and must be 0).
 *
 * The defining identity: the request equals the loop over k of the one-step MpStepActive request
 * with the mask
 *     m_k[w] = active[k][w] != 0 && stopped[w] == 0
 * where, after each such step, for the worlds that ran it,
 *     reason = (MP_STOP_LAST   if STEP_TYPE[w] == 2 after the step and `stop` has the bit)
 *            | (MP_STOP_REWARD if REWARD[w][p] != 0 for some player p after the step, likewise)
 *     if (reason) stopped[w] = reason
 * Everything MpStepActive says of a skipped world-step holds for the steps a stopped world skips:
 * it is not touched, its rows repeat by the carry rule, it stands on the step that stopped it, and
 * a world stopped on LAST takes its reset, or its registered episode start, in the first active
 * step of a later request in which its `stopped` byte is 0.  A world frozen on LAST
 * (MpConfig.auto_reset = 0) that runs a step is left on LAST with reward 0, so with MP_STOP_LAST it
 * stops again after one step.  A world never reset runs nothing and never stops.
 *
 *   stopped  device uint8 [N], read and written, or NULL.  On entry any non-zero byte means "this
 *            world does not run in this request"; that byte is left as it is.  A world that stops
 *            gets its reason bits.  One tensor handed to request after request makes a condition
 *            persistent: chunks of a long plan, K = 1 closed loops, action repeat.  NULL: every
 *            world starts unstopped and the reasons are not kept.
 *   ran      device int32 [N], written, or NULL: the number of steps world w ran in this request.
 *   returns  device float64 [N][P], written, or NULL: the discounted sum of REWARD over the steps
 *            that ran, in step order — g = 1; for each step that ran: ret = ret + g * r;
 *            g = g * gamma — every multiply and every add rounded to float64 on its own (no fused
 *            multiply-add), so it equals that loop in IEEE arithmetic bit for bit.  It is this
 *            request's sum: a caller that chunks a plan adds the chunks' sums itself.
 * stop = 0 with ran / returns is MpStepActive plus the count and the sum under the mask.
 * Bound pixel views are drawn once after the request for all worlds, and MpInfo.fused stays what
 * it was, as for MpStepActive.
 *
 * Refused before any launch, the engine left as it was.  MP_ERR_INVALID: everything MpStepActive
 * refuses (but a NULL active), with this request's name; stop outside the two bits; non-zero pad
 * or reserved words; a gamma that is not finite; a NULL active with a non-zero active_step_bytes;
 * stopped, ran or returns that is not device memory of the engine's device or whose extent (N, 4 N
 * and 8 N P bytes) does not lie inside one allocation; a ran that is not 4-byte or a returns that
 * is not 8-byte aligned; stopped, ran or returns overlapping each other, the actions, the mask or a
 * row buffer of the request (they are written while other worlds' waves still read and write
 * those).  MP_ERR_UNSUPPORTED: a rollout ring is bound; an engine created with
 * MpConfig.unfused = 2 that has a pixel view bound. */
enum {
  MP_STOP_LAST = 1,     /* the step left STEP_TYPE == 2 */
  MP_STOP_REWARD = 2,   /* the step left a non-zero REWARD for some player */
};
typedef struct {
  uint32_t struct_size;        /* = sizeof(MpStepUntil) */
  int32_t steps;               /* K */
  int32_t fields;              /* 0: discrete ids [K][N][P]; 1: raw fields [K][N][P][A] */
  int32_t num_rows;
  const int32_t* actions;      /* device */
  uint64_t actions_step_bytes; /* 0: the same block every step */
  const MpStepRow* rows;       /* HOST array [num_rows] */
  const uint8_t* active;       /* device uint8 [K][N], or NULL: all ones */
  uint64_t active_step_bytes;  /* 0: the same row every step; otherwise >= N */
  uint32_t stop;               /* MP_STOP_* bits; 0: nothing stops a world */
  uint32_t pad;                /* 0 */
  uint8_t* stopped;            /* device uint8 [N], read and written, or NULL */
  int32_t* ran;                /* device int32 [N], written, or NULL */
  double* returns;             /* device float64 [N][P], written, or NULL */
  double gamma;                /* finite; 1.0: the plain sum */
  uint64_t reserved[5];        /* 0 */
} MpStepUntil;

/* Stepping the worlds a device index list names: an MpStepUntil request whose launch has one wave
 * per ENTRY of the list instead of one per world of the engine — a tree search or a population
 * that keeps a pool of N worlds and acts on M of them a round hands over [K][M][P] actions and
 * gets [K][M] rows back, and the launch is ceil(M / 4) workgroups whatever N is.  Rides
 * mp_restore, recognised by its size: `bytes` = sizeof(MpStepListed), `host_buf` a HOST
 * MpStepListed with struct_size set to it.  include/mp_step_listed.h wraps it as inline C
 * functions.  Every other request and entry point keeps doing exactly what it does, and an engine
 * that never gets a list allocates nothing for it.
 *
 * The leading fields are MpStepUntil's, at its offsets; then `worlds`, device int32 [count], read
 * in place by the launch: entry i is stepped by wave i.  count = M is the host's; nothing about
 * the geometry is read from device memory.
 *
 * The defining identity.  Let mask[k][w] = 1 iff some entry i has worlds[i] == w and
 * active[k][i] != 0 (all ones with a NULL active), and full_actions[k][worlds[i]] = actions[k][i].
 * The request leaves every record, counter (mp_counters), in-place or bound non-pixel output,
 * event row and `stopped` byte exactly as the MpStepUntil request over all N worlds with that mask
 * and those actions leaves them.  Every per-call tensor is the gather of that request's:
 *   actions  [K][M][P] ([K][M][P][A] with fields = 1); actions_step_bytes as ever, sized for M.
 *   active   device uint8 [K][M] (active_step_bytes 0: one row [M] for every step; otherwise
 *            >= M), or NULL: all ones.
 *   rows     every kind's row k is [M][...]: row[k][i] == full_row[k][worlds[i]], the carry rule
 *            included (row 0 of a skipped step is carried from the world's in-place buffer into
 *            column i).  MP_STEP_ROW_STATE rows are [M][S], MP_STEP_ROW_HASH rows u64 [M].
 *   ran      device int32 [M], returns device float64 [M][P]: by entry.
 *   stopped  the exception: uint8 [N], indexed by WORLD, as argument and as result — the one
 *            tensor meant to persist over requests, which may name different lists.
 * The episode-start registration (rows [N]), next_orders and every in-place buffer are by world,
 * as ever.  An unlisted world is a skipped world in every step: nothing of it is touched.  Bound
 * pixel views are redrawn once after the request for all N worlds, as for a masked request;
 * MpInfo.fused and the next unlisted step are what they were.
 *
 * Bad entries.  worlds[i] outside [0, N) is never used as an index.  An entry that repeats an
 * earlier entry's world runs nothing: the lowest i steps the world (ownership is decided by a
 * small claim launch in front of the step kernels, so two waves never hold one record).  In both
 * cases element i of every per-call tensor (rows, ran, returns) is left as it was, and the next
 * synchronising call returns MP_ERR_INVALID once, naming this request, the entry and the value
 * (one of several bad entries is named); the engine stays usable.
 *
 * Refused before any launch, the engine left as it was.  MP_ERR_INVALID: everything MpStepUntil
 * refuses, with this request's name and the extents sized for M; NULL worlds; count < 1 or
 * count > N (more entries than worlds must repeat one); a worlds that is not 4-byte aligned
 * device memory of the engine's device with [worlds, worlds + count) inside one allocation; a
 * worlds that overlaps a row buffer, stopped, ran or returns; non-zero reserved words.
 * MP_ERR_UNSUPPORTED, as for a mask: a rollout ring is bound; an engine created with
 * MpConfig.unfused = 2 that has a pixel view bound. */
typedef struct {
  uint32_t struct_size;        /* = sizeof(MpStepListed) */
  int32_t steps;               /* K */
  int32_t fields;              /* 0: discrete ids [K][M][P]; 1: raw fields [K][M][P][A] */
  int32_t num_rows;
  const int32_t* actions;      /* device */
  uint64_t actions_step_bytes; /* 0: the same block every step */
  const MpStepRow* rows;       /* HOST array [num_rows]; every buffer has M columns */
  const uint8_t* active;       /* device uint8 [K][M], or NULL: all ones */
  uint64_t active_step_bytes;  /* 0: the same row every step; otherwise >= M */
  uint32_t stop;               /* MP_STOP_* bits; 0: nothing stops a world */
  uint32_t pad;                /* 0 */
  uint8_t* stopped;            /* device uint8 [N] (by world), read and written, or NULL */
  int32_t* ran;                /* device int32 [M], written, or NULL */
  double* returns;             /* device float64 [M][P], written, or NULL */
  double gamma;                /* finite; 1.0: the plain sum */
  uint64_t reserved[5];        /* 0 */
  const int32_t* worlds;       /* device int32 [count]: the world of entry i */
  int32_t count;               /* M: 1 <= M <= N */
  int32_t reserved2;           /* 0 */
  uint64_t reserved3[3];       /* 0 */
} MpStepListed;

/* Episode statistics on the device: per-player returns, episode lengths and per-player event counts
 * of every finished episode, folded into tensors the caller owns by ONE launch of k_episode_stats
 * behind every submission — no event row ever goes to the host.  Rides mp_restore, recognised by its
 * size: `bytes` = sizeof(MpEpisodeStats), `host_buf` a HOST MpEpisodeStats with struct_size set to
 * it.  include/mp_episode_stats.h wraps the four ops as inline C functions.
 *
 * A column (MpEventColumn) counts the events of one MpEventType per credited player: the 1-based
 * player is ((payload >> player_shift) & player_mask) of payload a (player_payload = 0) or b (1); a
 * value outside [1, P] credits nobody.  filter_payload != 0 adds the test
 * ((payload >> filter_shift) & filter_mask) == filter_value on payload a (1) or b (2): ore type,
 * item, class, mushroom type, level, coin types, and the halves of the packed payloads of types 15
 * and 16.  A PAIR column also takes a second 1-based player, ((other >> other_shift) & other_mask)
 * of the OTHER payload, and counts into [P][P] at (credited, other); an event whose second player is
 * outside [1, P] is not counted.  At most MP_STATS_MAX_COLUMNS columns and MP_STATS_MAX_PAIRS pair
 * columns; shifts < 32.
 *
 * The statistics, device tensors with the world axis leading (C = num_columns, C2 = num_pairs):
 *   open u8 [N]; episodes i32 [N]; dropped i32 [N];
 *   running, last: returns f64 [N][P], length i32 [N], counts i32 [N][C][P], pairs i32 [N][C2][P][P];
 *   total:         returns f64 [N][P], length i64 [N], counts i64 [N][C][P], pairs i64 [N][C2][P][P].
 * (counts may be NULL with C = 0, pairs with C2 = 0.)
 *
 * The rule, for one world and one step that ran, with the STEP_TYPE st, the REWARD r[P] and the
 * event rows E the step left (tally(E): every row the header counts, against every column):
 *   st == FIRST (reset, auto-reset step, load, registered start):
 *       running := 0, open := 1, running.counts / pairs += tally(E)
 *   otherwise, if open:
 *       running.returns[p] += r[p] (one f64 add a step, in step order), running.length += 1,
 *       running.counts / pairs += tally(E);
 *       if st == LAST: last := running, total += running, episodes += 1, open := 0
 *   otherwise nothing (a frozen world on LAST, a row loaded from a finished episode into a world
 *   with no open episode, an episode not seen from its FIRST).
 *   dropped += E's header `dropped`, on every step that ran.
 * An episode cut short by mp_reset, or by a load of a row that is not finished, is dropped: both
 * write FIRST, its running is zeroed, nothing is counted.  The exception, which follows from the
 * rule as it stands: a load of a row saved from a FINISHED episode writes LAST with zero rewards and
 * no events, so in a world whose episode is open it takes the "otherwise, if open" branch — the open
 * episode is closed as if that load were its last step: running.length += 1, last := running,
 * total += running, episodes += 1, open := 0.  A caller that loads finished rows over running
 * episodes and wants them left out subtracts `last` of those worlds from `total` after the load.
 * One wave owns a world's statistics and walks its steps in order; there is no global atomic, so
 * every value is bitwise reproducible.
 *
 * Which steps ran: a world never reset ran nothing; a masked mp_reset: the mask; MP_STATES_LOAD: the
 * worlds whose src[w] is a row; MpStepMany / MpStepTrajectory: all K steps; MpStepActive: the steps
 * whose mask byte is non-zero; MpStepUntil / MpStepListed: the first ran[i] active steps of column i
 * (a list: of the entries that own their world, statistics by world worlds[i], rows by column i).
 *
 * MP_STATS_REGISTER (eng != NULL): from now on every submission (mp_reset, mp_step*, the K-step
 *   requests, MP_STATES_LOAD) is followed on the engine's stream, without synchronisation, by one
 *   launch that folds what the submission wrote into the tensors named here, read and written in
 *   place; the caller keeps them alive and zeroes them first (or not: they are accumulators).  A
 *   single step reads the engine's in-place (or bound, or ring-slot) REWARD, STEP_TYPE and EVENTS.
 *   A K-step request on a registered engine must name the REWARD and STEP_TYPE rows, the EVENTS row
 *   when C + C2 > 0 (without one `dropped` is not counted for that request), and, for MpStepUntil and
 *   MpStepListed, `ran`: MP_ERR_INVALID before any launch otherwise.  mp_tune's probes are not
 *   folded.  The registration is engine configuration: a snapshot does not carry it.
 * MP_STATS_CLEAR (eng != NULL): the engine issues exactly the launches it issued before.
 * MP_STATS_TALLY (eng != NULL): the pure tally, no episode logic.  `events` is device int32
 *   [steps][count][MP_EVENT_ROWS][4]; running.counts (device int32 [count][C][P]) and running.pairs
 *   (device int32 [count][C2][P][P]) := the tally over the steps that ran: all, or those with a
 *   non-zero `active` byte (device u8 [steps][count], or NULL), of them the first ran[i] (device i32
 *   [count], or NULL).  Everything else of the request is ignored.  Enqueued, no synchronisation.
 * MP_STATS_HOST (eng == NULL): the rule above applied by the same functions compiled for the host
 *   to HOST rows — step_type i32 [steps][count], reward f64 [steps][count][num_players], events i32
 *   [steps][count][MP_EVENT_ROWS][4] (NULL with no columns), active / ran as for the tally — over
 *   HOST statistics of `count` worlds.  No device is touched.
 * Refused before any launch, MP_ERR_INVALID: a wrong struct_size, an unknown op, num_columns or
 * num_pairs outside their limits, NULL columns with a count > 0, a shift >= 32, a payload selector
 * out of range, non-zero reserved words; a NULL tensor the op needs; REGISTER / TALLY: a tensor
 * that is not device memory of the engine's device, whose extent is not inside one allocation, or
 * that is not aligned to its element; TALLY / HOST: steps or count < 1, HOST: num_players outside
 * [1, 16]. */
#define MP_STATS_MAX_COLUMNS 32
#define MP_STATS_MAX_PAIRS 4
enum { MP_STATS_REGISTER = 1, MP_STATS_CLEAR = 2, MP_STATS_TALLY = 3, MP_STATS_HOST = 4 };
typedef struct {
  int32_t type;            /* MpEventType */
  uint8_t player_payload;  /* 0: the credited player is in payload a; 1: in b */
  uint8_t player_shift;
  uint8_t filter_payload;  /* 0: no test; 1: test payload a; 2: test payload b */
  uint8_t filter_shift;
  uint32_t player_mask;
  uint32_t filter_mask;
  uint32_t filter_value;
  uint8_t other_shift;     /* pair columns: the second player, from the other payload */
  uint8_t reserved[3];     /* 0 */
  uint32_t other_mask;
  uint32_t reserved2;      /* 0 */
} MpEventColumn;
typedef struct {
  double* returns;         /* f64 [N][P] */
  void* length;            /* i32 [N] (total: i64 [N]) */
  void* counts;            /* i32 [N][C][P] (total: i64) */
  void* pairs;             /* i32 [N][C2][P][P] (total: i64) */
} MpStatsBank;
typedef struct {
  uint32_t struct_size;    /* = sizeof(MpEpisodeStats) */
  int32_t op;              /* MP_STATS_* */
  int32_t num_columns;     /* C  <= MP_STATS_MAX_COLUMNS */
  int32_t num_pairs;       /* C2 <= MP_STATS_MAX_PAIRS */
  const MpEventColumn* columns; /* HOST [num_columns] */
  const MpEventColumn* pairs;   /* HOST [num_pairs] */
  uint8_t* open;           /* u8 [N] */
  int32_t* episodes;       /* i32 [N] */
  int32_t* dropped;        /* i32 [N] */
  MpStatsBank running, last, total;
  /* TALLY and HOST: the rows */
  int32_t steps;           /* K */
  int32_t count;           /* the rows' columns (worlds) */
  int32_t num_players;     /* HOST: P */
  int32_t reserved;        /* 0 */
  const int32_t* step_type;
  const double* reward;
  const int32_t* events;
  const uint8_t* active;   /* u8 [steps][count], or NULL */
  const int32_t* ran;      /* i32 [count], or NULL */
  uint64_t reserved2[2];   /* 0 */
} MpEpisodeStats;

/* Throughput / event counters accumulated on device since creation
 * (synchronises).  These are what the multi-GPU bench all-reduces. */
enum {
  MP_CTR_WORLD_STEPS = 0, MP_CTR_AGENT_STEPS, MP_CTR_EPISODES,
  MP_CTR_REWARD_SUM /* in 1/1024 reward units */, MP_CTR_ZAPS, MP_CTR_AUX0
  /* clean_up: cleans; externality_mushrooms: (marking, frame) pairs in which a sanctions marking
     was on the map away from its living avatar (avatar_library.lua:1099-1110: connected at a
     distance) — a statistic */, MP_CTR_RESPAWNS, MP_CTR_BAD_ACTIONS, MP_CTR_COUNT
};
int mp_counters(MpEngine* eng, uint64_t out[MP_CTR_COUNT]);

/* Blocks until all work submitted on the engine's stream has finished. */
int mp_sync(MpEngine* eng);

/* Device memory for a view the caller is going to bind (unbind it before freeing
 * it).  chunk_bytes == 0: one hipMalloc.  chunk_bytes > 0: one virtual range mapped
 * onto separately created physical chunks of that size (HIP's virtual-memory API) —
 * another placement of the same bytes, and the speed of every step depends on where
 * the bound view lies (profiles/r04_write_fronts.md: the same launch, 99 - 122 us; a
 * property of the buffer's physical pages that no write order of the engine's removes).
 * (No reference counterpart: dmlab2d returns host arrays.) */
int mp_alloc_output(int device, uint64_t bytes, uint64_t chunk_bytes, void** out);
/* (views mapped from separately created 2 MB chunks are what the engine allocates for itself:
 * a physically contiguous view is written 25 - 45 % slower by the frame launch,
 * profiles/r05_alloc_method.md) */
/* (a mapped view's physical memory is released; its virtual range stays reserved for
 * the life of the process: reused ranges were seen to keep stale translations.  The
 * retired total is MpInfo.retired_va_bytes; mp_alloc_output / mp_place_output refuse to
 * map more once it would pass MpInfo.retired_va_limit — 16 TiB unless
 * mp_set_retired_va_limit says otherwise — with MP_ERR_HIP and a message that says so) */
int mp_free_output(int device, void* ptr);
int mp_set_retired_va_limit(int64_t bytes);
/* The two callbacks torch.cuda.memory.CUDAPluggableAllocator wants (signatures are
 * torch's): memory for a CALLER's tensors from the same scattered 2 MB chunks the engine
 * maps its own views from (requests of 32 MB and more; smaller ones are plain hipMalloc) —
 * a learner that must own the buffer it binds gets the engine's placement without handing
 * the allocation over.  meltingpot_amd/memory.py wraps them in a torch MemPool. */
void* mp_torch_alloc(long size, int device, void* stream);
void mp_torch_free(void* ptr, long size, int device, void* stream);

/* The plan follows the buffer.  Times the engine's candidate launch plans on the
 * pixel views bound right now and keeps the fastest for them (synchronises).  An
 * engine nothing has been done with yet (no reset, step or restore: the usual moment
 * to bind) is really stepped for it — all worlds reset, a few steps of uniformly random
 * actions per plan —
 * behind a device-side copy of the records, the counters and the engine's scalar outputs
 * that is put back on every path out of the call (the caller's bound scalar outputs are
 * unbound for the duration: nothing of the caller's but the pixel views being timed is
 * written); without room for that copy the probe runs dry; an
 * engine in use is timed dry (every bound view drawn exactly as a step draws it, no
 * world stepped, no record or scalar output written); a plan replaces the stock one
 * only by a margin (3 % stepped, 6 % dry).  Results never depend on the plan (ring depth,
 * worlds per batch, pooled share, store policy: frame.hip plan_frame); on an output
 * buffer the memory side serves unevenly a pooled plan is 3 - 8 % faster (sc1 stores
 * 13 % for commons_harvest), on an even one they are slower.  `us_per_launch` (may be NULL): the kept plan's time.  A no-op without a
 * bound pixel view, and for an engine created with MpConfig.dev (explicit plans).
 * With pixel views bound as a ring every slot is timed (it is its own buffer) and keeps its
 * own plan (us_per_launch: their mean) — the timed launches DRAW into the slots, so tune a
 * ring before the rollout it is going to hold.  Work in flight finishes first (a tune
 * between two steps is legal and leaves the records as they were). */
int mp_tune(MpEngine* eng, double* us_per_launch);

/* What mp_place_output measured. */
typedef struct {
  int32_t candidates;   /* buffers tried */
  int32_t picked;       /* index of the one kept */
  float us[32];         /* time per launch of each under the plan that suits it, us */
  int32_t stepped;      /* 1: timed with real steps behind a copy of the state (an engine
                           nothing had been done with AND room for the copy), 0: dry launches */
  /* (ABI 6) */
  int32_t requested;    /* candidates asked for (clamped to 1 .. 32, and to what max_bytes allows) */
  int32_t out_of_memory; /* > 0: a candidate could not be mapped (device memory, or the bound on
                           retired address space) and the probe went on with the ones it had */
  int32_t early_exit;   /* why fewer than `requested` were tried: 1 = a round (the first: eight) of candidates
                           all within 3 % (no lottery to win for this view on this box), 2 = a
                           candidate 8 % below the median was found, 0 = neither */
  float setup_ms;       /* wall time of the whole call: set-up cost a caller pays once */
} MpPlacement;

/* Allocates the output buffer of `kind` where this engine writes it fastest, and
 * binds it.  Up to `candidates` (<= 32) buffers of mp_obs_bytes(kind), each mapped
 * from 2 MB physical chunks — another scatter of pages each —, at most `max_bytes`
 * of them alive at any time (0: a quarter of the device's free memory; at least two
 * candidates are compared if memory allows), in rounds of up to twelve — a further
 * round only while no candidate stands out (8 % below the median); each is bound,
 * tuned (mp_tune) and timed; the fastest stays bound and is returned in *device_ptr,
 * the others are released before the call returns.  The caller frees the result with mp_free_output
 * after unbinding it (mp_bind_output(kind, NULL)) or destroying the engine.
 * A caller that binds its OWN buffer gets that buffer's speed; mp_tune is what it
 * can still do.  Synchronises.  Whatever happens — an error half way included — the engine's
 * records, counters and scalar outputs (its own and the caller's bound ones) are what they
 * were before the call, every candidate but the one returned is released, and on an error the
 * kind is bound to what it was bound to.  MP_ERR_INVALID when max_bytes does not hold one
 * view; when memory runs out half way the probe goes on with what it has and says so in
 * MpPlacement.out_of_memory. */
int mp_place_output(MpEngine* eng, MpObsKind kind, int32_t candidates, uint64_t max_bytes,
                    void** device_ptr, MpPlacement* report);

/* What the box's memory system gives the pixel view `kind` ON THE BUFFER BOUND RIGHT NOW
 * (a calibration for benchmark lines: the frame launch is HBM-write bound, boxes and buffers
 * differ — profiles/r05_alloc_method.md — and a line must be able to tell a slow box from a
 * regression).  Times, with events on the engine's stream, `reps` launches each of
 *   memset_us         hipMemsetAsync over the view (the runtime's own fill kernel);
 *   product_order_us  a bare store loop in the frame launch's write order: the current plan's
 *                     workgroups, each its own contiguous range of the view, its renderer
 *                     waves taking whole pass-sized spans (10 - 12 KB) from an LDS counter,
 *                     16-byte lane-contiguous non-temporal stores — no step, no drawing;
 *   front_4k_us       the same bytes as ONE chip-wide front of 4 KiB spans, one span per
 *                     workgroup and turn (the placement-insensitive order of
 *                     profiles/r05_kib_front.md).
 * OVERWRITES the view with junk (the next step or mp_observe redraws it); touches nothing
 * else of the engine.  Synchronises.  MP_ERR_INVALID unless `kind` is a pixel view bound with
 * mp_bind_output / mp_place_output (not a ring). */
typedef struct {
  uint64_t bytes;          /* the view's bytes = what each launch writes */
  float memset_us, product_order_us, front_4k_us;
  int32_t groups, waves;   /* the store loops' geometry: workgroups, storing waves each */
  uint32_t span_bytes;     /* product order: bytes per span (one renderer pass) */
} MpBoxFill;
int mp_box_fill(MpEngine* eng, MpObsKind kind, int32_t reps, MpBoxFill* out);

/* Diagnostics.  The frame kernel bounds every wait of its pipeline (2 s of wall
 * time); a wave that gives up records where in words 0-5 ({site, workgroup, wave,
 * batch, seen, wanted}; word 0 == 0: no stall), and every synchronising call above
 * reports it as MP_ERR_HIP until mp_reset(eng, seeds, NULL) — a reset of ALL
 * worlds — clears it (the worlds of a stalled launch are incomplete; resetting
 * them makes the engine usable again).  Word 8: 1 + the world that paid an
 * interaction reward outside every colour interval (the_matrix; reported once).
 * Words 9-11: an index a world-state launch skipped, or a row a checked load refused (word 9 =
 * world or position + 1, word 10 = the index or row, word 11 = what: 1 a load's src[], 2 a save's
 * world list, 3 an MpStatesObserve's rows[], 4 | rule << 8 a row an MpStatesCheck filter refused,
 * 5 an MpStatesCheck's rows[], 6 an MpStatesHash's rows[] or world list, 7 an MpStatesView's
 * rows[], 8 an MpStatesView's players[], 11 an MpEgoLayer's rows[], 12 an MpEgoLayer's players[], 13 an
 * MpViewHash's rows[], 14 an MpViewHash's players[], 15 an MpEgoPlanes' rows[], 16 an MpEgoPlanes'
 * players[], 17 an entry of an MpEgoPlanes' device class table (word 9 = the id + 1, word 10 = the
 * entry), 18 an MpAvatarIds' rows[], 19 an MpAvatarIds' players[] (9 and 10 are MpStepListed's worlds[])
 * — whose three words belong together); of several such reports
 * of one launch the three words may belong to different ones.  Words 12-15: the refused row of a checked load once more, claimed by ONE
 * refused world of the launch (word 12 = world + 1, 13 = the row, 14 = the rule, 15 = the offset
 * word), reported first.  Each is reported once by the next synchronising call (MP_ERR_INVALID)
 * and cleared.  The words live in host memory: this call never touches the
 * device, so it answers even while a kernel is stuck.  (Words 16.. are used by
 * the -DMP_FRAME_TRACE developer build.) */
int mp_fault_words(const MpEngine* eng, uint32_t out[64]);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* MP_ENGINE_H_ */
