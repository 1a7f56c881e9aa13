// frame_wpool.h — the frame launches that draw WORLD.RGB pooled by MP_WPOOL (2, 4 or 8;
// MpConfig.world_pool), alone or beside the per-agent view (full or pooled by its own factor).
// Included by one translation unit per factor, frame_wpool<k>.hip: the 15 k_frame
// instantiations per table type of the three factors compile in parallel with frame.hip's.
#pragma once
#include "frame_kernel.h"

#ifndef MP_WPOOL
#error "define MP_WPOOL (2, 4, 8) before including frame_wpool.h"
#endif

namespace {

template <int kW, class Tables, class Sites>
void launch_wpool_one(const DevTables& t, const Tables& c, const stepk::StepArgs& args,
                      uint8_t* out_a, uint8_t* out_w, const FramePlan& p, hipStream_t stream,
                      int pool_k) {
  const int pk = out_a && pool_k > 1 ? pool_k : 0;
  FrameConsts K = frame_consts(t, p, args.num_worlds, !std::is_same<Tables, NoTables>::value, pk, kW);
  const size_t lds = (size_t)K.lo.total;
  const dim3 grid(p.groups), block(p.nwaves * 64);
  if (!out_a) {
    K.npb_all = K.npb[1];
    hipLaunchKernelGGL((k_frame<Tables, Sites, 1, 0, kW>), grid, block, lds, stream, t, c, args,
                       out_a, out_w, K);
    return;
  }
  K.npb_all = K.npb[0] + K.npb[1];
  switch (pk) {
    case 2:
      hipLaunchKernelGGL((k_frame<Tables, Sites, 2, 2, kW>), grid, block, lds, stream, t, c, args,
                         out_a, out_w, K);
      break;
    case 4:
      hipLaunchKernelGGL((k_frame<Tables, Sites, 2, 4, kW>), grid, block, lds, stream, t, c, args,
                         out_a, out_w, K);
      break;
    case 8:
      hipLaunchKernelGGL((k_frame<Tables, Sites, 2, 8, kW>), grid, block, lds, stream, t, c, args,
                         out_a, out_w, K);
      break;
    default:
      hipLaunchKernelGGL((k_frame<Tables, Sites, 2, 0, kW>), grid, block, lds, stream, t, c, args,
                         out_a, out_w, K);
      break;
  }
}

template <int kW, class Tables, class Sites>
int allow_lds_wpool() {
  const void* k[5] = {
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 1, 0, kW>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 0, kW>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 2, kW>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 4, kW>),
      reinterpret_cast<const void*>(&k_frame<Tables, Sites, 2, 8, kW>)};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // namespace

template <int kWPool>
int prepare_frame_wpool() {
  int rc = allow_lds_wpool<kWPool, NoTables, NoSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, CleanUpTables, stepk::CleanUpSites>();
#if !defined(MP_FRAME_ISA_SUBSET)
  if (!rc) rc = allow_lds_wpool<kWPool, CommonsTables, stepk::CommonsSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, TerritoryTables, stepk::TerritorySites>();
  if (!rc) rc = allow_lds_wpool<kWPool, CoinsTables, stepk::CoinsSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, MatrixTables, stepk::MatrixSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, CoopTables, stepk::CoopSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, GiftTables, stepk::GiftSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, CookTables, stepk::CookSites>();
  if (!rc) rc = allow_lds_wpool<kWPool, MushroomTables, stepk::MushroomSites>();
#endif
  return rc;
}

template <int kWPool>
void launch_frame_wpool(const DevTables& t, const SubstrateTables* s, const stepk::StepArgs& args,
                        uint8_t* out_a, uint8_t* out_w, const FramePlan& p, hipStream_t stream,
                        int pool_k) {
  if (!s) {
    launch_wpool_one<kWPool, NoTables, NoSites>(t, NoTables(), args, out_a, out_w, p, stream, pool_k);
    return;
  }
#if defined(MP_FRAME_ISA_SUBSET)
  if (s->substrate == MPK_SUBSTRATE_CLEAN_UP)
    launch_wpool_one<kWPool, CleanUpTables, stepk::CleanUpSites>(t, s->cu, args, out_a, out_w, p, stream, pool_k);
#else
  switch (s->substrate) {
    case MPK_SUBSTRATE_CLEAN_UP:
      launch_wpool_one<kWPool, CleanUpTables, stepk::CleanUpSites>(t, s->cu, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COMMONS_HARVEST:
      launch_wpool_one<kWPool, CommonsTables, stepk::CommonsSites>(t, s->ch, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_TERRITORY:
      launch_wpool_one<kWPool, TerritoryTables, stepk::TerritorySites>(t, s->tr, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COINS:
      launch_wpool_one<kWPool, CoinsTables, stepk::CoinsSites>(t, s->co, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_THE_MATRIX:
      launch_wpool_one<kWPool, MatrixTables, stepk::MatrixSites>(t, s->mx, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COOP_MINING:
      launch_wpool_one<kWPool, CoopTables, stepk::CoopSites>(t, s->cm, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_GIFT_REFINEMENTS:
      launch_wpool_one<kWPool, GiftTables, stepk::GiftSites>(t, s->gr, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_COLLABORATIVE_COOKING:
      launch_wpool_one<kWPool, CookTables, stepk::CookSites>(t, s->cc, args, out_a, out_w, p, stream, pool_k);
      break;
    case MPK_SUBSTRATE_EXTERNALITY_MUSHROOMS:
      launch_wpool_one<kWPool, MushroomTables, stepk::MushroomSites>(t, s->em, args, out_a, out_w, p, stream, pool_k);
      break;
  }
#endif
}

template int prepare_frame_wpool<MP_WPOOL>();
template void launch_frame_wpool<MP_WPOOL>(const DevTables& t, const SubstrateTables* s,
                                           const stepk::StepArgs& args, uint8_t* out_a,
                                           uint8_t* out_w, const FramePlan& p, hipStream_t stream,
                                           int pool_k);
