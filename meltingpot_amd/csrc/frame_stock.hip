// frame_stock.hip — the frame kernels of the committed clean_up pack with its constants compiled
// in (stock.h): k_frame<CleanUpTables, ., kViews, 0, 0, StockCleanUp> for the three full views.
// The pooled views stay generic.  A translation unit of its own, compiled in parallel with
// frame.hip's; mp_create decides which engines launch these (SubstrateTables::stock).
#include "frame_kernel.h"
#include "stock.h"

namespace {

template <int kViews>
void launch_stock(const DevTables& t, const CleanUpTables& c, const stepk::StepArgs& args,
                  uint8_t* out_a, uint8_t* out_w, const FrameConsts& K, const FramePlan& p,
                  hipStream_t stream) {
  hipLaunchKernelGGL((k_frame<CleanUpTables, stepk::CleanUpSites, kViews, 0, 0, StockCleanUp>),
                     dim3(p.groups), dim3(p.nwaves * 64), (size_t)K.lo.total, stream, t, c, args,
                     out_a, out_w, K);
}

}  // namespace

int prepare_frame_stock() {
  const void* k[3] = {
      reinterpret_cast<const void*>(&k_frame<CleanUpTables, stepk::CleanUpSites, 0, 0, 0, StockCleanUp>),
      reinterpret_cast<const void*>(&k_frame<CleanUpTables, stepk::CleanUpSites, 1, 0, 0, StockCleanUp>),
      reinterpret_cast<const void*>(&k_frame<CleanUpTables, stepk::CleanUpSites, 2, 0, 0, StockCleanUp>)};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// launch_frame's stepping launch of the full views, for an engine whose pack is the stock one
// (t and c still travel as arguments: the kernel reads their pointers and unfolded members).
void launch_frame_stock(const DevTables& t, const CleanUpTables& c, const stepk::StepArgs& args,
                        uint8_t* out_a, uint8_t* out_w, const FramePlan& p, hipStream_t stream) {
  FrameConsts K = frame_consts(t, p, args.num_worlds, true, 0);
  if (out_a && out_w) {
    K.npb_all = K.npb[0] + K.npb[1];
    launch_stock<2>(t, c, args, out_a, out_w, K, p, stream);
  } else if (out_w) {
    K.npb_all = K.npb[1];
    launch_stock<1>(t, c, args, out_a, out_w, K, p, stream);
  } else {
    K.npb_all = K.npb[0];
    launch_stock<0>(t, c, args, out_a, out_w, K, p, stream);
  }
}
