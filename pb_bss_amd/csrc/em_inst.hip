// One translation unit per sensor count D (compiled with -DPBBSS_EM_D=<D>) so the
// heavy persistent-EM template instantiates in parallel under `make -j`.
#include "cacgmm_em.hpp"
#include "em_launch.hpp"

#ifndef PBBSS_EM_D
#error "compile with -DPBBSS_EM_D=<sensors>"
#endif

namespace pbbss {

template <int D, int K, typename YS, bool SPILL>
static int launch_variant(EmArgs a, const EmLaunchCfg& cfg, hipStream_t stream) {
  using Kern = EmKernel<D, K, YS, SPILL>;
  const size_t lds = Kern::lds_bytes(a.T);
  if (lds > cfg.lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  auto kfn = cacgmm_em_kernel<D, K, YS, SPILL>;
  int occ = blocks_per_cu(kfn, kEmThreads, lds);
  if (occ < 0) return PBBSS_ERR_HIP;
  if (occ < 1) occ = 1;
  int64_t grid = (int64_t)cfg.num_cu * occ;
  if (grid > a.B) grid = a.B;
  if (SPILL) {
    a.scratch_stride = Kern::scratch_bytes(a.T);
    a.scratch = static_cast<char*>(cfg.get_scratch(cfg.scratch_ctx, a.scratch_stride * grid));
    if (!a.scratch) return PBBSS_ERR_HIP;
  }
  a.lds_given = (unsigned)lds;
  if (a.xcount) a.xbuf_given = (unsigned)cfg.xbuf_bytes;
  if (cfg.ev_t0) {
    hipExtLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, cfg.ev_t0,
                          cfg.ev_t1, 0, a);
  } else {
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, a);
  }
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

// Remainder problems [b_first, b_first + p.r) as split groups on `side`, concurrent with the main
// launch (with_side_stream).  prepare_split: the host half that does not touch the side stream.
template <int D, int K, typename YS>
static int prepare_split(const SplitPlan& p) {
  const size_t lds = EmKernel<D, K, YS, false>::lds_bytes(p.window);
  return raise_lds_attribute(cacgmm_em_split_kernel<D, K, YS>, lds) ? PBBSS_OK : PBBSS_ERR_HIP;
}
template <int D, int K, typename YS>
static int launch_split(EmArgs a, int64_t b_first, const SplitPlan& p, const EmLaunchCfg& cfg,
                        hipStream_t side) {
  const size_t lds = EmKernel<D, K, YS, false>::lds_bytes(p.window);
  auto kfn = cacgmm_em_split_kernel<D, K, YS>;
  stamp_split(a, cfg, p, b_first, cfg.split_prio);
  a.spin_limit = cfg.spin_limit;
  a.xbuf_given = (unsigned)cfg.xbuf_bytes;
  hipLaunchKernelGGL(kfn, dim3((unsigned)(p.r * p.G)), dim3(kEmThreads), lds, side, a);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

template <int D, int K, typename YS>
static int launch_one(const EmArgs& a, const EmLaunchCfg& cfg, hipStream_t stream) {
  using Kern = EmKernel<D, K, YS, false>;
  if (Kern::lds_bytes(a.T) > cfg.lds_limit)
    return launch_variant<D, K, YS, true>(a, cfg, stream);  // long utterance: frames in HBM/L2
  // Tail handling: the remainder problems go to split groups over many CUs (em_launch.hpp)
  const SplitRule rule{kSplitMinIterations, 3 * (int64_t)cfg.num_cu, kSplitNoLimit, true, false};
  const SplitPlan p = plan_split(a, cfg, rule, Kern::split_slab_doubles);
  if (!p.ok) return launch_variant<D, K, YS, false>(a, cfg, stream);
  EmArgs main_a = a;
  main_a.B = a.B - p.r;
  // The main launch goes out first (with_side_stream); the members are independent of the main
  // workgroups.  (hipExtAnyOrderLaunch -- the split kernel as a barrier-less packet of the SAME
  // queue -- would need neither stream nor events, but is documented as unsupported on gfx9.)
  return with_side_stream(
      cfg, stream,
      [&] {
        const int rc = launch_variant<D, K, YS, false>(main_a, cfg, stream);
        return rc != PBBSS_OK ? rc : prepare_split<D, K, YS>(p);
      },
      [&](hipStream_t side) { return launch_split<D, K, YS>(a, a.B - p.r, p, cfg, side); });
}

template <int D>
int em_launch_d(int K, int y_is_c128, const EmArgs& a, const EmLaunchCfg& cfg, hipStream_t stream) {
  return dispatch_em_k(K, y_is_c128, [&](auto k, auto y) {
    return launch_one<D, k(), decltype(y)>(a, cfg, stream);
  });
}
template int em_launch_d<PBBSS_EM_D>(int, int, const EmArgs&, const EmLaunchCfg&, hipStream_t);

}  // namespace pbbss
