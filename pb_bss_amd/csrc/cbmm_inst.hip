// Complex-Bingham mixture EM kernel and the Bingham parameter solve, one translation unit per
// sensor count D (compiled with -DPBBSS_EM_D=<D>), like cw_inst.hip.
#include "cbmm.hpp"
#include "cbmm_launch.hpp"
#include "em_launch.hpp"

#ifndef PBBSS_EM_D
#error "compile with -DPBBSS_EM_D=<sensors>"
#endif

namespace pbbss {

template <int K, typename YS, bool SPILL>
static int cb_launch_variant(BinghamArgs ba, const EmLaunchCfg& cfg, hipStream_t stream) {
  using Kern = BinghamKernel<PBBSS_EM_D, K, YS, SPILL>;
  const size_t lds = Kern::lds_bytes(ba.em.T);
  if (lds > cfg.lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  auto kfn = cbmm_em_kernel<PBBSS_EM_D, K, YS, SPILL>;
  if (!raise_lds_attribute(reinterpret_cast<const void*>(kfn), lds)) return PBBSS_ERR_HIP;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, kEmThreads, lds) != hipSuccess)
    return PBBSS_ERR_HIP;
  if (occ < 1) occ = 1;
  int64_t grid = (int64_t)cfg.num_cu * occ;
  if (grid > ba.em.B) grid = ba.em.B;
  if (SPILL) {  // frame arrays of each workgroup in HBM scratch (cw_inst.hip: cw_launch_variant)
    ba.em.scratch_stride = Kern::Base::scratch_bytes(ba.em.T);
    ba.em.scratch =
        static_cast<char*>(cfg.get_scratch(cfg.scratch_ctx, ba.em.scratch_stride * grid));
    if (!ba.em.scratch) return PBBSS_ERR_HIP;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, ba);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

// frames LDS-resident when they fit, else the spilled variant (long utterances)
template <int K, typename YS>
static int cb_launch_one(const BinghamArgs& ba, const EmLaunchCfg& cfg, hipStream_t stream) {
  if (BinghamKernel<PBBSS_EM_D, K, YS, false>::lds_bytes(ba.em.T) > cfg.lds_limit)
    return cb_launch_variant<K, YS, true>(ba, cfg, stream);
  return cb_launch_variant<K, YS, false>(ba, cfg, stream);
}

template <typename YS>
static int cb_launch_k(int K, const BinghamArgs& ba, const EmLaunchCfg& cfg, hipStream_t stream) {
  switch (K) {
    case 1: return cb_launch_one<1, YS>(ba, cfg, stream);
    case 2: return cb_launch_one<2, YS>(ba, cfg, stream);
    case 3: return cb_launch_one<3, YS>(ba, cfg, stream);
    case 4: return cb_launch_one<4, YS>(ba, cfg, stream);
    default: return PBBSS_ERR_UNSUPPORTED;
  }
}

#define PBBSS_CAT2(a, b) a##b
#define PBBSS_CAT(a, b) PBBSS_CAT2(a, b)

int PBBSS_CAT(cb_launch_d, PBBSS_EM_D)(int K, int y_is_c128, const BinghamArgs& ba,
                                       const EmLaunchCfg& cfg, hipStream_t stream) {
  return y_is_c128 ? cb_launch_k<double>(K, ba, cfg, stream)
                   : cb_launch_k<float>(K, ba, cfg, stream);
}

int PBBSS_CAT(cb_solve_launch_d, PBBSS_EM_D)(const double* s, int64_t N, double eps, double maxc,
                                             double* lam, int32_t* status, int num_cu,
                                             hipStream_t stream) {
  int64_t grid = (int64_t)num_cu * 8;
  if (grid > N) grid = N;
  hipLaunchKernelGGL(cbingham_find_eigenvalues_kernel<PBBSS_EM_D>, dim3((unsigned)grid),
                     dim3(kWave), 0, stream, s, N, eps, maxc, lam, status);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

}  // namespace pbbss
