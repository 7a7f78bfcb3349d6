// Power-of-two pre-scale of the stand-alone batched solvers (heev, gev, solve; beamform.hip,
// generic.hip, generic_bf.hip).  Kept out of pbbss_dev.hpp: the fused EM kernels do not use it.
#pragma once
#include "pbbss_dev.hpp"

namespace pbbss {

// Exponent e with which the stand-alone solvers work on 2^-e A instead of A:
// 0 (untouched, bit for bit the unscaled result) unless the largest entry `amax` lies outside
// [2^-400, 2^400], where the squares and products inside the solvers leave the float64 range.
__device__ __forceinline__ int pow2_prescale_exponent(double amax) {
  const bool out = (amax > 0x1p400 && amax < 1.79e308) || (amax > 0.0 && amax < 0x1p-400);
  return out ? ilogb(amax) : 0;
}

}  // namespace pbbss
