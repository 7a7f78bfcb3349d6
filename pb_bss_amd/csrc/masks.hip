// Oracle masks (pb_bss/extraction/mask_module.py:90-550) on the device.
//
// Addressing.  The caller's array is never copied: pbbss_mask_geom carries four collapsed axes
// (sizes, element strides of the input and of the output) besides the source and the sensor
// stride, which covers (..., K, D, F, T) and (..., K, F, T, D) alike.  The last collapsed axis
// runs along the lanes, so loads and stores are coalesced where that axis is contiguous.
//
// Pointwise masks (mask_pointwise_kernel): one lane per TF point of one independent index.  The
// lane loads its K sources (pooling the D sensors of each), keeps them in registers, and writes
// the K mask values -- one read of the images, one write of the masks.  All arithmetic is float64
// on the widened input; the result is rounded once.  Powers are formed as the reference forms
// them (two products, one sum, sensors added in order, no fused multiply-add), so that binary
// decisions on exactly representable data agree bit for bit.
//
// Threshold masks (Lorenz :350-417, quantile :420-493) need an exact order statistic per row.
//   rows of at most kMaskSmallRow values: one launch, one workgroup per row, the values in LDS;
//     every element ranks itself against the row (counts, and for Lorenz the sum of the larger
//     elements, always in index order);
//   longer rows: value pass -> float64 workspace (rows, N); radix descent over the bit pattern
//     of the non-negative doubles (an order-preserving unsigned integer), 8 bits per level: a
//     histogram kernel writes per-workgroup partial counts (and sums), a pick kernel adds them in
//     a fixed order, chooses the bucket and narrows the prefix -- 8 x 2 launches; a successor
//     pass (smallest key above the selected one); a finish kernel (threshold and status); the
//     apply pass, which compares the SAME workspace values.
// No float atomics anywhere: a bucket's sum is accumulated by the one thread that owns the
// bucket, walking the workgroup's staged digits in index order.  No workgroup waits for another;
// launch boundaries are the only synchronisation.
#include "masks.hpp"
#include <limits>
#include "pbbss_dev.hpp"

// No fused multiply-adds the source does not spell out: binary decisions (ties of the binary
// mask, equal keys at a Lorenz crossing, s / s = 1 + 0i) must see the bits NumPy's separately
// rounded products and sums give.
#pragma clang fp contract(off)

namespace pbbss {
namespace {

constexpr int kMkThreads = 256;
constexpr int kMkStage = 2048;  // elements a histogram workgroup stages per step
constexpr unsigned long long kNoKey = ~0ull;

// One separately rounded product / sum.  These must be defined here, under the pragma: the
// toolkit's __dmul_rn and __dadd_rn are header inlines compiled outside it, keep the permission
// to contract, and fuse with each other once inlined (s / s then leaves the residual of the
// quotient in the imaginary part instead of 0).
__device__ __forceinline__ double mul_rn(double x, double y) { return x * y; }
__device__ __forceinline__ double add_rn(double x, double y) { return x + y; }

template <typename X2>
__device__ __forceinline__ void widen(const X2* p, double& re, double& im) {
  const X2 v = *p;
  re = (double)v.x;
  im = (double)v.y;
}

// re^2 + im^2 as NumPy evaluates x.real ** 2 + x.imag ** 2: three roundings
__device__ __forceinline__ double abs_square(double re, double im) {
  return add_rn(mul_rn(re, re), mul_rn(im, im));
}

// |re + i im| as NumPy's vector loop for np.abs of a complex array forms it on a machine with
// fused multiply-adds: larger * sqrt(fma(q, q, 1)), q = smaller / larger.  It is within two ulp
// of the magnitude, not correctly rounded, and the reference's np.abs(x) ** 2 carries exactly
// these bits into the Lorenz keys: integer-valued images, whose powers tie in exact arithmetic,
// come apart in the last place the same way here as there.
__device__ __forceinline__ double abs_complex(double re, double im) {
  const double a = fabs(re), b = fabs(im);
  if (a == std::numeric_limits<double>::infinity() || b == std::numeric_limits<double>::infinity())
    return std::numeric_limits<double>::infinity();
  if (a != a || b != b) return a + b;
  const double l = fmax(a, b), s = fmin(a, b);
  const double q = l == 0.0 ? 0.0 : s / l;
  return l * sqrt(fma(q, q, 1.0));
}

__device__ __forceinline__ unsigned long long key_of(double v) {
  return (unsigned long long)__double_as_longlong(v);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  return __longlong_as_double((long long)k);
}

struct Offsets {
  int64_t x, out;
  int64_t last;  // index along the last collapsed axis
};

// flat index over size[first .. 4) -> offsets
__device__ __forceinline__ Offsets offsets_of(const pbbss_mask_geom& g, int64_t idx, int first,
                                              int end) {
  Offsets o{0, 0, 0};
  for (int a = end - 1; a >= first; --a) {
    const int64_t q = idx / g.size[a];
    const int64_t r = idx - q * g.size[a];
    if (a == end - 1) o.last = r;
    o.x += r * g.x_stride[a];
    o.out += r * g.out_stride[a];
    idx = q;
  }
  return o;
}

template <typename O>
__device__ __forceinline__ void store_real(O* p, double v) {
  *p = (O)v;
}

// (a + ib) / (c + id) as NumPy divides complex numbers (Smith's method), operation for operation
// and without fused multiply-adds: s / s is 1 + 0i exactly, as it is there; 0 / 0 gives NaN
__device__ __forceinline__ void complex_div(double a, double b, double c, double d, double& re,
                                            double& im) {
  if (fabs(c) >= fabs(d)) {
    if (c == 0.0 && d == 0.0) {
      re = a / fabs(c);
      im = b / fabs(d);
    } else {
      const double rat = d / c, scl = 1.0 / add_rn(c, mul_rn(d, rat));
      re = mul_rn(add_rn(a, mul_rn(b, rat)), scl);
      im = mul_rn(add_rn(b, -mul_rn(a, rat)), scl);
    }
  } else {
    const double rat = c / d, scl = 1.0 / add_rn(mul_rn(c, rat), d);
    re = mul_rn(add_rn(mul_rn(a, rat), b), scl);
    im = mul_rn(add_rn(mul_rn(b, rat), -a), scl);
  }
}

template <typename X2, typename O, int MODE>
__global__ __launch_bounds__(kMkThreads) void mask_pointwise_kernel(
    const X2* __restrict__ x, O* __restrict__ out, pbbss_mask_geom g, double eps,
    const double* __restrict__ table, int64_t table_len, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (idx >= total) return;
  const Offsets o = offsets_of(g, idx, 0, 4);
  const int K = g.sources, D = g.sensors;
  constexpr bool kPower = MODE == PBBSS_MASK_IBM || MODE == PBBSS_MASK_WIENER ||
                          MODE == PBBSS_MASK_BIASED;
  double a[kMaskMaxK], b[kMaskMaxK];  // power, or the real and imaginary parts
#pragma unroll
  for (int k = 0; k < kMaskMaxK; ++k) {
    a[k] = 0.0;
    b[k] = 0.0;
    if (k < K) {
      const X2* xp = x + o.x + k * g.x_source_stride;
      if constexpr (kPower) {
        double re, im;
        widen(xp, re, im);
        double acc = abs_square(re, im);
        for (int d = 1; d < D; ++d) {
          widen(xp + d * g.x_sensor_stride, re, im);
          acc = add_rn(acc, abs_square(re, im));
        }
        a[k] = acc;
      } else {
        widen(xp, a[k], b[k]);
      }
    }
  }
  O* op = out + o.out;
  const int64_t ks = g.out_source_stride;

  if constexpr (MODE == PBBSS_MASK_IBM) {
    // np.argmax: the first NaN wins, else the first largest
    double bv = a[0];
    int bi = 0;
#pragma unroll
    for (int k = 1; k < kMaskMaxK; ++k)
      if (k < K && bv == bv && (a[k] > bv || a[k] != a[k])) {
        bv = a[k];
        bi = k;
      }
#pragma unroll
    for (int k = 0; k < kMaskMaxK; ++k)
      if (k < K) store_real(op + k * ks, k == bi ? 1.0 : 0.0);
  } else if constexpr (MODE == PBBSS_MASK_WIENER) {
    double tot = a[0];
#pragma unroll
    for (int k = 1; k < kMaskMaxK; ++k)
      if (k < K) tot = add_rn(tot, a[k]);
    const double den = tot + eps;
#pragma unroll
    for (int k = 0; k < kMaskMaxK; ++k)
      if (k < K) store_real(op + k * ks, a[k] / den);
  } else if constexpr (MODE == PBBSS_MASK_IRM) {
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < kMaskMaxK; ++k)
      if (k < K) {
        a[k] = abs_complex(a[k], b[k]);
        tot = k ? add_rn(tot, a[k]) : a[k];
      }
    const double den = tot + eps;
#pragma unroll
    for (int k = 0; k < kMaskMaxK; ++k)
      if (k < K) store_real(op + k * ks, a[k] / den);
  } else if constexpr (MODE == PBBSS_MASK_IAM || MODE == PBBSS_MASK_PSM ||
                       MODE == PBBSS_MASK_ICM) {
    double sr = a[0], si = b[0];
#pragma unroll
    for (int k = 1; k < kMaskMaxK; ++k)
      if (k < K) {
        sr = add_rn(sr, a[k]);
        si = add_rn(si, b[k]);
      }
    const double ao = abs_complex(sr, si);
#pragma unroll
    for (int k = 0; k < kMaskMaxK; ++k)
      if (k < K) {
        if constexpr (MODE == PBBSS_MASK_IAM) {
          store_real(op + k * ks, abs_complex(a[k], b[k]) / (ao + eps));
        } else if constexpr (MODE == PBBSS_MASK_PSM) {
          // |s| / (|o| + eps) * cos(angle s - angle o) without the angles
          // (|o| = 0: angle o = 0 and the reference is left with Re(s) / eps)
          store_real(op + k * ks,
                     ao == 0.0 ? a[k] / eps : (a[k] * sr + b[k] * si) / (ao * (ao + eps)));
        } else {
          double re, im;
          complex_div(a[k], b[k], sr, si, re, im);
          O v;
          v.x = (decltype(v.x))re;
          v.y = (decltype(v.y))im;
          op[k * ks] = v;
        }
      }
  } else {  // PBBSS_MASK_BIASED: K == 2, speech then noise
    const int64_t f = o.last % table_len;
    const double speech = a[0], noise = a[1];
    const double ts = speech / table[f], tn = speech / table[table_len + f];
    bool ms = ts > noise && ts > 0.005;
    bool mn = tn < noise || tn < 0.005;
    if (table[2 * table_len + f] != 0.0) {  // below low_cut / from high_cut on
      ms = false;
      mn = true;
    }
    op[0] = (O)ms;
    op[ks] = (O)mn;
  }
}

// ---- threshold masks -------------------------------------------------------------------------

// value of element n of row r: sensor-pooled |x|^2 (Lorenz: np.abs(x) ** 2 summed in sensor
// order) or |x| (quantile)
template <typename X2, bool LORENZ>
__device__ __forceinline__ double row_value(const X2* x, const pbbss_mask_geom& g, int64_t xoff) {
  double re, im;
  widen(x + xoff, re, im);
  double h = abs_complex(re, im);
  if constexpr (!LORENZ) return h;
  double acc = mul_rn(h, h);
  for (int d = 1; d < g.sensors; ++d) {
    widen(x + xoff + d * g.x_sensor_stride, re, im);
    h = abs_complex(re, im);
    acc = add_rn(acc, mul_rn(h, h));
  }
  return acc;
}

// NumPy's _lerp (lib/_function_base_impl.py): two roundings per branch, gamma == 0 returns a
__device__ __forceinline__ double lerp(double a, double b, double gamma) {
  const double diff = b - a;
  return gamma >= 0.5 ? add_rn(b, -mul_rn(diff, 1.0 - gamma))
                      : add_rn(a, mul_rn(diff, gamma));
}

template <typename O>
__device__ __forceinline__ void apply_point(O* op, double v, const double* thr,
                                            const MaskTargets& t, int64_t target_stride) {
  for (int j = 0; j < t.J; ++j) {
    const bool m = t.negative[j] ? v < thr[j] : v > thr[j];
    op[j * target_stride] = (O)(m ? t.high : t.low);
  }
}

// one workgroup per row, N <= kMaskSmallRow
template <typename X2, typename O, bool LORENZ>
__global__ __launch_bounds__(kMkThreads) void mask_small_row_kernel(
    const X2* __restrict__ x, O* __restrict__ out, pbbss_mask_geom g, MaskTargets t, int N,
    int32_t* __restrict__ status) {
  __shared__ double v[kMaskSmallRow];
  __shared__ unsigned long long best;
  __shared__ double sa[kMaskMaxQ], sb[kMaskMaxQ], thr[kMaskMaxQ];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const Offsets ro = offsets_of(g, row, 0, 2);
  __shared__ int has_nan;
  if (tid == 0) {
    best = kNoKey;
    has_nan = 0;
  }
  // A NaN in the row is neither below nor equal to anything, so the ranks need not cover every
  // target: an order statistic nobody claims stays NaN, and a row with a NaN gets NaN thresholds
  // altogether, which is NumPy's percentile of such a row.
  if (tid < kMaskMaxQ) sa[tid] = sb[tid] = std::numeric_limits<double>::quiet_NaN();
  __syncthreads();
  for (int n = tid; n < N; n += kMkThreads) {
    const Offsets co = offsets_of(g, n, 2, 4);
    const double val = row_value<X2, LORENZ>(x, g, ro.x + co.x);
    v[n] = val;
    if (val != val) has_nan = 1;
  }
  __syncthreads();
  if constexpr (LORENZ) {
    double total = 0.0;
    for (int j = 0; j < N; ++j) total += v[j];
    for (int n = tid; n < N; n += kMkThreads) {
      const double me = v[n];
      double above = 0.0;  // sum of the larger elements: the cumulative sum in front of `me`
      for (int j = 0; j < N; ++j) above += v[j] > me ? v[j] : 0.0;
      if ((above + me) / total < t.fraction) atomicMin(&best, key_of(me));
    }
    __syncthreads();
    if (tid == 0) {
      const bool ok = best != kNoKey;
      thr[0] = ok ? value_of(best) : std::numeric_limits<double>::quiet_NaN();
      status[row] = ok ? 0 : PBBSS_MASK_ST_NO_THRESHOLD;
    }
  } else {
    for (int n = tid; n < N; n += kMkThreads) {
      const double me = v[n];
      long long less = 0, equal = 0;
      for (int j = 0; j < N; ++j) {
        less += v[j] < me;
        equal += v[j] == me;
      }
      for (int j = 0; j < t.J; ++j) {
        const long long k = t.rank[j], k1 = k + 1 < N ? k + 1 : N - 1;
        if (less <= k && k < less + equal) sa[j] = me;
        if (less <= k1 && k1 < less + equal) sb[j] = me;
      }
    }
    __syncthreads();
    if (tid < t.J)
      thr[tid] = has_nan ? std::numeric_limits<double>::quiet_NaN()
                         : lerp(sa[tid], sb[tid], t.gamma[tid]);
    if (tid == 0) status[row] = 0;
  }
  __syncthreads();
  O* orow = out + ro.out;
  for (int n = tid; n < N; n += kMkThreads) {
    const Offsets co = offsets_of(g, n, 2, 4);
    apply_point(orow + co.out, v[n], thr, t, g.out_target_stride);
  }
}

// ---- long rows: workspace + radix descent ------------------------------------------------------

struct SelState {              // per (row, target)
  unsigned long long prefix;   // the resolved high bits of the key, right-aligned
  unsigned long long passed;   // elements on the far side of the range: below (quantile), above (Lorenz)
  unsigned long long equal;    // elements inside the range; after the last level: equal to the key
  unsigned long long succ;     // smallest key above the selected one (kNoKey: none)
  double sum_passed;           // Lorenz: sum of the elements above the range
  double total;                // Lorenz: sum of the row
};

struct RowGrid {  // block index -> (row, part)
  int parts;
  int64_t span;   // elements per part
};

template <typename X2, bool LORENZ>
__global__ __launch_bounds__(kMkThreads) void mask_value_kernel(const X2* __restrict__ x,
                                                                pbbss_mask_geom g, int64_t N,
                                                                int chunks,
                                                                double* __restrict__ vals) {
  const int64_t row = blockIdx.x / chunks;
  const int64_t n = (int64_t)(blockIdx.x % chunks) * kMkThreads + threadIdx.x;
  if (n >= N) return;
  const Offsets ro = offsets_of(g, row, 0, 2), co = offsets_of(g, n, 2, 4);
  vals[row * N + n] = row_value<X2, LORENZ>(x, g, ro.x + co.x);
}

// level l resolves bits [56 - 8 l, 64 - 8 l).  Block (row, j, part): thread b owns bucket b.
template <bool SUMS>
__global__ __launch_bounds__(kMkThreads) void mask_hist_kernel(
    const double* __restrict__ vals, int64_t N, int J, RowGrid rg, int level,
    const SelState* __restrict__ st, uint32_t* __restrict__ pcnt, double* __restrict__ psum) {
  __shared__ uint16_t s_dig[kMkStage];
  __shared__ double s_val[SUMS ? kMkStage : 1];
  __shared__ int s_any[kMkStage / kWave];
  const int tid = threadIdx.x;
  const int part = blockIdx.x % rg.parts;
  const int64_t rj = blockIdx.x / rg.parts;  // row * J + j
  const int64_t row = rj / J;
  const int shift = 56 - 8 * level;
  const unsigned long long prefix = level ? st[rj].prefix : 0ull;
  const int64_t begin = part * rg.span, end = min(N, begin + rg.span);
  const double* rv = vals + row * N;
  uint32_t cnt = 0;
  double sum = 0.0;
  for (int64_t base = begin; base < end; base += kMkStage) {
    for (int q = 0; q < kMkStage / kMkThreads; ++q) {
      const int i = q * kMkThreads + tid;
      const int64_t n = base + i;
      bool match = false;
      double val = 0.0;
      unsigned long long key = 0;
      if (n < end) {
        val = rv[n];
        key = key_of(val);
        match = level == 0 || (key >> (shift + 8)) == prefix;
      }
      s_dig[i] = match ? (uint16_t)((key >> shift) & 255u) : (uint16_t)0xffff;
      if constexpr (SUMS) s_val[i] = val;
      const unsigned long long any = __ballot(match);
      if ((tid & (kWave - 1)) == 0) s_any[i / kWave] = any != 0ull;
    }
    __syncthreads();
    for (int grp = 0; grp < kMkStage / kWave; ++grp) {
      if (!s_any[grp]) continue;  // uniform: every thread reads the same word
      for (int e = grp * kWave; e < (grp + 1) * kWave; ++e) {
        const bool mine = s_dig[e] == tid;
        cnt += mine;
        if constexpr (SUMS) sum += mine ? s_val[e] : 0.0;
      }
    }
    __syncthreads();
  }
  const int64_t slot = (rj * rg.parts + part) * 256 + tid;
  pcnt[slot] = cnt;
  if constexpr (SUMS) psum[slot] = sum;
}

template <bool LORENZ>
__global__ __launch_bounds__(kMkThreads) void mask_pick_kernel(
    const uint32_t* __restrict__ pcnt, const double* __restrict__ psum, int J, int parts,
    int level, MaskTargets t, SelState* __restrict__ st) {
  __shared__ unsigned long long c[256];
  __shared__ double s[256];
  const int tid = threadIdx.x;
  const int64_t rj = blockIdx.x;
  unsigned long long cnt = 0;
  double sum = 0.0;
  for (int p = 0; p < parts; ++p) {
    const int64_t slot = (rj * parts + p) * 256 + tid;
    cnt += pcnt[slot];
    if constexpr (LORENZ) sum += psum[slot];
  }
  c[tid] = cnt;
  s[tid] = sum;
  __syncthreads();
  if (tid != 0) return;
  SelState z = level ? st[rj] : SelState{0ull, 0ull, 0ull, kNoKey, 0.0, 0.0};
  int pick = -1;
  if constexpr (LORENZ) {
    if (level == 0) {
      double total = 0.0;
      for (int b = 255; b >= 0; --b) total += s[b];
      z.total = total;
    }
    // descending: buckets whose whole content stays below the fraction are passed
    int lowest = 0;
    for (int b = 255; b >= 0; --b) {
      if (!c[b]) continue;
      lowest = b;
      if ((z.sum_passed + s[b]) / z.total < t.fraction) {
        z.sum_passed += s[b];
        z.passed += c[b];
        continue;
      }
      pick = b;
      break;
    }
    if (pick < 0) {  // everything qualifies: the threshold is the smallest element
      pick = lowest;
      z.sum_passed -= s[lowest];
      z.passed -= c[lowest];
    }
  } else {
    const unsigned long long k = (unsigned long long)t.rank[rj % J];
    int highest = 0;
    for (int b = 0; b < 256; ++b) {
      if (!c[b]) continue;
      highest = b;
      if (z.passed + c[b] > k) {
        pick = b;
        break;
      }
      z.passed += c[b];
    }
    if (pick < 0) {  // rank beyond the row (refused by the entry point): the largest element
      pick = highest;
      z.passed -= c[highest];
    }
  }
  z.equal = c[pick];
  z.prefix = (z.prefix << 8) | (unsigned long long)pick;
  st[rj] = z;
}

// smallest key above the selected one
__global__ __launch_bounds__(kMkThreads) void mask_succ_kernel(const double* __restrict__ vals,
                                                               int64_t N, int J, RowGrid rg,
                                                               SelState* __restrict__ st) {
  __shared__ unsigned long long red[kMkThreads / kWave];
  const int tid = threadIdx.x;
  const int part = blockIdx.x % rg.parts;
  const int64_t rj = blockIdx.x / rg.parts;
  const int64_t row = rj / J;
  const unsigned long long u = st[rj].prefix;
  const int64_t begin = part * rg.span, end = min(N, begin + rg.span);
  unsigned long long m = kNoKey;
  for (int64_t n = begin + tid; n < end; n += kMkThreads) {
    const unsigned long long k = key_of(vals[row * N + n]);
    if (k > u && k < m) m = k;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off, kWave);
    m = o < m ? o : m;
  }
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kMkThreads / kWave; ++w) m = red[w] < m ? red[w] : m;
    if (m != kNoKey) atomicMin(&st[rj].succ, m);  // integer minimum: order-independent
  }
}

template <bool LORENZ>
__global__ __launch_bounds__(kMkThreads) void mask_finish_kernel(const SelState* __restrict__ st,
                                                                 int64_t rows, int J,
                                                                 MaskTargets t,
                                                                 double* __restrict__ thr,
                                                                 int32_t* __restrict__ status) {
  const int64_t rj = (int64_t)blockIdx.x * kMkThreads + threadIdx.x;
  if (rj >= rows * J) return;
  const SelState z = st[rj];
  const double u = value_of(z.prefix);
  if constexpr (LORENZ) {
    double th = u;
    int bad = 0;
    if (!((z.sum_passed + u) / z.total < t.fraction)) {
      // the first element of value u already fails: the crossing is the element above it
      if (z.passed > 0 && z.succ != kNoKey) {
        th = value_of(z.succ);
      } else {
        th = std::numeric_limits<double>::quiet_NaN();
        bad = PBBSS_MASK_ST_NO_THRESHOLD;
      }
    }
    thr[rj] = th;
    status[rj] = bad;
  } else {
    const int j = (int)(rj % J);
    const bool next_equal = z.passed + z.equal > (unsigned long long)t.rank[j] + 1ull;
    const double b = next_equal || z.succ == kNoKey ? u : value_of(z.succ);
    thr[rj] = lerp(u, b, t.gamma[j]);
    if (j == 0) status[rj / J] = 0;
  }
}

template <typename O>
__global__ __launch_bounds__(kMkThreads) void mask_apply_kernel(const double* __restrict__ vals,
                                                                const double* __restrict__ thr,
                                                                pbbss_mask_geom g, MaskTargets t,
                                                                int64_t N, int chunks,
                                                                O* __restrict__ out) {
  const int64_t row = blockIdx.x / chunks;
  const int64_t n = (int64_t)(blockIdx.x % chunks) * kMkThreads + threadIdx.x;
  if (n >= N) return;
  const Offsets ro = offsets_of(g, row, 0, 2), co = offsets_of(g, n, 2, 4);
  apply_point(out + ro.out + co.out, vals[row * N + n], thr + row * t.J, t, g.out_target_stride);
}

inline int mk_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

struct ThPlan {
  int64_t rows, N;
  bool small;
  RowGrid rg;
  size_t vals_b, state_b, pcnt_b, psum_b, thr_b;
};

ThPlan th_plan(const pbbss_mask_geom& g, const MaskTargets& t) {
  ThPlan p{};
  p.rows = g.size[0] * g.size[1];
  p.N = g.size[2] * g.size[3];
  p.small = p.N <= kMaskSmallRow;
  if (p.small) return p;
  // a part is a whole number of stages; at most 64 parts per row
  const int64_t stages = (p.N + kMkStage - 1) / kMkStage;
  const int64_t per = (stages + 63) / 64;
  p.rg.span = per * kMkStage;
  p.rg.parts = (int)((p.N + p.rg.span - 1) / p.rg.span);
  const size_t rj = (size_t)p.rows * t.J;
  p.vals_b = pad256((size_t)p.rows * p.N * sizeof(double));
  p.state_b = pad256(rj * sizeof(SelState));
  p.pcnt_b = pad256(rj * p.rg.parts * 256 * sizeof(uint32_t));
  p.psum_b = t.lorenz ? pad256(rj * p.rg.parts * 256 * sizeof(double)) : 0;
  p.thr_b = pad256(rj * sizeof(double));
  return p;
}

template <typename X2, typename O, int MODE>
int pw_launch(const void* x, const pbbss_mask_geom& g, double eps, const double* table,
              int64_t table_len, void* out, int64_t total, hipStream_t s) {
  const int64_t blocks = (total + kMkThreads - 1) / kMkThreads;
  hipLaunchKernelGGL((mask_pointwise_kernel<X2, O, MODE>), dim3((unsigned)blocks),
                     dim3(kMkThreads), 0, s, static_cast<const X2*>(x), static_cast<O*>(out), g,
                     eps, table, table_len, total);
  return mk_ok();
}

template <typename X2, typename R>
int pw_mode(const void* x, int mode, const pbbss_mask_geom& g, double eps, const double* table,
            int64_t table_len, void* out, int64_t total, hipStream_t s) {
  switch (mode) {
    case PBBSS_MASK_IBM: return pw_launch<X2, R, PBBSS_MASK_IBM>(x, g, eps, table, table_len, out, total, s);
    case PBBSS_MASK_WIENER: return pw_launch<X2, R, PBBSS_MASK_WIENER>(x, g, eps, table, table_len, out, total, s);
    case PBBSS_MASK_IRM: return pw_launch<X2, R, PBBSS_MASK_IRM>(x, g, eps, table, table_len, out, total, s);
    case PBBSS_MASK_IAM: return pw_launch<X2, R, PBBSS_MASK_IAM>(x, g, eps, table, table_len, out, total, s);
    case PBBSS_MASK_PSM: return pw_launch<X2, R, PBBSS_MASK_PSM>(x, g, eps, table, table_len, out, total, s);
    case PBBSS_MASK_ICM: return pw_launch<X2, X2, PBBSS_MASK_ICM>(x, g, eps, table, table_len, out, total, s);
    case PBBSS_MASK_BIASED: return pw_launch<X2, uint8_t, PBBSS_MASK_BIASED>(x, g, eps, table, table_len, out, total, s);
    default: return PBBSS_ERR_INVALID_ARG;
  }
}

template <typename X2, typename O, bool LORENZ>
int th_launch(const void* xv, const pbbss_mask_geom& g, const MaskTargets& t, const ThPlan& p,
              void* work, void* outv, int32_t* status, hipStream_t s) {
  const X2* x = static_cast<const X2*>(xv);
  O* out = static_cast<O*>(outv);
  if (p.small) {
    hipLaunchKernelGGL((mask_small_row_kernel<X2, O, LORENZ>), dim3((unsigned)p.rows),
                       dim3(kMkThreads), 0, s, x, out, g, t, (int)p.N, status);
    return mk_ok();
  }
  char* w = static_cast<char*>(work);
  double* vals = reinterpret_cast<double*>(w);
  w += p.vals_b;
  SelState* st = reinterpret_cast<SelState*>(w);
  w += p.state_b;
  uint32_t* pcnt = reinterpret_cast<uint32_t*>(w);
  w += p.pcnt_b;
  double* psum = reinterpret_cast<double*>(w);
  w += p.psum_b;
  double* thr = reinterpret_cast<double*>(w);
  const int chunks = (int)((p.N + kMkThreads - 1) / kMkThreads);
  const unsigned row_blocks = (unsigned)(p.rows * chunks);
  const int64_t rj = p.rows * t.J;
  const unsigned part_blocks = (unsigned)(rj * p.rg.parts);
  int rc;
  hipLaunchKernelGGL((mask_value_kernel<X2, LORENZ>), dim3(row_blocks), dim3(kMkThreads), 0, s, x,
                     g, p.N, chunks, vals);
  if ((rc = mk_ok()) != PBBSS_OK) return rc;
  for (int level = 0; level < 8; ++level) {
    hipLaunchKernelGGL((mask_hist_kernel<LORENZ>), dim3(part_blocks), dim3(kMkThreads), 0, s, vals,
                       p.N, t.J, p.rg, level, st, pcnt, psum);
    if ((rc = mk_ok()) != PBBSS_OK) return rc;
    hipLaunchKernelGGL((mask_pick_kernel<LORENZ>), dim3((unsigned)rj), dim3(kMkThreads), 0, s,
                       pcnt, psum, t.J, p.rg.parts, level, t, st);
    if ((rc = mk_ok()) != PBBSS_OK) return rc;
  }
  hipLaunchKernelGGL(mask_succ_kernel, dim3(part_blocks), dim3(kMkThreads), 0, s, vals, p.N, t.J,
                     p.rg, st);
  if ((rc = mk_ok()) != PBBSS_OK) return rc;
  hipLaunchKernelGGL((mask_finish_kernel<LORENZ>), dim3((unsigned)((rj + kMkThreads - 1) / kMkThreads)),
                     dim3(kMkThreads), 0, s, st, p.rows, t.J, t, thr, status);
  if ((rc = mk_ok()) != PBBSS_OK) return rc;
  hipLaunchKernelGGL((mask_apply_kernel<O>), dim3(row_blocks), dim3(kMkThreads), 0, s, vals, thr,
                     g, t, p.N, chunks, out);
  return mk_ok();
}

template <typename X2>
int th_out(const void* x, const pbbss_mask_geom& g, const MaskTargets& t, const ThPlan& p,
           void* work, void* out, int out_is_f64, int32_t* status, hipStream_t s) {
  if (t.lorenz)
    return out_is_f64 ? th_launch<X2, double, true>(x, g, t, p, work, out, status, s)
                      : th_launch<X2, float, true>(x, g, t, p, work, out, status, s);
  return out_is_f64 ? th_launch<X2, double, false>(x, g, t, p, work, out, status, s)
                    : th_launch<X2, float, false>(x, g, t, p, work, out, status, s);
}

bool geom_ok(const pbbss_mask_geom& g) {
  for (int a = 0; a < 4; ++a)
    if (g.size[a] < 1) return false;
  return true;
}

}  // namespace

int launch_mask_pointwise(const void* x, int x_is_c128, int mode, const pbbss_mask_geom& g,
                          double eps, const double* table, int64_t table_len, void* out,
                          hipStream_t s) {
  if (!geom_ok(g) || g.sources < 1 || g.sensors < 1) return PBBSS_ERR_INVALID_ARG;
  if (g.sources > kMaskMaxK || g.sensors > kMaskMaxD) return PBBSS_ERR_UNSUPPORTED;
  if (mode == PBBSS_MASK_BIASED) {
    if (!table || table_len < 1) return PBBSS_ERR_INVALID_ARG;
    if (g.sources != 2 || g.sensors != 1) return PBBSS_ERR_UNSUPPORTED;
  }
  // the total stays below 2^31 blocks of 256 points
  double total_d = 1.0;
  for (int a = 0; a < 4; ++a) total_d *= (double)g.size[a];
  if (total_d > 256.0 * 2147483647.0) return PBBSS_ERR_UNSUPPORTED;
  const int64_t total = g.size[0] * g.size[1] * g.size[2] * g.size[3];
  return x_is_c128 ? pw_mode<double2, double>(x, mode, g, eps, table, table_len, out, total, s)
                   : pw_mode<float2, float>(x, mode, g, eps, table, table_len, out, total, s);
}

static int th_check(const pbbss_mask_geom& g, const MaskTargets& t) {
  if (!geom_ok(g) || g.sensors < 1 || t.J < 1) return PBBSS_ERR_INVALID_ARG;
  if (g.sensors > kMaskMaxD || t.J > kMaskMaxQ) return PBBSS_ERR_UNSUPPORTED;
  const double rows = (double)g.size[0] * (double)g.size[1];
  const double N = (double)g.size[2] * (double)g.size[3];
  // block indices are 32-bit: rows x 256-element chunks, and rows x targets x parts (<= 64)
  if (rows * (N / 256.0 + 1.0) > 2147483647.0 || rows * t.J * 64.0 > 2147483647.0)
    return PBBSS_ERR_UNSUPPORTED;
  if (!t.lorenz)
    for (int j = 0; j < t.J; ++j)
      if (t.rank[j] < 0 || (double)t.rank[j] >= N || !(t.gamma[j] >= 0.0 && t.gamma[j] < 1.0))
        return PBBSS_ERR_INVALID_ARG;
  return PBBSS_OK;
}

size_t mask_threshold_work_bytes(const pbbss_mask_geom& g, const MaskTargets& t) {
  if (th_check(g, t) != PBBSS_OK) return 0;
  const ThPlan p = th_plan(g, t);
  return p.vals_b + p.state_b + p.pcnt_b + p.psum_b + p.thr_b;
}

int launch_mask_threshold(const void* x, int x_is_c128, const pbbss_mask_geom& g,
                          const MaskTargets& t, void* work, void* out, int out_is_f64,
                          int32_t* status, hipStream_t s) {
  const int rc = th_check(g, t);
  if (rc != PBBSS_OK) return rc;
  const ThPlan p = th_plan(g, t);
  if (!p.small && !work) return PBBSS_ERR_INTERNAL;
  return x_is_c128 ? th_out<double2>(x, g, t, p, work, out, out_is_f64, status, s)
                   : th_out<float2>(x, g, t, p, work, out, out_is_f64, status, s);
}

}  // namespace pbbss
