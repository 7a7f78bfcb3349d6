"""numpy.longdouble restatements of the extraction front end -- power spectral density matrices,
apply_beamforming_vector, normalize_observation -- with the case lists and the derived bounds of
tests/test_gpu_extraction_front_end.py.  tests/test_extraction_oracle.py checks the restatements
against oracle/beamformer.py and oracle.cacgmm.normalize_observation in float64 within the same
bounds, and the conditions the case lists have to meet.  Imports neither the GPU nor the product.

Every output of these operations is a short weighted sum, so a restatement in extended precision
(80-bit on x86-64, 64-bit significand) is exact for the purpose and the float64 rounding error of
a correct kernel can be bounded from the operation alone.  eps = 2^-52 throughout; complex64 input
is widened exactly; every reference is computed from the bits the kernel sees.

PSD, per problem b and class k:   |got - ref|_max <= (2 T + 16) eps max_i Re ref[b, k, i, i].
    Each entry is a T-term sum of w_t y_it conj(y_jt) with w >= 0, and by Cauchy-Schwarz
    sum_t w_t |y_it| |y_jt| <= sqrt(ref_ii ref_jj) <= max_i ref_ii: forming and adding the terms
    costs (T + 14) eps of that in any order; the sum of the mask (T eps) and the division by it
    (2 eps) move all entries by a relative (T + 2) eps.  Where the bound is 0 (an all-zero class or
    an all-zero input) every term is 0 and so must the output be, exactly.
apply, per output sample:         |got - ref| <= (D + 3) eps sum_d |w_d| |x_dt|.
normalize, per component:         |got - ref| <= (D + 4) eps for complex128 (outputs have modulus
    <= 1: D eps for the squared norm, the root, the reciprocal and the product one each); complex64
    output is compared with the reference rounded to float32 within one float32 ulp of the
    component, 2^-23 |ref|, plus the complex128 term.  All-zero frames stay exactly zero.
"""
import functools

import numpy as np

EPS = 2.0 ** -52
FLOOR = 1e-10          # beamformer.py:123: the mask sum is floored before the division
LD, CLD = np.longdouble, np.clongdouble
DTYPES = ('complex64', 'complex128')
MODES = ('normalized', 'plain', 'no mask')   # normalize=True, normalize=False, mask=None (K = 1)


def widen(x):
    """complex64 / complex128 -> clongdouble, exactly."""
    x = np.asarray(x)
    assert x.dtype in (np.complex64, np.complex128), x.dtype
    return x.astype(CLD)


def rand_c(rng, shape, dtype):
    """Circular complex normal samples of unit variance per component, rounded to `dtype`."""
    real = np.float32 if np.dtype(dtype) == np.complex64 else np.float64
    out = np.empty(shape, dtype)
    out.real = rng.standard_normal(shape, dtype=real)
    out.imag = rng.standard_normal(shape, dtype=real)
    return out


# ---- power spectral density matrices ------------------------------------------------------------
def psd(x, mask=None, normalize=True, block=512):
    """x (B, D, T) complex, mask (B, K, T) float64 or None -> (B, K, D, D) clongdouble
    (K = 1 without a mask): sum_t w_kt x_dt conj(x_et), w = mask / max(sum_t mask, 1e-10) with
    normalize, the mask itself without, 1 / T without a mask."""
    B, D, T = x.shape
    if mask is None:
        w = np.full((B, 1, T), LD(1) / LD(T))
    else:
        w = np.asarray(mask, dtype=np.float64).astype(LD)
        if normalize:
            w = w / np.maximum(w.sum(axis=-1, keepdims=True), LD(FLOOR))
    out = np.empty((B, w.shape[1], D, D), CLD)
    for b0 in range(0, B, block):      # blocks keep the widened copy of a big batch small
        xb = widen(x[b0:b0 + block])
        out[b0:b0 + block] = np.einsum('bkt,bdt,bet->bkde', w[b0:b0 + block], xb, xb.conj())
    # the upper triangle stands for both: Hermitian to the bit, as the sum is in exact arithmetic
    i, j = np.triu_indices(D, 1)
    out[..., j, i] = out[..., i, j].conj()
    d = np.arange(D)
    out[..., d, d] = out[..., d, d].real
    return out


def psd_bound(ref, T):
    """(B, K): (2 T + 16) eps max_i Re ref[b, k, i, i]."""
    diag = np.einsum('bkii->bki', ref).real.max(axis=-1)
    return ((2 * T + 16) * EPS * diag).astype(np.float64)


def psd_ratio(got, ref, T, slack=1.0):
    """Largest |got - ref|_max / (slack * bound) over the problems and classes.  Where the bound is
    0 the output has to be exactly 0: ratio 0 if it is, inf if not."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = slack * psd_bound(ref, T)
    err = np.abs(got - ref).max(axis=(-1, -2)).astype(np.float64)
    zero = bound == 0
    exact = np.abs(got).max(axis=(-1, -2)) == 0
    ratio = np.where(zero, np.where(exact, 0.0, np.inf), err / np.where(zero, 1.0, bound))
    return float(ratio.max())


def psd_mode_args(mask, mode):
    """(mask, normalize) of a call in `mode`."""
    return {'normalized': (mask, True), 'plain': (mask, False), 'no mask': (None, True)}[mode]


def psd_input(D, K, T, B, dtype, seed=0):
    """x (B, D, T) of `dtype` and a mask (B, K, T) in (0, 1): every (b, k) its own random row, so
    that a class or an entry written to the wrong slot changes the answer."""
    rng = np.random.default_rng([seed, D, K, T, B, DTYPES.index(np.dtype(dtype).name)])
    return rand_c(rng, (B, D, T), dtype), rng.uniform(size=(B, K, T))


# the fused kernel: psd_kernel<D, K, YS, SPILL>, D in 2..8, K in 1..4 per launch, K = 5, 6 as 4 + K - 4
FUSED_D = tuple(range(2, 9))
FUSED_K = tuple(range(1, 7))
GRID_B, GRID_T = 3, 70                 # two 64-frame chunks, the last one partial
FRAME_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
FRAME_DK = ((3, 2), (8, 4))
# more problems than workgroups can be resident: a compute unit holds at most 32 wavefronts, 8
# workgroups of four, so a grid has at most 8 CUs workgroups and 16 CUs + 3 problems send every
# workgroup round its persistent loop at least twice (most of them a third time)
TRIP_DK = ((3, 2), (8, 4))
TRIP_T = 70
MAX_WORKGROUPS_PER_CU = 8


def trip_batch(compute_units):
    return 16 * compute_units + 3


def trip_input(D, K, compute_units, T=TRIP_T, dtype='complex64'):
    """Different data and masks for every problem; problem b has an all-zero class when
    b % 5 == 0 and an all-zero frame when b % 7 == 0, so the flag word and the accumulators differ
    between consecutive trips of one workgroup."""
    B = trip_batch(compute_units)
    x, mask = psd_input(D, K, T, B, dtype, seed=1)
    for b in range(0, B, 5):
        mask[b, (b // 5) % K] = 0.0
    for b in range(0, B, 7):
        x[b, :, (b // 7) % T] = 0
    return x, mask


# the spilled variant: the frame-sized arrays of EmKernel (csrc/cacgmm_em.hpp) no longer fit
LDS_LIMIT = 160 * 1024                 # csrc/handle.hip: the whole LDS of a gfx950 compute unit
SPILL_CASES = ((8, 4, 'complex128'), (8, 4, 'complex64'), (3, 2, 'complex128'))
SPILL_TRIP_CASE = (3, 2, 'complex128')


def frame_bytes(D, K, dtype, T):
    """EmKernel<D, K, YS>::frame_bytes(T): observation [Tp/64][DP][64][4] of YS, 1 / |y|^2 [Tp]
    and weights [Tp/64][K][64] of float64, DP = (D + 1) / 2, Tp = T rounded up to 64."""
    ys = 4 if np.dtype(dtype) == np.complex64 else 8
    DP, Tp = (D + 1) // 2, -(-T // 64) * 64
    return DP * Tp * 4 * ys + Tp * 8 + K * Tp * 8


def spill_frames(D, K, dtype, limit=LDS_LIMIT):
    """The smallest multiple of 64, plus 6, whose frame arrays alone exceed `limit`: with the
    small matrices on top, lds_bytes(T) > limit whatever they take, so launch_psd_one has to pick
    SPILL = true.  (The multiple of 64 below may already spill because of the small arrays.)"""
    m = 64
    while frame_bytes(D, K, dtype, m + 6) <= limit:
        m += 64
    return m + 6


DEGENERATE_DK, DEGENERATE_T = (6, 3), 130
DEGENERATE_KINDS = ('zero class / sum below the floor / single frame', 'mask times 1e12',
                    '20 all-zero frames', 'control')
ZERO_FRAMES = (0, 1, 2, 62, 63, 64, 65, 66, 100, 101, 102, 103, 104, 120, 125, 126, 127, 128, 129, 77)


def degenerate_input(dtype):
    """B = 4 problems at (D, K) = (6, 3), T = 130, in the order of DEGENERATE_KINDS.  Problem 0:
    class 0 all zero, class 1 sums to 1e-13 (below the floor 1e-10: the floor wins and the result
    is sum (m / 1e-10) y y^H), class 2 nonzero in frame 71 only (rank one)."""
    (D, K), T = DEGENERATE_DK, DEGENERATE_T
    x, mask = psd_input(D, K, T, len(DEGENERATE_KINDS), dtype, seed=2)
    mask[0, 0] = 0.0
    mask[0, 1] *= 1e-13 / mask[0, 1].sum()
    mask[0, 2] = 0.0
    mask[0, 2, 71] = 0.37
    mask[1] *= 1e12
    x[2][:, list(ZERO_FRAMES)] = 0
    return x, mask


# pbbss_psd sends D > 8 or K > 6 to the generic kernel: both sides of both edges
ROUTING_CASES = ((8, 6), (8, 7), (9, 1), (9, 6))
ROUTING_B, ROUTING_T = 3, 70


def routing_input(D, K, dtype):
    """The K = 6 and K = 7 cases at one D share the data and the first six masks."""
    x, mask = psd_input(D, 7, ROUTING_T, ROUTING_B, dtype, seed=3)
    return x, np.ascontiguousarray(mask[:, :K])


# gen_cov_kernel<DP, KM, YS>: sensor widths DP = 16 (D <= 16), 32 (D <= 32), 36; class widths
# KM = 3 (a chunk of <= 3 classes) and 6; balanced chunks of at most 6 classes; 64-frame tiles
GENERIC_D = (9, 16, 17, 32, 33, 34)
GENERIC_K = (1, 3, 4, 6, 7, 12, 13, 19)
GENERIC_T = (63, 64, 65, 130)
GENERIC_B = 2


def generic_frames(D, K):
    """The frame count of cell (D, K): every T at every D, every T at every K."""
    return GENERIC_T[(GENERIC_D.index(D) + GENERIC_K.index(K)) % len(GENERIC_T)]


def generic_chunks(K):
    """Classes per launch of launch_gen_cov (csrc/generic.hip)."""
    n = -(-K // 6)
    out, k0 = [], 0
    for c in range(n):
        kc = -(-(K - k0) // (n - c))
        out.append(kc)
        k0 += kc
    return out


REFUSED_DK = ((1, 1), (35, 1), (9, 20), (8, 20))   # D = 1, D = 35, K = 20 on either route


# ---- apply_beamforming_vector -------------------------------------------------------------------
def apply_bf(w, x):
    """w (B, D) complex128, x (Bx, D, T) complex, B a multiple of Bx -> (B, T) clongdouble:
    sum_d conj(w[b, d]) x[b % Bx, d, t]."""
    B, Bx = w.shape[0], x.shape[0]
    assert B % Bx == 0
    xi = np.arange(B) % Bx
    return np.einsum('bd,bdt->bt', widen(w).conj(), widen(x)[xi])


def apply_bound(w, x):
    """(B, T): (D + 3) eps sum_d |w_d| |x_dt|."""
    B, Bx, D = w.shape[0], x.shape[0], w.shape[1]
    xi = np.arange(B) % Bx
    mag = np.einsum('bd,bdt->bt', np.abs(widen(w)), np.abs(widen(x))[xi])
    return ((D + 3) * EPS * mag).astype(np.float64)


def apply_ratio(got, w, x):
    ref, bound = apply_bf(w, x), apply_bound(w, x)
    assert got.shape == ref.shape and (bound > 0).all()
    return float((np.abs(got - ref).astype(np.float64) / bound).max())


APPLY_D = (1, 2, 5, 8, 9, 29)
APPLY_T = (1, 255, 256, 257)           # one 256-frame block, and one frame either side
APPLY_B = 3
APPLY_REFUSED_D = 30                   # beamformer.py:582
APPLY_STRIDE_CASE = (2, 2, 64 * 256 + 300)   # (B, D, T): the grid is capped at 64 blocks of 256
SEAM = 65535                           # grid.y limit: the batch goes out in launches of <= 65535
APPLY_SEAM_CASE = (SEAM + 2, 2, 3)     # (B, D, T)
SHARED_X_BATCH = 7
APPLY_SHARED_SEAM_CASE = (SHARED_X_BATCH * 9363, 2, 3)   # 65 541 vectors on 7 observations


def apply_input(B, D, T, dtype, x_batch=None, seed=0):
    """w (B, D) complex128 and x (x_batch or B, D, T) of `dtype`; observation j is scaled by
    j + 1 and shifted by j, so no two of a shared batch resemble each other."""
    rng = np.random.default_rng([seed, B, D, T, DTYPES.index(np.dtype(dtype).name)])
    w = rand_c(rng, (B, D), np.complex128)
    Bx = B if x_batch is None else x_batch
    x = rand_c(rng, (Bx, D, T), dtype)
    if x_batch is not None:
        j = np.arange(Bx).reshape(Bx, 1, 1)
        x = ((j + 1) * x + j).astype(dtype)
    return w, x


# ---- normalize_observation ----------------------------------------------------------------------
def normalize(y):
    """y (B, T, D) complex -> (B, D, T) clongdouble, unit norm over D; all-zero frames stay 0.
    The squared norm neither underflows nor overflows in extended precision for float64 input."""
    y = widen(y)
    n = np.sqrt((y.real ** 2 + y.imag ** 2).sum(axis=-1, keepdims=True))
    out = y / np.where(n == 0, LD(1), n)
    return np.ascontiguousarray(out.swapaxes(-1, -2))


def normalize_ratio(got, y):
    """Largest component error over its bound; got (B, D, T) of y's dtype."""
    ref = normalize(y)
    assert got.shape == ref.shape and got.dtype == y.dtype
    D = y.shape[-1]
    worst = 0.0
    for g, r in ((got.real, ref.real), (got.imag, ref.imag)):
        if got.dtype == np.complex64:
            want = r.astype(np.float32).astype(LD)
            bound = 2.0 ** -23 * np.abs(r) + (D + 4) * EPS
        else:
            want, bound = r, (D + 4) * EPS
        worst = max(worst, float((np.abs(g.astype(LD) - want) / bound).max()))
    return worst


NORMALIZE_T = (1, 63, 64, 65, 130)     # the 64-frame LDS tile of normalize_kernel
NORMALIZE_D = (1, 2, 7, 8, 9, 34)
NORMALIZE_B = 3
NORMALIZE_SEAM_CASE = (SEAM + 2, 2, 2)  # (B, T, D)


def normalize_zero_frames(T):
    """First and last frame of every tile, and of the call."""
    return sorted({t for t in (0, 63, 64, 127, 128, T - 1) if t < T})


def normalize_input(B, T, D, dtype, seed=0):
    """y (B, T, D); problem 1 has all-zero frames at normalize_zero_frames(T)."""
    rng = np.random.default_rng([seed, B, T, D, DTYPES.index(np.dtype(dtype).name)])
    y = rand_c(rng, (B, T, D), dtype)
    if B > 1:
        y[1, normalize_zero_frames(T)] = 0
    return y


EXTREME_T, EXTREME_D = 70, 4
EXTREME_TINY, EXTREME_HUGE = (3, 63, 64), (5, 69)   # frames scaled by 1e-170 and by 1e+170


def extreme_input():
    """complex128 (2, 70, 4): frames of magnitude 1e-170, whose squared norm underflows to 0 in
    float64, and of magnitude 1e+170, whose squared norm overflows."""
    y = rand_c(np.random.default_rng(4), (2, EXTREME_T, EXTREME_D), np.complex128)
    y[:, list(EXTREME_TINY)] *= 1e-170
    y[:, list(EXTREME_HUGE)] *= 1e170
    return y


# ---- reference channel: mvdr_souden -> select_reference_channel against the oracle ---------------
CHAIN_L, CHAIN_F = 3, 17
CHAIN_D = (3, 6, 8, 12)
CHAIN_GAP = 1e-6                       # the oracle's two largest SNRs differ by more than this
CHAIN_SEED = 0


@functools.lru_cache(maxsize=None)
def chain_input(D, seed=CHAIN_SEED):
    """Random Hermitian positive-definite (target, noise), each (L, F, D, D) complex128."""
    rng = np.random.default_rng([seed, D, 5])

    def posdef():
        a = rand_c(rng, (CHAIN_L, CHAIN_F, D, D + 2), np.complex128)
        m = a @ a.conj().swapaxes(-1, -2) / (D + 2)
        return 0.5 * (m + m.conj().swapaxes(-1, -2))
    target, noise = posdef(), posdef() + 0.05 * np.eye(D)
    for a in (target, noise):
        a.setflags(write=False)
    return target, noise
