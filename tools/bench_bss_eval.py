"""Device time of `pb_bss_amd.evaluation.mir_eval_sources` (csrc/bss_eval.hip) next to (a) the
float64 NumPy restatement on the host (tests/oracle_bss_eval.py, normal-equation route, one
channel, input already in host memory) and (b) the same metric written with torch ops on the same
device tensors: `torch.fft` correlations at a power-of-two length, `torch.linalg.cholesky` / `cholesky_solve`, `conv1d`
for the filters (an FFT product where conv1d refuses float64), the search over a table of
permutations.

Sizes: K = 2, 3 sources, K and K + 1 estimates, N = 64 000 and 128 000 samples, filter length
512; one utterance, and 8 channels that share their references (the `InputMetrics` layout: one
correlation and one factorisation of the references for all channels).  Per entry: ours_us /
torch_us (median of --reps calls between device events after warm-up; ours includes reading
the status word back, as every call does), the four phases of one call in us (correlations and
assembly, factorisation, triangular solves, synthesis and epilogue), numpy_host_us_per_channel
(one call), the largest difference in dB of both device results from the restatement, and
`loses_to_torch` where torch_us < ours_us.  One JSON line; --out writes it to a file as well.

    python tools/bench_bss_eval.py [--reps 5] [--out profiles/bss_eval.json]
"""
import argparse
import ctypes
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L = 512
CHANNELS = 8


def device_us(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(min(ts))


def make_case(seed, K, Ke, D, N):
    """references (K, N), estimations (Ke, D, N): a diagonally dominant mix per channel"""
    import oracle_bss_eval as ob
    rng = np.random.default_rng(seed)
    references = ob.ar1(rng, K, N)
    mix = rng.uniform(0.1, 0.3, (D, Ke, K))
    mix[:, np.arange(K), np.arange(K)] = 1.0
    estimations = np.einsum('dek,kn->edn', mix, references) \
        + 0.1 * rng.standard_normal((Ke, D, N))
    return references, estimations


# ---- the torch formulation ------------------------------------------------------------------
class TorchBssEval:
    def __init__(self, K, Ke, N, device):
        import torch
        self.t = torch
        self.n_out = N + L - 1
        self.n = 1 << (self.n_out - 1).bit_length()  # FFT length: the next power of two
        self.rhs_index = (-torch.arange(L, device=device)) % self.n
        self.perms = torch.tensor(list(itertools.permutations(range(Ke), K)), device=device)
        self.synthesis = 'conv1d'

    def filtered(self, taps, signals):
        """taps (R, L), signals (R, N) -> (R, N + L - 1): every row filtered by its taps"""
        t = self.t
        if self.synthesis == 'conv1d':
            try:
                x = t.nn.functional.pad(signals, (L - 1, L - 1))[None]
                return t.nn.functional.conv1d(x, taps.flip(-1)[:, None, :], groups=len(taps))[0]
            except RuntimeError:
                self.synthesis = 'fft'
        n = self.n
        return t.fft.irfft(t.fft.rfft(taps, n) * t.fft.rfft(signals, n), n)[..., :self.n_out]

    def __call__(self, ref, est):
        """ref (B, K, N), est (B, Ke, N) float64 -> sdr, sir, sar (B, K), selection (B, K)"""
        t = self.t
        B, K, N = ref.shape
        Ke = est.shape[1]
        n, n_out = self.n, self.n_out
        sf, ef = t.fft.rfft(ref, n), t.fft.rfft(est, n)
        c = t.fft.irfft(sf[:, :, None] * sf[:, None].conj(), n)          # (B, K, K, n)
        # Toeplitz blocks [l, m] = c[(m - l) mod n] as a strided view of the 2 L - 1 lags
        lags = t.cat([c[..., n - L + 1:], c[..., :L]], -1)
        blocks = lags.unfold(-1, L, 1).flip(-2)                            # (B, K, K, L, L)
        G = blocks.permute(0, 1, 3, 2, 4).reshape(B, K * L, K * L)
        d = t.fft.irfft(sf[:, None] * ef[:, :, None].conj(), n)[..., self.rhs_index]  # B Ke K L
        f_all = t.cholesky_solve(d.reshape(B, Ke, K * L).transpose(1, 2),
                                 t.linalg.cholesky(G))                     # (B, K L, Ke)
        diag = blocks[:, t.arange(K), t.arange(K)]                         # (B, K, L, L)
        f_one = t.cholesky_solve(d.permute(0, 2, 3, 1), t.linalg.cholesky(diag))  # (B, K, L, Ke)
        ref_rows = ref[:, None].expand(B, Ke, K, N).reshape(-1, N)
        p_all = self.filtered(f_all.transpose(1, 2).reshape(B * Ke * K, L), ref_rows) \
            .reshape(B, Ke, K, n_out).sum(2)                               # (B, Ke, n_out)
        p_one = self.filtered(f_one.permute(0, 3, 1, 2).reshape(B * Ke * K, L), ref_rows) \
            .reshape(B, Ke, K, n_out)
        e = t.nn.functional.pad(est, (0, L - 1))

        def energy(x):
            return (x * x).sum(-1)

        s = energy(p_one)
        sdr = 10 * t.log10(s / energy(e[:, :, None] - p_one))
        sir = 10 * t.log10(s / energy(p_all[:, :, None] - p_one))
        sar = (10 * t.log10(energy(p_all) / energy(e - p_all)))[:, :, None].expand_as(sdr)
        k = t.arange(K, device=ref.device)
        sel = self.perms[sir[:, self.perms, k].mean(-1).argmax(-1)]        # (B, K)
        pick = lambda table: table.gather(1, sel[:, None, :])[:, 0]       # table[b, sel[b, k], k]
        return pick(sdr), pick(sir), pick(sar), sel


def phase_us(fn):
    from pb_bss_amd import _lib
    lib = _lib.load()
    h = _lib.handle()
    _lib.check(lib.pbbss_set_timing(h, 1), 'set_timing')
    try:
        fn()
        ms = (ctypes.c_float * 4)()
        _lib.check(lib.pbbss_bss_eval_phase_ms(h, ms), 'phase_ms')
    finally:
        lib.pbbss_set_timing(h, 0)
    names = ('correlation', 'factorisation', 'solve', 'synthesis')
    return {name: float(v) * 1e3 for name, v in zip(names, ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--samples', type=int, nargs='*', default=[64000, 128000])
    args = ap.parse_args()
    import torch
    import oracle_bss_eval as ob
    from pb_bss_amd.evaluation import mir_eval_sources

    entries = []
    for N in args.samples:
        for K in (2, 3):
            for Ke in (K, K + 1):
                references, estimations = make_case(K * 10 + Ke, K, Ke, CHANNELS, N)
                t0 = time.perf_counter()
                expected = ob.bss_eval(references, estimations[:, 0], L, route='normal')
                numpy_us = (time.perf_counter() - t0) * 1e6
                ref = torch.from_numpy(references).cuda()
                est = torch.from_numpy(estimations).cuda()
                for layout, D in (('utterance', 1), ('channels_shared_references', CHANNELS)):
                    r = ref[:, None, :].expand(K, D, N)
                    e = est[:, :D]
                    ours = lambda: mir_eval_sources(r, e)
                    formulation = TorchBssEval(K, Ke, N, ref.device)
                    rb, eb = r.permute(1, 0, 2).contiguous(), e.permute(1, 0, 2).contiguous()
                    theirs = lambda: formulation(rb, eb)
                    got, got_torch = ours(), theirs()
                    diff = max(float(np.abs(g[:, 0].cpu().numpy() - x).max())
                               for g, x in zip(got[:3], expected[:3]))
                    diff_torch = max(float(np.abs(g[0].cpu().numpy() - x).max())
                                     for g, x in zip(got_torch[:3], expected[:3]))
                    assert got[3][:, 0].tolist() == expected[3].tolist()
                    ours_us, ours_min = device_us(ours, args.reps)
                    torch_us, torch_min = device_us(theirs, args.reps)
                    entries.append({
                        'layout': layout, 'channels': D, 'K': K, 'K_estimates': Ke, 'samples': N,
                        'filter_length': L, 'ours_us': ours_us, 'ours_us_min': ours_min,
                        'phases_us': phase_us(ours), 'torch_us': torch_us,
                        'torch_us_min': torch_min, 'torch_synthesis': formulation.synthesis,
                        'numpy_host_us_per_channel': numpy_us,
                        'torch_over_ours': torch_us / ours_us,
                        'numpy_over_ours': numpy_us * D / ours_us,
                        'loses_to_torch': bool(torch_us < ours_us),
                        'largest_difference_db': diff,
                        'torch_largest_difference_db': diff_torch,
                    })
                    print(json.dumps(entries[-1]), file=sys.stderr, flush=True)
    result = {'filter_length': L, 'entries': entries,
              'losses_to_torch': [f"{x['layout']} K={x['K']} Ke={x['K_estimates']} "
                                  f"N={x['samples']}" for x in entries if x['loses_to_torch']],
              'largest_difference_db': max(x['largest_difference_db'] for x in entries)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
