"""Device time of the deflation seed (csrc/initializer.hip) next to the 100-iteration cACGMM fit
it feeds, timed in the same run with device events after warm-up:

    (F, T, D, K) = (513, 500, 8, 3) and (257, 800, 6, 3), permutation_free True / False,
    one utterance and a batch of 64.

Per entry: seed_us (median of --reps calls), fit_ms, their ratio, the bytes the call must move
(Y once + K F T float64 out) and that traffic as a share of 8 TB/s over the measured time.  The
host time of the float64 restatement (tests/oracle_initializer.py) on this box stands for the
reference, as `cpu_baseline` does for the EM.  Asserts that the seed takes less time than the
fit.  One JSON line; --out writes it to a file as well.

    python tools/bench_initializer.py [--reps 20] [--out profiles/r07_initializer.json]
    python tools/bench_initializer.py --trace      # short run for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = [(513, 500, 8, 3), (257, 800, 6, 3)]
HBM_BYTES_PER_S = 8e12


def device_ms(fn, reps, warmup=3):
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
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--fit-reps', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--trace', action='store_true',
                    help='a few calls per configuration, one utterance, no fit, no CPU leg')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import oracle_initializer as oi
    from pb_bss_amd.distribution import CACGMMTrainer
    from pb_bss_amd.initializer.deflation import deflationSeed
    from pb_bss_amd.testing import synth
    out = {'iterations': args.iterations, 'entries': []}
    for (F, T, D, K) in SHAPES:
        Y, init = synth.make_stft(F, T, D, K, seed=0)
        cpu_s = {}
        if not (args.no_cpu or args.trace):
            for pf in (True, False):
                t0 = time.perf_counter()
                ref = oi.deflation_seed(Y, K, permutation_free=pf)
                cpu_s[pf] = time.perf_counter() - t0
                got = deflationSeed(Y, K, permutation_free=pf)
                err = float(np.abs(got - ref).max())
                assert err <= 1e-10, err
        for B in ((1,) if args.trace else (1, args.batch)):
            yd = torch.from_numpy(Y).cuda()[None].expand(B, F, T, D).contiguous()
            fit_ms = None
            if not args.trace:
                initd = torch.from_numpy(init).cuda()[None].expand(B, F, K, T).contiguous()
                fit_ms, _ = device_ms(
                    lambda: CACGMMTrainer().fit(yd, initialization=initd,
                                                iterations=args.iterations),
                    args.fit_reps, warmup=2)
                del initd
            for pf in (True, False):
                med, best = device_ms(lambda: deflationSeed(yd, K, permutation_free=pf),
                                      3 if args.trace else args.reps)
                nbytes = yd.numel() * yd.element_size() + B * K * F * T * 8
                e = dict(F=F, T=T, D=D, K=K, utterances=B, permutation_free=pf,
                         seed_us=med * 1e3, seed_us_min=best * 1e3, bytes=nbytes,
                         hbm_share=nbytes / (med * 1e-3) / HBM_BYTES_PER_S)
                if fit_ms is not None:
                    e.update(fit_ms=fit_ms, fit_over_seed=fit_ms / med)
                    assert med < fit_ms, (e, 'the seed must take less time than the fit it feeds')
                if pf in cpu_s:
                    e.update(cpu_restatement_ms=cpu_s[pf] * 1e3,
                             cpu_over_device=cpu_s[pf] * 1e3 * B / med)
                out['entries'].append(e)
                print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in e.items()},
                      file=sys.stderr)
            del yd
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
