"""Device time of k-means (csrc/kmeans.hip) on the embedding of BASELINE configs[4]: N = 256 500
rows, E = 40, float32, K in {2, 3, 8, 16, 64}, 1 and --batch problems.

Per case: the time of one Lloyd iteration (difference of two fits from the same centres that run
--short and --long iterations, tol = 0, on unstructured data so that neither stops early; the stop
flag is read once per fit), of the k-means++ seeding, of a whole default BinaryGMMTrainer().fit on
blob data (host draws and flag reads included); the share of the device-to-device copy bandwidth
measured in the same run that one read of the embedding per iteration is -- the 41 MB embedding
of a single problem is re-read from the Infinity Cache, so this is not an HBM figure; the same
iteration written with torch ops (cdist / argmin / index_add_ in float64 on the widened copy);
(one call on its own where a torch iteration takes more than 50 ms);
for a single problem sklearn's Lloyd iteration on the host where it is installed; and the largest
difference to the float64 restatement (tests/oracle_kmeans.py) after two iterations.
Times are medians of --reps calls between device events after warm-up, our and the torch variant
alternating.  One JSON line; --out writes it to a file as well.

    python tools/bench_kmeans.py [--reps 10] [--batch 64] [--out profiles/kmeans.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, E = 256500, 40


T0 = time.perf_counter()


def stage(text):
    print(f'[{time.perf_counter() - T0:7.1f} s] {text}', file=sys.stderr, flush=True)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(fns, reps, warmup=2):
    """median microseconds of each of `fns`, called in turn"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return [float(np.median(t)) for t in ts]


def copy_bandwidth(reps=10):
    import torch
    src = torch.empty(1 << 28, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    med, = alternate([lambda: dst.copy_(src)], reps)
    return 2 * src.numel() * 4 / (med * 1e-6)


def torch_iterations(x64, centers, iterations):
    """Lloyd iterations with torch ops; x64 (B, N, E) float64, centers (B, K, E)"""
    import torch
    B, n, e = x64.shape
    K = centers.shape[1]
    offset = (torch.arange(B, device=x64.device) * K)[:, None]
    flat = x64.reshape(B * n, e)
    for _ in range(iterations):
        labels = torch.cdist(x64, centers).argmin(-1)
        index = (labels + offset).reshape(-1)
        sums = torch.zeros((B * K, e), dtype=x64.dtype, device=x64.device).index_add_(0, index, flat)
        counts = torch.bincount(index, minlength=B * K).clamp_(min=1)
        centers = (sums / counts[:, None]).reshape(B, K, e)
    return centers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--short', type=int, default=4)
    ap.add_argument('--long', type=int, default=24)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import oracle_kmeans as ok
    from pb_bss_amd.distribution import BinaryGMMTrainer, kmeans as km
    try:
        from sklearn.cluster import KMeans as SkKMeans
    except ImportError:
        SkKMeans = None
    bandwidth = copy_bandwidth()
    out = {'rows': N, 'features': E, 'dtype': 'float32', 'copy_bytes_per_s': bandwidth,
           'copy_bytes_counted': 'read + written', 'entries': []}
    print({'copy_bytes_per_s': bandwidth}, file=sys.stderr, flush=True)
    gen = torch.Generator(device='cuda').manual_seed(0)
    steps = args.long - args.short
    for B in (1, args.batch):
        noise = torch.randn((B, N, E), generator=gen, device='cuda', dtype=torch.float32)
        x64 = noise.double()
        for K in (2, 3, 8, 16, 64):
            reps = args.reps if B == 1 else max(3, args.reps // 3)
            init = noise[:, :K].double().contiguous()
            trials = km._default_trials(K)
            randoms = np.random.RandomState(K).uniform(size=(B, 1 + (K - 1) * trials))
            fit = lambda m: km._call_fit(noise, K, None, init, m, 0.0, m)  # noqa: E731
            n_iter = fit(args.long)[3]
            assert int(n_iter.min()) == args.long, n_iter  # nothing stopped early
            ours = [lambda: fit(args.short), lambda: fit(args.long),
                    lambda: km._call_plusplus(noise, K, None, randoms, trials)]
            theirs = [lambda: torch_iterations(x64, init, args.short),
                      lambda: torch_iterations(x64, init, args.long)]
            # index_add_ of float64 rows into few classes can take seconds per iteration: where
            # one torch iteration takes more than 50 ms it is timed on its own, a single call
            torch_once = timed(lambda: torch_iterations(x64, init, 1))
            torch_once = timed(lambda: torch_iterations(x64, init, 1))
            stage(f'B={B} K={K}: one torch iteration {torch_once:.0f} us')
            if torch_once > 50e3:
                t_short, t_long, t_seed = alternate(ours, reps)
                torch_us = torch_once
            else:
                t_short, t_long, t_seed, tt_short, tt_long = alternate(ours + theirs, reps)
                torch_us = (tt_long - tt_short) / steps
            iter_us = (t_long - t_short) / steps
            stage(f'B={B} K={K}: iteration {iter_us:.1f} us, seeding {t_seed:.0f} us')
            # a whole default fit on blob data
            mu = torch.randn((B, K, E), generator=gen, device='cuda')
            lab = torch.randint(K, (B, N), generator=gen, device='cuda')
            blobs = (mu[torch.arange(B, device='cuda')[:, None], lab] + 0.3 * noise).contiguous()
            trainer = lambda: BinaryGMMTrainer().fit(blobs, K, random_state=0)  # noqa: E731
            fit_us, = alternate([trainer], max(3, reps // 2), warmup=1)
            stage(f'B={B} K={K}: default fit {fit_us:.0f} us')
            fit_iters = trainer().kmeans.n_iter_.cpu().numpy()
            nbytes = B * N * E * 4
            e = dict(problems=B, classes=K, lloyd_iteration_us=iter_us, seeding_us=t_seed,
                     default_fit_us=fit_us, default_fit_n_iter=[int(fit_iters.min()), int(fit_iters.max())],
                     bytes_per_iteration=nbytes,
                     copy_bandwidth_fraction_infinity_cache=nbytes / (iter_us * 1e-6) / bandwidth,
                     torch_iteration_us=torch_us, torch_single_call=bool(torch_once > 50e3),
                     torch_over_ours=torch_us / iter_us)
            if B == 1:
                xh = noise[0].cpu().numpy()
                wide = xh.astype(np.float64)
                ih = init[0].cpu().numpy()
                ref = ok.lloyd(wide, ih, max_iter=2, tol=0.0)
                c, labels, inertia, _ = km._call_fit(noise, K, None, init, 2, 0.0, 8)
                e['restatement_margin'] = ref['margin']
                e['labels_differing'] = int((labels[0].cpu().numpy() != ref['labels']).sum())
                e['largest_centre_difference'] = float(np.abs(c[0].cpu().numpy() - ref['centers']).max())
                e['inertia_relative_difference'] = abs(float(inertia[0]) / ref['inertia'] - 1)
                stage(f'B={B} K={K}: restatement compared')
                if SkKMeans is not None:
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore')
                        t0 = time.perf_counter()
                        sk = SkKMeans(n_clusters=K, init=ih.astype(np.float32), n_init=1, max_iter=10,
                                      tol=0.0).fit(xh)
                        e['sklearn_host_iteration_us'] = (time.perf_counter() - t0) * 1e6 / sk.n_iter_
                        t0 = time.perf_counter()
                        SkKMeans(n_clusters=K, random_state=0).fit(blobs[0].cpu().numpy())
                        e['sklearn_host_default_fit_us'] = (time.perf_counter() - t0) * 1e6
            out['entries'].append(e)
            if args.out:  # kept current, so that an interrupted run leaves what it measured
                with open(args.out, 'w') as f:
                    f.write(json.dumps(out) + '\n')
            print({k: (round(v, 3) if isinstance(v, float) else v) for k, v in e.items()},
                  file=sys.stderr, flush=True)
            del blobs, mu, lab
        del noise, x64
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
