"""Time of 100 iterations of `transform.GriffinLim` / `transform.MISI` next to the same iterations
spelled with the package's `transform.stft` / `istft` and torch's `abs` / `angle` / `polar` on
the device (the composition written below: the comparator), and to the float64 restatement of
the reference on the host (tests/oracle_griffin_lim.py, one mixture after the other).

Input: K = 3 sources, size 512, shift 128, 64 000 samples (497 frames), one mixture and a batch
of 16, device tensors, first guess y / K.  Per entry: fused_ms and composed_ms (median of --reps
calls, host clock around a call that ends in a device synchronise, both paths warmed up and
alternated in one process), their minima, host_ms (one run), the ratios, and the largest
difference between the results of the three.  One JSON line; --out writes it to a file as well.

Every device measurement runs in a child process under its own time limit (--limit seconds);
after a child that fails or runs out of time nothing more is started on the device.

    python tools/bench_griffin_lim.py [--reps 20] [--limit 240] [--out profiles/griffin_lim.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

K, SIZE, SHIFT, FRAMES, ITERATIONS = 3, 512, 128, 497, 100
CONFIGS = [('GriffinLim', 1), ('GriffinLim', 16), ('MISI', 1), ('MISI', 16)]  # (class, mixtures)


def inputs(mixtures):
    import oracle_griffin_lim as og
    cases = [og.gen_case(500 + b, K, FRAMES, SIZE, SHIFT) for b in range(mixtures)]
    assert cases[0]['y'].shape == (64000,)
    return np.stack([c['X'] for c in cases]), np.stack([c['y'] for c in cases])


def composed(X, y, misi, iterations):
    """the iterations with one device function per line of the reference's step"""
    import torch
    from pb_bss_amd.transform import istft, stft
    magnitude = X.abs()
    x_hat = (y / K).unsqueeze(-2).repeat_interleave(K, dim=-2)
    for _ in range(iterations):
        if misi:
            e = y - x_hat.sum(dim=-2)
            x_hat = x_hat + (e / K).unsqueeze(-2)
        X_dash_dash = stft(x_hat, SIZE, SHIFT, fading=False)
        X_dash = torch.polar(magnitude, torch.angle(X_dash_dash))
        x_hat = istft(X_dash, SIZE, SHIFT, fading=False)
    return x_hat


def child(cls, mixtures, reps, result_file):
    import torch
    from pb_bss_amd import transform
    X, y = inputs(mixtures)
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()

    def fused():
        model = getattr(transform, cls)(Xt, yt, first_guess='y', size=SIZE, shift=SHIFT)
        model.step(iterations=ITERATIONS)
        return model.x_hat

    paths = {'fused': fused, 'composed': lambda: composed(Xt, yt, cls == 'MISI', ITERATIONS)}
    results, times = {}, {name: [] for name in paths}
    for name, path in paths.items():  # warm-up: code objects, workspaces, the allocator
        results[name] = path()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, path in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            path()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for name in paths:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'] = float(min(times[name]))
    out['fused_vs_composed_max_difference'] = float(
        (results['fused'] - results['composed']).abs().max())
    np.save(result_file, results['fused'].cpu().numpy())
    print(json.dumps(out))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=20)
    parser.add_argument('--limit', type=float, default=240.0)
    parser.add_argument('--out')
    parser.add_argument('--child', nargs=3, metavar=('CLASS', 'MIXTURES', 'RESULT_FILE'))
    args = parser.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.reps, args.child[2])

    import oracle_griffin_lim as og
    entries = []
    scratch = tempfile.TemporaryDirectory()
    result_file = os.path.join(scratch.name, 'x_hat.npy')
    for cls, mixtures in CONFIGS:
        entry = {'class': cls, 'mixtures': mixtures, 'sources': K, 'size': SIZE, 'shift': SHIFT,
                 'samples': 64000, 'iterations': ITERATIONS}
        try:
            done = subprocess.run(
                [sys.executable, os.path.abspath(__file__), '--child', cls, str(mixtures),
                 result_file, '--reps', str(args.reps)],
                stdout=subprocess.PIPE, timeout=args.limit, check=True, text=True)
        except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as error:
            entry['error'] = repr(error)
            entries.append(entry)
            break  # nothing more on the device after a failure
        entry.update(json.loads(done.stdout.strip().splitlines()[-1]))
        got = np.load(result_file)
        X, y = inputs(mixtures)
        t0 = time.perf_counter()
        want = np.stack([og.run(og.RESTATED[cls], X[b], y[b], 'y', ITERATIONS, size=SIZE,
                                shift=SHIFT).x_hat for b in range(mixtures)])
        entry['host_ms'] = (time.perf_counter() - t0) * 1e3
        entry['composed_over_fused'] = entry['composed_ms'] / entry['fused_ms']
        entry['host_over_fused'] = entry['host_ms'] / entry['fused_ms']
        entry['fused_vs_host_max_difference'] = float(np.abs(got - want).max())
        entries.append(entry)
    line = json.dumps({'bench': 'griffin_lim', 'entries': entries})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 1 if any('error' in entry for entry in entries) else 0


if __name__ == '__main__':
    sys.exit(main())
