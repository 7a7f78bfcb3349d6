"""Time of WPE dereverberation on the device (csrc/wpe.hip through `pb_bss_amd.transform.wpe`)
next to the same algorithm spelled in torch ops on the same GPU (shifted slices, `einsum`,
`torch.linalg.cholesky` + `cholesky_solve`, complex128) and next to the float64 NumPy restatement
on the host (tests/oracle_wpe.py, input already in host memory).

Entries (complex64 frames (F, D, T), taps 10, delay 3, 3 iterations, psd_context 0, 'full'):
    headline      F = 513, T = 500, D = 8, one utterance
    headline_x64  the same, 64 utterances (B = 32832)
    f257_d6       F = 257, T = 800, D = 6
    f257_d6_x64   the same, 64 utterances
    long_row      one problem, T = 3000, D = 8
Per entry: ours_us (median of --reps warm calls, wall time around a call that ends with a device
synchronise), ours_min_us, kernel_us (device events around the launches of the whole call),
first_call_us, torch_us (64 utterances: one utterance at a time), torch_over_ours,
loses_to_torch, host_ms (64 utterances: one utterance times 64, `host_extrapolated`),
host_over_ours, max_difference (to the restatement, relative to max |X|), and per kernel
(`parts`: the weights, the correlations, the solve, the filter, each timed on its own through
its export, one iteration): kernel_us, what the step has to move and do from the shapes (bytes,
flop; correlations: 8 T (M (M + 1) / 2 + M D) per problem), the fractions of the FP64 peak and
of the HBM bandwidth reached, and which of the two is nearer (`binds`; 'latency' where both are
below 5 %).  `parity`: the distance of the device result from the restatement for every case of
the test sweep after one and three iterations, with its bound.  Nothing is promised: an entry
that loses says so.  One JSON line; --out writes it to a file as well.

Every device measurement runs in a child process under its own time limit (--limit seconds);
after a child that fails or runs out of time nothing more is started on the device.

    python tools/bench_wpe.py [--reps 30] [--limit 240] [--out profiles/wpe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

TAPS, DELAY, ITERATIONS = 10, 3, 3
CONFIGS = {'headline': (513, 8, 500, 1), 'headline_x64': (513, 8, 500, 64),
           'f257_d6': (257, 6, 800, 1), 'f257_d6_x64': (257, 6, 800, 64),
           'long_row': (1, 8, 3000, 1)}
PEAK_FP64 = 78.6e12   # MI355X, vector and matrix FP64 share one datapath
PEAK_HBM = 8.0e12


def inputs(name, utterances=None):
    """(U * F, D, T) complex64: the first utterance at U levels."""
    import oracle_wpe as ow
    F, D, T, U = CONFIGS[name]
    U = U if utterances is None else utterances
    y = ow.synth(F, D, T, seed=21).astype(np.complex64)
    level = (1 + np.arange(U, dtype=np.float32) / 64)[:, None, None, None]
    return (level * y).reshape(U * F, D, T)


def torch_wpe(y, taps, delay, iterations):
    import torch
    Y = y.to(torch.complex128)
    B, D, T = Y.shape
    Yt = torch.zeros((B, taps, D, T), dtype=Y.dtype, device=Y.device)
    for k in range(taps):
        Yt[:, k, :, delay + k:] = Y[:, :, :T - delay - k]
    Yt = Yt.reshape(B, taps * D, T)
    X = Y
    for _ in range(iterations):
        p = (X.real ** 2 + X.imag ** 2).mean(1)
        w = 1 / torch.maximum(p, 1e-10 * p.amax(-1, keepdim=True))
        Yw = Yt * w[:, None, :]
        R = torch.einsum('bit,bjt->bij', Yw, Yt.conj())
        P = torch.einsum('bit,bjt->bij', Yw, Y.conj())
        G = torch.cholesky_solve(P, torch.linalg.cholesky(R))
        X = Y - torch.einsum('bmd,bmt->bdt', G.conj(), Yt)
    return X.to(y.dtype)


def timed(call, reps):
    import torch
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return value, times


def kernel_us(call, reps=5):
    from pb_bss_amd import engine
    engine.set_timing(True)
    out = []
    for _ in range(reps):
        call()
        out.append(engine.last_kernel_ms() * 1e3)
    engine.set_timing(False)
    return float(np.median(out))


def part(us, nbytes, flop):
    fp64, hbm = flop / (us * 1e-6) / PEAK_FP64, nbytes / (us * 1e-6) / PEAK_HBM
    binds = 'latency' if max(fp64, hbm) < 0.05 else 'fp64' if fp64 > hbm else 'hbm'
    return {'kernel_us': us, 'bytes': nbytes, 'flop': flop, 'fp64_fraction': fp64,
            'hbm_fraction': hbm, 'binds': binds}


def child(name, reps, torch_reps, out_path):
    import torch
    from pb_bss_amd import engine, transform
    F, D, T, U = CONFIGS[name]
    B, M = F * U, D * TAPS
    y = torch.from_numpy(inputs(name)).cuda()

    def ours():
        return transform.wpe(y, TAPS, DELAY, ITERATIONS)
    x, first = timed(ours, 1)
    timed(ours, 3)
    x, times = timed(ours, reps)
    out = {'ours_us': float(np.median(times)), 'ours_min_us': float(min(times)),
           'kernel_us': kernel_us(ours), 'first_call_us': first[0]}
    _, inv = engine.wpe_power(y)
    R, P = engine.wpe_correlations(y, inv, TAPS, DELAY)
    G, _ = engine.wpe_filter_matrix(R, P)
    tri = M * (M + 1) // 2
    out['parts'] = {
        'weights': part(kernel_us(lambda: engine.wpe_power(y)), B * T * (D * 8 + 16),
                        B * T * (3 * D + 2)),
        'correlations': part(kernel_us(lambda: engine.wpe_correlations(y, inv, TAPS, DELAY)),
                             B * (T * (D * 8 + 8) + (M * M + M * D) * 16),
                             B * 8 * T * (tri + M * D)),
        'solve': part(kernel_us(lambda: engine.wpe_filter_matrix(R, P)),
                      B * (tri + 2 * M * D) * 16, B * 8 * (M ** 3 // 6 + M * M * D)),
        'filter': part(kernel_us(lambda: engine.wpe_apply_filter(y, G, TAPS, DELAY)),
                       B * (2 * T * D * 8 + M * D * 16), B * 8 * T * M * D)}
    per_call = F  # torch: one utterance at a time keeps its stacked copy at 513 x 80 x 500
    try:
        def spelled():
            return torch.cat([torch_wpe(y[u * per_call:(u + 1) * per_call], TAPS, DELAY, ITERATIONS)
                              for u in range(U)])
        timed(spelled, 1)
        tx, ttimes = timed(spelled, torch_reps)
        out['torch_us'] = float(np.median(ttimes))
    except RuntimeError as error:
        out['torch_error'] = str(error).splitlines()[0][:200]
        tx = None
    arrays = {'x': x[:F].cpu().numpy()}
    if tx is not None:
        arrays['torch_x'] = tx[:F].cpu().numpy()
    np.savez(out_path, **arrays)
    print(json.dumps(out))


def parity_child():
    """The distance of the device result from the restatement over the test sweep."""
    import oracle_wpe as ow
    import test_gpu_wpe as gpu
    from pb_bss_amd import transform
    rows = []
    for case in ow.CASES:
        D, taps, delay, T = case
        Y = ow.case_input(case)
        want = ow.wpe(Y, taps, delay, 3, snapshots=True)
        row = {'D': D, 'taps': taps, 'delay': delay, 'T': T}
        for n, ref, e in ((1, want[0], gpu.E_CASE[case][0]), (3, want[2], gpu.E_CASE[case][1])):
            got = transform.wpe(Y, taps, delay, n)
            row[f'distance_{n}'] = float(np.abs(got - ref).max() / np.abs(ref).max())
            row[f'bound_{n}'] = 16 * max(e, 1e-13)
        rows.append(row)
    print(json.dumps(rows))


def run_child(args, extra, limit):
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + extra,
                          stdout=subprocess.PIPE, timeout=limit, check=True, text=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--torch-reps', type=int, default=3)
    parser.add_argument('--limit', type=float, default=240.0)
    parser.add_argument('--out')
    parser.add_argument('--child', choices=list(CONFIGS) + ['parity'])
    parser.add_argument('--child-out')
    args = parser.parse_args()
    if args.child == 'parity':
        return parity_child()
    if args.child:
        return child(args.child, args.reps, args.torch_reps, args.child_out)

    import tempfile
    import oracle_wpe as ow
    entries, parity, failed = [], None, False
    try:
        parity = json.loads(run_child(args, ['--child', 'parity'], args.limit).stdout
                            .strip().splitlines()[-1])
    except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as error:
        parity, failed = {'error': repr(error)}, True
    for name, (F, D, T, U) in CONFIGS.items():
        if failed:
            break  # nothing more on the device after a failure
        entry = {'entry': name, 'F': F, 'D': D, 'T': T, 'utterances': U, 'taps': TAPS,
                 'delay': DELAY, 'iterations': ITERATIONS}
        with tempfile.TemporaryDirectory() as tmp:
            results = os.path.join(tmp, 'results.npz')
            try:
                done = run_child(args, ['--child', name, '--reps', str(args.reps), '--torch-reps',
                                        str(args.torch_reps), '--child-out', results], args.limit)
            except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as error:
                entry['error'] = repr(error)
                entries.append(entry)
                failed = True
                continue
            entry.update(json.loads(done.stdout.strip().splitlines()[-1]))
            with np.load(results) as f:
                got = {k: f[k] for k in f.files}
        y = inputs(name, 1)
        t0 = time.perf_counter()
        host = ow.wpe(y, TAPS, DELAY, ITERATIONS)
        entry['host_ms'] = (time.perf_counter() - t0) * 1e3 * U
        if U > 1:
            entry['host_extrapolated'] = True
        entry['host_over_ours'] = entry['host_ms'] * 1e3 / entry['ours_us']
        scale = np.abs(host).max()
        entry['max_difference'] = float(np.abs(got['x'] - host.astype(np.complex64)).max() / scale)
        if 'torch_us' in entry:
            entry['torch_over_ours'] = entry['torch_us'] / entry['ours_us']
            entry['loses_to_torch'] = entry['torch_over_ours'] < 1.0
            entry['torch_max_difference'] = float(
                np.abs(got['torch_x'] - host.astype(np.complex64)).max() / scale)
        entries.append(entry)
        print(f'{name}: done', file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'wpe', 'entries': entries, 'parity': parity})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
