"""Time of the complex circular-symmetric Gaussian on the device (csrc/ccsg.hip: `engine.ccsg_fit`
with a K-class saliency, `engine.ccsg_log_pdf`) next to the same computation spelled in torch
ops on the same GPU (fit: `torch.einsum` on the widened operands; log-pdf:
`torch.linalg.cholesky` + `solve_triangular`) and next to the float64 NumPy restatement on the
host (tests/oracle_ccsg.py, input already in host memory).

Entries (frames complex64, saliency float32, K = 3 unless stated):
    headline     F = 513, N = 500, D = 8
    f257_d6      F = 257, N = 800, D = 6
    generic_d16  F = 257, N = 500, D = 16
    headline_x64 the headline shape x 64 utterances (B = 32832)
Per entry and function: ours_us (median of --reps calls, wall time around a call that ends with
a device synchronise), ours_min_us, kernel_us (device events around the launches of the call,
pbbss_set_timing), first_call_us, torch_us, torch_over_ours, loses_to_torch, host_ms (one call
of the restatement; for headline_x64 one utterance times 64, `host_extrapolated`),
host_over_ours, the largest difference of both device results to the restatement, and
`bytes` / `flop`: what the algorithm has to move and do, from the shapes.  Nothing is promised:
an entry that loses says so.  One JSON line; --out writes it to a file as well.

Every device measurement runs in a child process under its own time limit (--limit seconds);
after a child that fails or runs out of time nothing more is started on the device.

    python tools/bench_ccsg.py [--reps 30] [--limit 240] [--out profiles/ccsg.json]
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

K = 3
CONFIGS = {'headline': (513, 500, 8), 'f257_d6': (257, 800, 6), 'generic_d16': (257, 500, 16),
           'headline_x64': (513 * 64, 500, 8)}
HOST_SLICE = {'headline_x64': 513}  # batch items of the host run (the rest is extrapolated)


def inputs(name, batch=None):
    """(y (B, N, D) complex64, saliency (B, K, N) float32); `batch`: the leading items only.  The
    64 utterances are the first one at 64 levels, so that a slice is generated without the rest."""
    import oracle_ccsg as oc
    B, N, D = CONFIGS[name]
    first = HOST_SLICE.get(name, B)
    y = oc.frames(11, (first, N, D), np.complex64)
    s = oc.saliency(11, (first, K, N), np.float32)
    if (batch or B) > first:
        level = (1 + np.arange(B // first, dtype=np.float32) / 64)[:, None, None, None]
        y = (level * y).reshape(B, N, D)
        s = np.tile(s, (B // first, 1, 1))
    return y[:batch], s[:batch]


def work(name):
    """(bytes, flop) of fit and log_pdf: compulsory traffic and the arithmetic of the algorithm
    (complex multiply-add = 8 flop; lower triangle only)."""
    B, N, D = CONFIGS[name]
    tri = D * (D + 1) // 2
    fit = (B * N * D * 8 + B * K * N * 4 + B * K * D * D * 16, B * K * N * (tri * 8 + 2 * tri))
    lp = (B * N * D * 8 + B * K * D * D * 16 + B * K * N * 8,
          B * K * (N * (D * (D - 1) // 2 * 8 + 6 * D) + D ** 3 // 3 * 8))
    return {'fit': fit, 'log_pdf': lp}


def torch_fit(y, s):
    import torch
    y = y.to(torch.complex128)
    s = s.to(torch.float64)
    den = s.sum(-1).clamp(min=float(np.finfo(np.float32).tiny))
    cov = torch.einsum('bkn,bnd,bne->bkde', s.to(torch.complex128), y, y.conj())
    return cov / den[..., None, None]


def torch_log_pdf(y, cov):
    import torch
    D = y.shape[-1]
    L = torch.linalg.cholesky(cov)
    yt = y.to(torch.complex128).transpose(-1, -2)[:, None].expand(-1, cov.shape[1], -1, -1)
    z = torch.linalg.solve_triangular(L, yt, upper=False)
    quad = (z.real ** 2 + z.imag ** 2).sum(-2)
    log_det = 2 * torch.log(torch.diagonal(L, dim1=-2, dim2=-1).real).sum(-1)
    return -D * np.log(np.pi) - log_det[..., None] - quad


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


def measure(ours, spelled, reps, torch_reps):
    from pb_bss_amd import engine
    value, first = timed(ours, 1)
    timed(ours, 3)
    value, times = timed(ours, reps)
    engine.set_timing(True)
    kernel = []
    for _ in range(5):
        ours()
        kernel.append(engine.last_kernel_ms() * 1e3)
    engine.set_timing(False)
    out = {'ours_us': float(np.median(times)), 'ours_min_us': float(min(times)),
           'kernel_us': float(np.median(kernel)), 'first_call_us': first[0]}
    try:
        timed(spelled, 2)
        torch_value, torch_times = timed(spelled, torch_reps)
        out['torch_us'] = float(np.median(torch_times))
    except RuntimeError as error:  # an operator torch does not have for this dtype on this build
        out['torch_error'] = str(error).splitlines()[0][:200]
        torch_value = None
    return value, torch_value, out


def child(name, reps, torch_reps, out_path):
    import torch
    from pb_bss_amd import engine
    y, s = (torch.from_numpy(v).cuda() for v in inputs(name))
    cov, torch_cov, fit = measure(lambda: engine.ccsg_fit(y, s), lambda: torch_fit(y, s), reps,
                                  torch_reps)
    lp, torch_lp, log_pdf = measure(lambda: engine.ccsg_log_pdf(y, cov)[0],
                                    lambda: torch_log_pdf(y, cov), reps, torch_reps)
    # a slice of the results for the comparison with the host restatement
    keep = HOST_SLICE.get(name, y.shape[0])
    arrays = {'cov': cov[:keep].cpu().numpy(), 'lp': lp[:keep].cpu().numpy()}
    if torch_cov is not None:
        arrays['torch_cov'] = torch_cov[:keep].cpu().numpy()
    if torch_lp is not None:
        arrays['torch_lp'] = torch_lp[:keep].cpu().numpy()
    np.savez(out_path, **arrays)
    print(json.dumps({'fit': fit, 'log_pdf': log_pdf}))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--torch-reps', type=int, default=5)
    parser.add_argument('--limit', type=float, default=240.0)
    parser.add_argument('--out')
    parser.add_argument('--child', choices=list(CONFIGS))
    parser.add_argument('--child-out')
    args = parser.parse_args()
    if args.child:
        return child(args.child, args.reps, args.torch_reps, args.child_out)

    import tempfile
    import oracle_ccsg as oc
    entries = []
    for name, (B, N, D) in CONFIGS.items():
        entry = {'entry': name, 'B': B, 'N': N, 'D': D, 'K': K}
        with tempfile.TemporaryDirectory() as tmp:
            results = os.path.join(tmp, 'results.npz')
            try:
                done = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), '--child', name, '--reps',
                     str(args.reps), '--torch-reps', str(args.torch_reps), '--child-out', results],
                    stdout=subprocess.PIPE, timeout=args.limit, check=True, text=True)
            except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as error:
                entry['error'] = repr(error)
                entries.append(entry)
                break  # nothing more on the device after a failure
            entry.update(json.loads(done.stdout.strip().splitlines()[-1]))
            with np.load(results) as f:
                got = {k: f[k] for k in f.files}
        keep = HOST_SLICE.get(name, B)
        y, s = inputs(name, keep)
        host = {}
        t0 = time.perf_counter()
        host['cov'] = oc.fit(y[:, None], s)
        entry['fit']['host_ms'] = (time.perf_counter() - t0) * 1e3 * (B / keep)
        t0 = time.perf_counter()
        host['lp'] = oc.log_pdf(y[:, None], got['cov'])
        entry['log_pdf']['host_ms'] = (time.perf_counter() - t0) * 1e3 * (B / keep)
        for what, key in (('fit', 'cov'), ('log_pdf', 'lp')):
            e = entry[what]
            e['bytes'], e['flop'] = work(name)[what]
            if keep != B:
                e['host_extrapolated'] = True
            e['host_over_ours'] = e['host_ms'] * 1e3 / e['ours_us']
            e['max_difference'] = float(np.abs(got[key] - host[key]).max())
            if 'torch_us' in e:
                e['torch_over_ours'] = e['torch_us'] / e['ours_us']
                e['loses_to_torch'] = e['torch_over_ours'] < 1.0
                e['torch_max_difference'] = float(np.abs(got['torch_' + key] - host[key]).max())
        entries.append(entry)
    line = json.dumps({'bench': 'ccsg', 'entries': entries})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 1 if any('error' in entry for entry in entries) else 0


if __name__ == '__main__':
    sys.exit(main())
