"""Time of the frame-recursive MVDR beamformer on the device (csrc/online_bf.hip through
`pb_bss_amd.extraction.recursive_mvdr_souden` and `OnlineMVDR.step_frame`) next to the same
recursion spelled in torch ops on the same GPU (complex128, per-frame `einsum` / outer products)
and next to the float64 NumPy restatement on the host (tests/oracle_online_beamformer.py).

Entries (complex64 frames (F, D, T), float64 masks, alpha 0.99, reference channel 0, vectors
requested):
    f513_d8       F = 513, T = 500, D = 8, one utterance
    f513_d8_x8    the same, 8 utterances (B = 4104)
    f257_d6       F = 257, T = 800, D = 6
    f257_d6_x8    the same, 8 utterances (B = 2056)
    step_frame    OnlineMVDR(F = 513, D = 8).step_frame: the time of one call, state on the device
Per entry: ours_us (median of --reps warm calls, wall time around a call that ends with a device
synchronise), ours_min_us, kernel_us (device events around the launch), per_frame_us (kernel_us
/ T: the serial chain of one bin, all bins running side by side), fp64_frac and hbm_frac (the
operations and bytes the recursion needs, counted from the shapes below, over kernel_us, against
78.6 TFLOP/s of FP64 vector peak and 8 TB/s), first_call_us, torch_us, torch_over_ours,
loses_to_torch, host_ms (the restatement on 4 bins, times B / 4: `host_extrapolated`),
max_difference (device against the restatement on those bins, relative to max |X|) and
torch_max_difference.  Nothing is promised: an entry that loses says so.  One JSON line; --out
writes it to a file as well.

Every device measurement runs in a child process under its own time limit (--limit seconds);
after a child that fails or runs out of time nothing more is started on the device.

    python tools/bench_online_beamformer.py [--reps 20] [--limit 240] \
        [--out profiles/online_beamformer.json]
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

ALPHA, REF, P0, HOST_BINS = 0.99, 0, 1.0, 4
FP64_VALU_PEAK_TF, HBM_PEAK_GBS = 78.6, 8000.0
# name: (F, D, T, utterances)
CONFIGS = {'f513_d8': (513, 8, 500, 1), 'f513_d8_x8': (513, 8, 500, 8),
           'f257_d6': (257, 6, 800, 1), 'f257_d6_x8': (257, 6, 800, 8),
           'step_frame': (513, 8, 200, 1)}


def flops_per_frame(D):
    """Real float64 operations of one frame of the definition: the two Hermitian updates on full
    matrices (8 D^2 + 2 D^2 each with the scaling), two matrix-vector products (8 D^2 each),
    Re tr (4 D^2), den and x (8 D each)."""
    return 40 * D * D + 16 * D


def bytes_per_frame(D):
    """complex64 frame in, two float64 masks in, complex64 x and complex128 w out."""
    return 8 * D + 16 + 8 + 16 * D


def inputs(name):
    """(U * F, D, T) complex64 and two (U * F, T) float64 masks: the first utterance at U levels."""
    F, D, T, U = CONFIGS[name]
    rng = np.random.default_rng(21)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    active = rng.uniform(size=(F, 1, T)) < 0.6
    y = (cn(F, D, 1) * cn(F, 1, T) * active + 0.3 * cn(F, D, T)).astype(np.complex64)
    s = np.clip(0.75 * active[:, 0] + 0.1 * rng.standard_normal((F, T)), 0.0, 1.0)
    level = (1 + np.arange(U, dtype=np.float32) / 64)[:, None, None, None]
    return ((level * y).reshape(U * F, D, T), np.tile(s, (U, 1)), np.tile(1.0 - s, (U, 1)))


class TorchRecursion:
    """The recursion in torch ops, one frame per step()."""

    def __init__(self, B, D, alpha, ref, p0, device):
        import torch
        self.alpha, self.ref = alpha, ref
        self.Phi = torch.zeros((B, D, D), dtype=torch.complex128, device=device)
        self.Psi = (torch.eye(D, dtype=torch.complex128, device=device) / p0).expand(
            B, D, D).contiguous()
        self.tiny = float(np.finfo(np.float64).tiny)

    def step(self, frame, s, v):
        import torch
        y = frame.to(torch.complex128)
        self.Phi = self.alpha * self.Phi + s[:, None, None] * (y[:, :, None] * y.conj()[:, None, :])
        n = torch.einsum('bij,bj->bi', self.Psi, y)
        den = self.alpha + v * (y.conj() * n).sum(-1).real
        k = (v / den)[:, None] * n
        self.Psi = (self.Psi - k[:, :, None] * n.conj()[:, None, :]) / self.alpha
        q = torch.einsum('bij,bj->bi', self.Psi, self.Phi[:, :, self.ref])
        lam = (self.Psi.real * self.Phi.real + self.Psi.imag * self.Phi.imag).sum((1, 2))
        w = q / lam.clamp_min(self.tiny)[:, None]
        return (w.conj() * y).sum(-1)


def torch_recursive(y, s, v):
    import torch
    B, D, T = y.shape
    rec = TorchRecursion(B, D, ALPHA, REF, P0, y.device)
    return torch.stack([rec.step(y[:, :, t], s[:, t], v[:, t]) for t in range(T)],
                       dim=-1).to(y.dtype)


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


def child(name, reps, torch_reps, out_path):
    import torch
    from pb_bss_amd import extraction
    F, D, T, U = CONFIGS[name]
    y, s, v = (torch.from_numpy(a).cuda() for a in inputs(name))
    if name == 'step_frame':
        online = extraction.OnlineMVDR(D, F, ALPHA, REF, P0)
        frames = y.transpose(1, 2).contiguous()  # (F, T, D)
        st, vt = s.t().contiguous(), v.t().contiguous()
        state = {'t': 0}

        def ours():
            state['t'] += 1
            i = state['t'] % T
            return online.step_frame(frames[:, i], st[i], vt[i])
        rec = TorchRecursion(F, D, ALPHA, REF, P0, y.device)

        def spelled():
            state['t'] += 1
            i = state['t'] % T
            return rec.step(frames[:, i], st[i], vt[i])
        x, first = timed(ours, 1)
        timed(ours, 10)
        _, times = timed(ours, reps * 5)
        out = {'ours_us': float(np.median(times)), 'ours_min_us': float(min(times)),
               'kernel_us': kernel_us(ours), 'first_call_us': first[0]}
        timed(spelled, 10)
        _, ttimes = timed(spelled, reps * 5)
        out['torch_us'] = float(np.median(ttimes))
        print(json.dumps(out))
        return

    def ours():
        return extraction.recursive_mvdr_souden(y, s, v, ALPHA, REF, P0, return_vector=True)[0]
    x, first = timed(ours, 1)
    timed(ours, 2)
    x, times = timed(ours, reps)
    out = {'ours_us': float(np.median(times)), 'ours_min_us': float(min(times)),
           'kernel_us': kernel_us(ours), 'first_call_us': first[0]}
    out['per_frame_us'] = out['kernel_us'] / T
    seconds = out['kernel_us'] * 1e-6
    out['fp64_frac'] = flops_per_frame(D) * T * F * U / seconds / 1e12 / FP64_VALU_PEAK_TF
    out['hbm_frac'] = bytes_per_frame(D) * T * F * U / seconds / 1e9 / HBM_PEAK_GBS
    arrays = {'x': x[:HOST_BINS].cpu().numpy()}
    if torch_reps > 0:
        try:
            def spelled():
                return torch_recursive(y, s, v)
            timed(spelled, 1)
            tx, ttimes = timed(spelled, torch_reps)
            out['torch_us'] = float(np.median(ttimes))
            arrays['torch_x'] = tx[:HOST_BINS].cpu().numpy()
        except RuntimeError as error:
            out['torch_error'] = str(error).splitlines()[0][:200]
    np.savez(out_path, **arrays)
    print(json.dumps(out))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=20)
    parser.add_argument('--torch-reps', type=int, default=2)
    parser.add_argument('--limit', type=float, default=240.0)
    parser.add_argument('--out')
    parser.add_argument('--child', choices=list(CONFIGS))
    parser.add_argument('--child-out')
    args = parser.parse_args()
    if args.child:
        return child(args.child, args.reps, args.torch_reps, args.child_out)

    import tempfile
    import oracle_online_beamformer as oo
    entries, failed = [], False
    for name, (F, D, T, U) in CONFIGS.items():
        if failed:
            break  # nothing more on the device after a failure
        entry = {'entry': name, 'F': F, 'D': D, 'T': T, 'utterances': U, 'alpha': ALPHA,
                 'ref_channel': REF, 'initial_noise_power': P0}
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
                failed = True
                continue
            entry.update(json.loads(done.stdout.strip().splitlines()[-1]))
            got = {}
            if os.path.exists(results):
                with np.load(results) as f:
                    got = {k: f[k] for k in f.files}
        if 'x' in got:
            y, s, v = (a[:HOST_BINS] for a in inputs(name))
            t0 = time.perf_counter()
            host = oo.recursive(y, s, v, ALPHA, REF, P0)[0]
            entry['host_ms'] = (time.perf_counter() - t0) * 1e3 * F * U / HOST_BINS
            entry['host_extrapolated'] = True
            entry['host_over_ours'] = entry['host_ms'] * 1e3 / entry['ours_us']
            scale = np.abs(host).max()
            entry['max_difference'] = float(
                np.abs(got['x'] - host.astype(np.complex64)).max() / scale)
            if 'torch_x' in got:
                entry['torch_max_difference'] = float(
                    np.abs(got['torch_x'] - host.astype(np.complex64)).max() / scale)
        if 'torch_us' in entry:
            entry['torch_over_ours'] = entry['torch_us'] / entry['ours_us']
            entry['loses_to_torch'] = entry['torch_over_ours'] < 1.0
        entries.append(entry)
        print(f'{name}: done', file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'online_beamformer', 'entries': entries})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
