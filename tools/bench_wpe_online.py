"""Time of frame-recursive WPE on the device (csrc/wpe_online.hip through
`pb_bss_amd.transform.recursive_wpe` and `OnlineWPE.step_frame`) next to the same recursion spelled
in torch ops on the same GPU (complex128, per-frame `einsum`, the textbook full-matrix update) and
next to the float64 NumPy restatement on the host (tests/oracle_wpe_online.py).

Entries (complex64 frames (F, D, T), taps 10, delay 3, alpha 0.9999, the causal power):
    f513_d8       F = 513, T = 500, D = 8, one utterance
    f513_d8_x8    the same, 8 utterances (B = 4104)
    f257_d6       F = 257, T = 800, D = 6
    step_frame    OnlineWPE(F = 513, D = 8).step_frame: the time of one call, state on the device
    m20, m32      F = 513, T = 500, D = 2 with 10 and 16 taps: small D * taps on the same
                  four-wavefront workgroup (no torch or host run)
Per entry: ours_us (median of --reps warm calls, wall time around a call that ends with a device
synchronise), ours_min_us, kernel_us (device events around the launch), per_frame_us (kernel_us
/ T: the serial chain of one bin, all bins running side by side), first_call_us, torch_us,
torch_over_ours, loses_to_torch, host_ms (the restatement on 4 bins, times F / 4:
`host_extrapolated`), max_difference (device against the restatement on those bins, relative to
max |X|) and torch_max_difference.  Nothing is promised: an entry that loses says so.  One JSON
line; --out writes it to a file as well.

Every device measurement runs in a child process under its own time limit (--limit seconds);
after a child that fails or runs out of time nothing more is started on the device.

    python tools/bench_wpe_online.py [--reps 20] [--limit 240] [--out profiles/wpe_online.json]
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

DELAY, ALPHA, HOST_BINS = 3, 0.9999, 4
# name: (F, D, T, utterances, taps, compared with torch and the host)
CONFIGS = {'f513_d8': (513, 8, 500, 1, 10, True), 'f513_d8_x8': (513, 8, 500, 8, 10, True),
           'f257_d6': (257, 6, 800, 1, 10, True), 'step_frame': (513, 8, 200, 1, 10, True),
           'm20': (513, 2, 500, 1, 10, False), 'm32': (513, 2, 500, 1, 16, False)}


def inputs(name):
    """(U * F, D, T) complex64: the first utterance at U levels."""
    import oracle_wpe as ow
    F, D, T, U = CONFIGS[name][:4]
    y = ow.synth(F, D, T, seed=21).astype(np.complex64)
    level = (1 + np.arange(U, dtype=np.float32) / 64)[:, None, None, None]
    return (level * y).reshape(U * F, D, T)


class TorchRecursion:
    """The recursion in torch ops, one frame per step()."""

    def __init__(self, B, D, taps, delay, alpha, device):
        import torch
        self.taps, self.delay, self.alpha, self.H = taps, delay, alpha, taps + delay
        M = D * taps
        self.P = torch.eye(M, dtype=torch.complex128, device=device).expand(B, M, M).contiguous()
        self.G = torch.zeros((B, M, D), dtype=torch.complex128, device=device)
        self.buf = torch.zeros((B, self.H + 1, D), dtype=torch.complex128, device=device)
        self.seen = 0

    def step(self, frame):
        import torch
        self.buf = torch.cat([self.buf[:, 1:], frame.to(torch.complex128)[:, None]], dim=1)
        self.seen += 1
        lam = (self.buf.real ** 2 + self.buf.imag ** 2).sum((1, 2)) / (
            self.buf.shape[2] * min(self.seen, self.H + 1))
        B = frame.shape[0]
        last = self.H - self.delay  # tap k reads buf[:, last - k]
        yt = self.buf[:, last - self.taps + 1:last + 1].flip(1).reshape(B, -1)
        x = self.buf[:, -1] - torch.einsum('bmd,bm->bd', self.G.conj(), yt)
        n = torch.einsum('bij,bj->bi', self.P, yt)
        den = self.alpha * lam + (yt.conj() * n).sum(-1).real
        k = torch.where(den[:, None] > 0, n / den[:, None], torch.zeros_like(n))
        self.P = (self.P - k[:, :, None] * n.conj()[:, None, :]) / self.alpha
        self.G = self.G + k[:, :, None] * x.conj()[:, None, :]
        return x


def torch_recursive(y, taps, delay, alpha):
    import torch
    B, D, T = y.shape
    rec = TorchRecursion(B, D, taps, delay, alpha, y.device)
    return torch.stack([rec.step(y[:, :, t]) for t in range(T)], dim=-1).to(y.dtype)


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
    from pb_bss_amd import transform
    F, D, T, U, taps, _ = CONFIGS[name]
    y = torch.from_numpy(inputs(name)).cuda()
    if name == 'step_frame':
        online = transform.OnlineWPE(taps, DELAY, ALPHA, channel=D, frequency_bins=F)
        frames = y.transpose(1, 2).contiguous()  # (F, T, D)
        state = {'t': 0}

        def ours():
            state['t'] += 1
            return online.step_frame(frames[:, state['t'] % T])
        rec = TorchRecursion(F, D, taps, DELAY, ALPHA, y.device)

        def spelled():
            state['t'] += 1
            return rec.step(frames[:, state['t'] % T])
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
        return transform.recursive_wpe(y, taps, DELAY, ALPHA)
    x, first = timed(ours, 1)
    timed(ours, 2)
    x, times = timed(ours, reps)
    out = {'ours_us': float(np.median(times)), 'ours_min_us': float(min(times)),
           'kernel_us': kernel_us(ours), 'first_call_us': first[0]}
    out['per_frame_us'] = out['kernel_us'] / T
    arrays = {'x': x[:HOST_BINS].cpu().numpy()}
    if torch_reps > 0:
        try:
            def spelled():
                return torch_recursive(y, taps, DELAY, ALPHA)
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
    import oracle_wpe_online as oo
    entries, failed = [], False
    for name, (F, D, T, U, taps, compare) in CONFIGS.items():
        if failed:
            break  # nothing more on the device after a failure
        entry = {'entry': name, 'F': F, 'D': D, 'T': T, 'utterances': U, 'taps': taps,
                 'delay': DELAY, 'alpha': ALPHA}
        with tempfile.TemporaryDirectory() as tmp:
            results = os.path.join(tmp, 'results.npz')
            try:
                done = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), '--child', name, '--reps',
                     str(args.reps), '--torch-reps', str(args.torch_reps if compare else 0),
                     '--child-out', results], stdout=subprocess.PIPE, timeout=args.limit,
                    check=True, text=True)
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
            y = inputs(name)[:HOST_BINS]
            t0 = time.perf_counter()
            host = oo.recursive(y, taps, DELAY, ALPHA)[0]
            if compare:
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
    line = json.dumps({'bench': 'wpe_online', 'entries': entries})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
