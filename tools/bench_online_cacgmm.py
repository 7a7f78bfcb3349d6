"""Time of the frame-recursive cACGMM mask estimator on the device (csrc/online_cacgmm.hip
through `pb_bss_amd.distribution.recursive_cacgmm` and `OnlineCACGMM.step_frame`) next to the same
recursion spelled in torch ops on the same GPU (complex128, all bins in one batch, one frame per
step) and next to the float64 NumPy restatement on the host (tests/oracle_online_cacgmm.py).

Entries (complex64 frames (F, D, T), alpha 0.99, affiliation_eps 1e-10, weights updated, the
quadratic form requested):
    f513_d8_k3       F = 513, T = 500, D = 8, K = 3, one utterance
    f513_d8_k3_x8    the same, 8 utterances (B = 4104)
    f257_d6_k3       F = 257, T = 800, D = 6, K = 3
    f257_d6_k3_x8    the same, 8 utterances (B = 2056)
    step_frame       OnlineCACGMM(F = 513, D = 8, K = 3).step_frame: the time of one call
Per entry: ours_us (median of --reps warm calls, wall time around a call that ends with a device
synchronise), ours_min_us, kernel_us (device events around the launch), per_frame_us (kernel_us
/ T: the serial chain of one bin, all bins running side by side), fp64_frac and hbm_frac (the
operations and bytes the recursion needs, counted from the shapes below, over kernel_us, against
78.6 TFLOP/s of FP64 vector peak and 8 TB/s), first_call_us, torch_us, torch_over_ours,
loses_to_torch, host_ms (the restatement on 4 bins, times B / 4: `host_extrapolated`),
max_difference (device against the restatement on those bins: the largest of gamma, q relative to
their maxima), share_of_floor_bound (max_difference over 16 * 1e-13, the floor of the bound of
tests/test_gpu_online_cacgmm.py) and torch_max_difference.  Nothing is promised: an entry that
loses says so.  One JSON line; --out writes it to a file as well.

Every device measurement runs in a child process under its own time limit (--limit seconds);
after a child that fails or runs out of time nothing more is started on the device.

    python tools/bench_online_cacgmm.py [--reps 20] [--limit 240] \
        [--out profiles/online_cacgmm.json]
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

ALPHA, EPS_AFF, COUNT0, HOST_BINS = 0.99, 1e-10, 10.0, 4
FP64_VALU_PEAK_TF, HBM_PEAK_GBS = 78.6, 8000.0
# name: (F, D, K, T, utterances)
CONFIGS = {'f513_d8_k3': (513, 8, 3, 500, 1), 'f513_d8_k3_x8': (513, 8, 3, 500, 8),
           'f257_d6_k3': (257, 6, 3, 800, 1), 'f257_d6_k3_x8': (257, 6, 3, 800, 8),
           'step_frame': (513, 8, 3, 200, 1)}


def flops_per_frame(D, K):
    """Real float64 operations of one frame of the definition: per class the matrix-vector
    product (8 D^2), the Hermitian rank-one update with its scaling on the full matrix (10 D^2)
    and q (4 D); the normalisation of the frame (6 D); the scalars are not counted."""
    return K * (18 * D * D + 4 * D) + 6 * D


def bytes_per_frame(D, K):
    """complex64 frame in, float64 gamma and q out."""
    return 8 * D + 16 * K


def inputs(name):
    """(U * F, D, T) complex64 -- the first utterance at U levels -- and the initial state
    (P0 (U * F, K, D, D), L0, Lambda0, pi0 (U * F, K)): K steering vectors per bin, a random
    active class per frame, sensor noise of standard deviation 0.3; B0_k = a_k a_k^H + 0.3 I."""
    F, D, K, T, U = CONFIGS[name]
    rng = np.random.default_rng(21)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    steer = cn(F, K, D)
    active = rng.integers(0, K, size=(F, T))
    y = np.take_along_axis(steer, active[:, :, None], axis=1).swapaxes(1, 2) * cn(F, 1, T)
    y = (y + 0.3 * cn(F, D, T)).astype(np.complex64)
    B0 = steer[..., :, None] * steer[..., None, :].conj() + 0.3 * np.eye(D)
    P0, L0 = np.linalg.inv(B0), np.linalg.slogdet(B0)[1]
    pi0 = np.full((F, K), 1.0 / K)
    level = (1 + np.arange(U, dtype=np.float32) / 64)[:, None, None, None]
    state = tuple(np.tile(a, (U,) + (1,) * (a.ndim - 1)) for a in (P0, L0, COUNT0 * pi0, pi0))
    return (level * y).reshape(U * F, D, T), state


def device_state(state):
    import torch
    from pb_bss_amd import distribution
    P, L, Lam, pi = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in state)
    return distribution.OnlineCACGMMState(
        P, L, Lam, pi, torch.zeros((P.shape[0],), dtype=torch.int64, device='cuda'))


class TorchRecursion:
    """The recursion in torch ops, one frame per step(), all bins in one batch."""

    def __init__(self, state, alpha, eps):
        self.P, self.L, self.Lam, self.pi = (a.clone() for a in state)
        self.alpha, self.eps = alpha, eps

    def step(self, frame):
        import torch
        y = frame.to(torch.complex128)
        D = y.shape[-1]
        nu = y.abs().square().sum(-1).sqrt()
        live = nu > 0
        z = y / torch.where(live, nu, torch.ones_like(nu))[:, None]
        n = torch.einsum('bkij,bj->bki', self.P, z)
        q = (z.conj()[:, None, :] * n).sum(-1).real
        lp = self.pi.log() - self.L - D * q.log()
        gamma = torch.softmax(lp, dim=1).clamp(self.eps, 1 - self.eps)
        old = self.alpha * self.Lam
        new, den = old + gamma, old + D * gamma
        coef = D * gamma / (q * den)
        P = (self.P - (coef[..., None] * n)[..., :, None] * n.conj()[..., None, :]) * \
            (new / old)[..., None, None]
        keep = live[:, None]
        self.P = torch.where(keep[..., None, None], P, self.P)
        self.L = torch.where(keep, self.L + D * (old / new).log() + (den / old).log(), self.L)
        self.Lam = torch.where(keep, new, self.Lam)
        gamma = torch.where(keep, gamma, self.pi)
        self.pi = self.Lam / self.Lam.sum(1, keepdim=True)
        return gamma, torch.where(keep, q, torch.zeros_like(q))


def torch_recursive(y, state):
    import torch
    rec = TorchRecursion(state, ALPHA, EPS_AFF)
    steps = [rec.step(y[:, :, t]) for t in range(y.shape[2])]
    return torch.stack([g for g, _ in steps], dim=-1), torch.stack([q for _, q in steps], dim=-1)


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
    from pb_bss_amd import distribution
    F, D, K, T, U = CONFIGS[name]
    y, state = inputs(name)
    y = torch.from_numpy(y).cuda()
    st = device_state(state)
    tstate = (st.precision, st.log_determinant, st.count, st.weight)
    if name == 'step_frame':
        online = distribution.OnlineCACGMM(st, ALPHA, affiliation_eps=EPS_AFF)
        frames = y.transpose(1, 2).contiguous()  # (F, T, D)
        at = {'t': 0}

        def ours():
            at['t'] += 1
            return online.step_frame(frames[:, at['t'] % T])
        rec = TorchRecursion(tstate, ALPHA, EPS_AFF)

        def spelled():
            at['t'] += 1
            return rec.step(frames[:, at['t'] % T])
        _, first = timed(ours, 1)
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
        return distribution.recursive_cacgmm(y, None, ALPHA, affiliation_eps=EPS_AFF, state=st,
                                             return_quadratic_form=True)
    _, first = timed(ours, 1)
    timed(ours, 2)
    (g, q), times = timed(ours, reps)
    out = {'ours_us': float(np.median(times)), 'ours_min_us': float(min(times)),
           'kernel_us': kernel_us(ours), 'first_call_us': first[0]}
    out['per_frame_us'] = out['kernel_us'] / T
    seconds = out['kernel_us'] * 1e-6
    out['fp64_frac'] = flops_per_frame(D, K) * T * F * U / seconds / 1e12 / FP64_VALU_PEAK_TF
    out['hbm_frac'] = bytes_per_frame(D, K) * T * F * U / seconds / 1e9 / HBM_PEAK_GBS
    arrays = {'gamma': g[:HOST_BINS].cpu().numpy(), 'q': q[:HOST_BINS].cpu().numpy()}
    if torch_reps > 0:
        try:
            def spelled():
                return torch_recursive(y, tstate)
            timed(spelled, 1)
            (tg, tq), ttimes = timed(spelled, torch_reps)
            out['torch_us'] = float(np.median(ttimes))
            arrays['torch_gamma'] = tg[:HOST_BINS].cpu().numpy()
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
    import oracle_online_cacgmm as oc
    entries, failed = [], False
    for name, (F, D, K, T, U) in CONFIGS.items():
        if failed:
            break  # nothing more on the device after a failure
        entry = {'entry': name, 'F': F, 'D': D, 'K': K, 'T': T, 'utterances': U, 'alpha': ALPHA,
                 'affiliation_eps': EPS_AFF, 'initial_count': COUNT0}
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
        if 'gamma' in got:
            y, state = inputs(name)
            t0 = time.perf_counter()
            host = oc.recursive(y[:HOST_BINS], tuple(a[:HOST_BINS] for a in state), ALPHA, EPS_AFF)
            entry['host_ms'] = (time.perf_counter() - t0) * 1e3 * F * U / HOST_BINS
            entry['host_extrapolated'] = True
            entry['host_over_ours'] = entry['host_ms'] * 1e3 / entry['ours_us']
            entry['max_difference'] = max(oc.relative(got['gamma'], host[0], 'gamma'),
                                          oc.relative(got['q'], host[1], 'q'))
            entry['share_of_floor_bound'] = entry['max_difference'] / (16 * 1e-13)
            if 'torch_gamma' in got:
                entry['torch_max_difference'] = oc.relative(got['torch_gamma'], host[0], 'gamma')
        if 'torch_us' in entry:
            entry['torch_over_ours'] = entry['torch_us'] / entry['ours_us']
            entry['loses_to_torch'] = entry['torch_over_ours'] < 1.0
        entries.append(entry)
        print(f'{name}: done', file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'online_cacgmm', 'entries': entries})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
