"""Device time of the evaluation metrics (csrc/eval.hip) next to the same metrics written with
torch ops on the same device tensors, the NumPy restatement of the reference on the host
(tests/oracle_evaluation.py, input already in host memory) and the device-to-device copy
bandwidth measured in the same run.

Sizes: 1 and --batch utterances, K_source = 3, K_target = 3 and 4, N = 128 000 samples (8 s at
16 kHz), float32 and float64.  `si_sdr` scores all K_source x K_target pairs (the outer form),
`output_sxr` takes (B, K_source, K_target, N) contributions, `input_sxr` (B, K_source, D =
K_target, N) images.  Bytes are counted from the shapes; `si_sdr` reads its rows twice.  Per
entry: ours_us / torch_us (median of --reps calls between device events after warm-up),
numpy_host_us (one call), bytes, the share of the copy bandwidth that traffic over ours_us is,
torch_over_ours, numpy_over_ours, and the largest difference in dB between the device result
and the restatement.  One JSON line; --out writes it to a file as well.

    python tools/bench_evaluation.py [--reps 20] [--batch 64] [--out profiles/evaluation.json]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

KS, N = 3, 128000


def device_us(fn, reps, warmup=3):
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


def copy_bandwidth(reps=10):
    """bytes read + bytes written per second of a device-to-device copy of 1 GiB"""
    import torch
    src = torch.empty(1 << 28, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    med, _ = device_us(lambda: dst.copy_(src), reps)
    return 2 * src.numel() * 4 / (med * 1e-6)


# ---- the torch formulations -----------------------------------------------------------------
def t_si_sdr(r, e):
    import torch
    r, e = r.double(), e.double()
    alpha = (r * e).sum(-1, keepdim=True) / (r * r).sum(-1, keepdim=True)
    target = alpha * r
    residual = e - target
    return 10 * torch.log10((target * target).sum(-1) / (residual * residual).sum(-1))


def t_power(x):
    x = x.double()
    return (x * x).mean(-1)


def t_output_sxr(co, no, selections):
    """selections (P, Ks) int64 on the device, itertools.permutations order"""
    import torch
    S, Np = t_power(co), t_power(no)
    Ks = S.shape[1]
    totals = S[:, torch.arange(Ks, device=S.device), selections].sum(-1)  # (B, P)
    sel = selections[totals.argmax(-1)]                                    # (B, Ks)
    picked = S.gather(2, sel[:, None, :].expand(-1, Ks, -1))               # S[b, n, sel[b, k]]
    SS = picked.diagonal(dim1=1, dim2=2)
    II = picked.sum(1) - SS
    NN = Np.gather(1, sel)
    return [(10 * torch.log10(SS / x)).mean(-1) for x in (II + NN, II, NN)], sel


def t_input_sxr(im, no):
    import torch
    S, Np = t_power(im), t_power(no)
    I = S.sum(1, keepdim=True) - S
    S, I, Np = S.mean(-1), I.mean(-1), Np.mean(-1, keepdim=True)
    return [(10 * torch.log10(S / x)).mean(-1) for x in (I + Np, I, Np)]


def host_us(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def difference(got, want):
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, 'detach') else got)
    want = np.asarray(want)
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)
    return float(np.abs(got[finite] - want[finite]).max()) if finite.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import oracle_evaluation as oe
    from pb_bss_amd.evaluation import si_sdr
    from pb_bss_amd.evaluation.sxr_module import input_sxr, output_sxr
    bandwidth = copy_bandwidth()
    out = {'samples': N, 'K_source': KS, 'copy_bytes_per_s': bandwidth,
           'copy_bytes_counted': 'read + written', 'entries': []}
    print({'copy_bytes_per_s': bandwidth}, file=sys.stderr, flush=True)
    gen = torch.Generator(device='cuda').manual_seed(0)

    def randn(*shape):
        return torch.randn(shape, generator=gen, device='cuda', dtype=torch.float64)

    for B, Kt, dtype in itertools.product((1, args.batch), (3, 4), (torch.float32, torch.float64)):
        size = 4 if dtype == torch.float32 else 8
        reps = args.reps if B == 1 else max(5, args.reps // 4)
        # sources, their mixtures as estimates; every source strongest in an output of its own
        sources = randn(B, KS, N)
        gain = 0.1 + 0.3 * torch.rand((B, KS, Kt), generator=gen, device='cuda', dtype=torch.float64)
        home = torch.argsort(torch.rand((B, Kt), generator=gen, device='cuda'), dim=-1)[:, :KS]
        gain.scatter_(2, home[:, :, None], 1.0 + torch.rand((B, KS, 1), generator=gen,
                                                            device='cuda', dtype=torch.float64))
        co = (gain[..., None] * sources[:, :, None, :] * (1 + 0.1 * randn(B, KS, Kt, N))).to(dtype)
        no = (0.2 * randn(B, Kt, N)).to(dtype)
        ref = sources.to(dtype)[:, :, None, :]                    # (B, Ks, 1, N)
        est = (co.double().sum(1) + no.double()).to(dtype)[:, None]  # (B, 1, Kt, N)
        selections = torch.tensor(list(itertools.permutations(range(Kt), KS)), device='cuda')
        co_h, no_h, ref_h, est_h = (x.double().cpu().numpy() for x in (co, no, ref, est))
        families = [
            ('si_sdr', lambda: si_sdr(ref, est), lambda: t_si_sdr(ref, est),
             lambda: oe.si_sdr(ref_h, est_h), 2 * (ref.numel() + est.numel()) * size),
            ('output_sxr', lambda: output_sxr(co, no).sdr,
             lambda: t_output_sxr(co, no, selections)[0][0],
             lambda: oe.output_sxr(co_h, no_h)[0].sdr, (co.numel() + no.numel()) * size),
            ('input_sxr', lambda: input_sxr(co, no).sdr, lambda: t_input_sxr(co, no)[0],
             lambda: oe.input_sxr(co_h, no_h).sdr, (co.numel() + no.numel()) * size),
        ]
        for name, ours, theirs, restated, nbytes in families:
            numpy_us, want = host_us(restated)
            worst = difference(ours(), want)
            torch_gap = difference(theirs(), want)
            med, best = device_us(ours, reps)
            tmed, tbest = device_us(theirs, reps)
            e = dict(function=name, utterances=B, K_target=Kt,
                     dtype=str(dtype).replace('torch.', ''), ours_us=med, ours_us_min=best,
                     torch_us=tmed, torch_us_min=tbest, numpy_host_us=numpy_us, bytes=nbytes,
                     copy_bandwidth_fraction=nbytes / (med * 1e-6) / bandwidth,
                     torch_over_ours=tmed / med, numpy_over_ours=numpy_us / med,
                     largest_difference_db=worst, torch_largest_difference_db=torch_gap)
            out['entries'].append(e)
            print({k: (round(v, 4) if isinstance(v, float) and k.endswith(('us', 'ours', 'fraction'))
                       else v) for k, v in e.items()}, file=sys.stderr, flush=True)
        del co, no, ref, est, sources
        torch.cuda.empty_cache()
    out['largest_difference_db'] = {
        name: max(e['largest_difference_db'] for e in out['entries'] if e['function'] == name)
        for name in ('si_sdr', 'output_sxr', 'input_sxr')}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
