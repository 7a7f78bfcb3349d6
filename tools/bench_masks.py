"""Device time of the oracle masks (csrc/masks.hip) next to the same masks written with torch
ops on the same device tensors -- what a user of the package could do before mask_module
existed -- at (K, D, F, T) = (3, 8, 513, 500) complex64, one utterance and a batch of 64.

Per mask family and size: ours_us and torch_us (median of --reps calls, device events after
warm-up), the bytes a single pass must move (images once + masks once), that traffic over the
measured time as a fraction of the 6.3 TB/s a device copy reaches, and torch_over_ours.  The
results of both formulations are compared once per family (two-valued masks: share of equal
decisions).  One JSON line; --out writes it to a file as well.

    python tools/bench_masks.py [--reps 10] [--batch 64] [--out profiles/mask_module.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

K, D, F, T = 3, 8, 513, 500
COPY_BYTES_PER_S = 6.3e12
EPS = 1e-18
WEIGHT = 0.999


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


# ---- the torch formulations: x (B, K, D, F, T) -----------------------------------------------
def t_power(x):
    return (x.real ** 2 + x.imag ** 2).sum(2)


def t_ibm(x):
    import torch
    p = t_power(x)
    best = p.argmax(1, keepdim=True)
    return (best == torch.arange(K, device=x.device).view(1, K, 1, 1)).to(p.dtype)


def t_wiener(x):
    p = t_power(x)
    return p / (p.sum(1, keepdim=True) + EPS)


def t_irm(x):
    m = x.abs()
    return m / (m.sum(1, keepdim=True) + EPS)


def t_iam(x):
    return x.abs() / (x.sum(1, keepdim=True).abs() + EPS)


def t_psm(x):
    import torch
    o = x.sum(1, keepdim=True)
    return x.abs() / (o.abs() + EPS) * torch.cos(x.angle() - o.angle())


def t_icm(x):
    return x / x.sum(1, keepdim=True)


def t_lorenz(x, fraction=0.98):
    p = (x.abs() ** 2).sum(2)
    rows = p.reshape(-1, F * T)
    s, _ = rows.sort(dim=-1, descending=True)
    lorenz = s.cumsum(-1) / s.sum(-1, keepdim=True)
    last = (lorenz < fraction).sum(-1, keepdim=True) - 1
    thr = s.gather(-1, last.clamp(min=0))
    return (0.5 + WEIGHT * ((rows > thr).to(p.dtype) - 0.5)).reshape(p.shape)


def t_quantile(x, spec, dim):
    """x real (..., N along dim); spec [(lower rank, gamma, negative)]"""
    import torch
    s, _ = x.sort(dim=dim)
    n = x.shape[dim]
    out = []
    for lower, gamma, negative in spec:
        a = s.narrow(dim, lower, 1)
        b = s.narrow(dim, min(lower + 1, n - 1), 1)
        thr = a + (b - a) * gamma
        m = (x < thr) if negative else (x > thr)
        out.append(0.5 + WEIGHT * (m.to(x.dtype) - 0.5))
    return torch.stack(out)


def t_biased(x, table):
    """x (B, 2, D, T, F)"""
    import torch
    p = x.real ** 2 + x.imag ** 2
    speech, noise = p[:, :1], p[:, 1:]
    ps, pn = speech / table[0], speech / table[1]
    ms = (ps > noise) & (ps > 0.005) & (table[2] == 0)
    mn = (pn < noise) | (pn < 0.005) | (table[2] != 0)
    return torch.cat([ms, mn], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import oracle_masks as om
    from pb_bss_amd.extraction import mask_module as mm
    out = {'shape': dict(K=K, D=D, F=F, T=T), 'dtype': 'complex64',
           'copy_bytes_per_s': COPY_BYTES_PER_S, 'entries': []}
    base = torch.from_numpy(om.gen(0, (K, D, F, T))).cuda()
    vuv = mm.voiced_unvoiced_split_characteristic(F)
    cut = np.zeros(F)
    cut[0:4] = 1  # low_cut=5; high_cut ends at axis 1 of the masks, the component axis here
    table = torch.from_numpy(np.stack([10 ** ((0 * vuv[0] + 5 * vuv[1]) / 10),
                                       10 ** ((-10 * vuv[0] - 10 * vuv[1]) / 10), cut])).cuda()
    spec = [mm._percentile_index(q, F) for q in (0.1, -0.9)]
    spec_ft = [mm._percentile_index(q, F * T) for q in (0.1, -0.9)]
    for B in (1, args.batch):
        x = base[None].expand(B, K, D, F, T).contiguous()
        xb = x[:, :2].permute(0, 1, 2, 4, 3).contiguous()  # (B, 2, D, T, F): bins last
        n_in = x.numel() * 8
        pooled, full = B * K * F * T * 4, B * K * D * F * T * 4
        families = [
            ('ideal_binary_mask', lambda: mm.ideal_binary_mask(x, 1, 2), lambda: t_ibm(x),
             n_in + pooled),
            ('wiener_like_mask', lambda: mm.wiener_like_mask(x, 1, 2), lambda: t_wiener(x),
             n_in + pooled),
            ('ideal_ratio_mask', lambda: mm.ideal_ratio_mask(x, 1), lambda: t_irm(x), n_in + full),
            ('ideal_amplitude_mask', lambda: mm.ideal_amplitude_mask(x, 1), lambda: t_iam(x),
             n_in + full),
            ('phase_sensitive_mask', lambda: mm.phase_sensitive_mask(x, 1), lambda: t_psm(x),
             n_in + full),
            ('ideal_complex_mask', lambda: mm.ideal_complex_mask(x, 1), lambda: t_icm(x),
             n_in + 2 * full),
            ('biased_binary_mask', lambda: mm.biased_binary_mask(xb, 1),
             lambda: t_biased(xb, table), xb.numel() * 8 + xb.numel()),
            ('lorenz_mask', lambda: mm.lorenz_mask(x, sensor_axis=2),
             lambda: t_lorenz(x), n_in + pooled),
            ('quantile_mask axis=-2', lambda: mm.quantile_mask(x, axis=-2),
             lambda: t_quantile(x.abs(), spec, -2), n_in + 2 * full),
            ('quantile_mask axis=(-2,-1)', lambda: mm.quantile_mask(x, axis=(-2, -1)),
             lambda: t_quantile(x.abs().reshape(B, K, D, F * T), spec_ft, -1), n_in + 2 * full),
        ]
        for name, ours, theirs, nbytes in families:
            a = ours()
            b = theirs().reshape(a.shape)
            if a.dtype.is_complex or name in ('wiener_like_mask', 'ideal_ratio_mask',
                                              'ideal_amplitude_mask', 'phase_sensitive_mask'):
                agree = float(torch.nan_to_num((a - b).abs(), nan=0.0).max())
                agreement = {'max_abs_difference': agree}
            else:
                same = (a.to(torch.float32) > 0.5) == (b.to(torch.float32) > 0.5)
                agreement = {'equal_decisions_share': float(same.double().mean())}
            del a, b
            reps = args.reps if B == 1 else max(3, args.reps // 2)
            med, best = device_us(ours, reps)
            tmed, tbest = device_us(theirs, reps)
            e = dict(mask=name, utterances=B, ours_us=med, ours_us_min=best, torch_us=tmed,
                     torch_us_min=tbest, bytes=nbytes,
                     copy_bandwidth_fraction=nbytes / (med * 1e-6) / COPY_BYTES_PER_S,
                     torch_over_ours=tmed / med, **agreement)
            out['entries'].append(e)
            print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in e.items()},
                  file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        del x, xb
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
