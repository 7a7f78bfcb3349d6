"""Time of one call of the streaming transforms on the device (csrc/stft_stream.hip through
`pb_bss_amd.transform.OnlineSTFT.step_block` / `OnlineISTFT.step_block`) next to the composition
of the entry points the package had before them, written here only:

    forward   a persistent buffer (C, window_length - shift + n): `copy_` of the block behind the
              kept samples, `stft(fading=False, pad=False)` of the buffer, a tail move
    inverse   `istft(fading=False)` of the block's frames, a tail add, a tail store

Entries: 1 and 16 frames per call at size 1024 / shift 256 and at size 512 / shift 128, 8 channels
of float32 samples -> complex64 'f t d' frames for the forward, 3 rows of complex64 frames for the
inverse.  Per entry: ours_us / composed_us (median of the warm calls, host clock around a call
that ends with a device synchronise; ours and the composition alternate in rounds in one
process), ours_min_us / composed_min_us, kernel_us (device events around the one launch of ours),
composed_device_us (device events around the composition's launches), first_call_us,
composed_over_ours, loses_to_composition, and the agreement of the two on the timed stream
(`equal` for the forward, which must be bit-identical; max_difference for the inverse, whose
composition adds the tail in another order).  Nothing is promised: an entry that loses says so.
One JSON line; --out writes it to a file as well.

The device work runs in a child process under its own time limit (--limit seconds).

    python tools/bench_stft_online.py [--reps 40] [--rounds 5] [--limit 240] \\
        [--out profiles/stft_online.json]
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

CHANNELS, ROWS = 8, 3
# name: (direction, size, shift, frames per call)
CONFIGS = {f'{d}_{size}_m{m}': (d, size, shift, m)
           for d in ('forward', 'inverse') for size, shift in ((1024, 256), (512, 128))
           for m in (1, 16)}


def timed(call, reps):
    import torch
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return times


def device_us(call, reps=20):
    """Device events around the call: first launch to last completion."""
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def kernel_us(call, reps=20):
    from pb_bss_amd import engine
    engine.set_timing(True)
    out = []
    for _ in range(reps):
        call()
        out.append(engine.last_kernel_ms() * 1e3)
    engine.set_timing(False)
    return float(np.median(out))


class ComposedSTFT:
    """The streaming forward transform from the offline entry point."""

    def __init__(self, channels, size, shift, n):
        import torch
        self.size, self.shift, self.keep, self.n = size, shift, size - shift, n
        self.buffer = torch.zeros((channels, self.keep + n), dtype=torch.float32, device='cuda')

    def step(self, block):
        from pb_bss_amd.transform import stft
        self.buffer[:, self.keep:].copy_(block)
        frames = stft(self.buffer, self.size, self.shift, fading=False, pad=False,
                      layout='f t d', dtype=np.complex64)
        self.buffer[:, :self.keep] = self.buffer[:, self.n:].clone()   # the ranges may overlap
        return frames


class ComposedISTFT:
    """The streaming inverse transform from the offline entry point."""

    def __init__(self, rows, size, shift):
        import torch
        self.size, self.shift = size, shift
        self.tail = torch.zeros((rows, size - shift), dtype=torch.float64, device='cuda')

    def step(self, frames):
        from pb_bss_amd.transform import istft
        y = istft(frames, self.size, self.shift, fading=False)
        keep = self.tail.shape[1]
        y[:, :keep] += self.tail
        self.tail.copy_(y[:, y.shape[1] - keep:])
        return y[:, :y.shape[1] - keep]


def measure(name, reps, rounds):
    import torch
    from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT
    direction, size, shift, m = CONFIGS[name]
    rng = np.random.default_rng(5)
    calls = 64
    if direction == 'forward':
        n = m * shift
        data = torch.from_numpy(rng.standard_normal((calls, CHANNELS, n)).astype(np.float32)).cuda()
        ours_obj = OnlineSTFT(CHANNELS, size, shift, fading=False, dtype=np.complex64)
        comp_obj = ComposedSTFT(CHANNELS, size, shift, n)
        # the composition's buffer starts with size - shift zeros: give our stream the same start,
        # so that both return the same m frames in every call
        zeros = torch.zeros((CHANNELS, size - shift), dtype=torch.float32, device='cuda')
        ours_obj.step_block(zeros)
        ours_step, comp_step = ours_obj.step_block, comp_obj.step
    else:
        F = size // 2 + 1
        z = rng.standard_normal((calls, ROWS, m, F)) + 1j * rng.standard_normal((calls, ROWS, m, F))
        data = torch.from_numpy(z.astype(np.complex64)).cuda()
        ours_obj = OnlineISTFT(size, shift, fading=False)
        comp_obj = ComposedISTFT(ROWS, size, shift)
        ours_step, comp_step = ours_obj.step_block, comp_obj.step
    state = {'ours': 0, 'comp': 0}

    def ours():
        state['ours'] += 1
        return ours_step(data[state['ours'] % calls])

    def composed():
        state['comp'] += 1
        return comp_step(data[state['comp'] % calls])

    # both streams see the same blocks in the same order: compare them call by call first
    first = timed(ours, 1)[0]
    comp_first = timed(composed, 1)[0]
    state['ours'] = state['comp'] = 0
    ours_obj.flush()
    if direction == 'forward':
        ours_obj.step_block(zeros)
    comp_obj = (ComposedSTFT(CHANNELS, size, shift, m * shift) if direction == 'forward'
                else ComposedISTFT(ROWS, size, shift))
    comp_step = comp_obj.step
    equal, worst, scale = True, 0.0, 0.0
    for _ in range(calls):
        a, b = ours(), composed()
        equal = equal and a.shape == b.shape and bool(torch.equal(a, b))
        if a.shape == b.shape and a.numel():
            worst = max(worst, float((a - b).abs().max()))
            scale = max(scale, float(b.abs().max()))
    out = {'first_call_us': first, 'composed_first_call_us': comp_first, 'equal': equal,
           'max_difference': worst / scale if scale else None}
    timed(ours, 20)
    timed(composed, 20)
    ours_t, comp_t = [], []
    for _ in range(rounds):
        ours_t += timed(ours, reps)
        comp_t += timed(composed, reps)
    out.update(ours_us=float(np.median(ours_t)), ours_min_us=float(min(ours_t)),
               composed_us=float(np.median(comp_t)), composed_min_us=float(min(comp_t)),
               kernel_us=kernel_us(ours), ours_device_us=device_us(ours),
               composed_device_us=device_us(composed))
    out['composed_over_ours'] = out['composed_us'] / out['ours_us']
    out['loses_to_composition'] = out['composed_over_ours'] < 1.0
    return out


def child(reps, rounds):
    entries = []
    for name, (direction, size, shift, m) in CONFIGS.items():
        entry = {'entry': name, 'direction': direction, 'size': size, 'shift': shift,
                 'frames_per_call': m,
                 **({'channels': CHANNELS, 'samples_per_call': m * shift}
                    if direction == 'forward' else {'rows': ROWS})}
        entry.update(measure(name, reps, rounds))
        entries.append(entry)
        print(f'{name}: done', file=sys.stderr, flush=True)
    print(json.dumps({'bench': 'stft_online', 'reps': reps * rounds, 'entries': entries}))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=40)
    parser.add_argument('--rounds', type=int, default=5)
    parser.add_argument('--limit', type=float, default=240.0)
    parser.add_argument('--out')
    parser.add_argument('--child', action='store_true')
    args = parser.parse_args()
    if args.child:
        return child(args.reps, args.rounds)
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--reps',
                               str(args.reps), '--rounds', str(args.rounds)],
                              stdout=subprocess.PIPE, timeout=args.limit, check=True, text=True)
    except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as error:
        print(json.dumps({'bench': 'stft_online', 'error': repr(error)}))
        return 1
    line = done.stdout.strip().splitlines()[-1]
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
