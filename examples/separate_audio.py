#!/usr/bin/env python3
"""Audio in -> audio out on one GPU, nothing but the waveforms crossing PCIe:

    audio (D, samples) --stft('f t d')--> Y (F, T, D) [--WPE-->] --cACGMM EM--> masks --DHTV alignment-->
      PSD --'mvdr_souden' | 'gev+ban'--> beamformed STFT (K, T, F) --istft--> audio (K, samples)

    python examples/separate_audio.py --seconds 8 --sensors 6 --sources 2 [--wpe [recursive]]

With --online the model is fitted and aligned on a first block only and the rest runs sample block
by sample block (block-frames * shift samples) through the streaming stages, the state of all of
them on the device; the audio is bit for bit what the offline stft / istft around the same stages
give:

    first block --OnlineSTFT--> --cACGMM EM--> masks --DHTV alignment--> one M-step --> CACGMM
    every block --OnlineSTFT--> [--OnlineWPE-->] --OnlineCACGMM--> masks (F, K, Tb)
                --OnlineMVDR per class--> (K, F, Tb) --OnlineISTFT('f t')--> audio (K, block)

    python examples/separate_audio.py --online [--first-block 2] [--block-frames 16] [--wpe recursive]

Synthetic scene: `sources` on/off-modulated noise bursts through random short room filters
plus sensor noise.  Prints the time per stage and, per source, the correlation of the best
matching output with the source image at the reference sensor before and after separation.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_scene(rng, seconds, rate, D, S, taps=64, noise=0.03):
    n = int(seconds * rate)
    t = np.arange(n) / rate
    src = []
    for s in range(S):
        gate = (np.sin(2 * np.pi * (0.7 + 0.45 * s) * t + 2.0 * s) > -0.2).astype(np.float64)
        colour = np.convolve(rng.standard_normal(n), rng.standard_normal(8) * np.hanning(8), 'same')
        src.append(gate * colour)
    src = np.stack(src)                                                     # (S, n)
    h = rng.standard_normal((S, D, taps)) * np.exp(-np.arange(taps) / 12.0)
    images = np.stack([[np.convolve(src[s], h[s, d])[:n] for d in range(D)] for s in range(S)])
    mix = images.sum(0) + noise * images.std() * rng.standard_normal((D, n))
    return mix.astype(np.float32), images[:, 0]                             # reference sensor 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=8.0)
    ap.add_argument('--rate', type=int, default=16000)
    ap.add_argument('--sensors', type=int, default=6)
    ap.add_argument('--sources', type=int, default=2)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--shift', type=int, default=256)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--init', choices=['random', 'deflation', 'flag'], default='random',
                    help="affiliation initialisation: the trainer's uniform random draw, the "
                         "device-side deflation seed (needs --size 512 or 1024: F in {257, 513}) or "
                         "time segments (pb_bss_amd.initializer)")
    ap.add_argument('--beamformer', default='mvdr_souden',
                    help="recipe for get_bf_vector; the printed correlation compares with the source "
                         "image at sensor 0, so it is meaningful for distortionless recipes "
                         "('mvdr_souden', 'wmwf'), not for 'gev+ban' (free phase per bin)")
    ap.add_argument('--wpe', nargs='?', const='offline', choices=('offline', 'recursive'),
                    help="dereverberate the STFT in front of the mixture model and the beamformer, "
                         "read and written in the 'f t d' layout, 10 taps, delay 3: 'offline' "
                         "(the default of a bare --wpe; pb_bss_amd.transform.wpe, 3 iterations) "
                         "or 'recursive' (transform.recursive_wpe: one filter update per frame, "
                         "alpha 0.9999)")
    ap.add_argument('--online', action='store_true',
                    help="fit and align on the first block only, then OnlineSTFT -> OnlineWPE (with "
                         "--wpe recursive) -> OnlineCACGMM -> OnlineMVDR -> OnlineISTFT over blocks "
                         "of block-frames * shift samples")
    ap.add_argument('--first-block', type=float, default=2.0,
                    help='--online: seconds of the block the offline model is fitted on')
    ap.add_argument('--block-frames', type=int, default=16,
                    help='--online: frames per block (the block is block-frames * shift samples)')
    ap.add_argument('--alpha', type=float, default=0.99,
                    help='--online: forgetting factor of the mask estimator and the beamformer')
    ap.add_argument('--save', metavar='FILE.npy',
                    help='write the separated audio (classes, samples) float64 to this file')
    args = ap.parse_args()
    if args.online and args.wpe == 'offline':
        ap.error("--online streams: use --wpe recursive")
    import torch
    from pb_bss_amd import initializer
    from pb_bss_amd.distribution import CACGMMTrainer
    from pb_bss_amd.extraction import (apply_beamforming_vector, get_bf_vector,
                                       get_power_spectral_density_matrix)
    from pb_bss_amd.permutation_alignment import DHTVPermutationAlignment
    from pb_bss_amd.transform import istft, recursive_wpe, stft, wpe

    rng = np.random.default_rng(0)
    mix, images = make_scene(rng, args.seconds, args.rate, args.sensors, args.sources)
    K = args.sources + 1                                                     # + noise class
    n = mix.shape[-1]

    # the printed correlation compares with the source images AT SENSOR 0: pin the filters that take a
    # reference channel to it (the automatic choice, beamformer.py:601-624, is free to pick another
    # sensor, whose image of the source has a different impulse response)
    bf_kw = {'ref_channel': 0} if args.beamformer in ('mvdr_souden', 'wmwf') else {}

    def run(x):
        np.random.seed(0)   # CACGMMTrainer draws its initialisation from NumPy's global generator
        marks = [('start', time.perf_counter())]

        def mark(name):
            torch.cuda.synchronize()
            marks.append((name, time.perf_counter()))

        Y = stft(x, args.size, args.shift, layout='f t d', dtype=np.complex64)   # (F, T, D)
        mark('stft')
        if args.wpe == 'recursive':
            Y = recursive_wpe(Y, layout='f t d')
            mark('recursive WPE 10 taps')
        elif args.wpe:
            Y = wpe(Y, layout='f t d')
            mark('WPE 10 taps x3')
        if args.init == 'random':
            start = dict(num_classes=K)
        elif args.init == 'deflation':                                       # (K,F,T) -> (F,K,T) view
            start = dict(initialization=initializer.deflation.deflationSeed(Y, K).transpose(0, 1))
        else:
            start = dict(initialization=initializer.deterministic.flag(Y, K, permutation_free=True,
                                                                       minimum=0.1 / K))
        masks = CACGMMTrainer().fit_predict(Y, iterations=args.iterations, **start)  # (F,K,T)
        mark(f'cACGMM x{args.iterations}')
        solver = DHTVPermutationAlignment.from_stft_size(args.size)
        kft = solver(masks.transpose(0, 1).contiguous())                     # (K, F, T)
        mark('DHTV alignment')
        X = Y.transpose(1, 2).contiguous()                                   # (F, D, T)
        psd = get_power_spectral_density_matrix(X, kft.transpose(0, 1).contiguous())  # (F,K,D,D)
        out = []
        for k in range(K):
            target = psd[:, k]
            w = get_bf_vector(args.beamformer, target, psd.sum(1) - target, **bf_kw)
            out.append(apply_beamforming_vector(w, X) * kft[k])             # masked beamformer (F, T)
        S = torch.stack(out).transpose(1, 2).contiguous()                    # (K, T, F)
        mark(f'PSD + {args.beamformer} + apply')
        y = istft(S, args.size, args.shift)[..., :n]                         # (K, samples)
        mark('istft')
        return y, marks

    notes = []

    def run_online(x):
        from pb_bss_amd.distribution import OnlineCACGMM
        from pb_bss_amd.extraction import OnlineMVDR
        from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT, OnlineWPE
        np.random.seed(0)
        marks = [('start', time.perf_counter())]

        def mark(name):
            torch.cuda.synchronize()
            marks.append((name, time.perf_counter()))

        D, F, Tb = x.shape[0], args.size // 2 + 1, args.block_frames
        block_samples = Tb * args.shift
        analysis = OnlineSTFT(D, args.size, args.shift, dtype=np.complex64)  # -> (F, m, D)
        synthesis = OnlineISTFT(args.size, args.shift, layout='f t')         # (K, F, m) ->
        T0 = max(1, int(args.first_block * args.rate / args.shift))
        T0 = -(-T0 // Tb) * Tb                                               # whole blocks
        n0 = min(x.shape[1], T0 * args.shift)
        head = analysis.step_block(x[:, :n0])                                # (F, T0, D)
        dereverb = OnlineWPE(channel=D, frequency_bins=F) if args.wpe else None
        head = dereverb.step_block(head) if dereverb else head
        masks = CACGMMTrainer().fit_predict(head, iterations=args.iterations, num_classes=K)
        solver = DHTVPermutationAlignment.from_stft_size(args.size)
        kft = solver(masks.transpose(0, 1).contiguous())                     # (K, F, T0), aligned
        # the model of the aligned classes: one M-step from the aligned masks
        model = CACGMMTrainer().fit(head, initialization=kft.transpose(0, 1).contiguous(),
                                    iterations=1)
        mark(f'first block ({head.shape[1]} frames): OnlineSTFT + cACGMM x{args.iterations} + '
             'DHTV + M-step')
        estimator = OnlineCACGMM(model, args.alpha)
        beamformers = [OnlineMVDR(D, F, args.alpha, 0) for _ in range(K)]
        out = []

        def separate(block):                                                 # (F, m, D), dereverberated
            aff = estimator.step_block(block)                                # (F, K, m), a-priori
            S = torch.stack([bf.step_block(block, aff[:, k], 1.0 - aff[:, k]) * aff[:, k]
                             for k, bf in enumerate(beamformers)])           # (K, F, m)
            out.append(synthesis.step_block(S))                              # (K, samples)

        for t0 in range(0, head.shape[1], Tb):
            separate(head[:, t0:t0 + Tb].contiguous())
        starts = list(range(n0, x.shape[1], block_samples))
        for s0 in starts + [None]:                                           # None: the end of the stream
            frames = analysis.flush() if s0 is None else analysis.step_block(x[:, s0:s0 + block_samples])
            if frames.shape[1]:
                separate(dereverb.step_block(frames) if dereverb else frames)
        out.append(synthesis.flush())
        y = torch.cat(out, dim=-1)[..., :n]                                  # (K, samples)
        flagged = int((estimator.status != 0).sum())
        latency = analysis.window_length - args.shift + block_samples
        mark(f'{len(starts)} blocks of {block_samples} samples: OnlineSTFT + '
             f'{"OnlineWPE + " if dereverb else ""}OnlineCACGMM + {K} OnlineMVDR + OnlineISTFT'
             f'{f" ({flagged} bins flagged)" if flagged else ""}')
        notes[:] = [f'algorithmic latency: {latency} samples = {latency / args.rate * 1e3:.1f} ms '
                    f'(window_length - shift = {analysis.window_length - args.shift} + the block '
                    f'of {block_samples})']
        return y, marks

    if args.online:
        run = run_online
    x = torch.from_numpy(mix).cuda()
    run(x[:, :max(args.rate, int(1.5 * args.first_block * args.rate)) if args.online
          else args.rate])                                                   # warm-up
    torch.cuda.synchronize()
    y, marks = run(x)
    est = y.cpu().numpy()
    if args.save:
        np.save(args.save, est)
    total = marks[-1][1] - marks[0][1]
    print(f'{args.sensors} sensors x {args.seconds:g} s @ {args.rate} Hz, {K} classes: '
          f'{total * 1e3:.2f} ms on the device = {args.seconds / total:.0f} x real time')
    for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
        print(f'  {name:32s} {(b - a) * 1e3:8.3f} ms')
    for note in notes:
        print(f'  {note}')

    def corr(a, b):
        return abs(np.dot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30)

    for s in range(args.sources):
        before = corr(mix[0].astype(np.float64), images[s])
        after = max(corr(est[k], images[s]) for k in range(K))
        print(f'  source {s}: correlation with its image at sensor 0: mixture {before:.3f} -> '
              f'best output {after:.3f}')


if __name__ == '__main__':
    main()
