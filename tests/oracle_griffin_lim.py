"""Float64 restatement of the reference's Griffin-Lim and MISI
(pb_bss/transform/griffin_lim_module.py) on the oracle STFT (oracle/stft.py, the restated
nara_wpe.utils.stft / istft the reference class calls), the seeded cases the CPU and GPU tests
share, `load_reference`, which imports the unmodified reference file, and the recorder of
tests/golden/griffin_lim.npz:

    python tests/oracle_griffin_lim.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from oracle import stft as ostft  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'griffin_lim.npz')
ITERATIONS = (1, 5, 20)
CLASSES = ('GriffinLim', 'MISI')
FIRST_GUESSES = ('istft', 'y')


# ---- the restatement ----------------------------------------------------------------------------
class GriffinLim:
    """X (K, T, F), y (n,).  `smallest` keeps, over all steps so far, the smallest bin magnitude
    of X'' relative to its largest: the conditioning of the phase projection."""

    def __init__(self, X, y=None, first_guess='istft', size=512, shift=128, fading=False):
        self.kw = dict(size=size, shift=shift, fading=fading)
        self.X = X
        self.X_dash_dash = X
        self.X_dash = X
        self.y = y
        self.smallest = np.inf
        if first_guess == 'istft':
            self.x_hat = ostft.istft(X, **self.kw)
        elif first_guess == 'y':
            K = X.shape[0]
            self.x_hat = np.repeat(np.asarray(y, dtype=np.float64)[None, :] / K, K, axis=0)
        else:
            raise ValueError(first_guess)

    def transformed(self):
        """the time signals a step transforms"""
        return self.x_hat

    def step(self):
        self.X_dash_dash = ostft.stft(self.transformed(), **self.kw)
        magnitude = np.abs(self.X_dash_dash)
        self.smallest = min(self.smallest, magnitude.min() / magnitude.max())
        self.X_dash = np.abs(self.X) * np.exp(1j * np.angle(self.X_dash_dash))
        self.x_hat = ostft.istft(self.X_dash, **self.kw)


class MISI(GriffinLim):
    def transformed(self):
        K = self.X.shape[0]
        e = self.y - np.sum(self.x_hat, axis=0)
        return self.x_hat + e / K


RESTATED = {'GriffinLim': GriffinLim, 'MISI': MISI}


def run(cls, X, y, first_guess, iterations, **kw):
    """the restated (or any other) class after `iterations` steps"""
    model = cls(X, y=y, first_guess=first_guess, **kw)
    for _ in range(iterations):
        model.step()
    return model


def movement(name, case, first_guess, iterations, relative=1e-15):
    """how far x_hat moves when every entry of X moves by `relative` of itself"""
    rng = np.random.default_rng(99)
    X = case['X']
    moved = X * (1 + relative * rng.uniform(-1, 1, X.shape))
    a = run(RESTATED[name], X, case['y'], first_guess, iterations, **case['kw'])
    b = run(RESTATED[name], moved, case['y'], first_guess, iterations, **case['kw'])
    return float(np.abs(a.x_hat - b.x_hat).max())


# ---- the reference --------------------------------------------------------------------------------
def load_reference():
    """(GriffinLim, MISI) of the unmodified reference file.  Its constructor imports
    nara_wpe.utils.stft / istft at every call: the oracle's two stand in, and stay registered."""
    from oracle import refshim
    refshim.load()
    if 'nara_wpe' not in sys.modules:
        package, utils = types.ModuleType('nara_wpe'), types.ModuleType('nara_wpe.utils')
        utils.stft, utils.istft = ostft.stft, ostft.istft
        package.utils = utils
        sys.modules['nara_wpe'], sys.modules['nara_wpe.utils'] = package, utils
    path = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss', 'transform', 'griffin_lim_module.py')
    spec = importlib.util.spec_from_file_location('_reference_griffin_lim_module', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.GriffinLim, module.MISI


# ---- seeded cases -----------------------------------------------------------------------------
def samples(T, size, shift, fading):
    return T * shift + size - shift - (2 * (size - shift) if fading else 0)


def gen_case(seed, K, T, size, shift, fading=False):
    """K amplitude-modulated noises and their sum y; X: their STFT magnitudes, each bin scaled by
    a factor in (0.2, 1) -- a mask that was not quite right --, with the phase of the mixture"""
    rng = np.random.default_rng(seed)
    n = samples(T, size, shift, fading)
    kw = dict(size=size, shift=shift, fading=fading)
    time = np.arange(n) / max(n, 64)
    envelope = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(2, 6, (K, 1)) * time
                                  + rng.uniform(0, 6, (K, 1)))
    sources = envelope * rng.standard_normal((K, n))
    y = sources.sum(axis=0)
    S = ostft.stft(sources, **kw)
    assert S.shape == (K, T, size // 2 + 1), (S.shape, K, T, size)
    X = np.abs(S) * rng.uniform(0.2, 1, S.shape) * np.exp(1j * np.angle(ostft.stft(y, **kw)))
    return dict(X=X, y=y, sources=sources, kw=kw)


# name -> (seed, K, T, size, shift, fading).  The seeds are ones for which the restatement alone is
# well conditioned over 20 steps of either class (smallest relative bin magnitude of X'' above
# 1e-5, x_hat moving by less than 1e-13 under a relative 1e-15 on X) and |y| stays below 5.
CASES = {
    'size64': (11, 3, 20, 64, 16, False),         # M = 32 points against 256 threads
    'size64_fading': (42, 3, 20, 64, 16, True),   # the fading offsets
    'size512': (13, 3, 13, 512, 128, False),      # the defaults; 13 frames, 4 per workgroup
    'size4096': (4, 1, 5, 4096, 1024, False),    # several points per thread; e / 1
    'one_frame': (5, 2, 1, 64, 16, False),
    'batch_a': (26, 3, 20, 64, 16, False),        # the two mixtures of the (2, 3, T, F) batch
    'batch_b': (17, 3, 20, 64, 16, False),
}
# what the golden file holds, kept to a couple of hundred KB: of these cases every STRIDE-th
# sample of x_hat after 1, 5 and 20 steps, and the two spectra of the small ones after 20
RECORDED = ('size64', 'size64_fading', 'size512', 'size4096', 'one_frame')
STRIDE = {'size64': 2, 'size64_fading': 2, 'size512': 8, 'size4096': 16}
SPECTRA = ('one_frame',)


def case(name):
    return gen_case(*CASES[name])


def golden_key(name, cls, first_guess, iterations, what='x_hat'):
    return f'{name}/{cls}/{first_guess}/{iterations}/{what}'


def golden_entries(classes, name):
    """key -> array: what the golden file holds of case `name`, computed with `classes`"""
    c = case(name)
    stride = STRIDE.get(name, 1)
    out = {}
    for cls in CLASSES:
        for first_guess in FIRST_GUESSES:
            model = classes[cls](c['X'], y=c['y'], first_guess=first_guess, **c['kw'])
            done = 0
            for iterations in ITERATIONS:
                for _ in range(iterations - done):
                    model.step()
                done = iterations
                out[golden_key(name, cls, first_guess, iterations)] = model.x_hat[:, ::stride]
            if name in SPECTRA:
                for what in ('X_dash', 'X_dash_dash'):
                    out[golden_key(name, cls, first_guess, done, what)] = getattr(model, what)
    return out


def record():
    reference = dict(zip(CLASSES, load_reference()))
    entries = {}
    for name in RECORDED:
        entries.update(golden_entries(reference, name))
    np.savez(GOLDEN, **entries)
    print(f'{GOLDEN}: {len(entries)} arrays, {os.path.getsize(GOLDEN)} bytes')


if __name__ == '__main__':
    record()
