"""NumPy restatement of the deflation seed (reference: pb_bss/initializer/deflation.py:6-89), the
float64 oracle of tests/test_gpu_initializer.py where the reference itself is not available.
Checked against the reference's recorded results (tests/golden/initializer_*.npz) and, where the
reference tree is present, against the live reference in tests/test_initializer_oracle.py.

Besides the posteriors it reports how well determined each decision of the algorithm was --
the relative gap between the two largest candidates of every arg-max and between the two
largest eigenvalues of every local PSD -- so that a test can state on the oracle side that a
comparison to 1e-10 is meaningful for its input.
"""
import numpy as np

TINY = np.finfo(np.float64).tiny


def unit_frames(Y):
    """Y / max(|Y|, tiny) along the last axis"""
    return Y / np.maximum(np.linalg.norm(Y, axis=-1, keepdims=True), TINY)


def synth_case(F, T, D, K, seed, dtype=np.complex64, zero_bin=3, zero_tail=10):
    """The test input of the fixtures: pb_bss_amd.testing.synth.make_stft with bin `zero_bin`
    silenced and (T >= 64) the last `zero_tail` frames zero-padded."""
    from pb_bss_amd.testing import synth
    Y, _ = synth.make_stft(F, T, D, K, seed=seed, dtype=dtype)
    Y = Y.copy()
    if zero_tail and T >= 64:
        Y[:, T - zero_tail:] = 0
    if zero_bin is not None:
        Y[zero_bin] = 0
    return Y


def deflation_seed(Y, sources, saliencies=None, permutation_free=True, neighbors=5,
                   similarity_transform=None, eps=0, details=None):
    """Y (F, T, D) complex -> (K, F, T) float64.  `details` (a dict) receives
    'peaks' (K-1, F), 'argmax_gap' and 'eig_gap' (one figure per round)."""
    Y = np.asarray(Y)
    Y = Y.astype(np.complex128)
    F, T, D = Y.shape
    K = int(sources)
    assert T > 2 * neighbors
    sal = np.linalg.norm(Y, axis=-1) if saliencies is None else np.array(saliencies, np.float64)
    Z = unit_frames(Y)
    rows = np.arange(F)[:, None]
    offsets = np.arange(-neighbors, neighbors + 1)[None, :]
    posterior = np.empty((K, F, T))
    peaks, argmax_gap, eig_gap = [], [], []
    for k in range(K - 1):
        if permutation_free:
            profile = sal.mean(axis=0)[None, :]
        else:
            profile = sal
        peak = np.broadcast_to(np.argmax(profile, axis=-1), (F,))
        ranked = np.sort(profile, axis=-1)
        live = ranked[:, -1] > 0
        argmax_gap.append(float(((ranked[live, -1] - ranked[live, -2]) / ranked[live, -1]).min())
                          if live.any() else np.inf)
        peak = np.clip(peak, neighbors, T - 1 - neighbors)
        peaks.append(peak.copy())
        window = peak[:, None] + offsets                     # (F, L)
        Yw = Y[rows, window]                                 # (F, L, D)
        w = sal[rows, window]
        w = w / np.maximum(w.sum(axis=-1, keepdims=True), 1e-10)
        psd = np.einsum('fl,fld,fle->fde', w, Yw, Yw.conj())
        lam, vec = np.linalg.eigh(psd)
        nonzero = lam[:, -1] > 0
        eig_gap.append(float(((lam[nonzero, -1] - lam[nonzero, -2]) / lam[nonzero, -1]).min())
                       if nonzero.any() else np.inf)
        mode = unit_frames(vec[..., -1])
        similarity = np.abs(np.einsum('ftd,fd->ft', Z.conj(), mode)) ** 2
        if similarity_transform is not None:
            similarity = similarity_transform(similarity, sal)
        posterior[k] = similarity
        sal = sal * (1 - similarity)
    posterior[K - 1] = 1 - posterior[:K - 1].sum(axis=0)
    posterior = np.maximum(posterior, eps)
    posterior = posterior / posterior.sum(axis=0, keepdims=True)
    if details is not None:
        details.update(peaks=np.stack(peaks), argmax_gap=argmax_gap, eig_gap=eig_gap)
    return posterior


def assert_well_determined(details, argmax_min=1e-9, eig_min=1e-3):
    """The oracle-side precondition of a 1e-10 comparison: every arg-max and every dominant
    eigenvector of the run was well determined."""
    assert min(details['argmax_gap']) >= argmax_min, details['argmax_gap']
    assert min(details['eig_gap']) >= eig_min, details['eig_gap']
