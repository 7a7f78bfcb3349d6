"""Write the oracle-mask fixtures tests/golden/mask_module_*.npz from the live, unmodified
reference (through oracle.refshim; needs the reference tree).  Deterministic.

    python tools/make_mask_golden.py

The inputs are regenerated from seeds by tests/oracle_masks.gen / gen_integer and widened to
complex128 (the comparison target of a complex64 run is this result, rounded); the files hold
the reference's outputs only.

mask_module_pointwise.npz   the six pointwise masks on gen(0, (3, 4, 9, 40)) (binary and
        Wiener-like pooled over sensor_axis=1 and per channel; the others on channel 0), and
        the binary mask of the integer-valued case gen_integer(1, (2, 5, 11, 40)).
mask_module_threshold.npz   lorenz_mask and quantile_mask on gen(0, (3, 4, 33, 150)) and on the
        integer case: two-valued arrays, which compress well.
mask_module_biased.npz      biased_binary_mask at 513 bins: (2, 7, 513) and (2, 513) images
        (only in the latter does high_cut=500 reach the array), and the voiced / unvoiced
        characteristic for a few arguments.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

VUV_ARGS = [(513,), (257,), (513, 200, 80), (129, 40, 31)]


def biased_input(shape):
    import oracle_masks as om
    x = om.gen(2, shape).astype(np.complex128)
    x[1] *= 0.3  # noise below speech often enough for both masks to be mixed
    return x


def main():
    from oracle import refshim
    refshim.load()
    from pb_bss.extraction import mask_module as ref
    import oracle_masks as om
    os.makedirs(GOLDEN, exist_ok=True)

    def save(name, arrays):
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path))

    x = om.gen(0, (3, 4, 9, 40)).astype(np.complex128)
    xi = om.gen_integer(1, (2, 5, 11, 40)).astype(np.complex128)
    one = x[:, 0]
    save('mask_module_pointwise.npz', dict(
        ibm_pooled=ref.ideal_binary_mask(x, sensor_axis=1),
        ibm=ref.ideal_binary_mask(x),
        wiener_pooled=ref.wiener_like_mask(x, sensor_axis=1),
        wiener_pooled_keepdims=ref.wiener_like_mask(x, sensor_axis=1, keepdims=True),
        wiener=ref.wiener_like_mask(x),
        wiener_source1=ref.wiener_like_mask(x, source_axis=1),
        irm=ref.ideal_ratio_mask(one),
        iam=ref.ideal_amplitude_mask(one),
        psm=ref.phase_sensitive_mask(one),
        icm=ref.ideal_complex_mask(one),
        ibm_integer=ref.ideal_binary_mask(xi, sensor_axis=1),
        wiener_integer=ref.wiener_like_mask(xi, sensor_axis=1),
    ))

    x = om.gen(0, (3, 4, 33, 150)).astype(np.complex128)
    mag = np.abs(x[:, 0])
    save('mask_module_threshold.npz', dict(
        lorenz_098=ref.lorenz_mask(x, sensor_axis=1),
        lorenz_050=ref.lorenz_mask(x, sensor_axis=1, lorenz_fraction=0.5),
        lorenz_last=ref.lorenz_mask(x, sensor_axis=1, axis=-1),
        lorenz_keepdims=ref.lorenz_mask(x, sensor_axis=1, keepdims=True, weight=0.9),
        lorenz_integer=ref.lorenz_mask(xi, sensor_axis=1, lorenz_fraction=0.9),
        quantile_f=ref.quantile_mask(mag, (0.25, -0.5), axis=-2),
        quantile_t=ref.quantile_mask(mag, 0.3, axis=-1),
        quantile_ft=ref.quantile_mask(mag, -0.2, axis=(-2, -1)),
        quantile_default=ref.quantile_mask(mag),
        quantile_integer=ref.quantile_mask(np.abs(xi[:, 0]), (0.25, -0.5), axis=(-2, -1)),
    ))

    arrays = dict(
        biased_7_513=ref.biased_binary_mask(biased_input((2, 7, 513))),
        biased_513=ref.biased_binary_mask(biased_input((2, 513))),
        biased_513_args=ref.biased_binary_mask(
            biased_input((2, 513)), threshold_unvoiced_speech=3, threshold_voiced_speech=-2,
            threshold_unvoiced_noise=-6, threshold_voiced_noise=-12, low_cut=9, high_cut=400),
    )
    for args in VUV_ARGS:
        voiced, unvoiced = ref.voiced_unvoiced_split_characteristic(*args)
        key = '_'.join(str(a) for a in args)
        arrays[f'voiced_{key}'] = voiced
        arrays[f'unvoiced_{key}'] = unvoiced
    save('mask_module_biased.npz', arrays)


if __name__ == '__main__':
    main()
