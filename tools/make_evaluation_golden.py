"""Write tests/golden/evaluation.npz from the live, unmodified reference: the inputs of a few
small cases (generated from seeds by tests/oracle_evaluation.py) and what
pb_bss/evaluation/module_si_sdr.py and sxr_module.py return for them.  Needs the reference tree;
its two files are loaded by path.  Deterministic.

    python tools/make_evaluation_golden.py

Keys: `<case>/<input>` for the inputs, `<case>/<result>` for the recorded results.
  si_sdr_doc         the reference row of the docstring examples and their eight results
  si_sdr_rows        (5, 1000) against (5, 1000)
  si_sdr_outer       (2, 1, 300) against (1, 3, 300)
  get_snr            (3, 4, 100) real and complex, axis None / -1 / (0, 2) and keepdims
  input_sxr_*        K = 3, D = 4 and K = 1, D = 2, N = 100, real and complex, the four flag pairs
  output_sxr_*       (Ks, Kt) in (2, 3), (3, 3), (1, 1), (1, 2), (4, 5), N = 100, seeds 0-3 of
                     the (2, 3) case, a complex case; averaged and per source
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'evaluation.npz')

OUTPUT_CASES = [('2_3', 0, 2, 3, np.float64), ('3_3', 0, 3, 3, np.float64),
                ('1_1', 0, 1, 1, np.float64), ('1_2', 0, 1, 2, np.float64),
                ('4_5', 0, 4, 5, np.float64), ('2_3_seed1', 1, 2, 3, np.float64),
                ('2_3_seed2', 2, 2, 3, np.float64), ('2_3_seed3', 3, 2, 3, np.float64),
                ('3_4_complex', 0, 3, 4, np.complex128)]
INPUT_CASES = [('3_4', 0, 3, 4, np.float64), ('1_2', 1, 1, 2, np.float64),
               ('3_4_complex', 2, 3, 4, np.complex128)]


def main():
    import oracle_evaluation as oe
    ref_si, ref_sxr = oe.load_reference()
    arrays = {}

    np.random.seed(0)
    reference = np.random.randn(100)
    arrays['si_sdr_doc/reference'] = reference
    doc = [(reference, reference), (reference, reference * 2), (reference, np.flip(reference)),
           (reference, reference + np.flip(reference)), (reference, reference + 0.5),
           (reference, reference * 2 + 1)]
    with np.errstate(divide='ignore', invalid='ignore'):
        arrays['si_sdr_doc/results'] = np.array([ref_si.si_sdr(r, e) for r, e in doc])
        arrays['si_sdr_doc/zero_estimate'] = ref_si.si_sdr(np.array([1., 0]), np.array([0., 0]))
        arrays['si_sdr_doc/two_rows'] = ref_si.si_sdr(
            np.array([reference, reference]), np.array([reference * 2 + 1, reference * 1 + 0.5]))

    r, e = oe.gen_si_sdr(0, (5, 1000))
    arrays.update({'si_sdr_rows/reference': r, 'si_sdr_rows/estimation': e,
                   'si_sdr_rows/result': ref_si.si_sdr(r, e)})
    r, e = oe.gen_si_sdr(1, (3, 300))
    r, e = r[:2, None], e[None]
    arrays.update({'si_sdr_outer/reference': r, 'si_sdr_outer/estimation': e,
                   'si_sdr_outer/result': ref_si.si_sdr(r, e)})

    for name, dtype in (('real', np.float64), ('complex', np.complex128)):
        X = oe.gen_signals(3, (3, 4, 100), dtype)
        N = 0.3 * oe.gen_signals(4, (3, 4, 100), dtype)
        arrays.update({f'get_snr_{name}/X': X, f'get_snr_{name}/N': N,
                       f'get_snr_{name}/all': ref_sxr.get_snr(X, N),
                       f'get_snr_{name}/last': ref_sxr.get_snr(X, N, axis=-1),
                       f'get_snr_{name}/pair': ref_sxr.get_snr(X, N, axis=(0, 2)),
                       f'get_snr_{name}/keepdims': ref_sxr.get_snr(X, N, axis=1, keepdims=True)})

    for name, seed, K, D, dtype in INPUT_CASES:
        images, noise = oe.gen_input_case(seed, (), K, D, 100, dtype)
        arrays.update({f'input_sxr_{name}/images': images, f'input_sxr_{name}/noise': noise})
        for sources in (True, False):
            for channels in (True, False):
                got = ref_sxr.input_sxr(images, noise, sources, channels)
                arrays[f'input_sxr_{name}/result_{int(sources)}{int(channels)}'] = np.stack(got)

    for name, seed, Ks, Kt, dtype in OUTPUT_CASES:
        contribution, noise = oe.gen_output_case(seed, (), Ks, Kt, 100, dtype)
        arrays.update({f'output_sxr_{name}/contribution': contribution,
                       f'output_sxr_{name}/noise': noise})
        for sources in (True, False):
            got = ref_sxr.output_sxr(contribution, noise, average_sources=sources)
            arrays[f'output_sxr_{name}/result_{int(sources)}'] = np.stack(got)

    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **arrays)
    print(GOLDEN, os.path.getsize(GOLDEN))


if __name__ == '__main__':
    main()
