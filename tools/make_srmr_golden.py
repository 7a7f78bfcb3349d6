#!/usr/bin/env python
"""Record tests/golden/srmr.npz: the outputs of the unmodified reference (pb_bss/evaluation/
module_srmr.py, framed by the zero-padding segment_axis stub of tests/oracle_srmr.py) for the
cases of oracle_srmr.cases(), which the tests rebuild from their seeds.

Per case: the SRMR of every row and the number of samples the reference's VAD keeps; for two
short signals the (n, N) output of the reference's gammatone_filterbank together with the input.
Every row must leave the scalar tail well determined: its cumulative percentage at least 1e-3
away from 90 at every channel, its bandwidth equal to no cutoff.  Needs the reference tree.

    python tools/make_srmr_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import oracle_srmr as osr  # noqa: E402


def main():
    reference, gammatone = osr.load_reference()
    golden = {}
    stops = set()
    for name, case in osr.cases().items():
        signal = np.asarray(case['signal'], dtype=np.float64)
        args = (case['sample_rate'], case['n'], case['low_freq'])
        rows = signal.reshape(-1, signal.shape[-1])
        golden[name + '/srmr'] = np.asarray(reference.srmr(signal, *args))
        golden[name + '/kept'] = np.array(
            [len(reference._preprocessing_vad(row, case['sample_rate'])) for row in rows])
        details = []
        osr.srmr(signal, *args, details=details)
        for row in details:
            assert np.abs(row['cumulative'] - 90).min() >= 1e-3, (name, row['cumulative'])
            assert row['bandwidth'] not in list(row['cutoffs']), (name, row['bandwidth'])
            stops.add(row['stopped_at'])
        print(name, golden[name + '/srmr'], golden[name + '/kept'],
              [row['stopped_at'] for row in details])
    assert {None, 6} <= stops, stops  # the loop both breaks at i = 6 and runs out
    for name, N, args in [('filterbank_a', 50, (16000, 23, 125, 0)),
                          ('filterbank_b', 300, (8000, 5, 80, 3000))]:
        x = osr.speechlike(40, N, args[0])
        golden[name + '/input'] = x
        golden[name + '/args'] = np.array(args)
        golden[name + '/output'] = np.stack(gammatone.gammatone_filterbank(x, *args))
    np.savez_compressed(osr.GOLDEN, **golden)
    print(osr.GOLDEN, os.path.getsize(osr.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
