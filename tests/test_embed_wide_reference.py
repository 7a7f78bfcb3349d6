"""CPU: the fixtures of the many-class mixtures (tests/golden/embed_wide_*.npz, recorded by
tools/make_golden_embed_wide.py) are what the UNMODIFIED reference produces, and the NumPy oracle
the GPU tests compare against reproduces them -- at the tolerances of tests/test_reference_live.py."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MIXTURES = ['embed_wide_vmfmm_n600_e10_k12', 'embed_wide_gmm_n600_e10_k12']
JOINT = 'embed_wide_gcacgmm_f6_t120_d5_k10_e8'


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as g:
        return {k: g[k] for k in g.files}


@pytest.mark.parametrize('name', MIXTURES)
def test_oracle_reproduces_wide_mixture_fixtures(name):
    from oracle import embed as oe
    g = load(name)
    it = int(g['iterations'])
    assert g['init'].shape[0] == 12 > 8
    if 'vmfmm' in name:
        o = oe.vmfmm_fit(g['y'], g['init'], it, saliency=g['saliency'])
        scale, aff = o['concentration'], oe.vmfmm_predict(o, g['y'])
    else:
        o = oe.gmm_fit(g['y'], g['init'], it, saliency=g['saliency'])
        scale, aff = o['covariance'], oe.gmm_predict(o, g['y'])
    np.testing.assert_allclose(o['mean'], g['mean'], atol=1e-11)
    np.testing.assert_allclose(scale, g['scale'], atol=1e-11, rtol=1e-12)
    np.testing.assert_allclose(o['weight'], g['weight'], atol=1e-12)
    np.testing.assert_allclose(aff, g['affiliation'], atol=1e-10)
    assert g['weight'].min() > 0.5 / 12  # no class starved


def test_oracle_reproduces_wide_joint_fixture():
    from oracle import embed as oe
    g = load(JOINT)
    Y, e = g['Y'].astype(np.complex128), g['embedding'].astype(np.float64)
    assert g['init'].shape[-2] == 10 > 8
    o = oe.joint_fit('gaussian', Y, e, g['init'], int(g['iterations']))
    np.testing.assert_allclose(o['mean'], g['mean'], atol=1e-11)
    np.testing.assert_allclose(o['covariance'], g['covariance'], atol=1e-11)
    np.testing.assert_allclose(oe.joint_model_predict(o, Y, e), g['affiliation'], atol=1e-10)


@pytest.mark.needs_reference
def test_live_reference_reproduces_wide_fixtures():
    from oracle import refshim
    refshim.load()
    from pb_bss.distribution import GCACGMMTrainer, GMMTrainer, VMFMMTrainer
    g = load(MIXTURES[0])
    m = VMFMMTrainer().fit(g['y'], initialization=g['init'], iterations=int(g['iterations']),
                           saliency=g['saliency'])
    np.testing.assert_allclose(m.vmf.mean, g['mean'], atol=1e-12)
    np.testing.assert_allclose(m.predict(g['y']), g['affiliation'], atol=1e-12)
    g = load(MIXTURES[1])
    m = GMMTrainer().fit(g['y'], initialization=g['init'], iterations=int(g['iterations']),
                         saliency=g['saliency'], covariance_type='spherical')
    np.testing.assert_allclose(m.gaussian.covariance, g['scale'], atol=1e-12)
    np.testing.assert_allclose(m.predict(g['y']), g['affiliation'], atol=1e-12)
    g = load(JOINT)
    Y, e = g['Y'].astype(np.complex128), g['embedding'].astype(np.float64)
    j = GCACGMMTrainer().fit(Y, e, initialization=g['init'], iterations=int(g['iterations']))
    np.testing.assert_allclose(j.predict(Y, e), g['affiliation'], atol=1e-12)
