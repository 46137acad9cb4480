"""The host port of the convergence diagnostics (bayesfast_amd/utils/diagnostics.py: split-R-hat, ESS, the posterior table) against
the loop-written reference of helpers/diag_reference.py, the reference itself against AR(1) ground truth, and the TraceTuple
methods on host parts.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import diag_reference as dr  # noqa: E402

from bayesfast_amd import _lib, parallel  # noqa: E402
from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple  # noqa: E402
from bayesfast_amd.utils import diagnostics as dg  # noqa: E402
from bayesfast_amd import utils  # noqa: E402

GRID = [(4, 100, 3), (2, 8, 2), (7, 333, 5), (64, 1000, 16), (16, 63, 130), (256, 501, 20)]
RTOL = 1e-9


def assert_table(got, ref, names=None, rtol=RTOL):
    """Every column equal to the reference's: NaN in the same places, rtol elsewhere."""
    for k in (names or getattr(got, 'names', None) or tuple(got)):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, k
        assert np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
        np.testing.assert_allclose(a, b, rtol=rtol, atol=0, err_msg=k)


def with_ties(x):
    """Every second draw repeats the previous one exactly (a rejected move)."""
    x = x.copy()
    x[:, 1::2] = x[:, 0:x.shape[1] - 1:2]
    return x


def test_exports():
    assert utils.rhat is dg.rhat and utils.ess is dg.ess and utils.summary is dg.summary


@pytest.mark.parametrize('shape', GRID)
def test_shape_grid(shape):
    """Every column of summary and both R-hats on AR(1) columns (phi cycling 0, 0.5, 0.9, 0.98; odd N included).  Geyer's
    truncation is a discrete decision: the inputs must keep every |P_k| up to the deciding pair away from 0 (margin >= 1e-9, a
    condition on the inputs; the smallest over this grid is 1.4e-4)."""
    x = dr.ar1(shape, seed=sum(shape))
    ref = dr.reference(x)
    print('margin', shape, ref['margin'].min())
    assert (ref['margin'] >= 1e-9).all()
    got = dg.summary(x)
    assert got.names == ('mean', 'sd', 'q5', 'q50', 'q95', 'mcse_mean', 'ess_bulk', 'ess_tail', 'rhat')
    assert_table(got, ref)
    assert_table({'rhat': dg.rhat(x), 'rhat_split': dg.rhat(x, 'split'), 'ess_bulk': dg.ess(x), 'ess_tail': dg.ess(x, 'tail'),
                  'ess_mean': dg.ess(x, 'mean')}, ref, ('rhat', 'rhat_split', 'ess_bulk', 'ess_tail', 'ess_mean'))
    assert set(got.as_dict()) == set(got.names) and len(str(got).splitlines()) == shape[2] + 1


@pytest.mark.parametrize('shape', [(4, 100, 3), (7, 333, 5)])
def test_exact_ties(shape):
    x = with_ties(dr.ar1(shape, seed=sum(shape) + 1))
    ref = dr.reference(x)
    assert (ref['margin'] >= 1e-9).all()
    assert_table(dg.summary(x), ref)
    assert_table({'rhat_split': dg.rhat(x, 'split')}, ref, ('rhat_split',))


def test_other_probabilities_and_2d():
    x = dr.ar1((6, 200, 2), seed=3)
    ref = dr.reference(x, probs=(0.025, 0.975), prob=(0.1, 0.5, 0.9))
    got = dg.summary(x, probs=(0.025, 0.975), prob=(0.1, 0.5, 0.9))
    assert got.names[2:4] == ('q2.5', 'q97.5')
    assert_table(got, ref)
    one = dg.summary(x[:, :, 1])
    assert_table(one, {k: v[1:] for k, v in dr.reference(x).items()})
    assert_table(dg.summary(x.astype(np.float32)), dr.reference(x.astype(np.float32)))


@pytest.mark.parametrize('phi,bound', [(0., 0.0588), (0.5, 0.1266), (0.9, 0.3546)])
def test_reference_against_ar1_truth(phi, bound):
    """The reference's ess_mean on 64 x 1000 AR(1) chains against S (1 - phi) / (1 + phi).  The bound is twice the largest relative
    deviation the reference showed over the seeds 0 .. 19: 0.0294 (phi = 0), 0.0633 (phi = 0.5), 0.1773 (phi = 0.9)."""
    x = dr.ar1((64, 1000, 1), phis=(phi,), seed=100)
    ref = dr.reference(x)
    truth = 64000 * (1 - phi) / (1 + phi)
    print('ar1', phi, ref['ess_mean'][0] / truth - 1, ref['ess_bulk'][0] / truth - 1)
    assert abs(ref['ess_mean'][0] / truth - 1) < bound
    assert_table({'ess_mean': dg.ess(x, 'mean')}, ref, ('ess_mean',))


def test_rhat_behaviour():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((64, 1000))
    assert abs(dg.rhat(x)[0] - 1) < 0.01 and abs(dg.rhat(x, 'split')[0] - 1) < 0.01
    y = x.copy()
    y[:32] += 1.   # half of the chains one standard deviation away
    assert dg.rhat(y)[0] > 1.05
    x8 = rng.standard_normal((8, 1000))
    y8 = x8.copy()
    y8[3] = x8[3] + 3.   # one of 8 chains a constant-offset copy of itself
    assert dg.rhat(y8)[0] > dg.rhat(x8)[0]
    assert_table({'rhat': np.concatenate([dg.rhat(y), dg.rhat(y8)])},
                 {'rhat': np.array([dr.reference_one(y)['rhat'], dr.reference_one(y8)['rhat']])})


def nan_cases():
    x = dr.ar1((4, 100, 7), seed=9)
    x[:, :, 1] = 1.5          # constant
    x[2, 17, 2] = np.nan
    x[0, 60, 3] = np.inf
    x[3, 99, 4] = -np.inf
    x[:, :, 5] = 0.1          # constants whose sum of n copies is not n times the constant: the rounded variance is not 0
    x[:, :, 6] = 0.001
    return x


def test_nan_placement():
    x = nan_cases()
    got, ref = dg.summary(x), dr.reference(x)
    assert_table(got, ref)
    assert np.isfinite([got[k][0] for k in got.names]).all()
    for i, c in ((1, 1.5), (5, 0.1), (6, 0.001)):
        assert got['mean'][i] == c and got['sd'][i] == 0. and got['q5'][i] == c and got['q50'][i] == c and got['q95'][i] == c
        for k in ('mcse_mean', 'ess_bulk', 'ess_tail', 'rhat'):
            assert np.isnan(got[k][i])
    for k in got.names:
        assert np.isnan(got[k][2:5]).all()
    # the calls that sort nothing see the constants too
    calls = {'rhat': dg.rhat(x), 'rhat_split': dg.rhat(x, 'split'), 'ess_bulk': dg.ess(x), 'ess_tail': dg.ess(x, 'tail'),
             'ess_mean': dg.ess(x, 'mean')}
    assert_table(calls, ref)
    for v in calls.values():
        assert np.array_equal(np.isnan(v), [False, True, True, True, True, True, True])


def test_validation():
    x = np.zeros((3, 3, 2))
    for f in (dg.rhat, dg.ess, dg.summary):
        with pytest.raises(ValueError):
            f(x)
        with pytest.raises(ValueError):
            f(np.zeros(10))
        with pytest.raises(ValueError):
            f(np.zeros((2, 10, 2, 2)))
    with pytest.raises(ValueError):
        dg.rhat(np.zeros((3, 10)), method='folded')
    with pytest.raises(ValueError):
        dg.ess(np.zeros((3, 10)), method='median')
    with pytest.raises(ValueError):
        dg.summary(np.zeros((3, 10)), probs=(1.5,))


def test_cpu_tensor_takes_the_host_port():
    import torch
    t = torch.as_tensor(dr.ar1((4, 50, 2), seed=1))
    assert_table(dg.summary(t), dr.reference(t.numpy()))
    assert_table(dg.summary(t.clone().requires_grad_()), dr.reference(t.numpy()))
    assert_table({'rhat': dg.rhat(t[:, :, 0].to(torch.float32))}, dr.reference(t[:, :, 0].to(torch.float32).numpy()), ('rhat',))


def host_tracetuple():
    c, n, d = 5, 40, 3
    tr = NTrace(n_chain=c, n_iter=n, n_warmup=12)
    s = dr.ar1((c, n, d), seed=11)
    st = np.zeros((c, n, _lib.STAT_STRIDE))
    st[:, :, 0] = dr.ar1((c, n, 1), seed=12)[:, :, 0]
    return TraceTuple(tr, s, st, s * 10 + 1, st[:, :, 0] - 1.)


@pytest.mark.parametrize('kw', [dict(), dict(since_iter=7), dict(include_warmup=True), dict(original_space=False),
                                dict(return_type='logp'), dict(return_type='logp', original_space=False, since_iter=20)])
def test_tracetuple_on_host_parts(kw):
    tt = host_tracetuple()
    x = tt.get(flatten=False, **kw)
    want = dg.summary(x)
    got = tt.summary(**kw)
    for k in want.names:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert len(got['mean']) == (1 if kw.get('return_type') == 'logp' else 3)
    assert_table(got, dr.reference(x))
    assert np.array_equal(tt.rhat(**kw), dg.rhat(x)) and np.array_equal(tt.rhat(method='split', **kw), dg.rhat(x, 'split'))
    assert np.array_equal(tt.ess(method='tail', **kw), dg.ess(x, 'tail'))
    with pytest.raises(ValueError):
        tt.summary(since_iter=39)
    with pytest.raises(ValueError):
        tt.rhat(return_type='weights')


def test_distributed_refusal(monkeypatch):
    tt = host_tracetuple()
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    for f in (tt.rhat, tt.ess, tt.summary):
        with pytest.raises(NotImplementedError, match=r'gather\(\)'):
            f()
