"""The host port of ``bayesfast_amd.utils.psis`` (Pareto-smoothed importance weights, the weighted posterior table) against the
loop-written reference of helpers/psis_reference.py, against ``summary`` with equal weights, against the closed form of a
generalised Pareto sample, on degenerate input and on bad arguments.  No GPU.

Tolerances: 1e-9 relative, the project's figure for a vectorised port against a loop reference.  For khat, sigma and
log_mean_weight the profile likelihoods multiply rounding by the tail size; what rounding alone does to them was measured by
running the reference in float64 and in numpy.longdouble on the inputs of the psis grid (``gaussian_pair(S, scale, seed=S)``) and
of the device tests up to S = 262145: at most 1.5e-11 for khat and sigma, 1.0e-10 for log_mean_weight (S = 100003, scale 0.8,
where the value is -6.3e-5), so 1e-9 stays (docs/EXPERIMENTS.md has the table)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import psis_reference as pr  # noqa: E402
from bayesfast_amd.utils import psis, weighted_summary, summary, PSISResult  # noqa: E402
from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple  # noqa: E402
from bayesfast_amd import _lib, parallel  # noqa: E402

RTOL = 1e-9
SIZES = (24, 25, 224, 225, 226, 1000, 4097, 100003)
TABLE_SHAPES = [(1, 3), (2, 2), (255, 1), (256, 17), (257, 16), (7, 333, 5), (65537, 2)]


def assert_psis(got, ref, rtol=RTOL):
    lw = np.asarray(got.log_weights.cpu() if hasattr(got.log_weights, 'cpu') else got.log_weights).reshape(-1)
    assert got.n_tail == ref['n_tail']
    for k in ('khat', 'sigma', 'log_mean_weight', 'ess'):
        a, b = getattr(got, k), float(ref[k])
        assert np.isnan(a) == np.isnan(b), (k, a, b)
        if not np.isnan(b):
            np.testing.assert_allclose(a, b, rtol=rtol, atol=0, err_msg=k)
    b = np.asarray(ref['log_weights'], dtype=np.float64)
    assert np.array_equal(np.isnan(lw), np.isnan(b))
    np.testing.assert_allclose(lw, b, rtol=rtol, atol=0)


def assert_table(got, ref):
    for k in got.names:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, k
        assert np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=0, err_msg=k)


def table_case(shape, kind, seed):
    """(x, weights) of one table test: gamma weights, 90 % exact zeros, or one dominant weight."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * (1. + np.arange(shape[-1])) + np.arange(shape[-1])
    w = rng.gamma(0.7, size=shape[:-1])
    if kind == 'zeros':
        w[rng.random(shape[:-1]) < 0.9] = 0.
        w.reshape(-1)[0] = 1.
    elif kind == 'dominant':
        w.reshape(-1)[w.size // 2] = 50. * w.sum()
    return x, w


@pytest.mark.parametrize('scale', (0.8, 1.2))
@pytest.mark.parametrize('s', SIZES)
def test_psis_host_port_against_the_reference(s, scale):
    logp, logq, _ = pr.gaussian_pair(s, scale, seed=s)
    ref = pr.psis_reference(logp - logq)
    got = psis(logp, logq)
    assert isinstance(got, PSISResult) and got.log_weights.shape == (s,)
    assert_psis(got, ref)
    assert_psis(psis((logp - logq).reshape(1, -1)), ref)
    if s >= 25:
        assert np.isfinite(got.khat) and got.n_tail == min(s // 5, int(np.ceil(3 * np.sqrt(s))))
        assert abs(np.logaddexp.reduce(got.log_weights)) < 1e-12
    else:
        assert got.khat == np.inf


@pytest.mark.parametrize('k', (0.3, 0.7))
@pytest.mark.parametrize('seed', (1, 2, 3))
def test_khat_against_the_generalised_pareto_shape(k, seed):
    """S = 20000 draws of genpareto(k) as weights: M = 425, and khat is within four asymptotic standard deviations of the shape's
    maximum-likelihood estimate, (1 + k) / sqrt(M), of k."""
    from scipy.stats import genpareto
    r = psis(np.log(genpareto(k).rvs(20000, random_state=seed)))
    assert r.n_tail == 425
    print(k, seed, r.khat - k)
    assert abs(r.khat - k) <= 4 * (1 + k) / np.sqrt(425)


def test_psis_degenerate_input():
    rng = np.random.default_rng(0)
    lw = rng.standard_normal(24)
    r = psis(lw)                                  # M = 4: nothing is smoothed
    assert r.khat == np.inf and r.n_tail == 4 and np.isnan(r.sigma)
    np.testing.assert_allclose(r.log_weights, lw - np.logaddexp.reduce(lw), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r.log_mean_weight, np.logaddexp.reduce(lw) - np.log(24), rtol=1e-12)
    assert_psis(r, pr.psis_reference(lw))
    lw = rng.standard_normal(25)
    r = psis(lw)                                  # M = 5: the smallest tail that is fitted
    assert r.n_tail == 5 and np.isfinite(r.khat) and r.sigma > 0
    assert_psis(r, pr.psis_reference(lw))
    order = np.argsort(lw)
    assert np.array_equal(np.argsort(r.log_weights[order[:20]]), np.arange(20))   # below the tail only shifted
    np.testing.assert_allclose(np.diff(r.log_weights[order[:20]]), np.diff(lw[order[:20]]), rtol=1e-9, atol=1e-13)
    r = psis(np.full(100, -3.))                   # all weights equal: a tail without spread
    assert r.khat == np.inf and r.n_tail == 20
    np.testing.assert_allclose(r.log_weights, -np.log(100), rtol=1e-14)
    np.testing.assert_allclose([r.ess, r.log_mean_weight], [100., -3.], rtol=1e-12)
    assert_psis(r, pr.psis_reference(np.full(100, -3.)))
    lw = rng.standard_normal(400)
    lw[17] = -np.inf                              # a zero weight: counted, sorted first
    r = psis(lw)
    assert r.log_weights[17] == -np.inf and np.isfinite(np.delete(r.log_weights, 17)).all() and r.n_tail == 60
    assert_psis(r, pr.psis_reference(lw))
    for v in (np.nan, np.inf):
        lw = rng.standard_normal(400)
        lw[3] = v
        r = psis(lw)
        assert np.isnan(r.log_weights).all() and all(np.isnan(getattr(r, k)) for k in ('khat', 'sigma', 'log_mean_weight', 'ess'))
        assert_psis(r, pr.psis_reference(lw))


@pytest.mark.parametrize('kind', ('gamma', 'zeros', 'dominant'))
@pytest.mark.parametrize('shape', TABLE_SHAPES)
def test_table_host_port_against_the_reference(shape, kind):
    if kind != 'gamma' and shape[0] > 1000:
        shape = (1001, 2)   # (the loop reference is slow; the large size is covered with the gamma weights)
    x, w = table_case(shape, kind, seed=sum(shape))
    ref = pr.table_reference(x, weights=w)
    assert (ref['margin'] >= 1e-9).all()
    got = weighted_summary(x, weights=w)
    assert got.names == ('mean', 'sd', 'q5', 'q50', 'q95', 'mcse_mean', 'ess', 'ess_kish')
    assert_table(got, ref)
    with np.errstate(divide='ignore'):
        lw = np.log(w).reshape(-1) + 3.
    assert_table(weighted_summary(x, log_weights=lw), ref)
    assert_table(weighted_summary(x.astype(np.float32), weights=w), pr.table_reference(x.astype(np.float32), weights=w))


def test_table_special_columns():
    x, w = table_case((300, 7), 'gamma', seed=3)
    w[[5, 6, 7]] = 0.
    x[:, 1] = 0.1                # constant
    x[10, 2] = np.nan            # non-finite at non-zero weight
    x[11, 3] = np.inf
    x[5, 4] = np.nan             # non-finite at zero weight: not part of the sample
    x[6, 4] = -np.inf
    x[:, 5] = 2.5
    x[7, 5] = -1.                # constant among the rows that count
    ref = pr.table_reference(x, weights=w, probs=(0.025, 0.5))
    got = weighted_summary(x, weights=w, probs=(0.025, 0.5))
    assert got.names[2:4] == ('q2.5', 'q50')
    assert_table(got, ref)
    assert all(np.isnan(got[k][[2, 3]]).all() for k in got.names)
    assert all(np.isfinite(got[k][[0, 4, 6]]).all() for k in got.names)
    for c, v in ((1, 0.1), (5, 2.5)):
        assert got['mean'][c] == v and got['q2.5'][c] == v and got['sd'][c] == 0. and np.isnan(got['mcse_mean'][c])
    one = weighted_summary(x[:1], weights=w[:1])              # one draw: the value, the rest NaN
    assert np.array_equal(one['mean'][[0, 6]], x[0, [0, 6]]) and np.array_equal(one['q50'][[0, 6]], x[0, [0, 6]])
    assert np.isnan(one['sd']).all() and np.isnan(one['ess']).all()
    assert_table(one, pr.table_reference(x[:1], weights=w[:1]))
    w1 = np.zeros(300)
    w1[20] = 4.                                               # one weight equal to 1 after normalisation
    one = weighted_summary(x, weights=w1)
    assert one['mean'][0] == x[20, 0] and one['q95'][6] == x[20, 6] and np.isnan(one['sd'][0]) and np.isnan(one['mcse_mean'][0])
    assert_table(one, pr.table_reference(x, weights=w1))
    neg = weighted_summary(x, weights=-w)                     # negative weights: no table
    assert all(np.isnan(neg[k]).all() for k in neg.names)


def test_equal_weights_give_the_unweighted_summary():
    x = np.random.default_rng(8).standard_normal((4, 250, 3)) * [1., 10., 0.1] + [0., 5., -2.]
    s = summary(x)
    for got in (weighted_summary(x, weights=np.ones((4, 250))), weighted_summary(x.reshape(1000, 3), log_weights=np.full(1000, -7.))):
        for k in ('mean', 'sd', 'q5', 'q50', 'q95'):
            np.testing.assert_allclose(got[k], s[k], rtol=1e-12, atol=0, err_msg=k)
        np.testing.assert_allclose(got['ess_kish'], 1000., rtol=1e-12)
        np.testing.assert_allclose(got['ess'], 1000., rtol=1e-12)   # (independent draws: n exactly)


def test_argument_errors():
    x = np.zeros((10, 2))
    w = np.ones(10)
    with pytest.raises(ValueError):
        weighted_summary(x)
    with pytest.raises(ValueError):
        weighted_summary(x, log_weights=w, weights=w)
    with pytest.raises(ValueError):
        weighted_summary(x, weights=np.ones(9))
    with pytest.raises(ValueError):
        weighted_summary(x, weights=np.ones((2, 5)))
    with pytest.raises(ValueError):
        weighted_summary(x, weights=w, probs=(0.5, 1.5))
    with pytest.raises(ValueError):
        weighted_summary(x, weights=w, probs=(-0.1,))
    with pytest.raises(ValueError):
        weighted_summary(np.zeros(10), weights=w)
    with pytest.raises(ValueError):
        psis(np.zeros(10), np.zeros(9))
    with pytest.raises(ValueError):
        psis(np.zeros(0))


def test_cpu_tensors_take_the_host_port_and_psis_is_exported_twice():
    import torch
    import bayesfast_amd.evidence as ev
    assert ev.psis is psis
    logp, logq, x = pr.gaussian_pair(500, 0.8, seed=4)
    r = psis(torch.as_tensor(logp), torch.as_tensor(logq))
    assert_psis(r, pr.psis_reference(logp - logq))
    t = weighted_summary(torch.as_tensor(x[:, None]), log_weights=torch.as_tensor(r.log_weights))
    assert_table(t, pr.table_reference(x[:, None], log_weights=r.log_weights))


def host_tracetuple():
    c, n, d = 5, 40, 3
    rng = np.random.default_rng(11)
    s = rng.standard_normal((c, n, d))
    st = np.zeros((c, n, _lib.STAT_STRIDE))
    st[:, :, 0] = rng.standard_normal((c, n))
    return TraceTuple(NTrace(n_chain=c, n_iter=n, n_warmup=12), s, st, s * 10 + 1, st[:, :, 0] - 1.)


@pytest.mark.parametrize('kw', [dict(), dict(since_iter=7), dict(include_warmup=True), dict(original_space=False),
                                dict(return_type='logp')])
def test_tracetuple_weighted_summary_on_host_parts(kw, monkeypatch):
    tt = host_tracetuple()
    x = tt.get(flatten=False, **kw)
    x = x[:, :, None] if x.ndim == 2 else x
    lw = np.random.default_rng(2).standard_normal(x.shape[:2])
    want = weighted_summary(x, log_weights=lw, probs=(0.1, 0.9))
    got = tt.weighted_summary(lw, probs=(0.1, 0.9), **kw)
    assert got.names == want.names and all(np.array_equal(got[k], want[k], equal_nan=True) for k in want.names)
    assert_table(got, pr.table_reference(x, log_weights=lw, probs=(0.1, 0.9)))
    with pytest.raises(ValueError):
        tt.weighted_summary(lw, since_iter=39)
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r'gather\(\)'):
        tt.weighted_summary(lw, **kw)
