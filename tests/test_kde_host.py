"""The host port of ``bayesfast_amd.utils.kde`` and ``parameter_shift`` (no GPU): against the reference's own class through the
fixture tests/golden/kde.npz (tests/golden/make_kde_golden.py), against ``scipy.stats.gaussian_kde`` (which takes its points
transposed), and against closed forms and explicit loops."""
import os

import numpy as np
import pytest
from scipy.special import ndtr
from scipy.stats import gaussian_kde

from bayesfast_amd.utils import kde, parameter_shift, ParameterShift

RTOL = 1e-10


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'kde.npz'))


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_against_the_reference(golden, name):
    from make_kde_golden import cases
    kw = cases()[name][3]
    w = golden[name + '_w'] if name + '_w' in golden.files else None
    x, q = golden[name + '_x'], golden[name + '_q']
    est = kde(x, weights=w, **kw)
    assert np.isclose(est.factor, golden[name + '_factor'], rtol=RTOL, atol=0)
    assert np.allclose(est.covariance, golden[name + '_covariance'], rtol=RTOL, atol=0)
    assert np.allclose(est.pdf(q), golden[name + '_pdf'], rtol=RTOL, atol=0)
    assert np.allclose(est(q), golden[name + '_pdf'], rtol=RTOL, atol=0)
    assert np.allclose(est.logpdf(q), golden[name + '_logpdf'], rtol=RTOL, atol=0)
    assert np.allclose(est.inv_cov @ est.covariance, np.eye(est.d), atol=1e-9)


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) @ rng.standard_normal((d, d)) + 5. * rng.standard_normal(d)
    return x, rng.uniform(0.1, 1., size=n), rng.standard_normal((40, d)) @ rng.standard_normal((d, d)) * 1.5


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('bw', ['scott', 'silverman', 0.45, 'callable', None])
@pytest.mark.parametrize('d', [1, 3])
def test_against_scipy(d, bw, weighted):
    x, w, q = _data(250, d, 11 * d)
    w = w if weighted else None
    rule = (lambda e: 0.3 * e.neff**-0.1) if bw == 'callable' else bw
    for bw_factor in (None, 0.8):
        est = kde(x if d > 1 else x[:, 0], bw_method=rule, bw_factor=bw_factor, weights=w)
        ref = gaussian_kde(x.T, bw_method=rule, weights=w)
        if bw_factor is not None:
            ref.set_bandwidth(ref.factor * bw_factor)
        assert est.n == 250 and est.d == d and np.isclose(est.neff, ref.neff, rtol=RTOL)
        assert np.isclose(est.factor, ref.factor, rtol=RTOL, atol=0)
        assert np.allclose(est.covariance, ref.covariance, rtol=RTOL, atol=0)
        assert np.allclose(est.inv_cov, np.linalg.inv(ref.covariance), rtol=1e-8, atol=0)
        assert np.allclose(est.pdf(q), ref.pdf(q.T), rtol=RTOL, atol=0)
        assert np.allclose(est.logpdf(q), ref.logpdf(q.T), rtol=RTOL, atol=0)
        if w is not None:
            assert np.allclose(est.weights, w / w.sum(), rtol=1e-15)
            lw = kde(x, bw_method=rule, bw_factor=bw_factor, log_weights=np.log(w) + 3.)
            assert np.allclose(lw.logpdf(q), ref.logpdf(q.T), rtol=RTOL, atol=0) and np.isclose(lw.neff, ref.neff, rtol=RTOL)
    # a (d,) vector is one point; set_bandwidth changes later evaluations
    assert np.array_equal(est.logpdf(q[0]), est.logpdf(q[:1]))
    est.set_bandwidth('silverman')
    assert np.isclose(est.factor, est.silverman_factor() * 0.8) and np.isclose(est.scotts_factor(), est.neff**(-1. / (d + 4)))
    # CPU tensors take the host port
    import torch
    t = kde(torch.as_tensor(x), weights=w, bw_method='silverman', bw_factor=0.8)
    assert isinstance(t.logpdf(torch.as_tensor(q)), np.ndarray) and np.array_equal(t.logpdf(torch.as_tensor(q)), est.logpdf(q))


def test_far_query():
    """40 in every coordinate of a 4-d standard normal sample: the density underflows, its logarithm does not."""
    x = np.random.default_rng(3).standard_normal((1000, 4))
    est, ref = kde(x), gaussian_kde(x.T)
    far = np.full((1, 4), 40.)
    assert est.pdf(far)[0] == 0.
    lp = est.logpdf(far)[0]
    assert np.isfinite(lp) and lp < -1e4 and np.isclose(lp, ref.logpdf(far.T)[0], rtol=RTOL, atol=0)


def test_cdf():
    x, w, _ = _data(300, 1, 5)
    g = np.linspace(x.min() - 3., x.max() + 3., 61)
    for weights in (None, w):
        est = kde(x[:, 0], 'silverman', weights=weights)
        wn = np.full(300, 1. / 300) if weights is None else w / w.sum()
        h = np.sqrt(est.covariance[0, 0])
        assert np.allclose(est.cdf(g), (wn[None, :] * ndtr((g[:, None] - x[None, :, 0]) / h)).sum(axis=1), rtol=1e-12, atol=1e-15)
        assert np.allclose(est.cdf(g[7]), est.cdf(g[7:8]))
    with pytest.raises(NotImplementedError, match='currently only supports cdf for 1-d kde'):
        kde(np.random.default_rng(0).standard_normal((50, 2))).cdf(np.zeros((1, 2)))


def test_logpdf_loo():
    x, w, _ = _data(200, 3, 6)
    for weights in (None, w):
        est = kde(x, 'silverman', weights=weights)
        wn = est.weights
        got = est.logpdf_loo()
        for i in range(200):
            keep = np.arange(200) != i
            # the full estimate's kernel and normalisation, row i deleted, the other weights renormalised
            diff = x[i] - x[keep]
            e = 0.5 * np.einsum('ij,jk,ik->i', diff, est.inv_cov, diff)
            ref = np.log((wn[keep] / wn[keep].sum() * np.exp(-e)).sum()) - 0.5 * np.log(np.linalg.det(2. * np.pi * est.covariance))
            assert np.isclose(got[i], ref, rtol=1e-9, atol=1e-12), i
        assert np.all(got < est.logpdf(x))
    # a zero-weight row changes nothing, whatever it holds
    w0 = np.append(w, 0.)
    x0 = np.vstack([x, np.full((1, 3), np.nan)])
    a, b = kde(x0, 'silverman', weights=w0), kde(x, 'silverman', weights=w)
    assert np.isclose(a.factor, b.factor, rtol=1e-15) and np.allclose(a.covariance, b.covariance, rtol=1e-13, atol=0)
    assert np.allclose(a.logpdf_loo()[:-1], b.logpdf_loo(), rtol=1e-12, atol=1e-12)
    assert np.allclose(a.logpdf(x[:9]), b.logpdf(x[:9]), rtol=1e-12, atol=1e-12)
    # a row of weight 1 (no covariance exists for such a sample, so the weights are put in place after the bandwidth is set)
    one = kde(x[:5], 0.5)
    one._weights = np.array([0., 0., 1., 0., 0.])
    one._logw = np.array([-np.inf, -np.inf, 0., -np.inf, -np.inf])
    loo = one.logpdf_loo()
    assert loo[2] == -np.inf and np.all(np.isfinite(np.delete(loo, 2)))


def test_resample():
    x, w, _ = _data(400, 3, 7)
    est = kde(x, 'silverman', weights=w)
    assert np.array_equal(est.resample(100, seed=4), est.resample(100, seed=4))
    assert est.resample(seed=1).shape == (int(est.neff), 3)
    n = 200000
    r = est.resample(n, seed=2)
    wn = w / w.sum()
    mean = wn @ x
    cov = (x - mean).T @ (wn[:, None] * (x - mean))       # the mixture's covariance: that of its means plus the kernel's
    target = cov + est.covariance
    se_mean = np.sqrt(np.diag(target) / n)
    assert np.all(np.abs(r.mean(axis=0) - mean) <= 5. * se_mean)
    # within 5 standard errors of (1 + factor^2) times the data's covariance
    c = np.cov(r, rowvar=False)
    y = r - r.mean(axis=0)
    se_cov = np.sqrt(np.maximum(np.einsum('ni,nj->ij', y**2, y**2) / n - c**2, 0.) / n)
    data_cov = est.covariance / est.factor**2
    assert np.all(np.abs(c - (1. + est.factor**2) * data_cov) <= 5. * se_cov)


def test_errors():
    x = np.random.default_rng(8).standard_normal((30, 3))
    with pytest.raises(ValueError, match='`dataset` should be a 1-d or 2-d array.'):
        kde(np.zeros((3, 3, 3)))
    with pytest.raises(ValueError, match='`dataset` input should have multiple elements.'):
        kde(np.zeros((1, 1)))
    with pytest.raises(ValueError, match="`bw_method` should be 'scott', 'silverman', a scalar or a callable."):
        kde(x, bw_method='wrong')
    with pytest.raises(ValueError, match='`weights` input should be of length n'):
        kde(x, weights=np.ones(29))
    with pytest.raises(ValueError, match='`weights` input should be one-dimensional.'):
        kde(x, weights=np.ones((30, 1)))
    with pytest.raises(ValueError, match='points have dimension 2, dataset has dimension 3'):
        kde(x).pdf(np.zeros((5, 2)))
    with pytest.raises(ValueError):
        kde(x, weights=np.ones(30), log_weights=np.zeros(30))


def _two_gaussians(seed, d, sep, n=4000):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, d))
    b = 0.7 * rng.standard_normal((n, d))
    b[:, 0] += sep
    return a, b


def test_parameter_shift_three_dimensions():
    """Unit covariance against 0.49 I, the means 3 apart along one axis, 4000 rows each, n_pairs = 4000: the exact probability is
    the chi-square cdf (3 degrees of freedom) at 9 / 1.49, 0.8903.

    The margin of ``prob`` is measured, not chosen: the host port with loo=True on the 20 cases
    ``_two_gaussians(1000 + s, 3, 3.)``, ``seed=s``, s = 0 .. 19, gave
        0.8532 0.9202 0.8952 0.9250 0.8715 0.9078 0.8950 0.8842 0.8800 0.9000
        0.8995 0.9115 0.8955 0.8940 0.8720 0.9392 0.8820 0.8895 0.8835 0.8562
    (mean 0.8928, standard deviation 0.0211; the noise of the single value p(0), not the binomial 0.005).  The largest deviation
    from 0.8903 is 0.0489 (s = 15); this test's own case (s = 20) has to stay within 1.5 times that."""
    from scipy.stats import chi2
    exact = chi2.cdf(9. / 1.49, 3)
    assert abs(exact - 0.8903) < 5e-5
    a, b = _two_gaussians(1020, 3, 3.)
    r = parameter_shift(a, b, n_pairs=4000, seed=20)
    print(r)
    assert isinstance(r, ParameterShift) and r.n_pairs == 4000 and r.d == 3 and not r.saturated
    assert abs(r.gaussian_prob - exact) <= 0.02
    assert abs(r.prob - exact) <= 1.5 * 0.0489
    assert np.isclose(r.prob_err, np.sqrt(r.prob * (1. - r.prob) / 4000))
    assert np.isclose(r.factor, (4000 * 5. / 4.)**(-1. / 7.)) and r.logpdf.shape == (4000,)
    assert r.prob == np.count_nonzero(r.logpdf > r.logpdf_zero) / 4000
    assert np.allclose(r.mean_shift, [-3., 0., 0.], atol=0.1) and np.allclose(r.cov_shift, 1.49 * np.eye(3), atol=0.12)
    from scipy.special import erfinv
    assert np.isclose(r.n_sigma, np.sqrt(2.) * erfinv(r.prob)) and np.isclose(r.gaussian_n_sigma, np.sqrt(2.) * erfinv(r.gaussian_prob))
    # the same seed gives the same pairs; weights that select half of a give the same answer within the noise
    assert parameter_shift(a, b, n_pairs=4000, seed=20).prob == r.prob
    lw = np.where(np.arange(4000) % 2 == 0, 0., -np.inf)
    rw = parameter_shift(a, b, log_weights_a=lw, n_pairs=4000, seed=20)
    assert abs(rw.prob - exact) <= 1.5 * 0.0489 and abs(rw.gaussian_prob - exact) <= 0.03
    # params selects columns
    rp = parameter_shift(a, b, params=[0], n_pairs=2000, seed=1)
    assert rp.d == 1 and abs(rp.gaussian_prob - chi2.cdf(9. / 1.49, 1)) <= 0.02
    with pytest.raises(ValueError):
        parameter_shift(a, b[:, :2])


def test_parameter_shift_six_dimensions_self_term():
    """d = 6, the means 3.5 apart (exact 0.778): with the self term the estimate saturates at 1; leave-self-out it does not."""
    a, b = _two_gaussians(2000, 6, 3.5)
    with_self = parameter_shift(a, b, n_pairs=4000, loo=False, seed=0)
    print(with_self)
    assert with_self.prob == 1. and with_self.saturated
    assert np.isclose(with_self.n_sigma, np.sqrt(2.) * __import__('scipy.special').special.erfinv(1. - 1. / 8000.))
    loo = parameter_shift(a, b, n_pairs=4000, loo=True, seed=0)
    print(loo)
    assert loo.prob < 0.95 and not loo.saturated
    assert abs(loo.gaussian_prob - 0.778) <= 0.03


def test_version():
    from bayesfast_amd import _lib
    assert _lib.lib().bfhip_version() >= 113
