"""The Gaussian mixture of ``bayesfast_amd.utils.gmm`` on the host route (no GPU): one pass (``_step_host``) against a brute-force
reference written here, the EM iteration against scikit-learn's, weights against repeated rows, the monotone log likelihood, recovery
of a two-component sample with the BIC choosing two, the value rules and the work-buffer rules of the library.

The bound of one pass is derived in tests/helpers/gmm_cases.py.  The EM tolerances: with the same initial parameters, ``tol=0`` and 25
iterations a NumPy prototype of the module's formulas agreed with scikit-learn 1.7.2 to 1.1e-14 (weights), 1.6e-13 (means), 4.5e-13
(covariances) and 4e-14 (log likelihood against ``lower_bound_``), and one iteration more or less differs by 1e-2, so the count is
pinned; integer weights against repeated rows agreed to 1.1e-13.  Both assert 1e-10: EM in mid-convergence may amplify rounding
differently in another BLAS."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

from gmm_cases import EPS, mixture, step_case, step_bounds   # noqa: E402

from bayesfast_amd.utils import gmm, gmm_step, GaussianMixture   # noqa: E402
from bayesfast_amd.utils.gmm import _step_host   # noqa: E402

DATA = [(3, 6., 4000), (5, 3., 2000), (27, 4., 3000)]


def brute(c):
    """logpdf, resp and stats from scipy's multivariate normal per component and Python sums per row."""
    from scipy.stats import multivariate_normal
    x, logw, centre = c['x'], c['logw'], c['centre']
    n, d = x.shape
    K = c['mean'].shape[0]
    lt = np.stack([np.log(c['pi'][k]) + multivariate_normal(c['mean'][k], c['covs'][k]).logpdf(x).reshape(n) for k in range(K)], axis=1)
    lp, r = np.empty(n), np.empty((n, K))
    for i in range(n):
        top = max(lt[i])
        lp[i] = top + math.log(math.fsum(math.exp(v - top) for v in lt[i]))
        r[i] = [math.exp(v - lp[i]) for v in lt[i]]
    w = np.ones(n) if logw is None else np.exp(logw)
    xc = x - centre
    st = np.empty(K * (1 + d + d * d) + 2)
    for k in range(K):
        st[k] = math.fsum(w[i] * r[i, k] for i in range(n))
        for a in range(d):
            st[K + k * d + a] = math.fsum(w[i] * r[i, k] * xc[i, a] for i in range(n))
            for b in range(d):
                st[K * (1 + d) + (k * d + a) * d + b] = math.fsum(w[i] * r[i, k] * xc[i, a] * xc[i, b] for i in range(n))
    st[-2] = math.fsum(w[i] * lp[i] for i in range(n))
    st[-1] = math.fsum(w)
    return st, lp, r


@pytest.mark.parametrize('n,d,K', [(257, 3, 2), (50, 27, 3)])
def test_step_against_brute_force(n, d, K):
    for weights in (True, False):
        c = step_case(n, d, K, seed=1, weights=weights)
        st, lp, r = _step_host(c['x'], c['logw'], c['centre'], c['mean'], c['whiten'], c['logc'])
        rst, rlp, rr = brute(c)
        f, fst = step_bounds(c['x'], c['logw'], c['centre'], c['mean'], c['whiten'], c['logc'], rlp, rr)
        print('n %d d %d K %d weights %s: ratios to the bound: logpdf %.3g resp %.3g stats %.3g' % (
            n, d, K, weights, np.abs(lp - rlp).max() / f, np.abs(r - rr).max() / f, (np.abs(st - rst) / np.maximum(fst, 1e-300)).max()))
        assert np.all(np.abs(lp - rlp) <= f) and np.all(np.abs(r - rr) <= f)
        assert np.all(np.abs(st - rst) <= fst)
        s2 = st[K * (1 + d):-2].reshape(K, d, d)
        assert np.array_equal(s2, s2.swapaxes(1, 2))
        # asking for less changes nothing
        only = gmm_step(c['x'], c['logw'], c['centre'], c['mean'], c['whiten'], c['logc'], stats=False, resp=False)
        assert only[0] is None and only[2] is None and np.array_equal(only[1], lp)


def _inits(x, lab):
    cov = np.cov(x.T)
    return dict(weights_init=np.array([0.5, 0.5]), means_init=np.stack([x[np.flatnonzero(lab)[0]], x[np.flatnonzero(~lab)[0]]]),
                covariances_init=np.stack([cov, cov]))


@pytest.mark.parametrize('d,sep,n', DATA)
def test_em_against_sklearn(d, sep, n):
    mix = pytest.importorskip('sklearn.mixture')
    import warnings
    x, lab = mixture(0, sep, n, d)
    ini = _inits(x, lab)
    g = gmm(x, 2, tol=0., max_iter=25, reg_covar=1e-6, **ini)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sk = mix.GaussianMixture(2, covariance_type='full', tol=0., max_iter=25, reg_covar=1e-6, weights_init=ini['weights_init'],
                                 means_init=ini['means_init'], precisions_init=np.linalg.inv(ini['covariances_init'])).fit(x)
    assert sk.n_iter_ == 25 and g.n_iter == 25 and not g.converged
    order = np.argsort(-sk.weights_, kind='stable')
    dw = np.abs(g.weights - sk.weights_[order]).max()
    dm = np.abs(g.means - sk.means_[order]).max()
    dc = np.abs(g.covariances - sk.covariances_[order]).max()
    dl = abs(g.log_likelihood - sk.lower_bound_)
    print('d %d: weights %.3g means %.3g covariances %.3g log_likelihood %.3g' % (d, dw, dm, dc, dl))
    assert dw <= 1e-10 and dm <= 1e-10 and dc <= 1e-10 and dl <= 1e-10
    assert g.history[-1] - g.history[0] > 1e-2      # the iteration moved: the comparison is not one of the initial values


@pytest.mark.parametrize('d,sep,n', DATA)
def test_weights_against_repetition(d, sep, n):
    x, lab = mixture(0, sep, n, d)
    ini = _inits(x, lab)
    w = np.random.default_rng(3).integers(0, 4, size=n)
    with np.errstate(divide='ignore'):
        a = gmm(x, 2, log_weights=np.log(w.astype(np.float64)), tol=0., max_iter=10, **ini)
    b = gmm(np.repeat(x, w, axis=0), 2, tol=0., max_iter=10, **ini)
    dm, dc, dl = np.abs(a.means - b.means).max(), np.abs(a.covariances - b.covariances).max(), abs(a.log_likelihood - b.log_likelihood)
    print('d %d: means %.3g covariances %.3g log_likelihood %.3g' % (d, dm, dc, dl))
    assert dm <= 1e-10 and dc <= 1e-10 and dl <= 1e-10
    assert abs(a.neff - w.sum()**2 / float((w**2).sum())) <= 1e-9 * a.neff and b.neff == w.sum()


def test_log_likelihood_is_monotone():
    x, _ = mixture(0, 6., 4000, 3)
    g = gmm(x, 2, reg_covar=0., tol=0., max_iter=60)
    h = g.history
    assert h.shape == (60,) and g.log_likelihood == h[-1]
    drop = (h[:-1] - h[1:]) / np.abs(h[1:])
    print('largest relative decrease', drop.max())
    assert np.all(drop <= 1e-12)


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('n,d', [(4000, 3), (2000, 5)])
def test_recovery_and_bic(seed, n, d):
    x, lab = mixture(seed, 6., n, d)
    g = gmm(x, (1, 2, 3), max_iter=200)
    print(g, g.bic_path)
    assert isinstance(g, GaussianMixture) and g.n_components == 2 and len(g.candidates) == 3 and g.bic_path.shape == (3, 5)
    assert np.array_equal(g.bic_path[:, 0], [1, 2, 3]) and g.bic == g.bic_path[:, 3].min()
    assert g.n_parameters == 1 + 2 * d + d * (d + 1) and g.neff == n
    assert abs(g.bic - (-2. * n * g.log_likelihood + g.n_parameters * np.log(n))) <= 1e-9 * abs(g.bic)
    assert g.weights[0] >= g.weights[1] and abs(g.weights.sum() - 1.) <= 1e-12
    assert abs(g.weights[1] - lab.mean()) <= 3. * np.sqrt(0.3 * 0.7 / n)
    centre = np.zeros((2, d))
    centre[1, 0] = 6.
    assert np.abs(g.means - centre).max() <= 0.15
    # soft labels: the labelled rows
    assert np.mean(g.labels() == lab) >= 0.99
    r = g.responsibilities()
    # exp(t - logpdf) carries the rounding of logpdf itself, eps |logpdf|, beside that of the two exponentials
    assert r.shape == (n, 2) and np.all(np.abs(r.sum(axis=1) - 1.) <= (4. + np.abs(g.logpdf(x))) * np.finfo(float).eps)
    # a density: logpdf agrees with the mixture written out, and resample draws from it
    from scipy.stats import multivariate_normal
    q = x[::97]
    dens = sum(g.weights[k] * multivariate_normal(g.means[k], g.covariances[k]).pdf(q) for k in range(2))
    assert np.allclose(g.pdf(q), dens, rtol=1e-10, atol=0) and np.allclose(g.logpdf(q), np.log(dens), rtol=0, atol=1e-10)
    s = g.resample(20000, seed=1)
    assert s.shape == (20000, d) and np.array_equal(s, g.resample(20000, seed=1))
    assert abs(np.mean(s[:, 0] > 3.) - g.weights[1]) <= 0.02
    share, comp, split = g.component_of_chain((8, n // 8))
    assert share.shape == (8, 2) and np.abs(share.sum(axis=1) - 1.).max() <= 1e-12 and comp.shape == (8,) and split.all()


def test_high_dimension_with_given_means():
    """d = 27: k-means++ among 26 noise dimensions starts badly (the documented limit), so the true centres, perturbed, are given."""
    x, lab = mixture(0, 4., 3000, 27)
    m0 = np.zeros((2, 27))
    m0[1, 0] = 4.
    m0 += np.random.default_rng(5).standard_normal((2, 27)) * 0.3
    g = gmm(x, 2, means_init=m0, max_iter=200)
    assert abs(g.weights[1] - lab.mean()) <= 3. * np.sqrt(0.3 * 0.7 / 3000) and np.mean(g.labels() == lab) >= 0.95


def test_value_rules():
    c = step_case(300, 4, 3, seed=2)
    args = lambda x, lw: (x, lw, c['centre'], c['mean'], c['whiten'], c['logc'])
    st, lp, r = _step_host(*args(c['x'], c['logw']))
    # a NaN row of weight -inf changes no bit of stats; its own logpdf and resp are NaN, nobody else's change
    lw = c['logw'].copy()
    lw[41] = -np.inf
    x0, xn = c['x'].copy(), c['x'].copy()
    x0[41] = 0.
    xn[41] = np.nan
    s0, lp0, r0 = _step_host(*args(x0, lw))
    sn, lpn, rn = _step_host(*args(xn, lw))
    assert np.array_equal(s0, sn) and np.isnan(lpn[41]) and np.isnan(rn[41]).all()
    assert np.array_equal(np.delete(lpn, 41), np.delete(lp0, 41)) and np.array_equal(np.delete(rn, 41, axis=0), np.delete(r0, 41, axis=0))
    # a NaN or +inf weight, or a non-finite row that carries weight: every entry of stats NaN; logpdf and resp do not look at logw
    for v in (np.nan, np.inf):
        lb = c['logw'].copy()
        lb[7] = v
        sb, lpb, rb = _step_host(*args(c['x'], lb))
        assert np.isnan(sb).all() and np.array_equal(lpb, lp) and np.array_equal(rb, r)
        xb = c['x'].copy()
        xb[7, 2] = v
        sb, lpb, rb = _step_host(*args(xb, c['logw']))
        assert np.isnan(sb).all() and np.isnan(lpb[7]) and np.isnan(rb[7]).all() and np.array_equal(np.delete(lpb, 7), np.delete(lp, 7))
    # a query at distance 1e4: every exp(t) underflows, the logpdf is finite and the responsibilities sum to 1
    far = np.full((1, 4), 1e4 / 2.)
    _, lpf, rf = _step_host(*args(far, None))
    assert np.isfinite(lpf[0]) and lpf[0] < -1e6 and abs(rf[0].sum() - 1.) <= 4 * np.finfo(float).eps


def test_one_component_is_the_weighted_moments():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((500, 3)) @ rng.standard_normal((3, 3)) + np.array([100., -3., 0.])
    lw = np.log(rng.uniform(size=500))
    g = gmm(x, 1, log_weights=lw, reg_covar=0., max_iter=3)
    w = np.exp(lw) / np.exp(lw).sum()
    mu = w @ x
    cov = (x - mu).T @ (w[:, None] * (x - mu))
    assert np.abs(g.means[0] - mu).max() <= 1e-12 * 100. and np.abs(g.covariances[0] - cov).max() <= 1e-12 * np.abs(cov).max()
    assert g.weights[0] == 1. and g.converged and g.n_collapsed == 0


def test_collapsed_component_is_counted():
    x, _ = mixture(0, 6., 4000, 3)
    m0 = np.array([[0., 0., 0.], [6., 0., 0.], [1e6, 0., 0.]])
    g = gmm(x, 3, means_init=m0, max_iter=40)
    print(g)
    assert g.n_collapsed == 1 and g.weights[2] < 1e-12 and np.array_equal(g.means[2], m0[2])
    assert np.isfinite(g.log_likelihood) and np.abs(g.means[:2] - m0[:2]).max() <= 0.15


def test_work_buffer_rules():
    from bayesfast_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert L.bfhip_version() >= 116
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'bfhip_gmm_step') and hasattr(raw, 'bfhip_gmm_work_bytes')
    wb = L.bfhip_gmm_work_bytes
    for bad in ((0, 3, 2), (10, 0, 2), (10, 3, 0), (10, 129, 2), (10, 3, 33), (2**31, 3, 2)):
        assert wb(*bad) == 0, bad
    assert wb(2**31 - 1, 128, 32) > 0
    last = 0
    for n in (1, 15, 16, 17, 255, 256, 257, 4099, 65536, 10**6, 10**7):
        b = wb(n, 27, 4)
        assert b >= last and b >= 8 * n * 4
        last = b
    # at most 8 n k bytes plus the partial statistics of 128 parts and 16 bytes per 64 rows (each rounded up to 256 bytes)
    n, d, k = 10**6, 27, 4
    assert wb(n, d, k) <= 8 * n * k + 16 * (n // 64 + 1) + 128 * k * (1 + d + d * d) * 8 + 3 * 256
    # a NULL context is refused before anything touches a GPU
    assert L.bfhip_gmm_step(None, 3, 2, 10, None, 3, None, None, None, None, None, None, None, None, 2, None, 0) == -1
