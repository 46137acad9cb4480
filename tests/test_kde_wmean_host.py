"""The kernel-weighted means of ``utils.kde`` on the host port: ``_wmean_host`` against a direct difference form in numpy.longdouble,
``grad_logpdf`` against central differences of ``logpdf``, ``regress(loo=True)`` against a loop over the rows, ``mean_shift`` against
the score at its end points, ``utils.modes`` on a two-component mixture, and the value rules of zero-weight rows and bad values.

Tolerance of the first comparison, derived as in ``tests/test_gpu_kde.py``: with R2 = |zq_i|^2 + max_j |z_j|^2 an exponent carries about
eps R2 of absolute error and a sum of n positive terms n eps relative, so every normalised weight p_ij is off by at most
b_i = eps (64 (1 + R2) + n) relative, the numerator and the denominator each; hence |mean - ref|[i, c] <= 2 b_i max_j |v_jc|."""
import numpy as np
import pytest

from bayesfast_amd.utils import kde, modes
from bayesfast_amd.utils.kde import _wmean_host

EPS = 2.2e-16
LD = np.longdouble


def reference(z, logw, zq, v, exclude_self=False):
    """(logsum, mean, b) by differences in longdouble over the rows that carry weight."""
    n = z.shape[0]
    on = logw > -np.inf
    idx = np.flatnonzero(on)
    zl, ql, lwl, vl = z[on].astype(LD), zq.astype(LD), logw[on].astype(LD), v[on].astype(LD)
    ls, mean = np.empty(zq.shape[0]), np.empty((zq.shape[0], v.shape[1]))
    for i in range(zq.shape[0]):
        t = lwl - 0.5 * ((ql[i] - zl)**2).sum(axis=1)
        keep = idx != i if exclude_self else np.ones(idx.size, dtype=bool)
        if not keep.any():
            ls[i], mean[i] = -np.inf, np.nan
            continue
        top = t[keep].max()
        p = np.exp(t[keep] - top)
        ls[i] = float(top + np.log(p.sum()))
        mean[i] = (p[:, None] * vl[keep]).sum(axis=0) / p.sum()
    r2 = (zq**2).sum(axis=1) + ((z[on]**2).sum(axis=1).max() if on.any() else 0.)
    return ls, mean, EPS * (64. * (1. + r2) + n)


def close(got_ls, got_mean, z, logw, zq, v, what, exclude_self=False):
    ls, mean, b = reference(z, logw, zq, v, exclude_self)
    vmax = np.abs(v[logw > -np.inf]).max(axis=0) if (logw > -np.inf).any() else np.zeros(v.shape[1])
    fin = np.isfinite(ls)
    assert np.array_equal(got_ls[~fin], ls[~fin]) and np.all(np.isnan(got_mean[~fin])), what
    r1 = float(np.max(np.abs(got_ls[fin] - ls[fin]) / b[fin])) if fin.any() else 0.
    r2 = float(np.max(np.abs(got_mean[fin] - mean[fin]) / (2. * b[fin, None] * np.maximum(vmax, 1e-300)[None, :]))) if fin.any() else 0.
    print(what, 'largest |host - ref| / bound: logsum', r1, 'mean', r2)
    assert r1 <= 1. and r2 <= 1., what


def test_wmean_host_against_differences():
    rng = np.random.default_rng(0)
    for n, m, d, k in ((300, 17, 3, 2), (1000, 33, 27, 5), (16, 5, 1, 1)):
        z, zq = rng.standard_normal((n, d)), rng.standard_normal((m, d)) * 1.3
        logw, v = np.log(rng.uniform(size=n)), rng.standard_normal((n, k)) * 3.
        ls, mean = _wmean_host(z, logw, zq, v)
        close(ls, mean, z, logw, zq, v, 'n %d d %d k %d' % (n, d, k))
        ls, mean = _wmean_host(z, logw, zq, z)
        close(ls, mean, z, logw, zq, z, 'v = z, n %d d %d' % (n, d))
        ls, mean = _wmean_host(z, logw, z, v, exclude_self=True)
        close(ls, mean, z, logw, z, v, 'exclude_self n %d d %d' % (n, d), exclude_self=True)
    # far queries: the density underflows, the mean is the nearest rows' and finite
    z, logw = rng.standard_normal((200, 4)), np.full(200, -np.log(200.))
    zq = np.array([[40., 0., 0., 0.], [0., -60., 0., 0.]])
    ls, mean = _wmean_host(z, logw, zq, z)
    assert np.all(ls < -600.) and np.exp(ls[1]) == 0. and np.all(np.isfinite(mean))
    assert mean[0, 0] > 2. and mean[1, 1] < -2.
    close(ls, mean, z, logw, zq, z, 'far queries')


def test_value_rules_host():
    rng = np.random.default_rng(1)
    n, m, d, k = 60, 7, 3, 4
    z, zq, v = rng.standard_normal((n, d)), rng.standard_normal((m, d)), rng.standard_normal((n, k))
    logw = np.log(rng.uniform(size=n))
    off = np.arange(n) % 3 == 1
    lw = np.where(off, -np.inf, logw)
    # rows of weight -inf are no part of the sample, whatever z and v hold there
    got = _wmean_host(np.where(off[:, None], np.nan, z), lw, zq, np.where(off[:, None], np.inf, v))
    want = _wmean_host(z[~off], lw[~off], zq, v[~off])
    assert np.allclose(got[0], want[0], rtol=0, atol=1e-13) and np.allclose(got[1], want[1], rtol=0, atol=1e-13)
    # a bad weight or a bad z row of non-zero weight: every output NaN
    for bad in (np.nan, np.inf):
        lb = logw.copy()
        lb[5] = bad
        ls, mean = _wmean_host(z, lb, zq, v)
        assert np.all(np.isnan(ls)) and np.all(np.isnan(mean))
        zb = z.copy()
        zb[7, 1] = bad
        ls, mean = _wmean_host(zb, logw, zq, v)
        assert np.all(np.isnan(ls)) and np.all(np.isnan(mean))
        # a bad value: its column, for every query, and nothing else
        vb = v.copy()
        vb[9, 2] = bad
        ls, mean = _wmean_host(z, logw, np.vstack([zq, np.full((1, d), 60.)]), vb)
        assert np.all(np.isfinite(ls)) and np.all(np.isnan(mean[:, 2])) and np.all(np.isfinite(np.delete(mean, 2, axis=1)))
    # a query with no term
    lw = np.full(n, -np.inf)
    lw[11] = 0.
    ls, mean = _wmean_host(z, lw, z, v, exclude_self=True)
    assert ls[11] == -np.inf and np.all(np.isnan(mean[11]))
    assert np.allclose(np.delete(mean, 11, axis=0), v[11][None, :], rtol=0, atol=1e-15)
    est = kde(z)
    with pytest.raises(ValueError):
        est.regress(v[:, 0], x=zq, loo=True)
    with pytest.raises(ValueError):
        est.regress(v[:-1])


def test_grad_logpdf_against_central_differences():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((500, 3)) * np.array([1., 2., 0.5]) + np.array([10., -3., 0.])
    w = rng.uniform(size=500)
    q = rng.standard_normal((9, 3)) * np.array([1., 2., 0.5]) + np.array([10., -3., 0.])
    for kw in (dict(), dict(bw_method='silverman', weights=w)):
        est = kde(x, **kw)
        g = est.grad_logpdf(q)
        assert g.shape == (9, 3)
        h = 1e-5
        for a in range(3):
            e = np.zeros(3)
            e[a] = h
            num = (est.logpdf(q + e) - est.logpdf(q - e)) / (2. * h)
            assert np.all(np.abs(g[:, a] - num) <= 1e-6 * (1. + np.abs(num))), (kw, a)
    est = kde(x[:, 0])
    g = est.grad_logpdf(q[:, 0])
    num = (est.logpdf(q[:, 0] + 1e-5) - est.logpdf(q[:, 0] - 1e-5)) / 2e-5
    assert g.shape == (9, 1) and np.all(np.abs(g[:, 0] - num) <= 1e-6 * (1. + np.abs(num)))


def test_regress_against_a_loop():
    rng = np.random.default_rng(3)
    n, d = 120, 2
    x = rng.standard_normal((n, d)) * np.array([1., 3.])
    w = rng.uniform(size=n)
    w[::7] = 0.
    vals = np.stack([np.sin(x[:, 0]), x[:, 1]**2, rng.standard_normal(n)], axis=1)
    est = kde(x, weights=w, bw_factor=0.7)
    got = est.regress(vals, loo=True)
    full = est.regress(vals)
    at = est.regress(vals[:, 1], x=x[:5] + 0.1)
    assert got.shape == (n, 3) and full.shape == (n, 3) and at.shape == (5,)
    wn = w / w.sum()

    def nw(point, skip):
        r = point[None, :] - x
        kern = wn * np.exp(-0.5 * np.einsum('ij,jk,ik->i', r, est.inv_cov, r))
        if skip is not None:
            kern[skip] = 0.
        return (kern[:, None] * vals).sum(axis=0) / kern.sum()
    for i in range(n):
        if w[i] > 0.:       # at a row of zero weight the query is the whitened origin: the row is no part of the sample
            assert np.allclose(got[i], nw(x[i], i), rtol=1e-10, atol=1e-12), i
            assert np.allclose(full[i], nw(x[i], None), rtol=1e-10, atol=1e-12), i
    for i in range(5):
        assert np.allclose(at[i], nw(x[i] + 0.1, None)[1], rtol=1e-10, atol=1e-12)


def test_mean_shift_ends_at_a_stationary_point():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1500, 3)) + np.array([1., -2., 0.5])
    est = kde(x)
    x0 = x[:40]
    xe, lp, n_iter, conv = est.mean_shift(x0)
    assert xe.shape == (40, 3) and lp.shape == (40,) and conv.shape == (40,) and conv.all()
    assert 8 <= n_iter < 1000 and n_iter % 8 == 0
    assert np.all(np.sqrt((est.grad_logpdf(xe)**2).sum(axis=1)) < 1e-6)
    assert np.allclose(lp, est.logpdf(xe), rtol=0, atol=1e-12) and np.all(lp >= est.logpdf(x0) - 1e-12)
    # a limit of iterations: flagged, not hidden
    xe, lp, n_iter, conv = est.mean_shift(x0, max_iter=3)
    assert n_iter == 3 and not conv.any()


def mixture(seed, sep, n=4000, d=3):
    rng = np.random.default_rng(seed)
    lab = rng.uniform(size=n) < 0.3
    x = rng.standard_normal((n, d))
    x[lab, 0] += sep
    return x, lab


@pytest.mark.parametrize('seed', range(5))
def test_modes_of_a_mixture(seed):
    """Two unit Gaussians 6 sd apart, 30 % and 70 %, n = 4000, d = 3, bw_factor = 2: two modes, no minor one, the shares within
    4 share_err.  A NumPy mean shift of the same data with other seeds took 63 to 79 iterations and found two modes on all five
    data sets; with the systematic seeds of ``modes`` it is 64 to 80 (looked at every 8) and shares of 0.684 to 0.723 for the larger."""
    x, lab = mixture(seed, 6.)
    mo = modes(x, bw_factor=2., n_seeds=256, seed=seed)
    print(mo, mo.x, mo.share_err)
    assert mo.n_modes == 2 and mo.n_minor == 0 and mo.n_not_converged == 0 and mo.x.shape == (2, 3)
    assert abs(mo.share[0] - 0.7) <= 4. * mo.share_err[0] and abs(mo.share[1] - 0.3) <= 4. * mo.share_err[1]
    assert abs(mo.x[0, 0]) < 0.5 and abs(mo.x[1, 0] - 6.) < 0.5 and mo.logpdf[0] > mo.logpdf[1]
    assert mo.label.shape == (256,) and mo.seed_index.shape == (256,) and mo.chain_mode is None
    # a seed climbs to the mode of its own component, but for the rows between the two (2.3 % of a component lie beyond 2 sd)
    assert np.mean(mo.label == lab[mo.seed_index]) > 0.9
    assert 0 < mo.n_iter < 1000 and abs(mo.factor - 2. * 4000.**(-1. / 7.)) < 1e-12


def test_modes_of_one_gaussian_and_weights():
    x, _ = mixture(0, 0.)
    mo = modes(x, bw_factor=2., n_seeds=256, seed=0)
    assert mo.n_modes == 1 and mo.n_minor == 0 and mo.share[0] == 1. and mo.share_err[0] == 0.
    # weights that remove the smaller component: its rows are never seeds and the mode is gone; params selects columns
    x, lab = mixture(1, 6.)
    mo = modes(x, log_weights=np.where(lab, -np.inf, 0.), params=[0, 2], bw_factor=2., n_seeds=128, seed=3)
    assert mo.n_modes == 1 and mo.x.shape == (1, 2) and not lab[mo.seed_index].any()
