"""The pairwise kernel sum on the device (csrc/bfhip_kde.h: ``bfhip_kde_logsum``) through ctypes and ``utils.kde.kde_logsum``, the
``kde`` class and ``parameter_shift`` on device tensors, against the host port and a direct difference form in numpy.longdouble.
Expected values are never the device's.

Tolerance, derived and not tuned.  In whitened units, with R2 = |zq_i|^2 + max_j |z_j|^2 over the rows that carry weight: an energy
from two norms and a dot product carries about eps R2 of absolute error, and a sum of n positive terms at most n eps relative, so
    |logsum_dev - logsum_ref| <= eps (64 (1 + R2) + n),   eps = 2.2e-16,
per query.  Every comparison prints the largest ratio to that bound before it asserts.

Shapes: d in {1, 3, 4, 5, 27, 64, 128} (every k-step class of the tile kernel but 12 and 24, which 45 and 90 add; 4 | 5 a k-step
boundary); n in {1, 15, 16, 17, 1000} (a data tile is 16 rows) and 767 | 768 | 769, where the partition rule of csrc/bfhip_kde.h
(parts of at least 256 rows, a multiple of 16) gives 3, 3 and 4 parts; m in {1, 15, 16, 17, 33} (a query tile is 16 rows, a
workgroup takes 64) and 8193, one more than a launch's chunk of queries."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
LD = np.longdouble


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context()


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return _ctx().tensor(np.ascontiguousarray(a, dtype=np.float64))


def plan(n):
    """kd_plan of csrc/bfhip_kde.h: (parts, rows of a part)."""
    p = min((n + 255) // 256, 256)
    r = (-(-n // p) + 15) // 16 * 16
    return -(-n // r), r


def reference(z, logw, zq, exclude_self=False):
    """log sum_j exp(logw_j - |zq_i - z_j|^2 / 2) by differences in longdouble, and the bound of every query."""
    n = z.shape[0]
    lw = np.zeros(n) if logw is None else logw
    on = lw > -np.inf
    zl, ql, lwl = z[on].astype(LD), zq.astype(LD), lw[on].astype(LD)
    idx = np.flatnonzero(on)
    out = np.empty(zq.shape[0])
    for i in range(zq.shape[0]):
        t = lwl - 0.5 * ((ql[i] - zl)**2).sum(axis=1)
        if exclude_self:
            t = t[idx != i]
        if t.size == 0:
            out[i] = -np.inf
            continue
        top = t.max()
        out[i] = float(top + np.log(np.exp(t - top).sum()))
    r2 = (zq**2).sum(axis=1) + ((z[on]**2).sum(axis=1).max() if on.any() else 0.)
    return out, EPS * (64. * (1. + r2) + n)


def logsum(z, logw, zq, exclude_self=False, pad=0, fill=np.nan):
    """The device's result; with ``pad`` the rows live in wider matrices whose extra columns hold ``fill``."""
    from bayesfast_amd.utils.kde import kde_logsum

    def wide(a):
        if not pad:
            return _dev(a)
        w = np.full((a.shape[0], a.shape[1] + pad), fill)
        w[:, :a.shape[1]] = a
        return _dev(w)[:, :a.shape[1]]
    zd = wide(z)
    qd = zd if exclude_self else wide(zq)
    return _np(kde_logsum(zd, None if logw is None else _dev(logw), qd, exclude_self))


def check(got, ref, bound, what):
    fin = np.isfinite(ref)
    ratio = float(np.max(np.abs(got[fin] - ref[fin]) / bound[fin])) if fin.any() else 0.
    print(what, 'largest |dev - ref| / bound', ratio)
    assert np.array_equal(got[~fin], ref[~fin]), what
    assert ratio <= 1., what


def case(n, m, d, seed=0, weights=True):
    rng = np.random.default_rng([seed, n, m, d])
    z = rng.standard_normal((n, d))
    zq = rng.standard_normal((m, d)) * 1.3
    logw = np.log(rng.uniform(size=n)) if weights else None
    return z, logw, zq


@pytest.mark.parametrize('d', [1, 3, 4, 5, 27, 45, 64, 90, 128])
def test_logsum_shapes(d):
    for n, m in [(n, 33) for n in (1, 15, 16, 17, 1000)] + [(1000, m) for m in (1, 15, 16, 17)]:
        z, logw, zq = case(n, m, d)
        ref, bound = reference(z, logw, zq)
        check(logsum(z, logw, zq), ref, bound, 'd %d n %d m %d' % (d, n, m))
    z, logw, zq = case(17, 5, d, weights=False)
    ref, bound = reference(z, None, zq)
    check(logsum(z, None, zq), ref, bound, 'd %d no weights' % d)


@pytest.mark.parametrize('n', [767, 768, 769])
def test_logsum_parts_and_strides(n):
    assert [plan(k)[0] for k in (767, 768, 769)] == [3, 3, 4]
    for d, pad in ((5, 0), (5, 3), (27, 1)):
        z, logw, zq = case(n, 17, d, seed=1)
        ref, bound = reference(z, logw, zq)
        check(logsum(z, logw, zq, pad=pad), ref, bound, 'n %d d %d pad %d' % (n, d, pad))


def test_logsum_query_chunks():
    """m = 8193: the second launch of queries holds one row; its result is that row's alone."""
    z, logw, zq = case(40, 8193, 3, seed=2)
    got = logsum(z, logw, zq)
    pick = np.r_[0:20, 8170:8193]
    ref, bound = reference(z, logw, zq[pick])
    check(got[pick], ref, bound, 'm 8193')
    assert np.array_equal(got[-1:], logsum(z, logw, zq[-1:]))


def test_refusals():
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    L = ctx._lib
    z = _dev(np.zeros((4, 129)))
    out, work = ctx.empty((4,)), ctx.empty((4096,), dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.bfhip_kde_work_bytes(4, 4, 129) == 0
    rc = L.bfhip_kde_logsum(ctx.handle, 129, 4, p(z), 129, None, 4, p(z), 129, 0, p(out), p(work), work.numel())
    assert rc == -4 and b'BFHIP_MAX_DIM' in L.bfhip_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    rc = L.bfhip_kde_logsum(ctx.handle, 3, 4, p(z), 2, None, 4, p(z), 3, 0, p(out), p(work), work.numel())
    assert rc == -1
    rc = L.bfhip_kde_logsum(ctx.handle, 3, 4, p(z), 3, None, 3, p(z), 3, 1, p(out), p(work), work.numel())
    assert rc == -1 and b'exclude_self' in L.bfhip_last_error()
    rc = L.bfhip_kde_logsum(ctx.handle, 3, 4, p(z), 3, None, 4, p(z), 3, 0, p(out), p(work), 8)
    assert rc == -1
    assert L.bfhip_kde_logsum(ctx.handle, 3, 2**31, p(z), 3, None, 4, p(z), 3, 0, p(out), p(work), work.numel()) == -4
    # the context works afterwards
    z, logw, zq = case(20, 3, 128, seed=3)
    ref, bound = reference(z, logw, zq)
    check(logsum(z, logw, zq), ref, bound, 'after the refusals')


def test_weights():
    n, m, d = 300, 17, 4
    z, logw, zq = case(n, m, d, seed=4)
    # a third of the weights zero, those rows NaN: they do not matter
    off = np.arange(n) % 3 == 1
    lw = np.where(off, -np.inf, logw)
    zn = np.where(off[:, None], np.nan, z)
    ref, bound = reference(z, lw, zq)
    got = logsum(zn, lw, zq)
    check(got, ref, bound, 'a third of the weights zero')
    assert np.array_equal(got, logsum(np.where(off[:, None], 0., z), lw, zq))
    # one weight equal to 1: the result is that row's energy
    lw = np.full(n, -np.inf)
    lw[137] = 0.
    ref, bound = reference(z, lw, zq)
    check(logsum(zn, lw, zq), ref, bound, 'one weight 1')
    # no weight at all
    assert np.array_equal(logsum(z, np.full(n, -np.inf), zq), np.full(m, -np.inf))


def test_far_queries_and_duplicates():
    n, d = 500, 4
    z, logw, _ = case(n, 1, d, seed=5)
    zq = np.vstack([np.full((1, d), 130.), np.full((1, d), -90.), np.array([[300., 0., 0., 0.]])])
    ref, bound = reference(z, logw, zq)
    got = logsum(z, logw, zq)
    assert np.all(np.isfinite(got)) and np.all(np.exp(got) == 0.) and np.all(got < -1e4)
    check(got, ref, bound, 'far queries')
    zd = np.repeat(z[:50], 7, axis=0)
    lwd = np.repeat(logw[:50], 7)
    zq = np.vstack([z[:20], z[100:110]])
    ref, bound = reference(zd, lwd, zq)
    check(logsum(zd, lwd, zq), ref, bound, 'duplicated rows')


def test_exclude_self():
    n, d = 777, 5
    z, logw, _ = case(n, 1, d, seed=6)
    logw[::5] = -np.inf
    got1 = logsum(z, logw, z, exclude_self=True, pad=2)
    ref1, bound = reference(z, logw, z, exclude_self=True)
    check(got1, ref1, bound, 'exclude_self')
    got0 = logsum(z, logw, z, pad=2)
    ref0, bound = reference(z, logw, z)
    check(got0, ref0, bound, 'self included')
    # the two differ exactly at the rows that carry weight, by that row's own term
    on = logw > -np.inf
    assert np.array_equal(got0[~on], got1[~on])
    assert np.all(got0[on] > got1[on])
    assert np.all(np.abs(got0[on] - np.logaddexp(got1[on], logw[on])) <= 2. * bound[on])


def test_bitwise():
    n, d = 1500, 27
    z, logw, zq = case(n, 600, d, seed=7)
    a = logsum(z, logw, zq)
    assert np.array_equal(a, logsum(z, logw, zq))
    assert np.array_equal(a[41:42], logsum(z, logw, zq[41:42]))
    assert np.array_equal(a[41:58], logsum(z, logw, zq[41:58]))
    assert np.array_equal(a[41:42], logsum(z, logw, np.vstack([zq[300:567], zq[41:42], zq[:100]]))[267:268])
    e = logsum(z, logw, z, exclude_self=True)
    assert np.array_equal(e, logsum(z, logw, z, exclude_self=True))


def test_nan_rules():
    n, m, d = 700, 40, 6
    z, logw, zq = case(n, m, d, seed=8)
    clean = logsum(z, logw, zq)
    q = zq.copy()
    q[13, 4] = np.nan
    got = logsum(z, logw, q)
    assert np.isnan(got[13]) and np.array_equal(np.delete(got, 13), np.delete(clean, 13))
    for v in (np.nan, np.inf):
        zb = z.copy()
        zb[400, 2] = v
        assert np.all(np.isnan(logsum(zb, logw, zq))), v
        lb = logw.copy()
        lb[699] = v
        assert np.all(np.isnan(logsum(z, lb, zq))), v
    lb = logw.copy()
    lb[400] = -np.inf
    zb = z.copy()
    zb[400] = np.nan
    z0 = z.copy()
    z0[400] = 0.
    assert np.array_equal(logsum(zb, lb, zq), logsum(z0, lb, zq))


# ---- the class on device tensors ---------------------------------------------------------------------------------------------------
def _est_bound(est_host, points):
    zq = (np.atleast_2d(points) - est_host._mean) @ est_host._white
    return EPS * (64. * (1. + (zq**2).sum(axis=1) + (est_host._z**2).sum(axis=1).max()) + est_host.n)


def test_kde_class():
    import torch
    from bayesfast_amd.utils import kde
    rng = np.random.default_rng(9)
    x = rng.standard_normal((900, 3)) * np.array([1., 2., 0.5]) + np.array([10., -3., 0.])
    w = rng.uniform(size=900)
    q = rng.standard_normal((33, 3)) * np.array([1., 2., 0.5]) * 1.5 + np.array([10., -3., 0.])
    for kw in (dict(), dict(bw_method='silverman', bw_factor=0.8, weights=w), dict(bw_method=0.3, log_weights=np.log(w))):
        host = kde(x, **kw)
        dev = kde(_dev(x), **{k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        assert dev.n == 900 and dev.d == 3 and dev.covariance.is_cuda and dev.inv_cov.is_cuda and dev.weights.is_cuda
        assert abs(dev.factor - host.factor) <= 1e-14 * host.factor and abs(dev.neff - host.neff) <= 1e-12 * host.neff
        assert np.allclose(_np(dev.covariance), host.covariance, rtol=1e-12, atol=0)
        bound = _est_bound(host, q)
        for pts in (q, _dev(q)):
            lp = dev.logpdf(pts)
            assert lp.is_cuda
            check(_np(lp), host.logpdf(q), bound, 'logpdf %s' % sorted(kw))
        assert np.allclose(_np(dev.pdf(q)), host.pdf(q), rtol=1e-11, atol=0)
        assert np.array_equal(_np(dev(q[0])), _np(dev.pdf(q[:1])))
        check(_np(dev.logpdf_loo()), host.logpdf_loo(), _est_bound(host, x), 'logpdf_loo %s' % sorted(kw))
        r = dev.resample(50, seed=3)
        assert r.is_cuda and r.shape == (50, 3) and torch.equal(r, dev.resample(50, seed=3))
        with pytest.raises(NotImplementedError):
            dev.cdf(q)
        with pytest.raises(ValueError):
            dev.logpdf(np.zeros((2, 4)))
    x1 = rng.standard_normal(400)
    host, dev = kde(x1, 'scott', weights=w[:400]), kde(_dev(x1), 'scott', weights=_dev(w[:400]))
    g = np.linspace(-4., 4., 37)
    c = dev.cdf(g)
    assert c.is_cuda and np.allclose(_np(c), host.cdf(g), rtol=1e-12, atol=1e-15)
    check(_np(dev.logpdf(g)), host.logpdf(g), _est_bound(host, g[:, None]), 'logpdf 1-d')
    with pytest.raises(NotImplementedError):
        kde(torch.zeros((10, 129), dtype=torch.float64, device='cuda'))


@pytest.fixture(scope='module')
def short_runs():
    import bayesfast_amd as bfa
    d = 4
    out = []
    for shift, seed in ((0., 7), (1.5, 8)):
        rng = np.random.default_rng(seed)
        su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
        den = bfa.SurrogateDensity(su, input_scales=np.stack([np.full(d, -8.), np.full(d, 9.)], 1))
        xf = rng.standard_normal((4 * su.n_param, d)) * 1.5
        den.fit(xf, -0.5 * ((xf - shift)**2).sum(axis=1))
        out.append(bfa.sample(den, bfa.NTrace(n_chain=64, n_iter=70, n_warmup=20, x_0=rng.standard_normal((64, d)) + shift,
                                              random_generator=seed), verbose=False))
    return out


def test_trace_kde(short_runs):
    from bayesfast_amd.utils import kde
    tt = short_runs[0]
    assert tt.device('samples').is_cuda
    x = tt.get(flatten=True)
    assert x.shape == (64 * 50, 4)
    q = x[::97] * 1.1
    for kw, sel in ((dict(), slice(None)), (dict(bw_method='silverman', params=[2, 0]), [2, 0])):
        dev = tt.kde(**kw)
        host = kde(x[:, sel], bw_method=kw.get('bw_method'))
        assert dev.dataset.is_cuda and dev.n == 3200
        check(_np(dev.logpdf(q[:, sel])), host.logpdf(q[:, sel]), _est_bound(host, q[:, sel]), 'TraceTuple.kde %s' % sorted(kw))
    lw = -0.1 * (x**2).sum(axis=1)
    check(_np(tt.kde(log_weights=lw.reshape(64, 50)).logpdf(q)), kde(x, log_weights=lw).logpdf(q), _est_bound(kde(x, log_weights=lw), q),
          'TraceTuple.kde weights')


def _shift_close(dev, host, delta_host):
    """logpdf and logpdf_zero within the bound; prob equal but for the samples whose log density lies within it of logpdf_zero."""
    from bayesfast_amd.utils import kde
    est = kde(delta_host, bw_method='silverman')
    bound = _est_bound(est, delta_host)
    b0 = float(_est_bound(est, np.zeros((1, delta_host.shape[1])))[0])
    assert dev.logpdf.is_cuda
    check(_np(dev.logpdf), host.logpdf, bound, 'shift logpdf')
    print('logpdf_zero', dev.logpdf_zero, host.logpdf_zero, b0)
    assert abs(dev.logpdf_zero - host.logpdf_zero) <= b0
    count = int(np.count_nonzero(np.abs(host.logpdf - host.logpdf_zero) <= bound + b0))
    print('prob', dev.prob, host.prob, 'samples within the bound of logpdf_zero', count)
    assert abs(dev.prob - host.prob) <= count / host.n_pairs + 1e-15
    assert dev.saturated == host.saturated and dev.n_pairs == host.n_pairs and abs(dev.factor - host.factor) <= 1e-14
    for k in ('gaussian_chi2', 'gaussian_prob'):
        assert abs(getattr(dev, k) - getattr(host, k)) <= 1e-10 * max(1., abs(getattr(host, k)))


def test_parameter_shift_device():
    from bayesfast_amd.utils import parameter_shift
    rng = np.random.default_rng(10)
    a = rng.standard_normal((3000, 3))
    b = rng.standard_normal((2500, 3)) * 0.7 + np.array([2., 0., 0.])
    lwa, lwb = -0.2 * (a**2).sum(axis=1), None
    for kw in (dict(), dict(loo=False), dict(log_weights_a=lwa, params=[0, 2])):
        host = parameter_shift(a, b, n_pairs=2000, seed=5, **kw)
        dev = parameter_shift(_dev(a), _dev(b), n_pairs=2000, seed=5, **kw)
        r2 = np.random.default_rng(5)
        wa = None
        if 'log_weights_a' in kw:
            wa = np.exp(lwa - lwa.max())
            wa /= wa.sum()
        ia, ib = r2.choice(3000, size=2000, p=wa), r2.choice(2500, size=2000)
        sel = kw.get('params', [0, 1, 2])
        _shift_close(dev, host, a[ia][:, sel] - b[ib][:, sel])


def test_trace_parameter_shift(short_runs):
    from bayesfast_amd.utils import parameter_shift
    ta, tb = short_runs
    xa, xb = ta.get(flatten=True), tb.get(flatten=True)
    host = parameter_shift(xa, xb, n_pairs=1500, seed=2, params=[0, 1])
    for other in (tb, tb.device('samples_original')[:, tb.n_warmup:]):
        dev = ta.parameter_shift(other, n_pairs=1500, seed=2, params=[0, 1])
        r2 = np.random.default_rng(2)
        ia, ib = r2.choice(xa.shape[0], size=1500), r2.choice(xb.shape[0], size=1500)
        _shift_close(dev, host, xa[ia][:, :2] - xb[ib][:, :2])
    assert 0. < host.prob < 1. and host.gaussian_n_sigma > 0.5
