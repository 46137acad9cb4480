"""The kernel-weighted means on the device (csrc/bfhip_kde.h: ``bfhip_kde_wmean``) through ctypes and ``utils.kde.kde_wmean``, the
``kde`` methods built on it, ``utils.modes`` and ``TraceTuple.modes`` on device tensors, against the host port and a direct difference
form in numpy.longdouble.  Expected values are never the device's.

Tolerance, derived and not tuned.  With b_i = eps (64 (1 + R2_i) + n), R2_i = |zq_i|^2 + max_j |z_j|^2 over the rows that carry weight
(the logsum bound of ``tests/test_gpu_kde.py``), every normalised weight p_ij carries b_i of relative error in its numerator and in
its denominator, so
    |mean_dev - mean_ref|[i, c] <= 2 b_i max_j |v_jc|,     |logsum_dev - logsum_ref| <= b_i,
the maximum over the rows that carry weight.  Every comparison prints the largest ratio to these bounds before it asserts.

Shapes: d in {1, 3, 4, 5, 27, 45, 64, 90, 128} (every k-step class of the tile kernel) times k in {1, 15, 16, 17, 33, 128} (every
class of column blocks, a block is 16 columns) and v = z, at (n, m) = (1000, 33); then at d = 5 and 27 n in {1, 15, 16, 17, 1000} and
767 | 768 | 769 (3, 3 and 4 parts) and m in {1, 15, 16, 17, 33}; m = 8193, one more than the largest chunk of queries, and m = 193
at n = 65536, k = 128, where 256 parts of 130 doubles shrink the chunk to 192."""
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


def chunk(n, k):
    """kd_wm_chunk of csrc/bfhip_kde.h: the queries of one launch."""
    p = min((n + 255) // 256, 256)
    r = (-(-n // p) + 15) // 16 * 16
    p = -(-n // r)
    return min(8192, max(64, (1 << 26) // (8 * p * (k + 2)) // 64 * 64))


def reference(z, logw, zq, v, exclude_self=False, rows=None):
    """(logsum, mean, b, vmax) by differences in longdouble over the rows that carry weight; ``rows``: the data row of every
    query, for exclude_self on a subset of the queries."""
    n = z.shape[0]
    lw = np.zeros(n) if logw is None else logw
    on = lw > -np.inf
    idx = np.flatnonzero(on)
    zl, ql, lwl, vl = z[on].astype(LD), zq.astype(LD), lw[on].astype(LD), v[on].astype(LD)
    ls, mean = np.empty(zq.shape[0]), np.empty((zq.shape[0], v.shape[1]))
    for i in range(zq.shape[0]):
        t = lwl - 0.5 * ((ql[i] - zl)**2).sum(axis=1)
        keep = idx != (i if rows is None else rows[i]) if exclude_self else np.ones(idx.size, dtype=bool)
        if not keep.any():
            ls[i], mean[i] = -np.inf, np.nan
            continue
        top = t[keep].max()
        p = np.exp(t[keep] - top)
        ls[i] = float(top + np.log(p.sum()))
        mean[i] = (p[:, None] * vl[keep]).sum(axis=0) / p.sum()
    r2 = (zq**2).sum(axis=1) + ((z[on]**2).sum(axis=1).max() if on.any() else 0.)
    vmax = np.abs(v[on]).max(axis=0) if on.any() else np.zeros(v.shape[1])
    return ls, mean, EPS * (64. * (1. + r2) + n), vmax


def wmean(z, logw, zq, v=None, exclude_self=False, pad=0, fill=np.nan):
    """The device's (logsum, mean); ``v=None``: v is z itself.  With ``pad`` the rows live in wider matrices whose extra columns
    hold ``fill``."""
    from bayesfast_amd.utils.kde import kde_wmean

    def wide(a):
        if not pad:
            return _dev(a)
        w = np.full((a.shape[0], a.shape[1] + pad), fill)
        w[:, :a.shape[1]] = a
        return _dev(w)[:, :a.shape[1]]
    zd = wide(z)
    qd = zd if exclude_self else wide(zq)
    ls, mean = kde_wmean(zd, None if logw is None else _dev(logw), qd, zd if v is None else wide(v), exclude_self)
    return _np(ls), _np(mean)


def check(got, ref, what):
    (gl, gm), (ls, mean, b, vmax) = got, ref
    fin = np.isfinite(ls)
    r1 = float(np.max(np.abs(gl[fin] - ls[fin]) / b[fin])) if fin.any() else 0.
    r2 = float(np.max(np.abs(gm[fin] - mean[fin]) / (2. * b[fin, None] * np.maximum(vmax, 1e-300)[None, :]))) if fin.any() else 0.
    print(what, 'largest |dev - ref| / bound: logsum', r1, 'mean', r2)
    assert gm.shape == mean.shape and np.array_equal(gl[~fin], ls[~fin]) and np.all(np.isnan(gm[~fin])), what
    assert r1 <= 1. and r2 <= 1., what


def case(n, m, d, k=0, seed=0, weights=True):
    rng = np.random.default_rng([seed, n, m, d, k])
    z = rng.standard_normal((n, d))
    zq = rng.standard_normal((m, d)) * 1.3
    logw = np.log(rng.uniform(size=n)) if weights else None
    v = rng.standard_normal((n, k)) * 3. + 1. if k else None
    return z, logw, zq, v


@pytest.mark.parametrize('d', [1, 3, 4, 5, 27, 45, 64, 90, 128])
def test_wmean_d_and_k(d):
    n, m = 1000, 33
    z, logw, zq, _ = case(n, m, d)
    check(wmean(z, logw, zq), reference(z, logw, zq, z), 'd %d v = z' % d)
    check(wmean(z, logw, zq, pad=3), reference(z, logw, zq, z), 'd %d v = z padded' % d)
    for k in (1, 15, 16, 17, 33, 128):
        z, logw, zq, v = case(n, m, d, k)
        check(wmean(z, logw, zq, v, pad=k % 3), reference(z, logw, zq, v), 'd %d k %d' % (d, k))
    z, _, zq, v = case(17, 5, d, 2, weights=False)
    check(wmean(z, None, zq, v), reference(z, None, zq, v), 'd %d no weights' % d)


@pytest.mark.parametrize('d', [5, 27])
def test_wmean_n_and_m(d):
    for n, m in [(n, 33) for n in (1, 15, 16, 17, 767, 768, 769)] + [(1000, m) for m in (1, 15, 16, 17)]:
        z, logw, zq, v = case(n, m, d, 17, seed=1)
        check(wmean(z, logw, zq), reference(z, logw, zq, z), 'd %d n %d m %d v = z' % (d, n, m))
        check(wmean(z, logw, zq, v, pad=2), reference(z, logw, zq, v), 'd %d n %d m %d k 17' % (d, n, m))


def test_wmean_query_chunks():
    """One more query than a launch takes: the last launch holds one row, and its result is that row's alone.  The chunk is 8192
    where the partials are small, and 192 at n = 65536, k = 128."""
    assert chunk(40, 2) == 8192 and chunk(65536, 128) == 192 and chunk(65536, 27) == 1088
    z, logw, zq, v = case(40, 8193, 3, 2, seed=2)
    got = wmean(z, logw, zq, v)
    pick = np.r_[0:20, 8170:8193]
    check((got[0][pick], got[1][pick]), reference(z, logw, zq[pick], v), 'm 8193')
    alone = wmean(z, logw, zq[-1:], v)
    assert np.array_equal(got[0][-1:], alone[0]) and np.array_equal(got[1][-1:], alone[1])
    z, logw, zq, v = case(65536, 193, 3, 128, seed=3)
    got = wmean(z, logw, zq, v)
    pick = np.r_[0:2, 191:193]
    check((got[0][pick], got[1][pick]), reference(z, logw, zq[pick], v), 'n 65536 k 128 m 193')
    alone = wmean(z, logw, zq[191:], v)
    assert np.array_equal(got[0][191:], alone[0]) and np.array_equal(got[1][191:], alone[1])


def test_running_maximum():
    n, d = 700, 4
    z, logw, zq, v = case(n, 20, d, 3, seed=4)
    # the data sorted by their distance to the first query: its best match comes last (the maximum rises throughout), and first
    order = np.argsort(((z - zq[0])**2).sum(axis=1))
    for name, o in (('best last', order[::-1]), ('best first', order)):
        check(wmean(z[o], logw[o], zq, v[o]), reference(z[o], logw[o], zq, v[o]), name)
        check(wmean(z[o], None, zq), reference(z[o], None, zq, z[o]), name + ', v = z, no weights')
    # queries at |zq| = 40 (a density of 1e-290) and 300, where pdf underflows: the mean is still the nearest rows' and finite
    far = np.vstack([np.array([[40., 0., 0., 0.]]), np.full((1, d), -20.), np.array([[0., 0., 300., 0.]])])
    got = wmean(z, logw, far, v)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and np.all(got[0] < -500.) and np.exp(got[0][2]) == 0.
    check(got, reference(z, logw, far, v), 'far queries')
    got = wmean(z, logw, far)
    assert got[1][0, 0] > 2. and np.all(got[1][1] < 0.) and got[1][2, 2] > 2.
    check(got, reference(z, logw, far, z), 'far queries, v = z')
    # duplicated rows
    zd, lwd, vd = np.repeat(z[:50], 7, axis=0), np.repeat(logw[:50], 7), np.repeat(v[:50], 7, axis=0)
    q = np.vstack([z[:20], z[100:110]])
    check(wmean(zd, lwd, q, vd), reference(zd, lwd, q, vd), 'duplicated rows')


def test_exclude_self():
    from bayesfast_amd.utils.kde import kde_logsum
    n, d = 777, 5
    z, logw, _, v = case(n, 1, d, 17, seed=6)
    logw[::5] = -np.inf
    for vv, name in ((v, 'k 17'), (None, 'v = z')):
        got = wmean(z, logw, z, vv, exclude_self=True, pad=2)
        ref = reference(z, logw, z, z if vv is None else vv, exclude_self=True)
        check(got, ref, 'exclude_self ' + name)
        check(wmean(z, logw, z, vv, pad=2), reference(z, logw, z, z if vv is None else vv), 'self included ' + name)
        # the logsum beside the means is bfhip_kde_logsum's, within the bound
        zd = _dev(z)
        ls = _np(kde_logsum(zd, _dev(logw), zd, exclude_self=True))
        assert np.all(np.abs(got[0] - ls) <= ref[2])
    # a single weighted row: no term is left
    lw = np.full(n, -np.inf)
    lw[137] = 0.
    ls, mean = wmean(z, lw, z, v, exclude_self=True)
    assert ls[137] == -np.inf and np.all(np.isnan(mean[137]))
    keep = np.arange(n) != 137
    assert np.all(np.isfinite(ls[keep])) and np.allclose(mean[keep], v[137][None, :], rtol=0, atol=1e-14 * np.abs(v[137]).max())


def test_bitwise():
    n, d = 1500, 27
    z, logw, zq, v = case(n, 600, d, 33, seed=7)
    for vv in (None, v):
        a = wmean(z, logw, zq, vv)
        same = lambda x, y: np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        cut = lambda x, s: (x[0][s], x[1][s])
        assert same(a, wmean(z, logw, zq, vv))
        assert same(cut(a, slice(41, 42)), wmean(z, logw, zq[41:42], vv))
        assert same(cut(a, slice(41, 58)), wmean(z, logw, zq[41:58], vv))
        assert same(cut(a, slice(41, 42)), cut(wmean(z, logw, np.vstack([zq[300:567], zq[41:42], zq[:100]]), vv), slice(267, 268)))
        e = wmean(z, logw, z, vv, exclude_self=True)
        assert same(e, wmean(z, logw, z, vv, exclude_self=True))


def test_refusals():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.utils.kde import kde_wmean
    ctx = _ctx()
    L = ctx._lib
    z = _dev(np.zeros((4, 129)))
    ls, mean, work = ctx.empty((4,)), ctx.empty((4, 129)), ctx.empty((1 << 16,), dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(d=3, n=4, ldz=3, k=3, v=z, ldv=3, m=4, zq=z, ldq=3, ex=0, ldo=3, wb=None, mean_=mean):
        return L.bfhip_kde_wmean(ctx.handle, d, n, p(z), ldz, None, k, p(v) if v is not None else None, ldv, m, p(zq), ldq, ex, p(ls),
                                 p(mean_) if mean_ is not None else None, ldo, p(work), work.numel() if wb is None else wb)
    assert L.bfhip_kde_wmean_work_bytes(4, 4, 129, 3) == 0 and L.bfhip_kde_wmean_work_bytes(4, 4, 3, 129) == 0
    assert L.bfhip_kde_wmean_work_bytes(4, 4, 3, 0) == 0 and L.bfhip_kde_wmean_work_bytes(4, 4, 3, 3) > 0
    rc = call(d=129, ldz=129, ldq=129)
    assert rc == -4 and b'd = 129' in L.bfhip_last_error() and b'BFHIP_MAX_DIM' in L.bfhip_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    rc = call(k=129, ldv=129, ldo=129)
    assert rc == -4 and b'k = 129' in L.bfhip_last_error()
    assert call(n=2**31) == -4 and b'2147483648' in L.bfhip_last_error()
    assert call(k=0) == -1 and call(d=0) == -1 and call(m=0) == -1 and call(v=None) == -1 and call(mean_=None) == -1
    assert call(ldz=2) == -1 and b'ldz = 2' in L.bfhip_last_error()
    assert call(ldq=2) == -1
    assert call(ldv=2) == -1 and b'ldv = 2' in L.bfhip_last_error()
    assert call(ldo=2) == -1 and b'ldo = 2' in L.bfhip_last_error()
    assert call(m=3, ex=1) == -1 and b'exclude_self' in L.bfhip_last_error()
    assert call(wb=8) == -1 and b'8 bytes' in L.bfhip_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(wb=8))
    assert call() == 0
    zz = _dev(np.zeros((5, 3)))
    with pytest.raises(ValueError):
        kde_wmean(zz, None, zz, zz[:4])
    with pytest.raises(ValueError):
        kde_wmean(zz, None, zz[:4], zz, exclude_self=True)
    with pytest.raises(ValueError):
        kde_wmean(zz, None, zz, zz.to(torch.float32))
    # the context works afterwards
    z, logw, zq, v = case(20, 3, 128, 5, seed=3)
    check(wmean(z, logw, zq, v), reference(z, logw, zq, v), 'after the refusals')


def test_value_rules():
    n, m, d, k = 700, 40, 6, 4
    z, logw, zq, v = case(n, m, d, k, seed=8)
    clean = wmean(z, logw, zq, v)
    # a row of weight -inf is no part of the sample, whatever z and v hold there
    off = np.arange(n) % 3 == 1
    lw = np.where(off, -np.inf, logw)
    for bad in (np.nan, np.inf):
        got = wmean(np.where(off[:, None], bad, z), lw, zq, np.where(off[:, None], bad, v))
        check(got, reference(z, lw, zq, v), 'a third of the weights zero')
        zero = wmean(np.where(off[:, None], 0., z), lw, zq, np.where(off[:, None], 0., v))
        assert np.array_equal(got[0], zero[0]) and np.array_equal(got[1], zero[1])
        got = wmean(np.where(off[:, None], bad, z), lw, zq)
        check(got, reference(z, lw, zq, z), 'a third of the weights zero, v = z')
    # a NaN in a query: that query alone
    q = zq.copy()
    q[13, 4] = np.nan
    got = wmean(z, logw, q, v)
    assert np.isnan(got[0][13]) and np.all(np.isnan(got[1][13]))
    assert np.array_equal(np.delete(got[0], 13), np.delete(clean[0], 13)) and np.array_equal(np.delete(got[1], 13, 0), np.delete(clean[1], 13, 0))
    far = np.vstack([zq, np.full((1, d), 60.)])
    for bad in (np.nan, np.inf):
        # a bad weight or a bad z row of non-zero weight: every output
        zb = z.copy()
        zb[400, 2] = bad
        lb = logw.copy()
        lb[699] = bad
        for got in (wmean(zb, logw, zq, v), wmean(zb, logw, zq), wmean(z, lb, zq, v)):
            assert np.all(np.isnan(got[0])) and np.all(np.isnan(got[1])), bad
        # a bad value: its column for every query, the far one included, and nothing else
        for bv in (bad, -bad):
            vb = v.copy()
            vb[400, 2] = bv
            got = wmean(z, logw, far, vb)
            assert np.all(np.isnan(got[1][:, 2])) and np.array_equal(got[0][:m], clean[0])
            assert np.array_equal(np.delete(got[1][:m], 2, axis=1), np.delete(clean[1], 2, axis=1))
    # no weight at all
    got = wmean(z, np.full(n, -np.inf), zq, v)
    assert np.array_equal(got[0], np.full(m, -np.inf)) and np.all(np.isnan(got[1]))


# ---- the class on device tensors ---------------------------------------------------------------------------------------------------
def _est_bound(est_host, zq):
    return EPS * (64. * (1. + (zq**2).sum(axis=1) + (est_host._z**2).sum(axis=1).max()) + est_host.n)


def test_kde_methods():
    from bayesfast_amd.utils import kde
    rng = np.random.default_rng(9)
    scale, centre = np.array([1., 2., 0.5]), np.array([10., -3., 0.])
    x = rng.standard_normal((900, 3)) * scale + centre
    w = rng.uniform(size=900)
    w[::11] = 0.
    q = rng.standard_normal((33, 3)) * scale * 1.5 + centre
    vals = np.stack([np.sin(x[:, 0]), x[:, 1]**2], axis=1)
    for kw in (dict(), dict(bw_method='silverman', bw_factor=0.8, weights=w)):
        host = kde(x, **kw)
        dev = kde(_dev(x), **{k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        zq = (q - host._mean) @ host._white
        b = _est_bound(host, zq)
        # the score: A (mean_z - zq), each whitened component within 2 b max |z|, and the whitening product's own rounding
        zmax = np.abs(host._z).max()
        tol = (2. * b * zmax + 64. * EPS * (np.abs(zq).max() + zmax))[:, None] * np.abs(host._white).sum(axis=1)[None, :]
        for pts in (q, _dev(q)):
            g = dev.grad_logpdf(pts)
            assert g.is_cuda and g.shape == (33, 3)
            ratio = np.abs(_np(g) - host.grad_logpdf(q)) / (2. * tol)      # both routes
            print('grad_logpdf', sorted(kw), 'largest ratio', ratio.max())
            assert ratio.max() <= 1.
        vmax = np.abs(vals[host.weights > 0]).max(axis=0)
        for args, zz in ((dict(x=q), zq), (dict(), host._z), (dict(loo=True), host._z)):
            r, want = dev.regress(_dev(vals), **args), host.regress(vals, **args)
            assert r.is_cuda and r.shape == want.shape
            ratio = np.abs(_np(r) - want) / (4. * _est_bound(host, zz)[:, None] * vmax[None, :])    # both routes within 2 b of the exact value
            print('regress', sorted(kw), sorted(args), 'largest ratio', np.nanmax(ratio))
            assert np.array_equal(np.isnan(_np(r)), np.isnan(want)) and np.nanmax(ratio) <= 1.
        r1 = dev.regress(vals[:, 1], x=q)
        assert r1.shape == (33,) and np.array_equal(_np(r1), _np(dev.regress(_dev(vals), x=q))[:, 1])
        with pytest.raises(ValueError):
            dev.regress(vals, x=q, loo=True)
        # mean shift: the two routes end at the same points, within 1e-6 in whitened units, where the host's score vanishes
        x0 = x[5:45][w[5:45] > 0]
        xd, lpd, nd, cd = dev.mean_shift(_dev(x0))
        xh, lph, nh, ch = host.mean_shift(x0)
        assert xd.is_cuda and lpd.is_cuda and cd.is_cuda and bool(cd.all()) and ch.all()
        dist = np.sqrt(((((_np(xd) - xh)) @ host._white)**2).sum(axis=1))
        print('mean_shift', sorted(kw), 'iterations', nd, nh, 'largest distance in whitened units', dist.max())
        assert dist.max() <= 1e-6 and abs(nd - nh) <= 8
        assert np.all(np.abs(_np(lpd) - host.logpdf(_np(xd))) <= 2. * _est_bound(host, (_np(xd) - host._mean) @ host._white))
        assert np.all(np.sqrt((host.grad_logpdf(_np(xd))**2).sum(axis=1)) < 1e-6)


def mixture(seed, sep, n=4000, d=3):
    rng = np.random.default_rng(seed)
    lab = rng.uniform(size=n) < 0.3
    x = rng.standard_normal((n, d))
    x[lab, 0] += sep
    return x, lab


def test_modes_device():
    from bayesfast_amd.utils import modes
    x, lab = mixture(0, 6.)
    host = modes(x, bw_factor=2., n_seeds=256, seed=0)
    dev = modes(_dev(x), bw_factor=2., n_seeds=256, seed=0)
    print(host, dev)
    assert host.n_modes == 2 and dev.n_modes == host.n_modes and dev.n_minor == host.n_minor == 0
    assert np.array_equal(dev.label, host.label) and np.array_equal(dev.seed_index, host.seed_index)
    assert np.array_equal(dev.share, host.share) and np.allclose(dev.x, host.x, rtol=0, atol=1e-5) and abs(dev.n_iter - host.n_iter) <= 8
    assert dev.n_not_converged == 0 and np.allclose(dev.logpdf, host.logpdf, rtol=0, atol=1e-9)


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


def test_trace_modes(short_runs):
    """One run of a unit Gaussian has one mode.  The two runs' draws together are two unit Gaussians 1.5 sd apart in each of four
    coordinates, 3 sd in all.  Checked on the host with independent normal draws of the same shape (2 x 3200 rows, three seeds,
    ``bw_factor=1.5``): two modes with shares 0.50 to 0.56 and no minor one, in 136 to 160 iterations; at Scott's own factor the
    same two and up to five one-seed modes.  So the test asks for two, and for the device route to label every seed as the host
    port does on the same draws."""
    from bayesfast_amd.utils import modes
    from bayesfast_amd.utils.modes import modes_from_seeds
    from bayesfast_amd.utils import kde
    ta, tb = short_runs
    assert ta.device('samples').is_cuda
    xa, xb = ta.get(flatten=True), tb.get(flatten=True)
    n_t = 50
    t = ((np.arange(4) + 0.5) * n_t / 4).astype(np.int64)
    rows = (np.arange(64)[:, None] * n_t + t[None, :]).reshape(-1)
    mo = ta.modes(bw_factor=1.5)
    host = modes_from_seeds(kde(xa, bw_factor=1.5), rows)
    print('one run', mo, host)
    assert mo.n_modes == 1 and host.n_modes == 1 and np.array_equal(mo.seed_index, rows) and np.array_equal(mo.label, host.label)
    assert mo.chain_mode.shape == (64,) and mo.chain_split.shape == (64,)
    assert np.array_equal(mo.chain_mode, np.zeros(64, dtype=np.int64)) or mo.n_minor > 0
    # with weights a chain's seeds are resampled within the chain; params selects
    lw = -0.1 * (xa**2).sum(axis=1)
    mw = ta.modes(log_weights=lw.reshape(64, 50), params=[0, 2], bw_factor=1.5, seed=3)
    assert mw.x.shape[1] == 2 and mw.n_modes == 1 and np.array_equal(mw.seed_index // n_t, np.repeat(np.arange(64), 4))
    # the two runs together, through utils.modes on a device tensor with one seed per 25 draws
    both = np.vstack([xa, xb])
    host = modes(both, bw_factor=1.5, n_seeds=256, seed=1)
    dev = modes(_dev(both), bw_factor=1.5, n_seeds=256, seed=1)
    print('two runs', dev, host, host.x)
    assert host.n_modes == 2 and abs(host.share[0] - 0.5) <= 4. * host.share_err[0]
    assert dev.n_modes == host.n_modes and dev.n_minor == host.n_minor and np.array_equal(dev.label, host.label)
    # a seed's mode is its run's, but for the draws between the two
    run = (host.seed_index >= xa.shape[0]).astype(np.int64)
    agree = np.mean(host.label == run)
    assert max(agree, 1. - agree) > 0.8
