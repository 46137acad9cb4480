"""GPU: the analytic and the Gauss-Newton Hessian of the pipeline density (bfhip_pipeline_logp_hess), its device-resident Newton
maximiser (bfhip_pipeline_laplace_opt) and the device route of ``Laplace.run`` for a ``Chi2PipelineDensity``.

Every expected value comes from the CPU oracle (helpers/laplace_cases.py: the fourth-order central difference of the oracle's
gradient with a tolerance measured on the oracle per point; a damped Newton iteration on the oracle) or from NumPy on the spec's own
coefficients -- never from the code under test."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import laplace_cases as lc  # noqa: E402
import pipeline_hess_cases as pc  # noqa: E402


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _np(t):
    return t.cpu().numpy()


def _fd(spec, x, original_space):
    H, tol = lc.hess_fd_with_tol(spec, x, original_space)
    if lc.jacobian_is_asymmetric(spec, original_space):
        H = 0.5 * (H + H.T)
    return H, tol


# ---- 1: the Hessian --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(pc.SHAPES))
def test_hessian_equals_differences_of_the_oracle_gradient(ctx, name):
    """Every shape, both spaces, points inside and outside the bound (the compressed shape with a decay term as well): |H - H_fd|
    within the tolerance measured on the oracle for that point plus 1e-12 d max|H|; H == H^T exactly; logp and grad of the same
    call are bfhip_logp_grad's (rtol 1e-10)."""
    from bayesfast_amd.device import DeviceDensity
    m, d, nq = pc.SHAPES[name]
    spec, pts = pc.hess_spec(m, d, nq, decay=name == 'compressed')
    dd = DeviceDensity(spec, ctx)
    for original_space in (True, False):
        x, rb = pc.points(spec, pts, original_space)
        f, g, H = (_np(t) for t in dd.pipeline_logp_grad_hess(x, original_space))
        f0, g0 = (_np(t) for t in dd.logp_and_grad(x, original_space))
        np.testing.assert_allclose(f, f0, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-10 * np.max(np.abs(g0)))
        for p in range(len(x)):
            Hfd, tol = _fd(spec, x[p], original_space)
            assert np.array_equal(H[p], H[p].T)
            err = float(np.max(np.abs(H[p] - Hfd)))
            print('%s original_space %d point %d (beta / alpha %.2f): |H - H_fd| %.3g, tolerance %.3g, max|H| %.3g'
                  % (name, original_space, p, rb[p], err, tol, np.max(np.abs(Hfd))))
            assert err <= tol


@pytest.mark.parametrize('m', [6, 40])
def test_hessian_with_cubic_configs(ctx, m):
    """Monomials of degree three (cubic-2: x_j^2 x_k and x_j^3; cubic-3: x_j x_k x_l) in every output, without (m = 6 < 27 monomials)
    and with (m = 40) output compression: the same assertions as above.  These monomials take paths of their own in the B tile's
    product rule and in the pair table of the upload (multiplicities 2 and 6, a coordinate as the remaining factor)."""
    from bayesfast_amd.device import DeviceDensity
    spec, pts = pc.cubic_spec(m)
    dd = DeviceDensity(spec, ctx)
    for original_space in (True, False):
        x, rb = pc.points(spec, pts, original_space)
        f, g, H = (_np(t) for t in dd.pipeline_logp_grad_hess(x, original_space))
        f0, g0 = (_np(t) for t in dd.logp_and_grad(x, original_space))
        np.testing.assert_allclose(f, f0, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-10 * np.max(np.abs(g0)))
        for p in range(len(x)):
            Hfd, tol = _fd(spec, x[p], original_space)
            assert np.array_equal(H[p], H[p].T)
            err = float(np.max(np.abs(H[p] - Hfd)))
            print('cubic m %d original_space %d point %d (beta / alpha %.2f): |H - H_fd| %.3g, tolerance %.3g' % (m, original_space, p, rb[p], err, tol))
            assert err <= tol


# ---- 2: Gauss-Newton -------------------------------------------------------------------------------------------------------------
def test_gauss_newton_equals_the_full_hessian_of_linear_outputs(ctx):
    """nq = 0: every output is linear, no transform, no input scales, so nothing carries a second derivative: inside the bound the
    two kinds agree to 1e-12 d max|H| and both equal the oracle difference."""
    from bayesfast_amd.device import DeviceDensity
    m, d = 40, 9
    spec, pts = pc.hess_spec(m, d, 0, transform=False)
    assert spec['ranges'] is None and spec['su_lo'] is None
    x = pts[:4]   # (the four ratios below 1: inside the bound, which the zero quadratic config keeps on)
    assert np.all(lc.bound_ratio(spec, x, True)[0] < 0.95)
    dd = DeviceDensity(spec, ctx)
    for original_space in (True, False):
        H = _np(dd.pipeline_logp_grad_hess(x, original_space)[2])
        Hg = _np(dd.pipeline_logp_grad_hess(x, original_space, gauss_newton=True)[2])
        for p in range(len(x)):
            hmax = float(np.max(np.abs(H[p])))
            assert np.max(np.abs(H[p] - Hg[p])) <= 1e-12 * d * hmax
            Hfd, tol = _fd(spec, x[p], original_space)
            assert np.max(np.abs(H[p] - Hfd)) <= tol and np.max(np.abs(Hg[p] - Hfd)) <= tol


@pytest.mark.parametrize('shape', [(40, 9, 4), (5, 9, 4), (100, 27, 9)])
def test_gauss_newton_drops_the_residual_curvature(ctx, shape):
    """nq > 0, no transform, inside the bound: H_full - H_gn = -sum_k r_k d2 f_k, formed in NumPy from the spec's quadratic
    coefficients and the unit precision (tolerance: 1e-12 d max|H|, the rounding of the two device matrices); and with the prior
    off the largest eigenvalue of H_gn is at most 1e-12 max|H| (negative semi-definite by construction)."""
    from bayesfast_amd.device import DeviceDensity
    m, d, nq = shape
    for prior in (True, False):
        spec, pts = pc.hess_spec(m, d, nq, transform=False, prior=prior)
        x, rb = pc.points(spec, pts, True)
        x = x[rb < 1.]
        dd = DeviceDensity(spec, ctx)
        H = _np(dd.pipeline_logp_grad_hess(x, True)[2])
        Hg = _np(dd.pipeline_logp_grad_hess(x, True, gauss_newton=True)[2])
        for p in range(len(x)):
            hmax = float(np.max(np.abs(H[p])))
            want = pc.residual_curvature(spec, x[p])
            err = float(np.max(np.abs((H[p] - Hg[p]) - want)))
            print('%r prior %d point %d: |(H - H_gn) + sum r d2f| %.3g, max|H| %.3g, max|sum r d2f| %.3g' % (shape, prior, p, err, hmax, np.max(np.abs(want))))
            assert err <= 1e-12 * d * hmax
            assert np.array_equal(Hg[p], Hg[p].T)
            if not prior:
                assert np.linalg.eigvalsh(Hg[p])[-1] <= 1e-12 * hmax


# ---- 3: batches ------------------------------------------------------------------------------------------------------------------
def test_hessian_batches(ctx):
    """n = 1, 17 and 300 points: a point's result does not depend on the batch it came in, bit for bit, nor on a single (d,) call.
    (300 points are one point per workgroup on a device of 150 CUs or more; test_results_do_not_depend_on_the_workgroup has the
    batches above the grid's cap.)"""
    from bayesfast_amd.device import DeviceDensity
    m, d, nq = 40, 9, 4
    spec, pts = pc.hess_spec(m, d, nq)
    rng = np.random.default_rng(12)
    x = rng.normal(size=(300, d)) * rng.choice([0.05, 0.6], size=(300, 1))
    rb, _ = lc.bound_ratio(spec, x, False)
    assert (rb > 1.).any() and (rb < 1.).any()
    dd = DeviceDensity(spec, ctx)
    for gn in (False, True):
        f, g, H = (_np(t) for t in dd.pipeline_logp_grad_hess(x, gauss_newton=gn))
        assert np.array_equal(H, np.swapaxes(H, 1, 2)) and np.all(np.isfinite(H))
        f17, g17, H17 = (_np(t) for t in dd.pipeline_logp_grad_hess(x[5:22], gauss_newton=gn))
        assert np.array_equal(H17, H[5:22]) and np.array_equal(g17, g[5:22]) and np.array_equal(f17, f[5:22])
        f1, g1, H1 = (_np(t) for t in dd.pipeline_logp_grad_hess(x[-1:], gauss_newton=gn))
        assert np.array_equal(H1, H[-1:]) and np.array_equal(f1, f[-1:]) and np.array_equal(g1, g[-1:])
        fs, gs, Hs = (_np(t) for t in dd.pipeline_logp_grad_hess(x[3], gauss_newton=gn))
        assert Hs.shape == (d, d) and np.array_equal(Hs, H[3]) and np.array_equal(gs, g[3])
    f0, g0 = (_np(t) for t in dd.logp_and_grad(x))
    np.testing.assert_allclose(f, f0, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-10 * np.max(np.abs(g0)))


def test_results_do_not_depend_on_the_workgroup(ctx):
    """The launches deal at most two workgroups per CU and a workgroup walks over its points, reusing its LDS block and its slot of
    the work buffer.  A batch of 2 x (2 x CUs) + 17 rows, sized from the device's CU count, gives every workgroup two or three
    points: rows equal the same rows in small batches and alone, bit for bit, for the Hessian (both kinds) and the maximiser."""
    import torch
    from bayesfast_amd.device import DeviceDensity
    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n = 2 * (2 * n_cu) + 17
    m, d, nq = 40, 9, 4
    spec, pts = pc.hess_spec(m, d, nq)
    rng = np.random.default_rng(21)
    x = rng.normal(size=(n, d)) * rng.choice([0.05, 0.6], size=(n, 1))
    rb, _ = lc.bound_ratio(spec, x, False)
    assert (rb > 1.).sum() > n // 4 and (rb < 1.).sum() > n // 4
    dd = DeviceDensity(spec, ctx)
    rows = [0, 1, 2 * n_cu - 1, 2 * n_cu, 2 * n_cu + 1, 4 * n_cu - 1, 4 * n_cu, 4 * n_cu + 5, n - 1]   # first, second and third points of workgroups
    for gn in (False, True):
        f, g, H = (_np(t) for t in dd.pipeline_logp_grad_hess(x, gauss_newton=gn))
        assert np.array_equal(H, np.swapaxes(H, 1, 2)) and np.all(np.isfinite(H))
        fs, gs, Hs = (_np(t) for t in dd.pipeline_logp_grad_hess(x[rows], gauss_newton=gn))
        assert np.array_equal(Hs, H[rows]) and np.array_equal(gs, g[rows]) and np.array_equal(fs, f[rows])
        for r in rows[2:7]:
            f1, g1, H1 = (_np(t) for t in dd.pipeline_logp_grad_hess(x[r], gauss_newton=gn))
            assert np.array_equal(H1, H[r]) and np.array_equal(g1, g[r]) and f1 == f[r]
        lo = 2 * n_cu - 3
        fb, gb, Hb = (_np(t) for t in dd.pipeline_logp_grad_hess(x[lo:lo + 40], gauss_newton=gn))
        assert np.array_equal(Hb, H[lo:lo + 40]) and np.array_equal(gb, g[lo:lo + 40]) and np.array_equal(fb, f[lo:lo + 40])
    mspec, x0 = pc.maximiser_spec(m, d, nq)
    starts = x0 + 0.1 * rng.normal(size=(n, d))
    md = DeviceDensity(mspec, ctx)
    for gn in (False, True):
        out = md.pipeline_maximize(starts, xtol=1e-5, gauss_newton=gn)
        xm, fm, Hm, info = (_np(out[k]) for k in ('x', 'logp', 'hess', 'info'))
        assert np.all(info[:, 1] == 0)
        sub = md.pipeline_maximize(starts[rows], xtol=1e-5, gauss_newton=gn)
        assert np.array_equal(_np(sub['x']), xm[rows]) and np.array_equal(_np(sub['hess']), Hm[rows])
        assert np.array_equal(_np(sub['logp']), fm[rows]) and np.array_equal(_np(sub['info']), info[rows])
        for r in rows[2:7]:
            one = md.pipeline_maximize(starts[r], xtol=1e-5, gauss_newton=gn)
            assert np.array_equal(_np(one['x'])[0], xm[r]) and np.array_equal(_np(one['hess'])[0], Hm[r])
            assert _np(one['logp'])[0] == fm[r] and np.array_equal(_np(one['info'])[0], info[r])


# ---- 4: the maximiser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gauss_newton', [False, True])
@pytest.mark.parametrize('shape', [(40, 9, 4), (100, 27, 9)])
def test_maximiser_reaches_the_oracle_maximum(ctx, shape, gauss_newton):
    """The assertions of test_gpu_laplace.py::test_maximiser_reaches_the_oracle_maximum: status 0 on an undamped step, fewer than 30
    iterations, mean |x - x*| <= xtol against the maximum the oracle's damped Newton converges to, f_max to 1e-9, and the returned
    matrix: the full kind within the oracle difference's tolerance, either kind bit for bit pipeline_logp_grad_hess at x."""
    from bayesfast_amd.device import DeviceDensity
    m, d, nq = shape
    spec, x0 = pc.maximiser_spec(m, d, nq)
    xs, fs, gs, _ = lc.oracle_newton(spec, x0)
    assert np.max(np.abs(gs)) < 1e-12
    xtol = 1e-5
    dd = DeviceDensity(spec, ctx)
    out = dd.pipeline_maximize(x0, xtol=xtol, gauss_newton=gauss_newton)
    x, f, H, info = (_np(out[k]) for k in ('x', 'logp', 'hess', 'info'))
    print('%r gauss_newton %d: %d iterations, status %d, last step %.3g, mean |x - x*| %.3g' % (shape, gauss_newton, info[0, 0], info[0, 1], info[0, 2],
                                                                                             np.sum(np.abs(x[0] - xs)) / d))
    assert info[0, 1] == 0 and info[0, 3] == 0. and info[0, 0] < 30 and info[0, 2] <= xtol
    assert np.sum(np.abs(x[0] - xs)) / d <= xtol
    assert abs(f[0] - fs) <= 1e-9 * max(1., abs(fs))
    f1, g1, H1 = (_np(t) for t in dd.pipeline_logp_grad_hess(x[0], False, gauss_newton))
    assert np.max(np.abs(g1)) <= 1e-3 and f1 == f[0]
    assert np.array_equal(H[0], H1) and np.array_equal(H[0], H[0].T)
    if not gauss_newton:
        Hfd, tol = _fd(spec, x[0], False)
        assert np.max(np.abs(H[0] - Hfd)) <= tol


def test_many_starts_in_one_launch(ctx):
    """33 distinct starts in one launch equal the same starts one by one, bit for bit; a start with a non-finite logp returns
    status 2 and leaves its neighbours alone."""
    from bayesfast_amd.device import DeviceDensity
    spec, x0 = pc.maximiser_spec(40, 9, 4)
    d = 9
    starts = x0 + 0.1 * np.random.default_rng(5).normal(size=(33, d))
    dd = DeviceDensity(spec, ctx)
    out = dd.pipeline_maximize(starts, xtol=1e-5)
    x, f, H, info = (_np(out[k]) for k in ('x', 'logp', 'hess', 'info'))
    assert np.all(info[:, 1] == 0)
    for s in range(33):
        one = dd.pipeline_maximize(starts[s], xtol=1e-5)
        assert np.array_equal(_np(one['x'])[0], x[s]) and np.array_equal(_np(one['info'])[0], info[s])
        assert np.array_equal(_np(one['hess'])[0], H[s]) and _np(one['logp'])[0] == f[s]
    bad = starts[:3].copy()
    bad[1, 2] = np.nan
    outb = dd.pipeline_maximize(bad, xtol=1e-5)
    ib = _np(outb['info'])
    assert ib[1, 1] == 2 and ib[1, 0] == 0
    assert np.array_equal(_np(outb['x'])[[0, 2]], x[[0, 2]]) and np.array_equal(ib[[0, 2]], info[[0, 2]])


# ---- 5: Chi2PipelineDensity.hess and Laplace.run -----------------------------------------------------------------------------------
def _pipeline_density(spec, ctx):
    """A Chi2PipelineDensity front of a spec: the package's class with its device density built from the spec."""
    from bayesfast_amd.core.density import Chi2PipelineDensity
    from bayesfast_amd.device import DeviceDensity

    class _SpecDensity(Chi2PipelineDensity):
        def __init__(self):
            self._dev = DeviceDensity(spec, ctx)
            self._d = spec['d']

        def spec(self):
            return spec

        def device(self, ctx=None):
            return self._dev

    return _SpecDensity()


def test_chi2_pipeline_density_hess(ctx):
    """Chi2PipelineDensity.hess at points inside the bound, both spaces, within the oracle difference's tolerance."""
    spec, pts = pc.hess_spec(40, 9, 4)
    den = _pipeline_density(spec, ctx)
    for original_space in (True, False):
        x, rb = pc.points(spec, pts, original_space)
        x = x[rb < 1.]
        H = den.hess(x, original_space=original_space)
        assert H.shape == (len(x), 9, 9)
        for p in range(len(x)):
            Hfd, tol = _fd(spec, x[p], original_space)
            assert np.max(np.abs(H[p] - Hfd)) <= tol
        assert np.array_equal(den.hess(x[0], original_space=original_space), H[0])
    Hg = den.hess(x, original_space=False, gauss_newton=True)
    assert Hg.shape == H.shape and not np.array_equal(Hg, H)


def _count_single_point_calls(monkeypatch, cls):
    """The counting pattern of helpers/laplace_seam.py, on the class whose methods a host optimiser would loop over."""
    calls = []
    for name in ('logp', 'grad', 'logp_and_grad'):
        real = getattr(cls, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(self, *a, **kw)

        monkeypatch.setattr(cls, name, counted)
    return calls


def test_laplace_run_takes_the_device_route(ctx, monkeypatch):
    """Laplace.run on a Chi2PipelineDensity: no per-point logp / grad call; x_max within the maximiser's tolerance of the host
    route's ('trust-exact'); cov = inv(make_positive(-H_fd)) at x_max (rtol 1e-6); hess_options gauss_newton gives the
    Gauss-Newton covariance; (n_start, d) starts are accepted."""
    from bayesfast_amd.core.density import Chi2PipelineDensity
    from bayesfast_amd.utils import Laplace, make_positive
    spec, x0 = pc.maximiser_spec(40, 9, 4)
    d = 9
    den = _pipeline_density(spec, ctx)
    host = Laplace(optimize_method='trust-exact', optimize_tol=1e-8, n_sample=16).run(den, x0)
    xtol = 1e-5
    res_b = Laplace(optimize_tol=xtol, n_sample=16).run(den.logp, x0)   # (the bound method, before the counters wrap it)
    calls = _count_single_point_calls(monkeypatch, Chi2PipelineDensity)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = Laplace(optimize_tol=xtol, n_sample=16).run(den, x0)
        res_g = Laplace(optimize_tol=xtol, n_sample=16, hess_options={'gauss_newton': True}).run(den, x0)
        starts = x0 + 0.1 * np.random.default_rng(1).normal(size=(5, d))
        res_m = Laplace(optimize_tol=xtol, n_sample=16).run(den, starts)
    assert calls == [], 'the device route called %r on the density' % (calls,)
    opt = res.opt_result
    assert opt.success and opt.status == 0 and opt.nhev == opt.nit + 1
    assert np.array_equal(res_b.x_max, res.x_max) and np.array_equal(res_b.cov, res.cov)
    # the host route stops at |grad| <= 1e-8: its distance to the maximum is far below xtol
    assert np.sum(np.abs(res.x_max - host.x_max)) / d <= xtol
    Hfd, tolH = _fd(spec, res.x_max, False)
    want = np.linalg.inv(make_positive(-Hfd, 1e5))
    np.testing.assert_allclose(res.cov, want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want)))
    Hg = _np(den.device().pipeline_logp_grad_hess(res_g.x_max, False, gauss_newton=True)[2])
    assert np.array_equal(res_g.cov, np.linalg.inv(make_positive(-Hg, 1e5)))
    assert np.sum(np.abs(res_g.x_max - host.x_max)) / d <= xtol
    assert res_m.opt_result.all_x.shape == (5, d) and np.all(res_m.opt_result.all_status == 0)
    assert np.sum(np.abs(res_m.x_max - host.x_max)) / d <= xtol


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """A scalar density is refused by the two new calls; the streamed form raises NotImplementedError naming it, Laplace.run still
    returns for it through the host route, and the context stays usable."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.utils import Laplace
    from bayesfast_amd.workloads import correlated_gaussian_spec
    sd = DeviceDensity(correlated_gaussian_spec(16)[0], ctx)
    x = np.zeros((2, 16))
    with pytest.raises(NotImplementedError, match='scalar surrogate density'):
        sd.pipeline_logp_grad_hess(x)
    with pytest.raises(NotImplementedError, match='scalar surrogate density'):
        sd.pipeline_maximize(x)
    sd.logp_grad_hess(x)
    spec = pc.streamed_spec()
    d = spec['d']
    den = _pipeline_density(spec, ctx)
    xs = 0.05 * np.random.default_rng(0).normal(size=(2, d))
    with pytest.raises(NotImplementedError, match='streamed'):
        den.device().pipeline_logp_grad_hess(xs)
    with pytest.raises(NotImplementedError, match='streamed'):
        den.device().pipeline_maximize(xs)
    with pytest.raises(NotImplementedError, match='streamed'):
        den.hess(xs, original_space=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = Laplace(n_sample=8, optimize_options={'maxiter': 3}).run(den, xs[0])
    assert np.all(np.isfinite(res.x_max)) and res.cov.shape == (d, d) and not hasattr(res.opt_result, 'all_x')
    f, g = den.device().logp_and_grad(xs)   # (and the context is still usable)
    assert np.all(np.isfinite(_np(f)))
