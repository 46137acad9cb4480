"""GPU: the analytic Hessian of the device density (bfhip_logp_hess) and the device-resident Newton maximiser (bfhip_laplace_opt)
behind ``Laplace.run``, against independent references taken on the CPU oracle (helpers/laplace_cases.py): the fourth-order central
difference H_fd of the oracle's gradient, with a tolerance measured on the oracle per point, and a damped Newton iteration on the
oracle converged to |grad| ~ 1e-13."""
import os
import sys
import warnings

import numpy as np
import pytest

from oracle import reference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import laplace_cases as lc  # noqa: E402


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _np(t):
    return t.cpu().numpy()


# ---- T1: the Hessian -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(lc.FEATURES))
@pytest.mark.parametrize('d', [2, 16, 27, 64, 128])
def test_logp_hess_equals_differences_of_the_oracle_gradient(ctx, d, name):
    """Every feature of the density record, both spaces, points inside and outside the bound and the decay ellipsoid: |H - H_fd|
    within the tolerance measured on the oracle for that point; H == H^T exactly; logp and grad of the same call are
    bfhip_logp_grad's (rtol 1e-10, its own tests' tolerance)."""
    from bayesfast_amd.device import DeviceDensity
    spec, scale_o, scale_s, pts = lc.feature_spec(d, name)
    dd = DeviceDensity(spec, ctx)
    covered = True
    for original_space in (True, False):
        x = pts if original_space else lc.from_original(spec, pts)
        ok, rb, rd = lc.keep_off_the_kinks(spec, x, original_space)
        assert ok.sum() >= 3   # (a condition on the inputs: no stencil straddles a kink)
        x = x[ok]
        covered = covered and lc.covers_both_sides(spec, rb[ok], rd[ok])
        f, g, H = (_np(t) for t in dd.logp_grad_hess(x, original_space))
        f0, g0 = (_np(t) for t in dd.logp_and_grad(x, original_space))
        np.testing.assert_allclose(f, f0, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-10 * np.max(np.abs(g0)))
        for p in range(len(x)):
            Hfd, tol = lc.hess_fd_with_tol(spec, x[p], original_space, scale_o if original_space else scale_s)
            if lc.jacobian_is_asymmetric(spec, original_space):
                Hfd = 0.5 * (Hfd + Hfd.T)
            assert np.array_equal(H[p], H[p].T)
            err = float(np.max(np.abs(H[p] - Hfd)))
            print('d %d %s original_space %d point %d: |H - H_fd| %.3g, tolerance %.3g' % (d, name, original_space, p, err, tol))
            assert err <= tol
    assert covered   # inside / outside the bound AND the decay ellipsoid, and a point between the two surfaces, in both spaces


@pytest.mark.parametrize('name', ['quadratic', 'everything'])
def test_logp_hess_batches(ctx, name):
    """n = 1, 17 and 300 points (a partial wave of workgroups, more workgroups than the device runs at once): a point's result does
    not depend on the batch it came in (bit for bit), and rows of the large batch equal H_fd."""
    from bayesfast_amd.device import DeviceDensity
    d = 64
    spec, scale_o, scale_s, pts = lc.feature_spec(d, name)
    rng = np.random.default_rng(12)
    lo = spec['su_lo'] if spec.get('su_lo') is not None else np.zeros(d)
    diff = spec['su_diff'] if spec.get('su_diff') is not None else np.ones(d)
    xo = lo + diff * np.clip(rng.normal(size=(400, d)) * rng.choice([0.4, 2.2], size=(400, 1)), -4., 4.)
    x = lc.from_original(spec, xo)
    ok, rb, _ = lc.keep_off_the_kinks(spec, x, False)
    x, rb = x[ok][:300], rb[ok][:300]   # more drawn than needed: exactly 300 rows after the filter
    assert len(x) == 300 and (rb > 1.).any() and (rb < 1.).any()
    dd = DeviceDensity(spec, ctx)
    f, g, H = (_np(t) for t in dd.logp_grad_hess(x))
    assert np.array_equal(H, np.swapaxes(H, 1, 2))
    f17, g17, H17 = (_np(t) for t in dd.logp_grad_hess(x[5:22]))
    assert np.array_equal(H17, H[5:22]) and np.array_equal(g17, g[5:22]) and np.array_equal(f17, f[5:22])
    f1, g1, H1 = (_np(t) for t in dd.logp_grad_hess(x[-1:]))
    assert np.array_equal(H1, H[-1:]) and np.array_equal(f1, f[-1:])
    fs, gs, Hs = (_np(t) for t in dd.logp_grad_hess(x[3]))   # a single point: (d,) in, (d, d) out
    assert Hs.shape == (d, d) and np.array_equal(Hs, H[3])
    f0, g0 = (_np(t) for t in dd.logp_and_grad(x))
    np.testing.assert_allclose(f, f0, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-10 * np.max(np.abs(g0)))
    for p in (0, 150, len(x) - 1):
        Hfd, tol = lc.hess_fd_with_tol(spec, x[p], False, scale_s)
        if lc.jacobian_is_asymmetric(spec, False):
            Hfd = 0.5 * (Hfd + Hfd.T)
        assert np.max(np.abs(H[p] - Hfd)) <= tol


@pytest.mark.parametrize('d', [2, 16, 27, 64, 128])
def test_logp_hess_of_a_plain_quadratic_in_the_bound_is_minus_p(ctx, d):
    """In the bound the Hessian of the plain quadratic surrogate is S = A + A^T, read from the uploaded matrix: the kernel multiplies
    it by 1 (no scaling, no link) and adds an exact 0, and S = -P is formed without rounding (the coefficients are -P / 2 doubled).
    So the bound is 0 -- no arithmetic touches the entries; one ulp of max |P| is allowed for."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, cov = correlated_gaussian_spec(d)
    rng = np.random.default_rng(d)
    L = np.eye(d) + 0.3 * np.tril(np.random.default_rng(123).normal(size=(d, d)), -1) / np.sqrt(d)
    P = L @ L.T
    x = 0.3 * rng.normal(size=(9, d))
    rb, _ = lc.bound_ratio(spec, x, True)
    assert np.all(rb < 0.95)
    for original_space in (True, False):
        H = _np(DeviceDensity(spec, ctx).logp_grad_hess(x, original_space)[2])
        assert np.max(np.abs(H + P)) <= np.finfo(np.float64).eps * np.max(np.abs(P))


def test_logp_hess_refuses_the_pipeline_density(ctx):
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.workloads import random_pipeline_spec
    pd = DeviceDensity(random_pipeline_spec(40, 9, 4, seed=2), ctx)
    x = np.random.default_rng(0).normal(size=(4, 9)) * 0.3
    with pytest.raises(NotImplementedError, match='pipeline density'):
        pd.logp_grad_hess(x)
    with pytest.raises(NotImplementedError, match='pipeline density'):
        pd.maximize(x)
    pd.logp_and_grad(x)   # (and the context is still usable)


# ---- T2: the maximiser ---------------------------------------------------------------------------------------------------------------
def _surrogate_density(spec, ctx):
    """A SurrogateDensity-like front of a spec for Laplace.run: the package's class with its device density built from the spec."""
    from bayesfast_amd.core.density import SurrogateDensity
    from bayesfast_amd.device import DeviceDensity

    class _SpecDensity(SurrogateDensity):
        def __init__(self):
            self._dev = DeviceDensity(spec, ctx)

        def spec(self):
            return spec

        def device(self, ctx=None):
            return self._dev

    return _SpecDensity()


T2_CASES = [(16, 'quadratic'), (64, 'quadratic'), (16, 'cubic'), (64, 'cubic'), (16, 'decay'), (64, 'decay')]


@pytest.mark.parametrize('d,kind', T2_CASES)
def test_maximiser_reaches_the_oracle_maximum(ctx, d, kind):
    """(i) sum |x_dev - x*| / d <= xtol against the maximum the oracle's damped Newton converges to tightly: inside Newton's
    convergence region the error after a step is below the step, and the kernel stops at mean |step| <= xtol on an undamped step.
    (iii) cov against inv(make_positive(-H_fd(x_max))), tolerance cond(H) x the Hessian tolerance, both from the oracle's matrix.
    (iv) samples are sobol.multivariate_normal(x_max, cov / beta, n_sample) bit for bit; untemper inverts beta = 0.25."""
    from bayesfast_amd.utils import Laplace, make_positive
    from bayesfast_amd.utils.sobol import multivariate_normal
    spec, x0 = lc.t2_spec(d, kind)
    H0 = lc.hess_fd(spec, x0)
    ev = np.linalg.eigvalsh(-0.5 * (H0 + H0.T))
    assert ev[0] < -1. and ev[-1] > 1.   # indefinite at the start: the plain Newton direction is not an ascent direction
    xs, fs, gs, _ = lc.oracle_newton(spec, x0)
    assert np.max(np.abs(gs)) < 1e-12
    xtol = 1e-5
    den = _surrogate_density(spec, ctx)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = Laplace(optimize_tol=xtol, n_sample=500, beta=0.25).run(den, x0)
    opt = res.opt_result
    print('d %d %s: %d iterations, status %d, last step %.3g, mean |x - x*| %.3g' % (d, kind, opt.nit, opt.status, opt.last_step,
                                                                                   np.sum(np.abs(res.x_max - xs)) / d))
    assert opt.success and opt.status == 0 and opt.damping == 0. and opt.nit < 30 and opt.nhev == opt.nit + 1
    assert np.sum(np.abs(res.x_max - xs)) / d <= xtol
    assert abs(res.f_max - fs) <= 1e-9 * max(1., abs(fs)) and abs(opt.fun + res.f_max) == 0.
    assert np.max(np.abs(opt.jac)) <= 1e-3
    Hfd, tolH = lc.hess_fd_with_tol(spec, res.x_max)
    A = -0.5 * (Hfd + Hfd.T)
    want = np.linalg.inv(make_positive(A, 1e5))
    err = float(np.max(np.abs(res.cov - want)))
    tol = float(np.linalg.cond(A)) * tolH
    print('   cov: |cov - inv(make_positive(-H_fd))| %.3g, tolerance %.3g' % (err, tol))
    assert err <= tol
    assert np.array_equal(res.samples, multivariate_normal(res.x_max, res.cov / 0.25, 500))
    un = Laplace.untemper_laplace_samples(res)
    np.testing.assert_allclose(un - res.x_max, 0.5 * (res.samples - res.x_max), rtol=1e-13, atol=1e-15)
    # the density's own entry points agree with what run() returned
    out = den.device().maximize(x0, xtol=xtol)
    assert np.array_equal(_np(out['x'])[0], res.x_max)
    assert np.array_equal(_np(out['hess'])[0], _np(den.device().logp_grad_hess(res.x_max)[2]))
    assert np.array_equal(den.hess(res.x_max, original_space=False), _np(out['hess'])[0])


@pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')
@pytest.mark.parametrize('d', [16, 64])
def test_maximiser_against_the_reference_laplace(ctx, d):
    """(ii) The reference's own Laplace.run (oracle/_ref), its logp / grad callables answered by the oracle:
    max |x_dev - x_ref| <= 2 r + xtol with r = max |H_fd^-1 g(x_ref)|, the reference's residual Newton step on the oracle."""
    from bayesfast_amd.utils import Laplace
    from oracle import oracle as orc
    bf = reference.load()
    spec, x0 = lc.t2_spec(d, 'quadratic')
    logp = lambda x: float(orc.logp_and_grad(spec, np.asarray(x)[None], original_space=False)[0][0])
    grad = lambda x: orc.logp_and_grad(spec, np.asarray(x)[None], original_space=False)[1][0]
    ref = bf.utils.Laplace(n_sample=10).run(logp=logp, x_0=x0, grad=grad)
    xtol = 1e-5
    res = Laplace(optimize_tol=xtol, n_sample=10).run(_surrogate_density(spec, ctx), x0)
    Hfd = lc.hess_fd(spec, ref.x_max)
    r = float(np.max(np.abs(np.linalg.solve(0.5 * (Hfd + Hfd.T), grad(ref.x_max)))))
    err = float(np.max(np.abs(res.x_max - ref.x_max)))
    print('d %d: |x_dev - x_ref| %.3g, r %.3g' % (d, err, r))
    assert err <= 2. * r + xtol


def test_many_starts_in_one_launch(ctx):
    """(v) 300 starts, the first three repeated at the end: repeated rows give bit-identical results (a start's result depends on
    its row and the density only), the returned start is the argmax of all_fun, every status is 0."""
    from bayesfast_amd.utils import Laplace
    d = 16
    spec, _ = lc.t2_spec(d, 'quadratic')
    x0 = np.random.default_rng(3).normal(size=(300, d))
    x0[-3:] = x0[:3]
    den = _surrogate_density(spec, ctx)
    out = den.device().maximize(x0, xtol=1e-5)
    x, f, H, info = (_np(out[k]) for k in ('x', 'logp', 'hess', 'info'))
    assert np.array_equal(x[-3:], x[:3]) and np.array_equal(f[-3:], f[:3]) and np.array_equal(H[-3:], H[:3])
    assert np.array_equal(info[-3:], info[:3])
    one = den.device().maximize(x0[1], xtol=1e-5)          # ... nor on the number of starts
    assert np.array_equal(_np(one['x'])[0], x[1]) and np.array_equal(_np(one['info'])[0], info[1])
    print('iterations per start: min %d, mean %.2f, max %d' % (info[:, 0].min(), info[:, 0].mean(), info[:, 0].max()))
    assert np.all(info[:, 1] == 0)
    res = Laplace(n_sample=10).run(den, x0)
    opt = res.opt_result
    assert np.array_equal(opt.all_x, x) and np.array_equal(opt.all_fun, f) and np.all(opt.all_status == 0)
    best = int(np.argmax(opt.all_fun))
    assert np.array_equal(res.x_max, x[best]) and res.f_max == f[best]
    xs, fs, _, _ = lc.oracle_newton(spec, x0[0])           # one concave maximum: every start finds it
    assert np.max(np.sum(np.abs(x - xs), axis=1)) / d <= 1e-5


def test_singular_hessian_returns(ctx):
    """(vi) The donut's OptimizeStep density: a LINEAR surrogate of m = |x| under the Gaussian link, so -H = prec l l^T has rank one
    and the maximiser is a line.  The call returns finite numbers with status 0, 1 or 3, and make_positive treats the matrix as the
    reference's does (floor at the only positive eigenvalue)."""
    from bayesfast_amd.utils import Laplace, make_positive
    l = np.array([0.70, 0.72])
    poly = dict(input_size=2, output_size=1, use_bound=False,
                configs=[dict(order='linear', input_mask=np.arange(2), output_mask=np.arange(1), coef=np.array([[0.05, l[0], l[1]]]))])
    spec = dict(d=2, ranges=None, hard_bounds=None, su_lo=None, su_diff=None, poly=poly, use_decay=False,
                link=dict(kind='gaussian', y=5., prec=4., logp0=0.))
    den = _surrogate_density(spec, ctx)
    out = den.device().maximize(np.array([[10., 10.], [0., 0.], [3., -2.]]), max_iter=50)
    x, f, H, info = (_np(out[k]) for k in ('x', 'logp', 'hess', 'info'))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(f)) and np.all(np.isfinite(H)) and np.all(np.isfinite(info))
    assert set(info[:, 1].astype(int)) <= {0, 1, 3}
    np.testing.assert_allclose(H[0], -4. * np.outer(l, l), rtol=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = Laplace(n_sample=8).run(den, np.array([10., 10.]))
    pos = make_positive(-H[0], 1e5)
    np.testing.assert_allclose(np.linalg.eigvalsh(pos), [4. * l @ l] * 2, rtol=1e-12)
    if reference.is_built():
        np.testing.assert_allclose(pos, reference.load().utils.misc.make_positive(-H[0].copy(), 1e5), rtol=1e-12, atol=1e-14)
    assert np.all(np.isfinite(res.cov)) and np.all(np.isfinite(res.samples))


def test_donut_optimize_step_density_returns(ctx):
    """(vi) on the donut itself (helpers/donut.py): the OptimizeStep's density, a LINEAR surrogate of m = |x| fitted on the recipe's
    Sobol points around (10, 10), under the Gaussian link, decay term on -- first as the recipe's iteration 0 (the decay term makes
    -H definite far out), then refitted on the Laplace samples as its iteration 1, where -H = prec l l^T has rank one inside the decay
    ellipsoid and the line of maxima ends on the decay surface.  Both calls return finite numbers with status 0, 1 or 3, and
    make_positive treats the Hessian as the reference's does."""
    import donut
    import bayesfast_amd as bfa
    from bayesfast_amd.utils import Laplace, make_positive
    from bayesfast_amd.utils.sobol import multivariate_normal
    su = bfa.PolyModel('linear', input_size=2, output_size=1)
    den = bfa.SurrogateDensity(su, decay_options=dict(use_decay=True), link=bfa.GaussianLink(donut.A, 2. / donut.B))
    x_fit = multivariate_normal([10, 10], np.eye(2), 20)[:2 * su.n_param]
    x0 = x_fit[0]
    for it in range(2):
        den.fit(x_fit, donut.true_logp(x_fit), y=donut.f_0(x_fit))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            res = Laplace(beta=100.).run(den, x0)
        opt = res.opt_result
        H = den.hess(res.x_max, original_space=False)
        _, rd = lc.bound_ratio(den.spec(), res.x_max[None], False)
        print('donut iteration %d: x_max %r, status %d after %d iterations, lambda %.3g, beta_d / alpha_d %.5f, eig(-H) %r'
              % (it, res.x_max, opt.status, opt.nit, opt.damping, rd[0], np.linalg.eigvalsh(-H)))
        assert opt.status in (0, 1, 3) and np.isfinite(res.f_max)
        assert np.all(np.isfinite(res.x_max)) and np.all(np.isfinite(H)) and np.all(np.isfinite(res.cov)) and np.all(np.isfinite(res.samples))
        assert np.array_equal(H, H.T)
        pos = make_positive(-H, 1e5)
        assert np.linalg.eigvalsh(pos)[0] > 0.
        np.testing.assert_allclose(res.cov, np.linalg.inv(pos), rtol=1e-10)
        if reference.is_built():
            np.testing.assert_allclose(pos, reference.load().utils.misc.make_positive(-H.copy(), 1e5), rtol=1e-12, atol=1e-14)
        x_fit, x0 = res.samples[:2 * su.n_param], res.x_max
    assert rd[0] <= 1.   # iteration 1 ends inside (or on the inside of) the decay ellipsoid

