"""The Laplace approximation without a GPU: the arithmetic of the device kernels compiled for the host, make_positive, the
``Laplace`` class and its host route.

Expected values come from the oracle (differences of ``oracle.logp_and_grad``, helpers/laplace_cases.py), from closed forms, or
from the reference's own functions (oracle/_ref, where built) -- never from the code under test."""
import os
import sys
import warnings

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import reference

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, 'helpers'), os.path.join(HERE, 'hess_host')):
    if p not in sys.path:
        sys.path.insert(0, p)

import laplace_cases as lc  # noqa: E402


# ---- (a) bfhip_hess.h on the host ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(lc.FEATURES))
@pytest.mark.parametrize('d', [2, 5, 16])
def test_header_hessian_equals_differences_of_the_oracle_gradient(d, name):
    """bf_hess_eval / bf_hess_entry (one host thread) against H_fd = (4 D(h) - D(2h)) / 3 of the oracle's gradient, h = 1e-3 of each
    coordinate's scale, in both spaces, inside and outside the bound and the decay ellipsoid.  Tolerance: measured on the oracle
    (laplace_cases.hess_fd_with_tol).  The value and the gradient of the same call are the oracle's to rounding."""
    import hess_host
    spec, scale_o, scale_s, pts = lc.feature_spec(d, name)
    covered = True
    for original_space in (True, False):
        x = pts if original_space else lc.from_original(spec, pts)
        ok, rb, rd = lc.keep_off_the_kinks(spec, x, original_space)
        assert ok.sum() >= 3   # (a condition on the inputs: no stencil straddles a kink)
        x = x[ok]
        covered = covered and lc.covers_both_sides(spec, rb[ok], rd[ok])
        f, g, H = hess_host.logp_grad_hess(spec, x, original_space)
        f0, g0 = orc.logp_and_grad(spec, x, original_space=original_space)
        np.testing.assert_allclose(f, f0, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(g, g0, rtol=1e-11, atol=1e-11 * np.max(np.abs(g0)))
        for p in range(len(x)):
            Hfd, tol = lc.hess_fd_with_tol(spec, x[p], original_space, scale_o if original_space else scale_s)
            if lc.jacobian_is_asymmetric(spec, original_space):
                Hfd = 0.5 * (Hfd + Hfd.T)
            assert np.array_equal(H[p], H[p].T)
            err = float(np.max(np.abs(H[p] - Hfd)))
            print('d %d %s original_space %d point %d: |H - H_fd| %.3g, tolerance %.3g' % (d, name, original_space, p, err, tol))
            assert err <= tol
    assert covered   # inside / outside the bound AND the decay ellipsoid, and a point between the two surfaces, in both spaces


@pytest.mark.parametrize('kind', ['quadratic', 'cubic', 'decay'])
@pytest.mark.parametrize('d', [16, 64])
def test_header_newton_reaches_the_oracle_maximum(d, kind):
    """bf_newton_max (one host thread) on the maximiser's test densities: -H is indefinite at the start (asserted on the oracle),
    the iteration ends undamped (status 0) and within xtol of the maximum the oracle's own damped Newton converges to tightly."""
    import hess_host
    spec, x0 = lc.t2_spec(d, kind)
    H0 = lc.hess_fd(spec, x0)
    ev = np.linalg.eigvalsh(-0.5 * (H0 + H0.T))
    assert ev[0] < -1. and ev[-1] > 1.
    xs, fs, gs, _ = lc.oracle_newton(spec, x0)
    assert np.max(np.abs(gs)) < 1e-12
    xtol = 1e-5
    x, f, H, info = hess_host.maximize(spec, x0[None], 200, xtol)
    assert info[0, 1] == 0 and info[0, 3] == 0. and info[0, 2] <= xtol and info[0, 0] < 30
    assert np.sum(np.abs(x[0] - xs)) / d <= xtol
    assert abs(f[0] - fs) <= 1e-9 * max(1., abs(fs))
    assert np.array_equal(H[0], H[0].T)


# ---- (b) make_positive -------------------------------------------------------------------------------------------------------------
def _spd_with(eigs, seed=0):
    from scipy.stats import special_ortho_group
    Q = special_ortho_group.rvs(len(eigs), random_state=np.random.RandomState(seed))
    return (Q * np.asarray(eigs, dtype=np.float64)) @ Q.T


def test_make_positive_semantics():
    """Eigenvalues below and AT max / max_cond are raised to the smallest one above it; those above stay (utils/misc.py:12-18)."""
    from bayesfast_amd.utils import make_positive
    eigs = np.array([-3., 1e-4, 2e-3, 0.5, 2., 100.])   # max / max_cond = 1e-3 with max_cond = 1e5: -3 and 1e-4 below, 2e-3 the floor
    out = make_positive(_spd_with(eigs), 1e5)
    np.testing.assert_allclose(np.linalg.eigvalsh(out), [2e-3, 2e-3, 2e-3, 0.5, 2., 100.], rtol=1e-9)
    out = make_positive(np.diag([1., 4., 16.]), 4.)      # 4 is AT max / max_cond: not above it, so it is raised to 16
    np.testing.assert_allclose(np.linalg.eigvalsh(out), [16., 16., 16.], rtol=1e-12)
    with pytest.raises(ValueError, match='all the eigenvalues are non-positive.'):
        make_positive(-np.eye(3))
    with pytest.raises(ValueError):
        make_positive(np.zeros((2, 2)))


@pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')
def test_make_positive_equals_the_reference():
    from bayesfast_amd.utils import make_positive
    ref = reference.load().utils.misc.make_positive
    for seed, eigs, mc in ((1, [-3., 1e-4, 2e-3, 0.5, 2., 100.], 1e5), (2, [1e-9, 1., 3.], 1e5), (3, [0.2, 1., 3.], 1e5),
                           (4, [1., 4., 16.], 4.), (5, [-1., -0.5, 2.], 10.)):
        A = _spd_with(eigs, seed)
        np.testing.assert_allclose(make_positive(A.copy(), mc), ref(A.copy(), mc), rtol=1e-12, atol=1e-13 * max(np.abs(eigs)))
    with pytest.raises(ValueError):
        ref(-np.eye(3))


# ---- (c) the class ---------------------------------------------------------------------------------------------------------------
def test_laplace_constructor_validation():
    from bayesfast_amd.utils import Laplace
    for kw, msg in ((dict(optimize_tol=-1.), 'invalid value for optimize_tol.'), (dict(optimize_tol='a'), 'invalid value for optimize_tol.'),
                    (dict(optimize_options=3), 'invalid value for optimize_options.'), (dict(max_cond=0.), 'max_cond should be a positive float.'),
                    (dict(n_sample=0), 'invalid value for n_sample.'), (dict(beta=-2.), 'beta should be a positive float.'),
                    (dict(mvn_generator=3), 'invalid value for mvn_generator.'), (dict(grad_options=3), 'invalid value for grad_options.'),
                    (dict(hess_options=3), 'invalid value for hess_options.')):
        with pytest.raises(ValueError, match=msg):
            Laplace(**kw)
    lap = Laplace()
    assert (lap._optimize_method, lap._optimize_tol, lap._optimize_options, lap._max_cond, lap._n_sample, lap._beta) == \
        ('Newton-CG', 1e-5, {}, 1e5, 2000, 1.)
    assert Laplace(optimize_tol=None, n_sample=None)._n_sample is None
    with pytest.raises(ValueError, match='logp should be callable.'):
        lap.run(3., np.zeros(2))
    with pytest.raises(ValueError, match='invalid value for x_0.'):
        lap.run(lambda x: 0., np.zeros((2, 2)))   # (several starts are the device route's)
    with pytest.raises(ValueError, match='laplace_result should be a LaplaceResult.'):
        Laplace.untemper_laplace_samples((1, 2))


@pytest.mark.parametrize('with_grad', [False, True])
def test_host_route_on_a_plain_callable(with_grad):
    """A 5-d correlated Gaussian as a plain callable (differenced here: nothing imports numdifftools): x_max is the mean -- Newton-CG
    stops at sum |step| <= d tol and inside its convergence region the error after a step is below the step, so max |x - mean| <=
    d tol -- and cov is the Gaussian's covariance (the differences of a quadratic are exact to rounding: 1e-6 relative is generous)."""
    from bayesfast_amd.utils import Laplace, LaplaceResult
    from bayesfast_amd.utils.sobol import multivariate_normal
    rng = np.random.default_rng(2)
    d = 5
    Lc = np.eye(d) + 0.4 * np.tril(rng.normal(size=(d, d)), -1)
    cov, mean = Lc @ Lc.T, rng.normal(size=d)
    prec = np.linalg.inv(cov)
    logp = lambda x: -0.5 * (np.asarray(x) - mean) @ prec @ (np.asarray(x) - mean)
    grad = (lambda x: -prec @ (np.asarray(x) - mean)) if with_grad else None
    tol = 1e-5
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = Laplace(optimize_tol=tol, n_sample=64, beta=0.25).run(logp, mean + rng.normal(size=d), grad=grad)
    assert isinstance(res, LaplaceResult) and res._fields == ('x_max', 'f_max', 'samples', 'cov', 'beta', 'opt_result')
    assert res.opt_result.success
    assert np.max(np.abs(res.x_max - mean)) <= d * tol
    assert abs(res.f_max) <= 1e-8
    np.testing.assert_allclose(res.cov, cov, rtol=1e-6, atol=1e-6 * np.max(np.abs(cov)))
    assert np.array_equal(res.samples, multivariate_normal(res.x_max, res.cov / 0.25, 64))
    un = Laplace.untemper_laplace_samples(res)
    np.testing.assert_allclose(un - res.x_max, 0.5 * (res.samples - res.x_max), rtol=1e-13, atol=1e-15)


def test_numdifftools_is_not_imported():
    import bayesfast_amd.utils.laplace as m
    src = open(m.__file__).read()
    assert 'import numdifftools' not in src and 'from numdifftools' not in src


# ---- (d) the host route on one of the package's densities: one launch per difference Hessian -------------------------------------
def test_host_route_differences_the_device_gradient_in_one_launch(monkeypatch):
    """A SurrogateDensity behind the oracle stand-in, optimize_method='trust-exact' (so: the host route): every Hessian the optimiser
    asks for is ONE gradient call on the 4 d stencil points; the result is the oracle's maximum within the optimiser's own residual Newton step, the covariance H_fd's."""
    import oracle_standin
    from bayesfast_amd.core.density import SurrogateDensity
    from bayesfast_amd.modules.poly import PolyModel
    from bayesfast_amd.utils import Laplace, make_positive
    oracle_standin.install(monkeypatch)
    d = 6
    rng = np.random.default_rng(4)
    G = rng.normal(size=(d, d)) / np.sqrt(d)
    P = np.eye(d) + G @ G.T
    A = -0.5 * P
    pm = PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(use_bound=False))
    pm.configs[0]._coef = np.concatenate(([-0.5 * 0.09 * P.sum()], 0.3 * P.sum(axis=1)))[None]   # -(x - 0.3)^T P (x - 0.3) / 2
    pm.configs[1]._coef = np.triu(A * (2. - np.eye(d)))[None]
    den = SurrogateDensity(pm, input_scales=np.tile(np.array([-8., 8.]), (d, 1)), hard_bounds=True, decay_options=dict(use_decay=False))
    shapes = []
    real_grad = SurrogateDensity.grad

    def counting_grad(self, pts, original_space=True):
        shapes.append(np.shape(pts))
        assert original_space is False
        return real_grad(self, pts, original_space)

    monkeypatch.setattr(SurrogateDensity, 'grad', counting_grad)
    x0 = den.from_original(np.full(d, 0.1))
    res = Laplace(optimize_method='trust-exact', optimize_tol=1e-6, n_sample=16).run(den.logp, x0)
    assert res.opt_result.success
    n_hess = sum(1 for s in shapes if s == (4 * d, d))
    assert n_hess >= 2 and all(s in ((4 * d, d), (d,)) for s in shapes)   # batches of the whole stencil, never d separate calls
    assert n_hess == res.opt_result.nhev + 1                               # the optimiser's, and one more at the maximum
    spec = den.spec()
    xs, fs, gs, _ = lc.oracle_newton(spec, x0)
    Hfd, tol = lc.hess_fd_with_tol(spec, xs)
    # the optimiser stops at |grad| <= its tolerance: its distance to the maximum is its own residual Newton step, taken on the oracle
    _, g_res = orc.logp_and_grad(spec, res.x_max[None], original_space=False)
    r = float(np.max(np.abs(np.linalg.solve(0.5 * (Hfd + Hfd.T), g_res[0]))))
    assert np.max(np.abs(res.x_max - xs)) <= 2. * r + 1e-12
    assert abs(res.f_max - fs) <= float(np.max(np.abs(g_res))) * r * d + 1e-12
    want = np.linalg.inv(make_positive(-0.5 * (Hfd + Hfd.T), 1e5))
    np.testing.assert_allclose(res.cov, want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want)))
