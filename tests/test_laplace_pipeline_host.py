"""No GPU: the routing of ``Laplace.run`` for a ``Chi2PipelineDensity``, behind an oracle stand-in of the device density
(helpers/oracle_standin_pipeline_laplace.py): the device route is chosen, ``gauss_newton`` is passed through, (n_start, d) starts are
accepted, a refusal of the device falls back to the host route, and the result is the LaplaceResult built from the stand-in's
numbers."""
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import laplace_cases as lc  # noqa: E402
import pipeline_hess_cases as pc  # noqa: E402
from oracle_standin_pipeline_laplace import OraclePipelineLaplaceDensity  # noqa: E402


def _density(spec, refuse=False):
    from bayesfast_amd.core.density import Chi2PipelineDensity
    dev = OraclePipelineLaplaceDensity(spec, refuse=refuse)

    class _SpecDensity(Chi2PipelineDensity):
        def __init__(self):
            self._d = spec['d']

        def spec(self):
            return spec

        def device(self, ctx=None):
            return dev

    return _SpecDensity(), dev


@pytest.fixture(scope='module')
def case():
    spec, x0 = pc.maximiser_spec(40, 9, 4)
    xs, fs, gs, _ = lc.oracle_newton(spec, x0)
    assert np.max(np.abs(gs)) < 1e-12
    H = lc.hess_fd(spec, xs)
    return spec, x0, xs, fs, 0.5 * (H + H.T)


def test_run_takes_the_device_route_and_builds_the_result_from_its_numbers(case):
    from bayesfast_amd.utils import Laplace, LaplaceResult, make_positive
    from bayesfast_amd.utils.sobol import multivariate_normal
    spec, x0, xs, fs, H = case
    den, dev = _density(spec)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = Laplace(n_sample=32, beta=0.25).run(den, x0)
    assert dev.calls == [('pipeline_maximize', 1, False)]   # one launch ...
    assert dev.n_logp_and_grad == 1                         # ... and the gradient at x_max: no per-point loop of a host optimiser
    assert isinstance(res, LaplaceResult)
    cov = np.linalg.inv(make_positive(-H, 1e5))
    assert np.array_equal(res.x_max, xs) and res.f_max == fs and np.array_equal(res.cov, cov) and res.beta == 0.25
    assert np.array_equal(res.samples, multivariate_normal(xs, cov / 0.25, 32))
    opt = res.opt_result
    assert opt.success and opt.status == 0 and opt.fun == -fs and opt.nhev == opt.nit + 1 and np.max(np.abs(opt.jac)) < 1e-10
    assert opt.all_x.shape == (1, 9)
    # the bound method is the same density
    den2, dev2 = _density(spec)
    res2 = Laplace(n_sample=32, beta=0.25).run(den2.logp, x0)
    assert dev2.calls[0] == ('pipeline_maximize', 1, False) and np.array_equal(res2.x_max, xs)


def test_gauss_newton_is_passed_through(case):
    from bayesfast_amd.utils import Laplace
    spec, x0, xs, fs, H = case
    den, dev = _density(spec)
    Laplace(n_sample=8, hess_options={'gauss_newton': True}).run(den, x0)
    assert dev.calls == [('pipeline_maximize', 1, True)]
    den, dev = _density(spec)
    Laplace(n_sample=8, hess_options={'step': 1e-3}).run(den, x0)
    assert dev.calls[0] == ('pipeline_maximize', 1, False)


def test_several_starts_are_accepted(case):
    from bayesfast_amd.utils import Laplace
    spec, x0, xs, fs, H = case
    den, dev = _density(spec)
    starts = x0 + 0.05 * np.random.default_rng(3).normal(size=(4, 9))
    res = Laplace(n_sample=8).run(den, starts)
    assert dev.calls[0] == ('pipeline_maximize', 4, False)
    opt = res.opt_result
    assert opt.all_x.shape == (4, 9) and opt.all_fun.shape == (4,) and np.all(opt.all_status == 0)
    best = int(np.argmax(opt.all_fun))
    assert np.array_equal(res.x_max, opt.all_x[best]) and res.f_max == opt.all_fun[best]
    np.testing.assert_allclose(opt.all_x, np.tile(xs, (4, 1)), atol=1e-9)   # one maximum near the starts: the oracle finds it from each


def test_other_methods_and_callables_stay_on_the_host_route(case):
    from bayesfast_amd.utils import Laplace
    spec, x0, xs, fs, H = case
    den, dev = _density(spec)
    res = Laplace(optimize_method='trust-exact', optimize_tol=1e-8, n_sample=8).run(den, x0)
    assert dev.calls == [] and dev.n_logp_and_grad > 0 and not hasattr(res.opt_result, 'all_x')
    assert np.max(np.abs(res.x_max - xs)) <= 1e-6
    with pytest.raises(ValueError, match='invalid value for x_0.'):
        Laplace(optimize_method='trust-exact').run(den, np.zeros((2, 9)))


def test_a_refusal_of_the_device_falls_back_to_the_host_route(case):
    """NotImplementedError from pipeline_maximize (the streamed form): run() answers through scipy, silently, as before."""
    from bayesfast_amd.utils import Laplace, make_positive
    spec, x0, xs, fs, H = case
    den, dev = _density(spec, refuse=True)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = Laplace(optimize_tol=1e-8, n_sample=8).run(den, x0)
    assert dev.calls == [('pipeline_maximize', 1, False)] and dev.n_logp_and_grad > 0
    assert not hasattr(res.opt_result, 'all_x') and res.opt_result.success
    # Newton-CG stops at mean |step| <= 1e-8: inside its convergence region the error after a step is below the step
    assert np.max(np.abs(res.x_max - xs)) <= 9 * 1e-8 + 1e-9
    want = np.linalg.inv(make_positive(-H, 1e5))
    np.testing.assert_allclose(res.cov, want, rtol=1e-6, atol=1e-6 * np.max(np.abs(want)))
    with pytest.raises(ValueError, match='invalid value for x_0.'):   # several starts are the device route's
        Laplace().run(den, np.zeros((2, 9)))


# ---- the seam: the reference's own Recipe under integrate.patch(bf, laplace=True) hands a Chi2PipelineDensity to run() -------------
from oracle import reference  # noqa: E402


@pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')
def test_seam_hands_the_pipeline_density_to_the_device_route(monkeypatch):
    """A model-chi2-prior recipe (the shape of test_integrate_reference.py's DES-shaped one, decay off): one OptimizeStep iteration
    with laplace=False -- the reference's Laplace, its differenced Hessian, scipy's Newton-CG on the recipe's lambdas -- and with
    laplace=True.  Under laplace=True run() reaches pipeline_maximize of the (stand-in) device density; both runs fit the same
    surrogate on the same points, and x_max agrees within 2 r + xtol, r = max |H_fd^-1 g(x_ref)| the reference's own residual Newton
    step taken on the oracle."""
    import oracle_standin
    from bayesfast_amd import integrate
    from bayesfast_amd.core.density import SurrogateDensity
    from oracle import oracle as orc
    bf = reference.load()
    oracle_standin.install(monkeypatch)
    made = []

    def device(self, ctx=None):
        made.append(OraclePipelineLaplaceDensity(self.spec()))
        return made[-1]

    monkeypatch.setattr(SurrogateDensity, 'device', device)
    rng = np.random.default_rng(91)
    d, m = 6, 22
    lo, hi = -1. - rng.uniform(size=d), 1.5 + rng.uniform(size=d)
    para_range = np.stack([lo, hi], 1)
    W1 = rng.normal(size=(m, d)) * 1.5
    x_true = lo + (hi - lo) * rng.uniform(0.4, 0.6, size=d)
    model = lambda x: W1 @ x + 0.05 * np.sin(2. * x[0])
    dvec = model(x_true) + rng.normal(size=m)
    out = {}
    for lap in (False, True):
        unpatch = integrate.patch(bf, laplace=lap)
        try:
            ns = integrate.reference_classes(bf)
            bf.utils.random.set_generator(27)
            bf.utils.parallel.set_backend(1)
            like = ns.GaussianLikelihood(dvec, logp0=-1.5, input_vars='m', output_vars='like')
            post = ns.GaussianPrior(d, indices=[1, 4, 5], mu=x_true[[1, 4, 5]], sigma=[0.3, 0.4, 0.25], c0=0.7, input_vars=['like', 'x'],
                                    output_vars='logp')
            den = bf.Density(density_name='logp', module_list=[bf.Module(fun=model, input_vars='x', output_vars='m'), like, post],
                             input_vars='x', input_shapes=d, input_scales=para_range, hard_bounds=True)
            den.set_decay_options(use_decay=False)
            su = ns.PolyModel('linear', input_size=d, output_size=m, input_vars='x', output_vars='m', input_scales=para_range)
            x_0 = bf.utils.sobol.multivariate_normal(x_true, np.diag(((hi - lo) / 50)**2), 40)
            rec = bf.recipe.Recipe(density=den, optimize=bf.recipe.OptimizeStep(surrogate_list=su, alpha_n=2, x_0=x_0, max_iter=1,
                                                                               run_sampling=False, eps_pp=1e-30, eps_pq=1e-30),
                                   sample=[bf.recipe.SampleStep(surrogate_list=su, alpha_n=2)], post={})
            assert isinstance(rec.recipe_trace._s_optimize.laplace, ns.Laplace) == lap
            made.clear()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                rec._opt_step()
            result = rec.recipe_trace._r_optimize[0]
            den.surrogate_list, den.use_surrogate = result.surrogate_list, True
            out[lap] = (result, [c for dev in made for c in dev.calls], integrate.as_surrogate_density(den).spec())
        finally:
            unpatch()
    assert [c[0] for c in out[True][1]] == ['pipeline_maximize']
    assert out[False][1] == []
    spec = out[False][2]
    assert spec.get('chi2') is not None
    x_ref, x_dev = out[False][0].x_max.x_trans, out[True][0].x_max.x_trans
    _, g = orc.logp_and_grad(spec, x_ref[None], original_space=False)
    Hfd = lc.hess_fd(spec, x_ref)
    r = float(np.max(np.abs(np.linalg.solve(0.5 * (Hfd + Hfd.T), g[0]))))
    err = float(np.max(np.abs(x_dev - x_ref)))
    print('|x_dev - x_ref| %.3g, r %.3g' % (err, r))
    assert err <= 2. * r + 1e-5


def test_only_the_pipeline_maximisers_refusal_falls_back(case):
    """A NotImplementedError from anywhere else on the device route -- a scalar density's maximiser, the gradient at the maximum -- is
    not a refusal of the pipeline maximiser: run() raises it, as it did before the pipeline density had a device route."""
    from bayesfast_amd.core.density import SurrogateDensity
    from bayesfast_amd.utils import Laplace
    spec, x0, xs, fs, H = case

    class _Refusing:
        MAXIMIZE_STATUS = OraclePipelineLaplaceDensity.MAXIMIZE_STATUS

        def maximize(self, *a, **kw):
            raise NotImplementedError('scalar maximiser')

    class _Scalar(SurrogateDensity):
        def __init__(self):
            self._d = 9

        def spec(self):
            return dict(d=9, chi2=None)

        def device(self, ctx=None):
            return _Refusing()

    with pytest.raises(NotImplementedError, match='scalar maximiser'):
        Laplace(n_sample=8).run(_Scalar(), x0)
    den, dev = _density(spec)
    dev.logp_and_grad = lambda *a, **kw: (_ for _ in ()).throw(NotImplementedError('gradient'))
    with pytest.raises(NotImplementedError, match='gradient'):
        Laplace(n_sample=8).run(den, x0)
