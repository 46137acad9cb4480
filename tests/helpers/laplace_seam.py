"""One body for the two seam tests of the Laplace approximation (test_laplace_seam.py: oracle stand-ins, no GPU;
test_gpu_laplace_seam.py: the real device): the reference's own Recipe (oracle/_ref) under ``integrate.patch(bf, laplace=...)``."""
import os
import warnings

import numpy as np

import laplace_cases as lc

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def donut_recipe_reaches_the_ring(bf, integrate):
    """(a) The donut recipe under patch(bf, laplace=True): finished, and the last four steps on the ring within the bounds of
    test_integrate_reference.py::test_reference_recipe_runs_config1_on_the_seam (same numbers, same fixture).  The optimiser's log
    is not compared: the OptimizeStep's surrogate is linear under a Gaussian link, its maximiser is (nearly) a line."""
    import donut
    unpatch = integrate.patch(bf, laplace=True)
    try:
        ns = integrate.reference_classes(bf)
        z = np.load(os.path.join(HERE, 'golden', 'recipe.npz'))
        rec = donut.build_recipe(bf, poly_model=ns.PolyModel,
                                 likelihood=ns.GaussianLikelihood(donut.A, 2. / donut.B, input_vars='m', output_vars='logp'))
        assert isinstance(rec.recipe_trace._s_optimize.laplace, ns.Laplace)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            rec.run()
        rt = rec.recipe_trace
        assert tuple(rt.finished) == (True, True, True)
        steps = rt.results.sample
        assert len(steps) == 10
        ring = np.array([donut.ring_statistics(r.samples) for r in steps])
        want, got = z['ring'][-4:], ring[-4:]
        assert abs(got[:, 0].mean() - want[:, 0].mean()) < 0.06, (got[:, 0], want[:, 0])
        assert abs(got[:, 1].mean() - want[:, 1].mean()) < 0.05, (got[:, 1], want[:, 1])
        assert got[:, 2].max() < 0.15
    finally:
        unpatch()


D = 6


def _concave_recipe(bf, ns):
    """A 6-d correlated Gaussian behind input scales, a quadratic surrogate, an OptimizeStep of three iterations without sampling."""
    rng = np.random.default_rng(21)
    G = rng.normal(size=(D, D)) / np.sqrt(D)
    P = np.eye(D) + G @ G.T
    mean = 0.4 * rng.normal(size=D)
    ranges = np.stack((mean - 6. - rng.uniform(size=D), mean + 6. + rng.uniform(size=D)), axis=1)

    def logp(x):
        r = np.asarray(x, dtype=np.float64) - mean
        return np.atleast_1d(-0.5 * r @ P @ r)

    bf.utils.random.set_generator(5)
    bf.utils.parallel.set_backend(1)
    den = bf.Density(module_list=[bf.Module(fun=logp, input_vars='x', output_vars='logp')], input_shapes=[D], input_vars='x',
                     density_name='logp', input_scales=ranges, hard_bounds=True)
    den.set_decay_options(use_decay=False)
    su = ns.PolyModel('quadratic', input_size=D, output_size=1, input_vars='x', output_vars='logp', input_scales=ranges)
    x_0 = mean + 1.5 * bf.utils.sobol.multivariate_normal(np.zeros(D), np.eye(D), 4 * su.n_param)
    opt = bf.recipe.OptimizeStep(surrogate_list=su, alpha_n=2, x_0=x_0, max_iter=3, run_sampling=False, eps_pp=1e-30, eps_pq=1e-30)
    sam = bf.recipe.SampleStep(surrogate_list=su, alpha_n=2)   # (a Recipe wants one; only the OptimizeStep is run)
    return bf.recipe.Recipe(density=den, optimize=opt, sample=[sam], post={})


def _count_single_point_calls(monkeypatch):
    """Counts the calls of SurrogateDensity.logp / grad / logp_and_grad (the per-point entry points a host optimiser loops over)."""
    from bayesfast_amd.core.density import SurrogateDensity
    calls = []
    for name in ('logp', 'grad', 'logp_and_grad'):
        real = getattr(SurrogateDensity, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(self, *a, **kw)

        monkeypatch.setattr(SurrogateDensity, name, counted)
    return calls


def concave_recipe_agrees_with_the_reference_route(bf, integrate, monkeypatch):
    """(b) The same recipe's OptimizeStep (the reference's own Recipe._opt_step, three iterations) with laplace=False -- the
    reference's Laplace with its differenced Hessian and scipy's Newton-CG -- and with laplace=True.  Per iteration: x_max agrees
    within 2 r + xtol, r = max |H_fd^-1 g(x_ref)| the reference's own residual Newton step taken on the oracle, and logq_trans
    within max |g(x_ref)| r d; and on the device route Laplace.run makes no single-point logp / grad call on the density."""
    from oracle import oracle as orc
    results = {}
    for lap in (False, True):
        unpatch = integrate.patch(bf, laplace=lap)
        try:
            ns = integrate.reference_classes(bf)
            rec = _concave_recipe(bf, ns)
            assert isinstance(rec.recipe_trace._s_optimize.laplace, ns.Laplace) == lap
            calls = _count_single_point_calls(monkeypatch) if lap else []
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                rec._opt_step()
            results[lap] = (rec.recipe_trace._r_optimize[:3], list(calls), rec)
        finally:
            unpatch()
    ref, dev = results[False][0], results[True][0]
    assert len(ref) == 3 and len(dev) == 3
    assert results[True][1] == [], 'the device route called %r on the density' % (results[True][1],)
    xtol = 1e-5
    rec_ref, rec_dev = results[False][2], results[True][2]
    for i in range(3):
        # r: the reference's own residual Newton step, taken on the oracle on the surrogate the REFERENCE run optimised in iteration i
        spec = integrate.as_surrogate_density(_density_with(rec_ref, ref[i])).spec()
        x_ref, x_dev = ref[i].x_max.x_trans, dev[i].x_max.x_trans
        f_ref, g = orc.logp_and_grad(spec, x_ref[None], original_space=False)
        Hfd = lc.hess_fd(spec, x_ref)
        r = float(np.max(np.abs(np.linalg.solve(0.5 * (Hfd + Hfd.T), g[0]))))
        err = float(np.max(np.abs(x_dev - x_ref)))
        # Iteration 0 fits both runs on the same points: one surrogate.  Later iterations refit on each run's own Laplace samples, so
        # the two surrogates differ by their fits; the target is exactly quadratic, so both fits recover it to the rounding of the
        # least-squares solve.  That difference is measured on the oracle (both surrogates at x_ref) and must be rounding-sized:
        # eps x cond(design) with cond up to 1e6, i.e. below 1e-9 of the value's scale.
        spec_dev = integrate.as_surrogate_density(_density_with(rec_dev, dev[i])).spec()
        f_dev_at_ref, _ = orc.logp_and_grad(spec_dev, x_ref[None], original_space=False)
        d_fit = abs(float(f_dev_at_ref[0]) - float(f_ref[0]))
        assert d_fit <= 1e-9 * max(1., abs(float(f_ref[0])))
        d_q = abs(dev[i].f_max.logq_trans - ref[i].f_max.logq_trans)
        print('iteration %d: |x_dev - x_ref| %.3g, r %.3g; |delta logq_trans| %.3g, surrogates differ by %.3g' % (i, err, r, d_q, d_fit))
        assert err <= 2. * r + xtol
        assert d_q <= float(np.max(np.abs(g))) * r * D + d_fit + 1e-12


def _density_with(rec, result):
    """The recipe's Density with the surrogate list of one OptimizeStep iteration in use."""
    den = rec.density
    den.surrogate_list = result.surrogate_list
    den.use_surrogate = True
    return den


def plain_patch_keeps_the_reference_laplace(bf, integrate):
    """(c) Under plain patch(bf) the Laplace the recipe uses is the reference's own object and class."""
    ref_cls = bf.utils.laplace.Laplace
    unpatch = integrate.patch(bf)
    try:
        ns = integrate.reference_classes(bf)
        assert bf.core.recipe.Laplace is ref_cls and bf.utils.Laplace is ref_cls
        mine = ref_cls(beta=3.)
        step = bf.recipe.OptimizeStep(surrogate_list=ns.PolyModel('linear', input_size=2, output_size=1), laplace=mine)
        assert step.laplace is mine and type(step.laplace) is ref_cls
        assert type(bf.recipe.OptimizeStep().laplace) is ref_cls
        assert bf.core.recipe.Recipe._opt_surro.__module__.endswith('core.recipe')
        # the seam's subclass is accepted by OptimizeStep as well (it IS a reference Laplace)
        assert isinstance(bf.recipe.OptimizeStep(laplace=ns.Laplace(beta=2.)).laplace, ref_cls)
    finally:
        unpatch()
    assert bf.core.recipe.Laplace is ref_cls
