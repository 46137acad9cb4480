"""Device copies follow the host state they were built from.  Three objects keep a device copy and decide for themselves when it
is stale: ``SIT`` (its rotations, ``_rotations_on_device``), ``PolyModel`` (``device_model``) and ``SurrogateDensity``
(``device``).  Every kernel test elsewhere fits an object once and evaluates it; here objects are refitted, or their options
changed, AFTER the device copy exists, and the results are compared with fp64 references evaluated on the object's CURRENT host
state: the oracle for the surrogates and densities, and for SIT a host composition of its own arrays with the oracle's splines
(tests/helpers/sit_host.py), plus a fresh object built from the same arrays.

CPU tests (no GPU) pin the invalidation contract with stand-ins for the device objects; the GPU tests run the real kernels."""
import copy
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))


def _same(a, b):
    """Nested specs (dicts / lists of arrays and scalars) equal value for value."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b))


def _laplace_mix(rng, n, d, scale=1.):
    """Rotated Laplace / uniform / cubed-normal columns: non-Gaussian, so FastICA has directions to find."""
    s = np.stack([rng.laplace(size=n) if k % 3 == 0 else (rng.uniform(-1, 1, size=n) if k % 3 == 1 else rng.normal(size=n)**3)
                  for k in range(d)], 1)
    return scale * s @ (np.eye(d) + 0.4 * rng.normal(size=(d, d))) + rng.normal(size=d)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the invalidation contract, with recording stand-ins for the device objects
# ---------------------------------------------------------------------------------------------------------------------

class _RecordingPolyModel:
    """``DevicePolyModel`` answered by the oracle on a snapshot of the spec it was built from."""
    built = []

    def __init__(self, poly, ctx=None):
        from oracle_standin import _CpuCtx
        self.poly, self.ctx = copy.deepcopy(poly), _CpuCtx()
        _RecordingPolyModel.built.append(self.poly)

    def fun_and_jac(self, x, jac=True):
        import torch
        from oracle import oracle as orc
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
        f, j = orc.poly_fun_and_jac(self.poly, np.atleast_2d(x).reshape(-1, self.poly['input_size']))
        return torch.from_numpy(f), (torch.from_numpy(j) if jac else None)


def _recording_density():
    from oracle_standin import OracleDensity

    class _RecordingDensity(OracleDensity):
        built = []

        def __init__(self, spec, ctx=None):
            super().__init__(copy.deepcopy(spec), ctx)
            _RecordingDensity.built.append(self.spec)
    return _RecordingDensity


def _host_fitted_polymodel(rng, d=3, m=2):
    """A quadratic PolyModel with the bound on, 'fitted' on the host: coefficients through ``PolyConfig._set`` and the bound through
    ``_bound_stats`` / ``_apply_bound`` (the device evaluation it needs is the stand-in's)."""
    from bayesfast_amd import PolyModel
    pm = PolyModel('quadratic', input_size=d, output_size=m)
    for c in pm.configs:
        for q in range(c.output_size):
            c._set(rng.normal(size=c._a_shape), q)
    xf = rng.normal(size=(60, d))
    pm._apply_bound(*pm._bound_stats(xf, rng.normal(size=60)))
    return pm


def test_polymodel_device_model_is_rebuilt_after_bound_options_and_set(monkeypatch):
    """``set_bound_options`` (alpha, use_bound) and ``PolyConfig._set`` after an evaluation: the next evaluation runs on a device model
    built from the current ``poly_spec()`` (the cache key used to be the coefficient array's id, which in-place writes keep)."""
    import bayesfast_amd.device as dev
    from oracle import oracle as orc
    monkeypatch.setattr(dev, 'DevicePolyModel', _RecordingPolyModel)
    _RecordingPolyModel.built = []
    rng = np.random.default_rng(3)
    pm = _host_fitted_polymodel(rng)
    x = rng.normal(size=(25, 3)) * 4.                 # (most of them beyond the bound)

    def check():
        f, j = pm.fun_and_jac_batch(x)
        assert _same(_RecordingPolyModel.built[-1], pm.poly_spec())
        f0, j0 = orc.poly_fun_and_jac(pm.poly_spec(), x)
        np.testing.assert_allclose(f.numpy(), f0, rtol=1e-13, atol=0)
        np.testing.assert_allclose(j.numpy(), j0, rtol=1e-13, atol=0)
        return f.numpy()

    f_first = check()
    n = len(_RecordingPolyModel.built)
    pm.fun_and_jac_batch(x)
    assert len(_RecordingPolyModel.built) == n        # (no change, no rebuild)
    alpha = 0.5 * pm.bound_options.alpha
    pm.set_bound_options(alpha=alpha)
    assert not np.allclose(check(), f_first)
    pm.set_bound_options(use_bound=False)
    assert pm.poly_spec()['use_bound'] is False
    check()
    pm.set_bound_options(use_bound=True, alpha=alpha)   # (set_bound_options resets alpha: given again)
    check()
    c = pm.configs[1]
    c._set(rng.normal(size=c._a_shape), 1)             # in place: the same coefficient array
    check()
    pm._apply_bound(*pm._bound_stats(rng.normal(size=(60, 3)) * 2., rng.normal(size=60)))
    check()
    # the resolved bound is part of the key: the device model of poly_spec(use_bound=False) is another model
    pm.device_model(use_bound=False)
    assert _RecordingPolyModel.built[-1]['use_bound'] is False
    check()


def test_surrogate_density_device_follows_changes_made_through_its_surrogate(monkeypatch):
    """``SurrogateDensity.device()`` after ``density.surrogate.set_bound_options`` or a coefficient change made on the surrogate
    itself: rebuilt from the current ``density.spec()``, and ``logp_and_grad`` is the oracle's on that spec."""
    import bayesfast_amd.device as dev
    from bayesfast_amd import SurrogateDensity
    from oracle import oracle as orc
    Rec = _recording_density()
    monkeypatch.setattr(dev, 'DevicePolyModel', _RecordingPolyModel)
    monkeypatch.setattr(dev, 'DeviceDensity', Rec)
    rng = np.random.default_rng(4)
    den = SurrogateDensity(_host_fitted_polymodel(rng, d=3, m=1))
    x = rng.normal(size=(20, 3)) * 4.

    def check():
        lp, g = den.logp_and_grad(x)
        assert _same(Rec.built[-1], den.spec())
        lp0, g0 = orc.logp_and_grad(den.spec(), x, original_space=True)
        np.testing.assert_allclose(lp, lp0, rtol=1e-13, atol=0)
        np.testing.assert_allclose(g, g0, rtol=1e-13, atol=0)
        return lp

    lp_first = check()
    n = len(Rec.built)
    den.logp_and_grad(x)
    assert len(Rec.built) == n
    den.surrogate.set_bound_options(alpha=0.4 * den.surrogate.bound_options.alpha)
    assert not np.allclose(check(), lp_first)
    den.surrogate.set_bound_options(use_bound=False)
    check()
    c = den.surrogate.configs[0]
    c._set(rng.normal(size=c._a_shape), 0)
    check()
    den.set_decay_options(use_decay=False, gamma=0.2)  # (the density's own options: dropped as before)
    check()


class _ScaleTable:
    """A stand-in for an iteration's ``SplineTable``: coordinate j maps y -> a_j y."""

    def __init__(self, a):
        import torch
        self.a = torch.as_tensor(a)

    def apply(self, mode, y):
        import torch
        return {'evaluate': y * self.a, 'derivative': torch.ones_like(y) * self.a, 'solve': y / self.a}[mode]


def _host_sit(monkeypatch):
    """SIT on CPU tensors: ``_ctx`` a CPU context, FastICA and the spline construction replaced by seeded stand-ins (a random
    orthogonal unmixing, a random scale per coordinate) -- what the fit does with their results is SIT's own code."""
    from oracle_standin import _CpuCtx
    from bayesfast_amd.transforms import SIT
    ctx = _CpuCtx()
    monkeypatch.setattr(SIT, '_ctx', lambda self: ctx)

    def ica(self, x):
        d = int(x.shape[1])
        q, _ = np.linalg.qr(self.random_generator.normal(size=(d, d)))
        return q, x.mean(0).numpy()

    monkeypatch.setattr(SIT, '_ica', ica)
    monkeypatch.setattr(SIT, '_gaussianize', lambda self, y: _ScaleTable(self.random_generator.uniform(0.5, 2., size=int(y.shape[1]))))
    return SIT


def _host_forward(sit, x):
    y, log_j = np.array(x), np.zeros(len(x))
    for i in range(sit.i_iter):
        y = (y - sit._m[i]) @ sit._A[i].T
        a = sit._tables[i].a.numpy()
        log_j += np.sum(np.log(a))
        y = y * a
    return y, log_j + np.sum(sit._logdetA)


def test_sit_rotation_cache_follows_refits(monkeypatch):
    """``SIT._rotations_on_device`` after a refit on new data of the same ``n_iter`` (the same ``i_iter``, the cache's key), on data
    of another dimension, and after a continued fit (``fit(n_run=1)``: the cache grows with ``i_iter``): the device copies are the
    current ``_m``, ``A.T``, ``B.T``, and the transforms use them."""
    SIT = _host_sit(monkeypatch)
    rng = np.random.default_rng(0)
    sit = SIT(n_iter=2, random_generator=1)

    def check(pts):
        m, At, Bt = sit._rotations_on_device()
        assert len(m) == len(At) == len(Bt) == sit.i_iter
        for i in range(sit.i_iter):
            np.testing.assert_array_equal(m[i].numpy(), sit._m[i])
            np.testing.assert_array_equal(At[i].numpy(), sit._A[i].T)
            np.testing.assert_array_equal(Bt[i].numpy(), sit._B[i].T)
        y, lj = sit.forward_transform(pts)
        y0, lj0 = _host_forward(sit, pts)
        np.testing.assert_allclose(y, y0, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(lj, lj0, rtol=1e-13, atol=1e-13)
        x, _ = sit.backward_transform(y)
        np.testing.assert_allclose(x, pts, rtol=0, atol=1e-11)

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sit.fit(_laplace_mix(rng, 500, 5))
        check(rng.normal(size=(30, 5)))
        sit.fit(_laplace_mix(rng, 500, 5, scale=3.))
        assert sit.i_iter == 2
        check(rng.normal(size=(30, 5)))
        sit.fit(n_run=1)
        assert sit.i_iter == 3
        check(rng.normal(size=(30, 5)))
        sit.fit(_laplace_mix(rng, 500, 4, scale=0.5))   # 5 -> 4
        assert sit.i_iter == 3 and sit.dim == 4
        check(rng.normal(size=(30, 4)))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernels on refitted objects
# ---------------------------------------------------------------------------------------------------------------------

def _check_sit(sit, pts, n_s):
    """Every transform of the SIT (host and device entry points) against the host composition of its current arrays (1e-10
    relative) and against a fresh SIT built from those arrays (1e-11 absolute)."""
    import torch
    import sit_host
    from bayesfast_amd.transforms import SIT
    p = sit_host.parts(sit)
    fresh = SIT._from_parts(*p)
    ctx = sit._ctx()
    lq = sit.logq(pts)
    y, lj = sit.forward_transform(pts)
    ys = sit.sample(n_s)[2]                             # the Sobol-normal points that sample() and _sample_device transform
    xb, ljb = sit.backward_transform(ys)
    xs = sit.sample(n_s)[0]
    lq_d = sit._logq_device(ctx.tensor(pts)).cpu().numpy()
    xs_d = sit._sample_device(n_s)
    assert isinstance(xs_d, torch.Tensor)
    xs_d = xs_d.cpu().numpy()
    # the host composition of the current arrays
    y0, lj0 = sit_host.forward(p, pts)
    xb0, ljb0 = sit_host.backward(p, ys)
    lq0 = sit_host.logq(p, pts)
    for got, want in ((lq, lq0), (lq_d, lq0), (y, y0), (lj, lj0), (xb, xb0), (ljb, ljb0), (xs, xb0), (xs_d, xb0)):
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
    # a fresh object from the same arrays
    yf, ljf = fresh.forward_transform(pts)
    xbf, ljbf = fresh.backward_transform(ys)
    for got, want in ((lq, fresh.logq(pts)), (lq_d, fresh._logq_device(ctx.tensor(pts)).cpu().numpy()), (y, yf), (lj, ljf),
                      (xb, xbf), (ljb, ljbf), (xs, fresh.sample(n_s)[0]), (xs_d, fresh._sample_device(n_s).cpu().numpy())):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-11)


@pytest.mark.gpu
def test_sit_refit_uses_the_new_rotations():
    """fit(x1), evaluate (the rotation cache fills), then fit(x2) with the same n_iter -- another scale and rotation, then another
    dimension (5 -> 4) -- and a continued fit (``fit(n_run=1)``): logq, forward / backward transforms, sample() and the device entry
    points are those of the current model."""
    from bayesfast_amd.transforms import SIT
    from bayesfast_amd.device import get_context
    ctx = get_context(0)
    rng = np.random.default_rng(31)
    sit = SIT(n_iter=2, random_generator=7)
    pts5, pts4 = rng.normal(size=(40, 5)), rng.normal(size=(40, 4))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sit.fit(_laplace_mix(rng, 4000, 5))
        sit.logq(pts5)
        sit._sample_device(64)
        _check_sit(sit, pts5, 200)
        sit.fit(_laplace_mix(rng, 4000, 5, scale=2.5))
        assert sit.i_iter == 2
        _check_sit(sit, pts5, 200)
        sit.fit(n_run=1)
        assert sit.i_iter == 3
        _check_sit(sit, pts5, 200)
        sit.fit(ctx.tensor(_laplace_mix(rng, 4000, 4, scale=0.4)))   # (the device-tensor branch of fit)
        assert sit.i_iter == 3 and sit.dim == 4
        _check_sit(sit, pts4, 200)


def _gaussian(d, seed):
    rng = np.random.default_rng(seed)
    L = np.tril(rng.normal(size=(d, d)) * 0.3) + np.diag(rng.uniform(0.5, 2., size=d))
    cov = L @ L.T
    return cov, np.linalg.inv(cov), rng.normal(size=d)


@pytest.mark.gpu
def test_gbs_run_twice_on_one_object_is_a_fresh_gbs():
    """Two ``GBS.run`` calls on one object, the second on samples of another Gaussian (host route: arrays; device route: the TraceTuple
    of ``sample()`` with a SurrogateDensity's logp): the second log-evidence is that of a fresh GBS whose SIT starts from the same
    generator state, and recovers the analytic normaliser within its error."""
    import bayesfast_amd as bfa
    from bayesfast_amd.evidence import GBS
    d, c0 = 6, -2.5
    rng = np.random.default_rng(8)

    def exact(cov):
        return c0 + 0.5 * d * np.log(2 * np.pi) + 0.5 * np.linalg.slogdet(cov)[1]

    def logp_of(prec, mu):
        return lambda x: c0 - 0.5 * np.einsum('...i,ij,...j->...', x - mu, prec, x - mu)

    (cov1, prec1, mu1), (cov2, prec2, mu2) = _gaussian(d, 1), _gaussian(d, 2)
    # host route
    x1 = rng.normal(size=(4, 3000, d)) @ np.linalg.cholesky(cov1).T + mu1
    x2 = rng.normal(size=(4, 3000, d)) @ np.linalg.cholesky(cov2).T * 1. + mu2
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = GBS(sit=dict(n_iter=4, random_generator=5), n_q=8000)
        g.run(x1, logp_of(prec1, mu1))
        state = copy.deepcopy(g.sit.random_generator)
        logz, err = g.run(x2, logp_of(prec2, mu2))
        logz_f, err_f = GBS(sit=dict(n_iter=4, random_generator=state), n_q=8000).run(x2, logp_of(prec2, mu2))
    assert abs(logz - logz_f) < 1e-9 and abs(err - err_f) < 1e-9 * err_f, (logz, logz_f)
    assert 0. < err < 0.1
    assert abs(logz - exact(cov2)) < 3. * err + 0.02, (logz, err, exact(cov2))
    # device route: quadratic surrogates of the two Gaussians, NUTS, the TraceTuples straight to GBS
    tts, dens = [], []
    for k, (cov, prec, mu) in enumerate(((cov1, prec1, mu1), (cov2, prec2, mu2))):
        su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
        den = bfa.SurrogateDensity(su)
        xf = rng.normal(size=(4 * su.n_param, d)) @ np.linalg.cholesky(cov).T * 1.6 + mu
        den.fit(xf, logp_of(prec, mu)(xf))
        tts.append(bfa.sample(den, {'n_chain': 16, 'n_iter': 1200, 'n_warmup': 400, 'random_generator': 4 + k}, verbose=False))
        dens.append(den)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        g = GBS(sit=dict(n_iter=4, random_generator=6), n_q=8000)
        g.run(tts[0], dens[0].logp)
        state = copy.deepcopy(g.sit.random_generator)
        logz, err = g.run(tts[1], dens[1].logp)
        logz_f, err_f = GBS(sit=dict(n_iter=4, random_generator=state), n_q=8000).run(tts[1], dens[1].logp)
    assert abs(logz - logz_f) < 1e-9 and abs(err - err_f) < 1e-9 * err_f, (logz, logz_f)
    assert 0. < err < 0.1
    assert abs(logz - exact(cov2)) < 3. * err + 0.02, (logz, err, exact(cov2))


def _fitted_multi_output(rng, d, m):
    """A quadratic multi-output PolyModel fitted with the bound on (alpha from alpha_p = 100: the farthest fit point)."""
    from bayesfast_amd import PolyModel
    pm = PolyModel('quadratic', input_size=d, output_size=m)
    xf = rng.normal(size=(3 * pm.n_param, d))
    Q = rng.normal(size=(m, d, d)) * 0.3
    yf = np.einsum('ni,kij,nj->nk', xf, Q, xf) + xf @ rng.normal(size=(d, m)) + 0.05 * np.sum(xf**3, 1)[:, None]
    pm.fit(xf, yf, logp=yf[:, 0])
    return pm


@pytest.mark.gpu
def test_polymodel_evaluation_follows_bound_options_and_coefficients():
    """After ``fun_and_jac_batch`` beyond the bound: ``set_bound_options(alpha=...)``, ``use_bound=False``, ``PolyConfig._set`` of
    the second config, and a refit -- each time the batched kernel (and the scalar entry points) against the oracle on the current
    ``poly_spec()``; the same through ``Chi2PipelineDensity.logp_and_grad_device`` and its fused ``logp_and_grad``."""
    from bayesfast_amd import Chi2PipelineDensity
    from oracle import oracle as orc
    rng = np.random.default_rng(41)
    d, m = 5, 3
    pm = _fitted_multi_output(rng, d, m)
    den = Chi2PipelineDensity(pm, rng.normal(size=m), prec_diag=rng.uniform(0.5, 2., size=m))
    x = rng.normal(size=(48, d)) * 2.5
    spec = pm.poly_spec()
    beta = np.sqrt(np.einsum('ij,jk,ik->i', x - spec['mu'], spec['hess'], x - spec['mu']))
    assert (beta > spec['alpha']).sum() > 10

    def check():
        f, j = pm.fun_and_jac_batch(x)
        f0, j0 = orc.poly_fun_and_jac(pm.poly_spec(), x)
        np.testing.assert_allclose(f.cpu().numpy(), f0, rtol=1e-11, atol=1e-11 * np.abs(f0).max())
        np.testing.assert_allclose(j.cpu().numpy(), j0, rtol=1e-10, atol=1e-10 * np.abs(j0).max())
        f1, j1 = pm.fun_and_jac(x[7])
        np.testing.assert_allclose(f1[0], f0[7], rtol=1e-11, atol=1e-11 * np.abs(f0).max())
        lp0, g0 = orc.logp_and_grad(den.spec(), x)
        lpd, gd = den.logp_and_grad_device(x)
        np.testing.assert_allclose(lpd.cpu().numpy(), lp0, rtol=1e-11, atol=1e-10)
        np.testing.assert_allclose(gd.cpu().numpy(), g0, rtol=1e-10, atol=1e-10 * np.abs(g0).max())
        lp, g = den.logp_and_grad(x)
        np.testing.assert_allclose(lp, lp0, rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(g, g0, rtol=1e-9, atol=1e-9 * np.abs(g0).max())
        return f0

    f_first = check()
    alpha = 0.5 * pm.bound_options.alpha
    pm.set_bound_options(alpha=alpha)
    assert not np.allclose(check(), f_first)
    pm.set_bound_options(use_bound=False)
    check()
    pm.set_bound_options(use_bound=True, alpha=alpha)   # (set_bound_options resets alpha: given again)
    check()
    c = pm.configs[1]
    for q in range(c.output_size):
        c._set(rng.normal(size=c._a_shape) * 0.2, q)
    check()
    xf = rng.normal(size=(3 * pm.n_param, d)) * 1.5
    yf = np.sin(xf[:, :m]) + 0.1 * xf[:, ::-1][:, :m]**2
    pm.fit(xf, yf, logp=yf[:, 0])
    check()


@pytest.mark.gpu
def test_surrogate_density_sample_follows_changes_made_through_its_surrogate():
    """``density.device()`` built, then ``density.surrogate.set_bound_options(...)`` and a direct refit of ``density.surrogate``:
    ``logp_and_grad`` is the oracle's on the current ``density.spec()``, and ``sample()`` (64 chains) takes the first draws
    ``oracle.nuts_run_many`` takes on that spec."""
    from bayesfast_amd import PolyModel, SurrogateDensity, sample, NTrace
    from oracle import oracle as orc
    d = 5
    rng = np.random.default_rng(51)
    _, prec, mu = _gaussian(d, 3)

    def logp(x):
        return -0.5 * np.einsum('...i,ij,...j->...', x - mu, prec, x - mu) - 0.03 * np.sum((x - mu)**3, -1)

    den = SurrogateDensity(PolyModel('cubic-2', input_size=d, output_size=1))
    xf = rng.normal(size=(3 * den.surrogate.n_param, d)) + mu
    den.fit(xf, logp(xf))
    x = rng.normal(size=(40, d)) * 3. + mu
    x0 = rng.normal(size=(64, d)) * 2.5 + mu

    def check(seed):
        lp, g = den.logp_and_grad(x)
        lp0, g0 = orc.logp_and_grad(den.spec(), x, original_space=True)
        np.testing.assert_allclose(lp, lp0, rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(g, g0, rtol=1e-9, atol=1e-9 * np.abs(g0).max())
        tt = sample(den, NTrace(n_chain=64, n_iter=240, n_warmup=120, x_0=x0, random_generator=seed), verbose=False)
        so, sto, _ = orc.nuts_run_many(den.spec(), x0, tt._trace.seed(), 240, 120)
        k = 6
        assert np.array_equal(tt.stat('tree_size')[:, :k].astype(int), sto['tree_size'][:, :k].astype(int))
        np.testing.assert_allclose(tt.samples[:, :k], so[:, :k], rtol=1e-8, atol=1e-8)
        return lp0

    lp_first = check(3)
    den.surrogate.set_bound_options(alpha=0.3 * den.surrogate.bound_options.alpha)
    assert not np.allclose(check(4), lp_first)
    xf2 = rng.normal(size=(3 * den.surrogate.n_param, d)) * 1.3 + mu
    den.surrogate.fit(xf2, (logp(xf2) + 0.5 * xf2[:, 0])[:, None], logp(xf2))
    check(5)


@pytest.mark.gpu
def test_polar_ns_on_a_second_device():
    """``bfhip_polar_ns`` at d = 128 (the form that holds X in LDS: its dynamic LDS size is above the default limit, an attribute of the
    kernel on each device) on device 0, then on device 1: the orthogonal polar factor on both."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two visible GPUs: the LDS attribute is per device (%d visible)' % torch.cuda.device_count())
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context, _ptr
    d = 128
    rng = np.random.default_rng(d)
    A = rng.normal(size=(d, d)) * 0.03 + np.diag(rng.uniform(0.05, 2., size=d))
    u, s, vt = np.linalg.svd(A)
    for dev in (0, 1):
        ctx = get_context(dev)
        a = ctx.tensor(A)
        work = torch.empty(2 * d * d + 80, dtype=torch.float64, device=a.device)
        x = torch.empty_like(a)
        _lib.check(ctx._lib.bfhip_polar_ns(ctx.handle, d, _ptr(a), _ptr(x), 60, _ptr(work), _ptr(work[-1:])))
        x = x.cpu().numpy()
        assert float(work[-1]) < 1e-13, dev
        np.testing.assert_allclose(x, u @ vt, rtol=0, atol=5e-13 * s.max() / s.min())
        np.testing.assert_allclose(x @ x.T, np.eye(d), rtol=0, atol=1e-13)
