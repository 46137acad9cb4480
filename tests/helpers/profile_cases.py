"""Independent references of the profile tests (test_profile_host.py, test_gpu_profile.py).

The profile objective is the ORIGINAL-space density parametrised by the sampling coordinates, F(x) = logp_orig(T(x)).  Here it is
the oracle's ``logp_and_grad(original_space=True)`` composed with the constraint transform written in NumPy (laplace_cases), and its
conditional maxima come from a damped Newton iteration on the free coordinates with the Hessian of the free block by differences
of that gradient, in the manner of ``laplace_cases.oracle_newton``.  Nothing in this file calls the code under test."""
import numpy as np

from oracle import oracle as orc

import laplace_cases as lc


def transform_jacobian(spec, x):
    """dT_i/dx_i of the constraint transform at the sampling coordinates x (..., d)."""
    x = np.asarray(x, dtype=np.float64)
    if spec.get('ranges') is None:
        return np.ones_like(x)
    rg = spec['ranges'][:, 1] - spec['ranges'][:, 0]
    hb = np.asarray(spec['hard_bounds'] if spec.get('hard_bounds') is not None else np.zeros((x.shape[-1], 2)), dtype=bool)
    both, lower, upper = hb[:, 0] & hb[:, 1], hb[:, 0] & ~hb[:, 1], ~hb[:, 0] & hb[:, 1]
    with np.errstate(all='ignore'):
        s = 1. / (1. + np.exp(-x))
        dt = np.where(both, s * (1. - s), np.where(lower, np.exp(x), np.where(upper, -np.exp(x), 1.)))
    return dt * rg


def log_jacobian(spec, x):
    """sum_i log|T'_i(x_i)|"""
    return np.sum(np.log(np.abs(transform_jacobian(spec, x))), axis=-1)


def objective(spec, x, original=True):
    """F (n,) and dF/dx (n, d) at the sampling coordinates x (n, d): the oracle in the original space, chained through T; with
    ``original=False`` the sampling-space density itself (the other objective of the profile calls)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if not original:
        return orc.logp_and_grad(spec, x, original_space=False)
    f, g = orc.logp_and_grad(spec, lc.to_original(spec, x), original_space=True)
    return f, g * transform_jacobian(spec, x)


def _free_hess(spec, x, free, h, original=True):
    """(4 D(h) - D(2 h)) / 3 of the objective's gradient on the free block, D the central difference."""
    idx = np.flatnonzero(free)

    def central(step):
        pts = np.repeat(x[None], 2 * idx.size, axis=0)
        pts[np.arange(idx.size), idx] += step
        pts[idx.size + np.arange(idx.size), idx] -= step
        g = objective(spec, pts, original)[1][:, idx]
        return ((g[:idx.size] - g[idx.size:]) / (2. * step)).T
    H = (4. * central(h) - central(2. * h)) / 3.
    return 0.5 * (H + H.T)


def conditional_max(spec, x0, fixed, max_iter=100, gtol=1e-11, h=1e-3, original=True):
    """argmax of F over the coordinates with fixed == 0, the others held at x0: (x, F(x), max |dF/dx| over the free ones)."""
    x = np.array(x0, dtype=np.float64)
    free = ~np.asarray(fixed, dtype=bool)
    nf = int(free.sum())

    def fg(z):
        f, g = objective(spec, z[None], original)
        return float(f[0]), g[0][free]

    f, g = fg(x)
    if nf == 0:
        return x, f, 0.
    for _ in range(max_iter):
        if np.max(np.abs(g)) <= gtol:
            break
        A = -_free_hess(spec, x, free, h, original)
        lam, lam0 = 0., 1e-3 * max(float(np.max(np.abs(np.diag(A)))), 1e-300)
        for _ in range(60):
            try:
                L = np.linalg.cholesky(A + lam * np.eye(nf))
                step = np.linalg.solve(L.T, np.linalg.solve(L, g))
                xt = x.copy()
                xt[free] += step
                ft, gt = fg(xt)
                if np.isfinite(ft) and ft >= f - 1e-13 * max(1., abs(f)):
                    break
            except np.linalg.LinAlgError:
                pass
            lam = lam0 if lam == 0. else 10. * lam
        else:
            break
        x, f, g = xt, ft, gt
        if np.sum(np.abs(step)) / nf < 1e-15:
            break
    return x, f, float(np.max(np.abs(g)))


def reference_line(spec, fixed, walk, x_start, values, original=True):
    """The line of ``bfhip_profile_lines`` by the reference: for every value the conditional maximum, started from the one before.
    -> x (n_val, d), F (n_val,), max |gradient| over the free coordinates (n_val,)."""
    prev = np.array(x_start, dtype=np.float64)
    xs, fs, gs = [], [], []
    for v in ([None] if walk < 0 else values):
        s = prev.copy()
        if walk >= 0:
            s[walk] = v
        prev, f, g = conditional_max(spec, s, fixed, original=original)
        xs.append(prev)
        fs.append(f)
        gs.append(g)
    return np.array(xs), np.array(fs), np.array(gs)


def on_a_kink(spec, x):
    """Whether the point x lies within 5 % of the decay term's surface beta_d^2 = alpha_2.  The term is gamma max(beta_d^2 - alpha_2, 0):
    its gradient jumps across the surface, so a conditional maximum that the ramp pushes back onto the surface is a point where the
    density is not differentiable.  No gradient criterion holds there -- the reference iteration above alternates between the two
    sides -- and the device iteration reports such a point as status 3 (short but damped).  The tests keep their lines off it, as
    laplace_cases.keep_off_the_kinks keeps the Hessian's points off it; test_profile_host.py pins what happens on it."""
    if not spec.get('use_decay'):
        return False
    rd = lc.bound_ratio(spec, np.asarray(x)[None], False)[1][0]
    return bool(abs(rd - 1.) <= 0.05)


def check_line(spec, res, fixed, walk, x_start, values, xtol, original=True):
    """One line of a result dict (x (n_val, d), logp (n_val,), info (n_val, 4) as NumPy arrays) against reference_line, with the
    tolerances of the maximiser's tests at EVERY value: status 0, mean |x - x*| <= xtol over the free coordinates, the value to 1e-9
    relative; fixed coordinates keep their bits.  A condition on the inputs, asserted first: no reference optimum of the line lies
    on the decay term's kink (on_a_kink) -- the caller chooses its values accordingly -- and the reference converged at every one.
    Prints every figure before it asserts; returns the iteration counts."""
    fixed = np.asarray(fixed, dtype=bool)
    free = ~fixed
    xr, fr, gr = reference_line(spec, fixed, walk, x_start, values, original)
    assert not any(on_a_kink(spec, xk) for xk in xr), 'a reference optimum lies on the decay surface: choose other values'
    assert np.all(gr < 1e-9), 'the reference did not converge: %s' % gr
    for k in range(len(fr)):
        dx = float(np.sum(np.abs(res['x'][k][free] - xr[k][free])) / max(1, int(free.sum())))
        df = (float(res['logp'][k]) - fr[k]) / max(1., abs(fr[k]))
        print('walk %d value %d: status %d, iterations %d, mean |x - x*| %.3g (xtol %.3g), value off by %.3g relative'
              % (walk, k, res['info'][k, 1], res['info'][k, 0], dx, xtol, df))
        assert res['info'][k, 1] == 0
        assert dx <= xtol
        assert abs(df) <= 1e-9
        want = np.array(x_start, dtype=np.float64)
        if walk >= 0:
            want[walk] = values[k]
        assert np.array_equal(res['x'][k][fixed].view(np.uint64), want[fixed].view(np.uint64))
    return res['info'][:, 0]


def masks(d, rng):
    """Three masks of fixed coordinates and a walk coordinate in each: one fixed, two fixed, d - 1 fixed."""
    out = []
    for n_fixed in (1, 2, d - 1) if d > 2 else (1, 1, 1):
        idx = np.sort(rng.choice(d, n_fixed, replace=False))
        m = np.zeros(d, dtype=bool)
        m[idx] = True
        out.append((m, int(idx[rng.integers(n_fixed)])))
    return out


def linear_gaussian_spec(m=40, d=9, seed=2):
    """A pipeline with LINEAR outputs (nq = 0), no transform, the bound far away, unit precision and the diagonal Gaussian prior: the
    posterior is a Gaussian.  -> (spec, mean, covariance), the two from the spec's coefficients: f = c + A x,
    logp = -|f - y|^2 / 2 - sum_i prec_i (x_i - mu_i)^2 / 2 + const."""
    from bayesfast_amd.workloads import random_pipeline_spec
    spec = random_pipeline_spec(m, d, 0, seed=seed, bound=False, transform=False)
    assert spec['ranges'] is None and spec['su_lo'] is None
    lin = [c for c in spec['poly']['configs'] if c['order'] == 'linear'][0]['coef']
    c, A = lin[:, 0], lin[:, 1:]
    assert np.array_equal(np.asarray(spec['chi2']['prec_diag']), np.ones(m))
    pmu, pprec = np.asarray(spec['prior']['mu']), np.asarray(spec['prior']['prec_diag'])
    cov = np.linalg.inv(A.T @ A + np.diag(pprec))
    mean = cov @ (A.T @ (np.asarray(spec['chi2']['y']) - c) + pprec * pmu)
    return spec, mean, cov


def spec_density(spec, ctx):
    """A Chi2PipelineDensity front of a pipeline spec -- the package's class with its device density built from the spec -- that
    ``sample`` takes: the constraint transform's settings are the spec's."""
    from bayesfast_amd.core.density import Chi2PipelineDensity
    from bayesfast_amd.device import DeviceDensity

    class _SpecDensity(Chi2PipelineDensity):
        def __init__(self):
            self._dev = DeviceDensity(spec, ctx)
            self._d = spec['d']
            self._input_scales = None if spec.get('ranges') is None else np.ascontiguousarray(spec['ranges'], dtype=np.float64)
            self._hard_bounds = None if spec.get('hard_bounds') is None else np.ascontiguousarray(spec['hard_bounds'], dtype=np.uint8)

        def spec(self):
            return spec

        def device(self, ctx=None):
            return self._dev

    return _SpecDensity()
