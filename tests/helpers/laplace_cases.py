"""Inputs and independent references of the Laplace tests (test_laplace_host.py, test_gpu_laplace.py, the seam tests).

Everything expected here comes from the CPU oracle (``oracle.logp_and_grad``): the reference Hessian is a fourth-order central
difference of the ORACLE's gradient, the reference maximum a damped Newton iteration on the oracle.  Nothing in this file calls
the code under test."""
import numpy as np

from oracle import oracle as orc


# ---- the independent Hessian ---------------------------------------------------------------------------------------------------
def _central(spec, x, original_space, h):
    """D(h)_ij = (g_i(x + h_j e_j) - g_i(x - h_j e_j)) / 2 h_j from one batch of 2 d oracle gradients."""
    d = x.size
    pts = np.concatenate((x + np.diag(h), x - np.diag(h)))
    _, g = orc.logp_and_grad(spec, pts, original_space=original_space)
    return ((g[:d] - g[d:]) / (2. * h)[:, None]).T


def hess_fd(spec, x, original_space=False, scale=None, h=1e-3):
    """H_fd(h) = (4 D(h) - D(2 h)) / 3, steps h in units of each coordinate's scale."""
    x = np.asarray(x, dtype=np.float64)
    hv = h * (np.ones(x.size) if scale is None else np.asarray(scale, dtype=np.float64))
    return (4. * _central(spec, x, original_space, hv) - _central(spec, x, original_space, 2. * hv)) / 3.


def hess_fd_with_tol(spec, x, original_space=False, scale=None, h=1e-3):
    """(H_fd(h), tolerance): 10 x max |H_fd(h) - H_fd(h / 10)|, the reference's own error measured on the oracle (the factor covers
    the smaller step's rounding error, which the difference underestimates), plus 1e-12 d max|H| for the rounding of the code
    under test.  A tolerance above 1e-7 max|H| would hide a wrong term: then the step is wrong for the case, and this asserts."""
    H = hess_fd(spec, x, original_space, scale, h)
    H10 = hess_fd(spec, x, original_space, scale, h / 10.)
    hmax = float(np.max(np.abs(H)))
    tol = 10. * float(np.max(np.abs(H - H10)))
    assert tol <= 1e-7 * hmax, 'the difference step does not suit this case: %g > 1e-7 x %g' % (tol, hmax)
    return H, tol + 1e-12 * x.size * hmax


def jacobian_is_asymmetric(spec, original_space):
    """The decay term's gradient carries no transform Jacobian (core/density.py:745), so in the sampling space the Jacobian of the
    gradient is not symmetric where the decay term is on; the Hessian is its symmetric part there (as the reference's Laplace
    takes it, utils/laplace.py:162-164)."""
    return bool(spec.get('use_decay')) and spec.get('ranges') is not None and not original_space


# ---- constraint transform (transforms/_constraint.pyx) in numpy, for building test points ----------------------------------------
def from_original(spec, xo):
    xo = np.asarray(xo, dtype=np.float64)
    if spec.get('ranges') is None:
        return xo.copy()
    lo, rg = spec['ranges'][:, 0], spec['ranges'][:, 1] - spec['ranges'][:, 0]
    hb = np.asarray(spec['hard_bounds'] if spec.get('hard_bounds') is not None else np.zeros((xo.shape[-1], 2)), dtype=bool)
    t = (xo - lo) / rg
    both, lower, upper = hb[:, 0] & hb[:, 1], hb[:, 0] & ~hb[:, 1], ~hb[:, 0] & hb[:, 1]
    with np.errstate(all='ignore'):
        return np.where(both, np.log(t / (1. - t)), np.where(lower, np.log(t), np.where(upper, np.log(1. - t), t)))


def to_original(spec, x):
    x = np.asarray(x, dtype=np.float64)
    if spec.get('ranges') is None:
        return x.copy()
    lo, rg = spec['ranges'][:, 0], spec['ranges'][:, 1] - spec['ranges'][:, 0]
    hb = np.asarray(spec['hard_bounds'] if spec.get('hard_bounds') is not None else np.zeros((x.shape[-1], 2)), dtype=bool)
    both, lower, upper = hb[:, 0] & hb[:, 1], hb[:, 0] & ~hb[:, 1], ~hb[:, 0] & hb[:, 1]
    with np.errstate(all='ignore'):
        t = np.where(both, 1. / (1. + np.exp(-x)), np.where(lower, np.exp(x), np.where(upper, 1. - np.exp(x), x)))
    return lo + t * rg


def bound_ratio(spec, x, original_space):
    """beta / alpha of the polynomial's bound and beta_d / alpha_d of the decay term at the points x (nan where the term is off)."""
    xo = np.atleast_2d(x) if original_space else to_original(spec, np.atleast_2d(x))
    po = spec['poly']
    rb = rd = np.full(xo.shape[0], np.nan)
    if po.get('use_bound'):
        xs = (xo - spec['su_lo']) / spec['su_diff'] if spec.get('su_lo') is not None else xo
        xm = xs - po['mu']
        rb = np.einsum('ni,ij,nj->n', xm, po['hess'], xm)**0.5 / po['alpha']
    if spec.get('use_decay'):
        xm = xo - spec['decay_mu']
        rd = (np.einsum('ni,ij,nj->n', xm, spec['decay_hess'], xm) / spec['decay_alpha2'])**0.5
    return rb, rd


# ---- the feature matrix --------------------------------------------------------------------------------------------------------
FEATURES = {
    # name: cubic, decay (1 its own matrix, 2 the bound's arrays), transform, su (1 folded at upload, 2 kept as a device-side step), link
    'quadratic': dict(),
    'cubic': dict(cubic=1),
    'su_folded': dict(su=1),
    'su_kept': dict(su=2),
    'su_kept_cubic': dict(su=2, cubic=1),
    'transform': dict(transform=1),
    'decay_own': dict(decay=1),
    'decay_shared': dict(decay=2),
    'link': dict(link=1),
    'transform_decay_link': dict(transform=1, decay=1, link=1),
    'everything': dict(cubic=1, decay=1, transform=1, su=2, link=1),
}


def feature_spec(d, name, seed=0):
    """(spec, scale_original, scale_sampling, points_original (n, d)): a random single-output surrogate density with the features of
    FEATURES[name]; the points lie inside and outside the bound and the decay ellipsoid, one of them between the two surfaces, and
    strictly inside the hard bounds (keep_off_the_kinks drops any that come within 5 % of a surface)."""
    ft = dict(cubic=0, decay=0, transform=0, su=0, link=0)
    ft.update(FEATURES[name])
    rng = np.random.default_rng(1000 * d + 7 * seed + sum(ord(c) for c in name))
    # negative definite quadratic part (a log density), random linear part
    G = rng.normal(size=(d, d)) / np.sqrt(d)
    P = np.eye(d) + 0.3 * (G + G.T) + G @ G.T
    quad = np.triu(-0.5 * P * (2. - np.eye(d)))
    cfgs = [dict(order='linear', input_mask=np.arange(d), output_mask=np.arange(1), coef=0.3 * rng.normal(size=(1, d + 1))),
            dict(order='quadratic', input_mask=np.arange(d), output_mask=np.arange(1), coef=quad[None])]
    if ft['cubic']:   # masked cubic-2 and cubic-3 configs, the shape of the planck-like workload (workloads.py)
        n2, n3 = min(d, 5), min(d, 6)
        m2, m3 = np.sort(rng.choice(d, n2, replace=False)), np.sort(rng.choice(d, n3, replace=False))
        cfgs.append(dict(order='cubic-2', input_mask=m2, output_mask=np.arange(1), coef=0.05 * rng.normal(size=(1, n2, n2))))
        if n3 >= 3:
            a3 = np.zeros((1, n3, n3, n3))
            for j in range(n3):
                for k in range(j + 1, n3):
                    for l in range(k + 1, n3):
                        a3[0, j, k, l] = 0.05 * rng.normal()
            cfgs.append(dict(order='cubic-3', input_mask=m3, output_mask=np.arange(1), coef=a3))
    xs_fit = rng.normal(size=(40 * d + 40, d))
    poly = dict(input_size=d, output_size=1, configs=cfgs, use_bound=False)
    poly.update(orc.set_bound(poly, xs_fit, rng.normal(size=xs_fit.shape[0]), dict(alpha_p=80.)))
    spec = dict(d=d, poly=poly, ranges=None, hard_bounds=None, su_lo=None, su_diff=None, use_decay=False, link=None)
    lo, diff = np.zeros(d), np.ones(d)
    if ft['su']:
        diff = rng.uniform(0.7, 1.5, size=d)
        lo = rng.normal(size=d) * 0.1 if ft['su'] == 1 else (40. + 10. * rng.uniform(size=d)) * diff * rng.choice([-1., 1.], size=d)
        spec['su_lo'], spec['su_diff'] = lo, diff
    xo_fit = lo + diff * xs_fit
    if ft['decay'] == 2:   # the bound's own centre and matrix, bit for bit (the usual case); the radius is set below
        assert not ft['su']
        spec.update(orc.set_decay(xs_fit, alpha_p=90.))
        assert np.array_equal(spec['decay_hess'], poly['hess']) and np.array_equal(spec['decay_mu'], poly['mu'])
    elif ft['decay']:
        spec.update(orc.set_decay(np.mean(xo_fit, axis=0) + 0.7 * (xo_fit - np.mean(xo_fit, axis=0)) + 0.05 * diff, alpha_p=90.))
    if ft['transform']:   # all four kinds: both bounds, lower only, upper only, none
        spec['ranges'] = np.stack((lo - diff * (4.5 + rng.uniform(size=d)), lo + diff * (4.5 + rng.uniform(size=d))), axis=1)
        hb = np.zeros((d, 2), np.uint8)
        kind = np.arange(d) % 4
        hb[kind == 0] = 1
        hb[kind == 1, 0] = 1
        hb[kind == 2, 1] = 1
        spec['hard_bounds'] = hb
    if ft['link']:
        spec['link'] = dict(kind='gaussian', y=0.3, prec=0.7, logp0=-1.2)
    # points at chosen beta / alpha of the bound along random directions (the pairs 0.7 / 0.85 and 1.3 / 1.6 on one ray each), kept
    # strictly inside the hard bounds.  The decay surface is then laid BETWEEN the two points of a pair, so that the two C^1
    # surfaces are told apart: its own ellipsoid between 0.7 and 0.85 (inside the bound, decay on), the shared one between 1.3 and
    # 1.6 (outside the bound, decay off).
    mu, Hb, alpha = np.asarray(poly['mu']), np.asarray(poly['hess']), float(poly['alpha'])
    rays = [rng.normal(size=d) for _ in range(4)]
    rays = [z / np.sqrt(z @ Hb @ z) for z in rays]
    ratios = ((0.4, 0), (0.7, 1), (0.85, 1), (1.3, 2), (1.6, 2), (2.5, 3))
    xs_pts = np.array([np.clip(mu + rho * alpha * rays[k], -4.2, 4.2) for rho, k in ratios])
    pts = lo + diff * xs_pts
    if ft['decay']:
        pair = pts[[3, 4]] if ft['decay'] == 2 else pts[[1, 2]]
        xm = pair - spec['decay_mu']
        bd = np.einsum('ni,ij,nj->n', xm, spec['decay_hess'], xm)**0.5
        assert bd[1] > 1.15 * bd[0]
        spec['decay_alpha2'] = float(bd[0] * bd[1])
    return spec, np.std(xo_fit, axis=0), np.std(from_original(spec, np.clip(xo_fit, lo - 4. * diff, lo + 4. * diff)), axis=0), pts


def covers_both_sides(spec, rb, rd):
    """Whether the kept points exercise every branch the spec has: inside and outside the bound; with a decay term also inside and
    outside its ellipsoid, and at least one point that lies on different sides of the two surfaces."""
    ok = bool(np.any(rb > 1.) and np.any(rb < 1.))
    if spec.get('use_decay'):
        ok = ok and bool(np.any(rd > 1.) and np.any(rd < 1.) and np.any((rb > 1.) != (rd > 1.)))
    return ok


def keep_off_the_kinks(spec, x, original_space):
    """The rows of x at least 5 % off both C^1 surfaces (a condition on the inputs: no stencil may straddle a kink)."""
    rb, rd = bound_ratio(spec, x, original_space)
    ok = np.ones(len(x), dtype=bool)
    for r in (rb, rd):
        ok &= np.isnan(r) | (np.abs(r - 1.) > 0.05)
    return ok, rb, rd


# ---- the independent maximiser -------------------------------------------------------------------------------------------------
def oracle_newton(spec, x0, scale=None, max_iter=100, gtol=1e-12):
    """A damped Newton iteration on the oracle in the sampling space: Hessian by hess_fd, Levenberg damping while -H + lambda I does
    not factor or the step does not ascend.  Runs until |grad|_inf <= gtol (or the step stalls); returns (x, logp, grad, n_iter)."""
    x = np.array(x0, dtype=np.float64)
    d = x.size

    def fg(z):
        f, g = orc.logp_and_grad(spec, z[None], original_space=False)
        return float(f[0]), g[0]

    f, g = fg(x)
    it = 0
    for it in range(max_iter):
        if np.max(np.abs(g)) <= gtol:
            break
        H = hess_fd(spec, x, False, scale)
        A = -0.5 * (H + H.T)
        lam, lam0 = 0., 1e-3 * max(float(np.max(np.abs(np.diag(A)))), 1e-300)
        for _ in range(60):
            try:
                L = np.linalg.cholesky(A + lam * np.eye(d))
                if np.min(np.diag(L))**2 <= 1e-12 * np.max(np.abs(np.diag(A))):
                    raise np.linalg.LinAlgError   # numerically singular: a step along its null space is noise
                step = np.linalg.solve(L.T, np.linalg.solve(L, g))
                ft, gt = fg(x + step)
                if np.isfinite(ft) and ft >= f - 1e-13 * max(1., abs(f)):
                    break
            except np.linalg.LinAlgError:
                pass
            lam = lam0 if lam == 0. else 10. * lam
        else:
            break
        x, f, g = x + step, ft, gt
        if np.sum(np.abs(step)) / d < 1e-15:
            break
    return x, f, g, it


def t2_spec(d, kind='quadratic'):
    """The maximiser's test densities: ``correlated_gaussian_spec(d)`` behind hard bounds [-3, 5] on every coordinate (the Hessian is
    indefinite at the start x_0 = default_rng(3).normal(size=d)); 'cubic' adds masked cubic terms, 'decay' a decay term of its own."""
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, _ = correlated_gaussian_spec(d)
    spec = dict(spec, ranges=np.tile(np.array([-3., 5.]), (d, 1)), hard_bounds=np.ones((d, 2), np.uint8), link=None)
    rng = np.random.default_rng(17)
    if kind == 'cubic':
        n2, n3 = 5, 6
        m2, m3 = np.sort(rng.choice(d, n2, replace=False)), np.sort(rng.choice(d, n3, replace=False))
        a3 = np.zeros((1, n3, n3, n3))
        for j in range(n3):
            for k in range(j + 1, n3):
                for l in range(k + 1, n3):
                    a3[0, j, k, l] = 0.02 * rng.normal()
        po = dict(spec['poly'])
        po['configs'] = list(po['configs']) + [
            dict(order='cubic-2', input_mask=m2, output_mask=np.arange(1), coef=0.02 * rng.normal(size=(1, n2, n2))),
            dict(order='cubic-3', input_mask=m3, output_mask=np.arange(1), coef=a3)]
        spec['poly'] = po
    elif kind == 'decay':
        po = spec['poly']
        spec.update(use_decay=True, decay_mu=np.asarray(po['mu']) + 0.05, decay_hess=np.asarray(po['hess']),
                    decay_alpha2=(0.25 * float(po['alpha']))**2, decay_gamma=0.1)
    return spec, np.random.default_rng(3).normal(size=d)
