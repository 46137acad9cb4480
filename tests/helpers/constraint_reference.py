"""Extended-precision reference of the constraint transform and of a quadratic density behind it (TEST INFRASTRUCTURE ONLY).

Written from the definitions with mpmath at 60 digits (420 where the logistic kind's 1 - t cancels); shares no code with ``bayesfast_amd`` or ``oracle``.  A coordinate with the
range (lo, hi), rg = hi - lo, and the hard-bound flags (lower, upper) maps the sampler's coordinate x to the model's coordinate T(x):

    kind 0  (0, 0)   T = lo + rg x
    kind 1  (1, 1)   T = lo + rg / (1 + exp(-x))
    kind 2  (1, 0)   T = lo + rg exp(x)
    kind 3  (0, 1)   T = lo + rg (1 - exp(x))

``to_original`` returns T, T', T''; ``from_original`` the inverse map and its first two derivatives; ``log_jac`` returns log|T'| and
its first two derivatives.  ``logp_grad_hess`` evaluates logp(x) = f(T(x)) + sum_i log|T_i'(x_i)| for a spec whose surrogate is a plain
quadratic (bound test and decay term off or out of reach -- asserted), with its gradient and Hessian.
"""
import mpmath as mp
import numpy as np

DPS = 60
# the logistic kind is evaluated as its definition states it, 1 - t included: at |x| = 745 that difference is 1e-324, so the
# definition needs 324 digits and more to leave 60 good ones
DPS_LOGISTIC = 420

# where the probes sit (the logistic kind's cancellation sets in at x of a few tens; from 37 the naive 1 - t is zero)
PROBES_TWO_SIDED = [s * v for v in (12., 20., 30., 36.5, 37.5, 40., 300., 700.) for s in (1., -1.)]
PROBES_ONE_SIDED = [-700., -300., -40., -12., 3.]


def kinds_of(hard_bounds):
    hb = np.asarray(hard_bounds).astype(bool)
    return np.where(hb[:, 0] & hb[:, 1], 1, np.where(hb[:, 0], 2, np.where(hb[:, 1], 3, 0)))


def _f(v):
    return mp.mpf(float(v))


def to_original(x, kind, lo, hi):
    """(T, T', T'') at x as mpf."""
    with mp.workdps(DPS):
        x, lo, hi = _f(x), _f(lo), _f(hi)
        rg = hi - lo
        if kind == 1:
            with mp.workdps(DPS_LOGISTIC):
                t = 1 / (1 + mp.exp(-x))
                return lo + rg * t, rg * t * (1 - t), rg * t * (1 - t) * (1 - 2 * t)
        if kind == 2:
            e = mp.exp(x)
            return lo + rg * e, rg * e, rg * e
        if kind == 3:
            e = mp.exp(x)
            return lo + rg * (1 - e), -rg * e, -rg * e
        return lo + rg * x, rg, mp.mpf(0)


def from_original(xo, kind, lo, hi):
    """(x, dx/dT, d2x/dT2) at T = xo as mpf; the caller keeps xo strictly inside the bounds."""
    with mp.workdps(DPS):
        xo, lo, hi = _f(xo), _f(lo), _f(hi)
        rg = hi - lo
        t = (xo - lo) / rg
        if kind == 1:
            return mp.log(t) - mp.log(1 - t), 1 / (t * (1 - t)) / rg, (2 * t - 1) / (t * (1 - t))**2 / rg**2
        if kind == 2:
            return mp.log(t), 1 / t / rg, -1 / t**2 / rg**2
        if kind == 3:
            return mp.log(1 - t), -1 / (1 - t) / rg, -1 / (1 - t)**2 / rg**2
        return t, 1 / rg, mp.mpf(0)


def log_jac(x, kind, lo, hi):
    """(log|T'|, d/dx, d2/dx2) at x as mpf."""
    with mp.workdps(DPS):
        x, lo, hi = _f(x), _f(lo), _f(hi)
        lrg = mp.log(abs(hi - lo))
        if kind == 1:
            # log t + log(1 - t) with t = 1 / (1 + exp(-x)): -log(1 + e^-x) - log(1 + e^x)
            with mp.workdps(DPS_LOGISTIC):
                t = 1 / (1 + mp.exp(-x))
                return lrg - mp.log(1 + mp.exp(-x)) - mp.log(1 + mp.exp(x)), 1 - 2 * t, -2 * t * (1 - t)
        if kind in (2, 3):
            return lrg + x, mp.mpf(1), mp.mpf(0)
        return lrg, mp.mpf(0), mp.mpf(0)


def _quadratic_of(spec):
    """c0, lin (d,), symmetric S (d, d) as object arrays of mpf: f(u) = c0 + lin.u + u^T S u / 2 in the surrogate's input u."""
    d = int(spec['d'])
    poly = spec['poly']
    assert int(poly['output_size']) == 1 and spec.get('link') is None and spec.get('chi2') is None
    c0 = mp.mpf(0)
    lin = np.array([mp.mpf(0)] * d, dtype=object)
    S = np.array([[mp.mpf(0)] * d for _ in range(d)], dtype=object)
    for cf in poly['configs']:
        im = np.asarray(cf['input_mask'])
        coef = np.asarray(cf['coef'], dtype=np.float64)
        if cf['order'] == 'linear':
            c0 += _f(coef[0, 0])
            for a, i in enumerate(im):
                lin[i] += _f(coef[0, 1 + a])
        else:
            assert cf['order'] == 'quadratic', 'the reference is a plain quadratic'
            for a, i in enumerate(im):
                for b, j in enumerate(im):
                    if b >= a and coef[0, a, b] != 0.:   # f has the term coef[a, b] u_i u_j for a <= b only
                        S[i, j] += _f(coef[0, a, b])
                        S[j, i] += _f(coef[0, a, b])
    return c0, lin, S


def logp_grad_hess(spec, x, want_hess=True):
    """x (n, d) float64 -> logp (n,), grad (n, d), hess (n, d, d) (or None) of the transformed density, rounded to float64 from 60 digits.
    Asserts that every point lies inside the surrogate's bound and the decay term's ellipsoid, so the density IS the quadratic."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n, d = x.shape
    assert d == int(spec['d'])
    tr = spec.get('ranges') is not None
    kinds = kinds_of(spec['hard_bounds']) if tr else np.zeros(d, int)
    rgs = np.asarray(spec['ranges'], dtype=np.float64) if tr else None
    su = spec.get('su_lo') is not None
    logp, grad = np.empty(n), np.empty((n, d))
    hess = np.empty((n, d, d)) if want_hess else None
    with mp.workdps(DPS):
        c0, lin, S = _quadratic_of(spec)
        sdiff = np.array([_f(v) if su else mp.mpf(1) for v in (spec['su_diff'] if su else np.ones(d))], dtype=object)
        slo = np.array([_f(v) if su else mp.mpf(0) for v in (spec['su_lo'] if su else np.zeros(d))], dtype=object)
        poly = spec['poly']
        if poly.get('use_bound'):
            bmu = np.array([_f(v) for v in np.asarray(poly['mu']).reshape(d)], dtype=object)
            bH = np.array([[_f(v) for v in row] for row in np.asarray(poly['hess']).reshape(d, d)], dtype=object)
        for p in range(n):
            T = np.empty(d, dtype=object)
            J = np.empty(d, dtype=object)
            J2 = np.empty(d, dtype=object)
            lj = np.empty((d, 3), dtype=object)
            for i in range(d):
                if tr:
                    T[i], J[i], J2[i] = to_original(x[p, i], kinds[i], rgs[i, 0], rgs[i, 1])
                    lj[i] = log_jac(x[p, i], kinds[i], rgs[i, 0], rgs[i, 1])
                else:
                    T[i], J[i], J2[i] = _f(x[p, i]), mp.mpf(1), mp.mpf(0)
                    lj[i] = (mp.mpf(0), mp.mpf(0), mp.mpf(0))
            u = (T - slo) / sdiff
            if poly.get('use_bound'):
                um = u - bmu
                beta2 = um.dot(bH.dot(um))
                assert beta2 < _f(poly['alpha'])**2, 'point %d lies outside the surrogate bound: the reference is only the quadratic' % p
            if spec.get('use_decay'):
                dm = T - np.array([_f(v) for v in np.asarray(spec['decay_mu']).reshape(d)], dtype=object)
                dH = np.array([[_f(v) for v in row] for row in np.asarray(spec['decay_hess']).reshape(d, d)], dtype=object)
                assert dm.dot(dH.dot(dm)) < _f(spec['decay_alpha2']), 'point %d is in the decay term\'s reach' % p
            Su = S.dot(u)
            f = c0 + lin.dot(u) + u.dot(Su) / 2
            a = J / sdiff        # du/dx
            b = J2 / sdiff       # d2u/dx2
            fu = lin + Su        # df/du
            logp[p] = float(f + sum(lj[:, 0]))
            g = fu * a + lj[:, 1]
            grad[p] = [float(v) for v in g]
            if want_hess:
                for i in range(d):
                    for j in range(d):
                        h = a[i] * S[i, j] * a[j]
                        if i == j:
                            h += fu[i] * b[i] + lj[i, 2]
                        hess[p, i, j] = float(h)
    return logp, grad, hess


def narrow_bounded_spec(d, input_scales=None, lo=-1., hi=2., seed=123):
    """``correlated_gaussian_spec(d)`` behind the transform with the narrow range (lo, hi) on every coordinate, the hard-bound kinds
    cycling two-sided / lower / upper / none, and the surrogate's bound moved out of reach (alpha = 1e30: the bound test stays in the
    kernels' path, every point is inside).  With ``input_scales`` the surrogate takes u = (T - su_lo) / su_diff: 'folded' has scales near
    the range, which the upload folds into the polynomial's coefficients; 'kept' has them 40 widths from the origin, which stay a
    step of the kernels (``device.folds_input_scales``)."""
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, _ = correlated_gaussian_spec(d, seed=seed)
    spec = dict(spec, poly=dict(spec['poly'], alpha=1e30))
    spec['ranges'] = np.tile(np.array([[lo, hi]], dtype=np.float64), (d, 1))
    spec['hard_bounds'] = np.array([[1, 1], [1, 0], [0, 1], [0, 0]], dtype=np.uint8)[np.arange(d) % 4]
    if input_scales:
        assert input_scales in ('folded', 'kept')
        rng = np.random.default_rng(seed + 1)
        spec['su_lo'] = (-0.5 if input_scales == 'folded' else -60.) + 0.1 * rng.normal(size=d)
        spec['su_diff'] = 1.5 + 0.2 * rng.uniform(size=d)
    return spec


def probe_points(spec, n, seed=5, limit=700., mix_lanes=False, up_rows=None):
    """n points: coordinates from N(0, 0.3^2), with two probe coordinates per point pinned to the values of PROBES_* (|value| <= limit)
    for the coordinate's kind, walking through all of them.  ``mix_lanes`` pins every bounded coordinate among the first eight at once
    on half of the points, so probes of different kinds sit on neighbouring lanes of one wave.  ``up_rows``: the only points that may
    carry the one-sided kinds' positive probe (elsewhere the walk skips it)."""
    d = int(spec['d'])
    kinds = kinds_of(spec['hard_bounds'])
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.normal(size=(n, d))
    two = [v for v in PROBES_TWO_SIDED if abs(v) <= limit]
    one = [v for v in PROBES_ONE_SIDED if abs(v) <= limit]
    k = [0, 0, 0, 0]   # one walk through the probe values per kind
    for p in range(n):
        dims = range(min(d, 8)) if (mix_lanes and p % 2) else [(3 * p) % d, (3 * p + 5) % d]
        for i in dims:
            vals = two if kinds[i] == 1 else one
            if kinds[i]:
                v = vals[k[kinds[i]] % len(vals)]
                if kinds[i] > 1 and v > 0. and up_rows is not None and p not in up_rows:
                    k[kinds[i]] += 1
                    v = vals[k[kinds[i]] % len(vals)]
                x[p, i] = v
                k[kinds[i]] += 1
    return x


def probes_covered(spec, x, limit=700.):
    """every probe value of every kind occurs somewhere in x"""
    kinds = kinds_of(spec['hard_bounds'])
    ok = True
    for kind, vals in ((1, PROBES_TWO_SIDED), (2, PROBES_ONE_SIDED), (3, PROBES_ONE_SIDED)):
        seen = set(np.asarray(x)[:, kinds == kind].ravel().tolist())
        ok = ok and all(v in seen for v in vals if abs(v) <= limit)
    return ok
