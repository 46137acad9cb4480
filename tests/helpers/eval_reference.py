"""Extended-precision reference of the stand-alone density evaluation and of one leapfrog step (TEST INFRASTRUCTURE ONLY).

``logp_and_grad`` restates ``Density.logp_and_grad`` for a density spec (the dict ``DeviceDensity`` takes, single-output surrogate) in
``numpy.longdouble``, from the formulas of the reference:

- polynomial and the linear extrapolation outside the bound: modules/poly.py:466-503;
- cubic kernels: modules/_poly.pyx:49-137 (quadratic ones: :13-43);
- input scaling, link, decay, transform: core/module.py:76-83, 226; core/density.py:503-507, 552-560, 724-754;
- constraint transform: transforms/_constraint.pyx:133-215, the logistic kind on the side where nothing cancels (a = exp(-|x|),
  s = 1 / (1 + a): t = s or a s, J = a s^2 rg, J'' / J = -+(1 - a) s, log|J| = -|x| + log(s^2 |rg|)) -- the mathematically exact
  form, where the reference's t (1 - t) loses digits from |x| of a few tens.

``leapfrog`` restates ``CpuLeapfrogIntegrator._step`` with a diagonal metric (samplers/hmc_utils/integration.py:68-95, metrics.py:88-91).

It imports neither the package under test nor the C oracle.

Every value comes with its SCALE: the same formula with every term replaced by its magnitude.  The class ``V`` carries the pair
(value v, magnitude m >= |v|) through the arithmetic.  A sum of terms takes the sum of their magnitudes and a product of two terms
the product of theirs; where a factor is itself a sum that cancels (m > |v|), its excess m - |v| goes on to first order, as the
rounding error it stands for does:

    input          m = |v|
    a +- b         m = m_a + m_b
    a b            m = |a| m_b + m_a |b| - |a b|                    (= |a| |b| for two plain terms)
    a / b          m = m_a / |b| + |a| m_b / b^2 - |a / b|
    sqrt(a)        m = (sqrt(a) + m_a / sqrt(a)) / 2
    exp(a)         m = exp(a) (1 + m_a - |a|)
    log(a)         m = |log a| + (m_a - |a|) / |a|
    M x            m = |M| m_x

so that the rounding error of a float64 evaluation, in whatever order it sums, is a small multiple of 2^-52 m.  (Multiplying the
magnitudes themselves at every product compounds: behind a kept input scaling, (x - lo) / diff with |lo| of 50 widths, then the
quadratic, then the link's square, m came out 1e10 times the value, and the comparison could no longer see a coefficient wrong
by 1e-9 -- test_eval_reference_host.py checks exactly that.)  The magnitude runs through the extrapolation
(coef = (f0 - f_mu) / alpha - j0 . (x - mu) / beta cancels: its m does not), the link, the decay term and the Jacobian; in the
leapfrog step the end point's m is that of q + eps var (p + eps g / 2), so the density's sensitivity to the rounding of its own
argument is part of the scale.  logp has one scale per point, vectors the largest over a point's components.
"""
import numpy as np

LD = np.longdouble
EPS = 2.**-52


class V:
    """(value, magnitude) arrays in longdouble; see the module docstring for the rules."""
    __slots__ = ('v', 'm')

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=LD)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=LD)

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(o)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.m)

    def __mul__(self, o):
        o = V.of(o)
        a, b = np.abs(self.v), np.abs(o.v)
        return V(self.v * o.v, a * o.m + self.m * b - a * b)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        a, b = np.abs(self.v), np.abs(o.v)
        return V(self.v / o.v, self.m / b + a * o.m / (b * b) - a / b)

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __getitem__(self, k):
        return V(self.v[k], self.m[k])

    def sum(self, axis=-1):
        return V(self.v.sum(axis=axis), self.m.sum(axis=axis))

    def abs(self):
        return V(np.abs(self.v), self.m)


def vexp(a):
    e = np.exp(a.v)
    return V(e, e * (1 + a.m - np.abs(a.v)))


def vlog(a):
    l = np.log(a.v)
    return V(l, np.abs(l) + (a.m - np.abs(a.v)) / np.abs(a.v))


def vsqrt(a):
    r = np.sqrt(a.v)
    with np.errstate(divide='ignore', invalid='ignore'):
        return V(r, np.where(r > 0, 0.5 * (r + a.m / r), 0))


def vwhere(c, a, b):
    a, b = V.of(a), V.of(b)
    return V(np.where(c, a.v, b.v), np.where(c, a.m, b.m))


def matvec(M, x):
    """y_i = sum_k M[i, k] x_k for every row of x (n, d); M exact."""
    M = np.asarray(M, dtype=LD)
    return V(x.v @ M.T, x.m @ np.abs(M).T)


def kinds_of(hard_bounds, d):
    hb = np.zeros((d, 2), bool) if hard_bounds is None else np.asarray(hard_bounds).astype(bool)
    return np.where(hb[:, 0] & hb[:, 1], 1, np.where(hb[:, 0], 2, np.where(hb[:, 1], 3, 0)))


def constraint(x, kinds, ranges):
    """The constraint transform of x (n, d) as V: (T(x), J = T', log|J| per coordinate, J'' / J); _constraint.pyx:133-215."""
    x = V.of(x)
    rg = V(ranges[:, 1]) - V(ranges[:, 0])
    lo = V(ranges[:, 0])
    ax = x.abs()
    arg = vwhere(kinds == 1, -ax, x)
    a = vexp(arg)
    s = 1 / (1 + a)
    a_s = a * s
    one, zero = V(np.ones_like(x.v)), V(np.zeros_like(x.v))
    lrg = vlog(rg.abs())
    # kind 0: T = lo + rg x
    t, jt, gj, lj = x, one, zero, lrg + zero
    # kind 1: t = 1 / (1 + exp(-x)); J = rg t (1 - t); J'' / J = 1 - 2 t; log|J| = log t + log(1 - t) + log|rg|
    k = kinds == 1
    g1 = (1 - a) * s
    t = vwhere(k, vwhere(x.v >= 0, s, a_s), t)
    jt = vwhere(k, a_s * s, jt)
    gj = vwhere(k, vwhere(x.v >= 0, -g1, g1), gj)
    lj = vwhere(k, vlog(s * s * rg.abs()) - ax, lj)
    # kind 2: T = lo + rg exp(x);  kind 3: T = lo + rg (1 - exp(x))
    k = kinds == 2
    t, jt = vwhere(k, a, t), vwhere(k, a, jt)
    k = kinds == 3
    t, jt = vwhere(k, 1 - a, t), vwhere(k, -a, jt)
    k = kinds >= 2
    gj, lj = vwhere(k, one, gj), vwhere(k, x + lrg, lj)
    return lo + t * rg, jt * rg, lj, gj


def _poly(poly, x):
    """sum over the configs of PolyModel (poly.py:470-477), single output: f (n,), j (n, d) as V.  x: V (n, d)."""
    n, d = x.v.shape
    f = V(np.zeros(n))
    jv, jm = np.zeros((n, d), LD), np.zeros((n, d), LD)

    def scatter(mask, g):
        jv[:, mask] += g.v
        jm[:, mask] += g.m

    for cf in poly['configs']:
        mask = np.asarray(cf['input_mask'], dtype=np.int64)
        c = np.asarray(cf['coef'], dtype=np.float64)[0]
        xi = x[:, mask]
        k = mask.size
        if cf['order'] == 'linear':       # poly.py:340-352: column 0 is the constant
            f = f + ((xi * V(c[1:])).sum() + float(c[0]))
            scatter(mask, V(np.broadcast_to(c[1:], (n, k))))
        elif cf['order'] == 'quadratic':  # _poly.pyx:13-43: only j <= k is defined
            U = np.triu(c)
            f = f + (matvec(U, xi) * xi).sum()
            scatter(mask, matvec(U + U.T, xi))
        elif cf['order'] == 'cubic-2':    # _poly.pyx:49-80: f = sum_j x_j^2 (A x)_j
            t = matvec(c, xi)
            f = f + (t * xi * xi).sum()
            scatter(mask, 2. * xi * t + matvec(c.T, xi * xi))
        elif cf['order'] == 'cubic-3':    # _poly.pyx:86-137: f = sum_{j<k<l} a_jkl x_j x_k x_l
            gv, gm = np.zeros((n, k), LD), np.zeros((n, k), LD)
            for j in range(k):
                for kk in range(j + 1, k):
                    for l in range(kk + 1, k):
                        a = float(c[j, kk, l])
                        if a == 0.:
                            continue
                        xj, xk, xl = xi[:, j], xi[:, kk], xi[:, l]
                        f = f + a * xj * xk * xl
                        for col, term in ((j, a * xk * xl), (kk, a * xj * xl), (l, a * xj * xk)):
                            gv[:, col] += term.v
                            gm[:, col] += term.m
            scatter(mask, V(gv, gm))
        else:
            raise ValueError(cf['order'])
    return f, V(jv, jm)


def _poly_bounded(poly, x):
    """PolyModel._fun_and_jac with the linear extrapolation outside the alpha-ellipsoid (poly.py:466-503)."""
    f, j = _poly(poly, x)
    all_linear = all(cf['order'] == 'linear' for cf in poly['configs'])
    if not poly.get('use_bound') or all_linear:
        return f, j
    mu, H, alpha, f_mu = V(np.asarray(poly['mu'], np.float64)), np.asarray(poly['hess'], np.float64), float(poly['alpha']), \
        float(np.asarray(poly['f_mu']).reshape(-1)[0])
    xm = x - mu
    beta = vsqrt((matvec(H.T, xm) * xm).sum())        # np.dot(np.dot(x - mu, hess), x - mu)**0.5, :468
    oob = beta.v > alpha
    if not oob.any():
        return f, j
    with np.errstate(divide='ignore', invalid='ignore'):
        b = beta[:, None]
        x0 = vwhere(oob[:, None], (alpha * x + (b - alpha) * mu) / b, x)       # :482
        f0, j0 = _poly(poly, x0)
        fe = (beta * f0 - (beta - alpha) * f_mu) / alpha                        # :487
        gb = matvec(H, xm) / b                                                  # :490
        coef = (f0 - f_mu) / alpha - (j0 * xm).sum() / beta                     # :495
        je = j0 + coef[:, None] * gb                                            # :496
    return vwhere(oob, fe, f), vwhere(oob[:, None], je, j)


def _eval(spec, x, original_space):
    """Density.logp_and_grad (core/density.py:724-754) on x: V (n, d); returns logp V (n,), grad V (n, d)."""
    d = int(spec['d'])
    tr = spec.get('ranges') is not None and not original_space
    if tr:   # density.py:503-507
        xo, J, lj, gj = constraint(x, kinds_of(spec.get('hard_bounds'), d), np.asarray(spec['ranges'], np.float64))
    else:
        xo = x
    su = spec.get('su_lo') is not None
    xs = (xo - V(np.asarray(spec['su_lo'], np.float64))) / V(np.asarray(spec['su_diff'], np.float64)) if su else xo   # module.py:76-83
    f, g = _poly_bounded(spec['poly'], xs)
    if su:
        g = g / V(np.asarray(spec['su_diff'], np.float64))   # module.py:226
    if tr:
        g = g * J                                             # density.py:558
    link = spec.get('link')
    if link is not None:   # the module after the surrogate, density.py:552-560: logp = logp0 - prec (m - y)^2 / 2
        assert link['kind'] == 'gaussian'
        r = f - float(link['y'])
        dphi = -(float(link['prec']) * r)
        f = float(link.get('logp0', 0.)) - 0.5 * (r * (float(link['prec']) * r))
        g = dphi[:, None] * g
    if spec.get('use_decay'):   # density.py:740-746, in the original space and without the transform's Jacobian
        xd = xo - V(np.asarray(spec['decay_mu'], np.float64))
        hv = matvec(np.asarray(spec['decay_hess'], np.float64).T, xd)
        ex = (hv * xd).sum() - float(spec['decay_alpha2'])
        on = ex.v > 0
        gamma = float(spec['decay_gamma'])
        f = f - gamma * V(np.where(on, ex.v, 0), np.where(on, ex.m, 0))
        g = g - vwhere(on[:, None], 2. * gamma * hv, V(np.zeros_like(hv.v)))
    if tr:   # density.py:747-750
        f = f + lj.sum()
        g = g + gj
    return f, g


def logp_and_grad(spec, x, original_space=False):
    """x (n, d) float64 -> logp (n,), grad (n, d) in longdouble, and their scales: logp_scale (n,), grad_scale (n,)."""
    f, g = _eval(spec, V(np.atleast_2d(np.asarray(x, np.float64))), original_space)
    return f.v, g.v, f.m, g.m.max(axis=1)


def leapfrog(spec, var, eps, q, p, grad):
    """One step of CpuLeapfrogIntegrator._step with the diagonal metric var, for n chains at once (integration.py:68-95).
    var, q, p, grad (n, d), eps (n,) float64 -> {name: (value, scale)} for q, p, v, grad (scale (n,): largest over the components),
    logp and energy."""
    var, q, p, grad = (V(np.atleast_2d(np.asarray(a, np.float64))) for a in (var, q, p, grad))
    e = V(np.asarray(eps, np.float64).reshape(-1, 1))
    dt = 0.5 * e
    p1 = p + dt * grad            # :80
    q1 = q + e * (var * p1)       # :82-85
    lp, g1 = _eval(spec, q1, False)   # :87
    p2 = p1 + dt * g1             # :90
    v2 = var * p2                 # :92, metrics.py:88-91
    energy = 0.5 * (p2 * v2).sum() - lp   # :93
    vec = lambda a: (a.v, a.m.max(axis=1))
    return dict(q=vec(q1), p=vec(p2), v=vec(v2), grad=vec(g1), logp=(lp.v, lp.m), energy=(energy.v, energy.m))
