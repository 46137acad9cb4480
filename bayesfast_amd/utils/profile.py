"""Profiles of a surrogate or pipeline density on the device: along a parameter, and along pairs of parameters, the maximum over
all the other parameters at every grid value of the ones held fixed.

``delta = 2 (logp_max - logp_profile)`` gives frequentist intervals, and where it disagrees with the marginal posterior of a
nuisance-heavy model, the marginal is telling about the prior's volume rather than the data.  On a polynomial surrogate a profile
costs no call of the true model: every grid point is a masked Newton maximisation on the analytic Hessian, started at its
neighbour's optimum, and thousands of grid lines run in one launch (``DeviceDensity.profile_lines``,
``DeviceDensity.pipeline_profile_lines``).

The function profiled is the ORIGINAL-space density (no log-Jacobian of the constraint transform), parametrised by the sampling
coordinates, so hard bounds stay respected.  It is whatever density was built: with a prior, a profile posterior; for a profile
likelihood build the density without the prior.  Device only, one process.  A maximum on a hard bound lies at infinity in the
sampling coordinates: such points run to ``max_iter`` and are flagged in ``status``.  Where a decay term is on, a conditional
maximum can sit on the term's surface, where the density has a kink: that point is flagged ``3`` (short but damped).  A pipeline
density in its streamed form is refused (NotImplementedError)."""
from collections import namedtuple

import numpy as np

from .laplace import make_positive

__all__ = ['profile', 'Profile', 'ProfileInterval']

ProfileInterval = namedtuple('ProfileInterval', 'lower, upper, lower_reached, upper_reached')

IMPROVED_RTOL = 1e-9   # a grid point better than the maximum by more than this (times max(1, |logp_max|)): x_0 led to a local maximum


def _crossing(v, r, t):
    """First crossing of r with t walking along the arrays (v, r start at the maximum, r >= 0 there), linear in r; (value, reached)."""
    ok = np.isfinite(r) & np.isfinite(v)
    v, r = v[ok], r[ok]
    if v.size == 0:
        return np.nan, False
    if r[0] >= t:
        return float(v[0]), True
    for k in range(1, v.size):
        if r[k] >= t:
            return float(v[k - 1] + (t - r[k - 1]) * (v[k] - v[k - 1]) / (r[k] - r[k - 1])), True
    return float(v[-1]), False


class Profile:
    """The result of ``profile``.  Indexed by parameter number i (and pairs (i, j)); every value is in ORIGINAL units.

    x_max (d,), logp_max : the maximum of the original-space density, and its value (updated when a grid point beat it)
    params : the profiled parameters;  values[i] (n_i,) : the grid, ascending;  logp[i], delta[i] = 2 (logp_max - logp[i])
    x[i] (n_i, d) : the conditional optima;  status[i], n_iter[i] : per grid point, as ``DeviceDensity.MAXIMIZE_STATUS``
    pairs, values2d[(i, j)] = (grid of i, grid of j), delta2d[(i, j)] (n_i, n_j), status2d[(i, j)], n_iter2d[(i, j)]
    status_max : the status of the maximisation from x_0;  scale (d,) : the grid scale, in sampling coordinates
    n_not_converged : the maximisation from x_0 and the grid points (1-D and 2-D) whose status is neither 0 (converged) nor 4 (not
        run); they are reported all the same
    improved_at : [] or the list of (where, logp) of grid points that beat the maximum found from x_0 -- x_0 led to a local maximum;
        where = i or (i, j); logp_max and x_max are then the best point seen, 1-D or 2-D, so that no delta is negative beyond rounding
    """

    def __init__(self, x_max, logp_max, params, values, logp, x, status, n_iter, pairs=(), values2d=None, logp2d=None, status2d=None,
                 n_iter2d=None, improved_at=(), status_max=0, scale=None):
        self.x_max = np.asarray(x_max, dtype=np.float64)
        self.logp_max = float(logp_max)
        self.params = tuple(params)
        self.values, self.logp, self.x, self.status, self.n_iter = values, logp, x, status, n_iter
        self.pairs = tuple(pairs)
        self.values2d = values2d or {}
        self.logp2d = logp2d or {}
        self.status2d = status2d or {}
        self.n_iter2d = n_iter2d or {}
        self.improved_at = list(improved_at)
        self.status_max = int(status_max)
        self.scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        self.delta = {i: 2. * (self.logp_max - np.asarray(f)) for i, f in self.logp.items()}
        self.delta2d = {p: 2. * (self.logp_max - np.asarray(f)) for p, f in self.logp2d.items()}

    @property
    def n_not_converged(self):
        n = int(self.status_max != 0)
        for st in list(self.status.values()) + list(self.status2d.values()):
            st = np.asarray(st)
            n += int(np.sum((st != 0) & (st != 4)))
        return n

    def interval(self, i, level=0.6827):
        """The interval of parameter i at confidence ``level``: where ``delta[i]`` crosses the chi-square quantile of one degree of
        freedom on either side of the profile's minimum, interpolated linearly in the signed square root of delta (exact for a
        Gaussian, whose signed root is a straight line).  A ``ProfileInterval(lower, upper, lower_reached, upper_reached)``: a side
        on which delta never reaches the threshold returns the grid's end and ``False``."""
        from scipy.stats import chi2
        v, dl = np.asarray(self.values[i], dtype=np.float64), np.asarray(self.delta[i], dtype=np.float64)
        t = float(np.sqrt(chi2.ppf(level, 1)))
        finite = np.isfinite(dl)
        if not finite.any():
            return ProfileInterval(np.nan, np.nan, False, False)
        c = int(np.argmin(np.where(finite, dl, np.inf)))   # (the root changes sign at the profile's minimum: each side is walked from it)
        r = np.sqrt(np.maximum(dl, 0.))
        up, up_ok = _crossing(v[c:], r[c:], t)
        lo, lo_ok = _crossing(v[c::-1], r[c::-1], t)
        return ProfileInterval(lo, up, lo_ok, up_ok)

    @staticmethod
    def levels2d(levels=(0.6827, 0.9545)):
        """The thresholds of ``delta2d`` at the given confidence levels, two degrees of freedom: the ``levels`` of a ``contour``."""
        return -2. * np.log1p(-np.asarray(levels, dtype=np.float64))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
class _Lines:
    """The profile launches of one device density (scalar or pipeline), results on the host."""

    def __init__(self, dev, gauss_newton, max_iter, xtol):
        self.dev, self.d = dev, dev.d
        self.pipeline = dev.spec.get('chi2') is not None
        self.kw = dict(objective='original', max_iter=max_iter, xtol=xtol)
        if self.pipeline:
            self.kw['gauss_newton'] = bool(gauss_newton)

    def run(self, fixed, walk, x_start, values, points=True):
        """One launch; logp and info come to the host, the points x too unless ``points`` is False: they then stay where the launch
        wrote them, under 'x_device' (the 2-D launch's points are 8 n_val d bytes per line, and only a better maximum needs one)."""
        f = self.dev.pipeline_profile_lines if self.pipeline else self.dev.profile_lines
        out = f(fixed, walk, x_start, values, **self.kw)
        res = {k: out[k].cpu().numpy() for k in (('x', 'logp', 'info') if points else ('logp', 'info'))}
        if not points:
            res['x_device'] = out['x']
        return res

    def hessian(self, x):
        """-> the Hessian at x of the objective, in the sampling coordinates: the sampling-space density's, without the log-Jacobian's
        second derivative (-2 s (1 - s) where both bounds are hard, 0 for the other kinds of the transform)."""
        if self.pipeline:
            H = self.dev.pipeline_logp_grad_hess(x, False, gauss_newton=self.kw['gauss_newton'])[2].cpu().numpy()
        else:
            H = self.dev.logp_grad_hess(x, False)[2].cpu().numpy()
        sp = self.dev.spec
        if sp.get('ranges') is not None and sp.get('hard_bounds') is not None:
            both = np.asarray(sp['hard_bounds'], dtype=bool).all(axis=1)
            s = 1. / (1. + np.exp(-np.asarray(x, dtype=np.float64)))
            H = H + np.diag(np.where(both, 2. * s * (1. - s), 0.))
        return H

    def to_original(self, x):
        if self.dev.spec.get('ranges') is None:
            return np.array(x, dtype=np.float64)
        return self.dev.constraint('to_original', np.asarray(x, dtype=np.float64)).cpu().numpy()

    def from_original(self, x):
        if self.dev.spec.get('ranges') is None:
            return np.array(x, dtype=np.float64)
        return self.dev.constraint('from_original', np.asarray(x, dtype=np.float64)).cpu().numpy()

    def coordinate(self, which, i, v, at):
        """The transform of coordinate i alone at the values v (the others at ``at``, which the transform of i does not read)."""
        pts = np.repeat(np.asarray(at, dtype=np.float64)[None], len(v), axis=0)
        pts[:, i] = v
        return (self.to_original if which == 'to_original' else self.from_original)(pts)[:, i]


def _device_of(density, ctx=None):
    if hasattr(density, 'profile_lines'):   # a DeviceDensity (or what stands in for one)
        return density
    if hasattr(density, 'device') and hasattr(density, 'spec'):
        return density.device(ctx) if ctx is not None else density.device()
    raise ValueError('density should be a SurrogateDensity, a Chi2PipelineDensity or a DeviceDensity.')


def _outward(grid, centre):
    """The ascending grid split at ``centre`` into the two lines walked outward from it: (indices up, indices down)."""
    idx = np.arange(grid.size)
    return idx[grid >= centre], idx[grid < centre][::-1]


def _pad(rows):
    n = max(1, max(len(r) for r in rows))
    out = np.full((len(rows), n), np.nan)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out


def profile(density, x_0=None, params=None, pairs=None, n_grid=21, span=4., scale=None, grid=None, gauss_newton=False, max_iter=50,
            xtol=1e-6, _start_sampling=None):
    """Profile the density along ``params`` (default: all) and along ``pairs`` of them (``'all'``, a list of (i, j), or None).

    1. The maximum of the original-space density from ``x_0`` (original units; default: the middle of the sampling space).
    2. A grid per parameter: ``grid`` (a dict or sequence, parameter -> values in original units) or ``n_grid`` points (odd, so that
       the maximum is one) at maximum +- ``span`` x ``scale`` in the SAMPLING coordinates, reported in original units.  ``scale``
       (d,), sampling coordinates; default sqrt(diag((-H)^-1)) at the maximum through ``make_positive``.
    3. The 1-D profiles in one launch: two lines per parameter, walking outward from the maximum.
    4. The 2-D profiles in a second launch: for the pair (i, j) and every grid value of i, two lines that hold {i, j}, start at the
       1-D profile's optimum for that value and walk j's grid outward from that optimum's j.

    ``gauss_newton`` (pipeline densities) steps on the Gauss-Newton matrix.  ``max_iter``, ``xtol``: per grid point, as
    ``DeviceDensity.maximize``.  Returns a ``Profile``."""
    dev = _device_of(density)
    d = dev.d
    ln = _Lines(dev, gauss_newton, int(max_iter), float(xtol))
    n_grid = int(n_grid)
    if n_grid < 3 or n_grid % 2 == 0:
        raise ValueError('n_grid should be an odd integer, at least 3.')
    if not float(span) > 0:
        raise ValueError('span should be positive.')
    params = list(range(d)) if params is None else [int(i) for i in np.atleast_1d(params)]
    if not params or any(i < 0 or i >= d for i in params) or len(set(params)) != len(params):
        raise ValueError('invalid value for params.')
    if pairs is None:
        pairs = []
    elif isinstance(pairs, str):
        if pairs != 'all':
            raise ValueError("pairs should be 'all', a list of pairs, or None.")
        pairs = [(i, j) for a, i in enumerate(params) for j in params[a + 1:]]
    else:
        pairs = [(int(i), int(j)) for i, j in pairs]
        if any(i == j or i not in params or j not in params for i, j in pairs):
            raise ValueError('every pair should consist of two different profiled parameters.')

    # ---- 1: the maximum ----
    if _start_sampling is not None:
        x0s = np.asarray(_start_sampling, dtype=np.float64).reshape(d)
    elif x_0 is not None:
        x0s = ln.from_original(np.asarray(x_0, dtype=np.float64).reshape(1, d))[0]
    elif dev.spec.get('ranges') is not None:
        x0s = np.zeros(d)
    else:
        po = dev.spec['poly']
        x0s = np.zeros(d) if po.get('mu') is None else np.asarray(po['mu'], dtype=np.float64).copy()
        if dev.spec.get('su_lo') is not None:
            x0s = np.asarray(dev.spec['su_lo']) + np.asarray(dev.spec['su_diff']) * x0s
    top = ln.run(np.zeros(d, dtype=np.uint8), -1, x0s[None], None)
    xm, fm, st_top = top['x'][0, 0], float(top['logp'][0, 0]), int(top['info'][0, 0, 1])
    if not np.isfinite(fm):
        raise ValueError('the density is not finite at x_0.')

    # ---- 2: the grids, in the sampling coordinates ----
    if scale is None:
        scale = np.sqrt(np.diag(np.linalg.inv(make_positive(-ln.hessian(xm)))))
    scale = np.asarray(scale, dtype=np.float64).reshape(d)
    if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
        raise ValueError('scale should be positive.')
    half = (n_grid - 1) // 2
    grids = {}
    for i in params:
        given = None
        if grid is not None:
            given = grid.get(i) if hasattr(grid, 'get') else grid[params.index(i)]
        if given is None:
            grids[i] = xm[i] + (float(span) * scale[i] / half) * np.arange(-half, half + 1)
        else:
            g = np.unique(np.asarray(given, dtype=np.float64).ravel())
            if g.size < 1 or not np.all(np.isfinite(g)):
                raise ValueError('invalid grid for parameter %d.' % i)
            grids[i] = np.sort(ln.coordinate('from_original', i, g, ln.to_original(xm[None])[0]))

    # ---- 3: the 1-D profiles ----
    fixed, walk, vals, where = [], [], [], []
    for i in params:
        m = np.zeros(d, dtype=np.uint8)
        m[i] = 1
        for side in _outward(grids[i], xm[i]):
            fixed.append(m)
            walk.append(i)
            vals.append(grids[i][side])
            where.append((i, side))
    res = ln.run(np.array(fixed), np.array(walk, dtype=np.int32), np.repeat(xm[None], len(walk), axis=0), _pad(vals))
    xs1 = {i: np.full((grids[i].size, d), np.nan) for i in params}
    f1 = {i: np.full(grids[i].size, np.nan) for i in params}
    st1 = {i: np.full(grids[i].size, 4, dtype=int) for i in params}
    it1 = {i: np.zeros(grids[i].size, dtype=int) for i in params}
    for l, (i, side) in enumerate(where):
        n = side.size
        xs1[i][side], f1[i][side] = res['x'][l, :n], res['logp'][l, :n]
        st1[i][side], it1[i][side] = res['info'][l, :n, 1].astype(int), res['info'][l, :n, 0].astype(int)

    # ---- 4: the 2-D profiles ----
    f2, st2, it2, at2, x2_device = {}, {}, {}, {}, None
    if pairs:
        fixed, walk, vals, start, where = [], [], [], [], []
        for i, j in pairs:
            m = np.zeros(d, dtype=np.uint8)
            m[[i, j]] = 1
            for a in range(grids[i].size):
                s = xs1[i][a]
                for side in (_outward(grids[j], s[j]) if np.isfinite(s[j]) else (np.arange(0), np.arange(0))):
                    fixed.append(m)
                    walk.append(j)
                    vals.append(grids[j][side])
                    start.append(s)
                    where.append((i, j, a, side))
        for p in pairs:
            f2[p] = np.full((grids[p[0]].size, grids[p[1]].size), np.nan)
            st2[p] = np.full(f2[p].shape, 4, dtype=int)
            it2[p] = np.zeros(f2[p].shape, dtype=int)
            at2[p] = np.zeros(f2[p].shape + (2,), dtype=np.int64)   # (line, column) of the launch that holds the grid point
        if where:
            res = ln.run(np.array(fixed), np.array(walk, dtype=np.int32), np.array(start), _pad(vals), points=False)
            x2_device = res['x_device']
            for l, (i, j, a, side) in enumerate(where):
                n = side.size
                f2[(i, j)][a, side] = res['logp'][l, :n]
                st2[(i, j)][a, side] = res['info'][l, :n, 1].astype(int)
                it2[(i, j)][a, side] = res['info'][l, :n, 0].astype(int)
                at2[(i, j)][a, side, 0], at2[(i, j)][a, side, 1] = l, np.arange(n)

    # ---- a grid point that beats the maximum: x_0 led to a local one ----
    improved, best, x_best = [], fm, xm
    tol = IMPROVED_RTOL * max(1., abs(fm))
    for i in params:
        for a in np.flatnonzero(np.isfinite(f1[i]) & (f1[i] > fm + tol)):
            improved.append((i, float(f1[i][a])))
            if f1[i][a] > best:
                best, x_best = float(f1[i][a]), xs1[i][a]
    for p in pairs:
        for a, b in zip(*np.nonzero(np.isfinite(f2[p]) & (f2[p] > fm + tol))):
            improved.append((p, float(f2[p][a, b])))
            if f2[p][a, b] > best:   # (the one point of the 2-D launch that is fetched)
                best, x_best = float(f2[p][a, b]), x2_device[int(at2[p][a, b, 0]), int(at2[p][a, b, 1])].cpu().numpy()
    to_o = lambda x: ln.to_original(np.where(np.isfinite(x), x, 0.)) + np.where(np.isfinite(x), 0., np.nan)
    values = {i: ln.coordinate('to_original', i, grids[i], xm) for i in params}
    prof = Profile(ln.to_original(x_best[None])[0], best, params, values, f1, {i: to_o(xs1[i]) for i in params}, st1, it1, pairs,
                   {p: (values[p[0]], values[p[1]]) for p in pairs}, f2, st2, it2, improved, st_top, scale)
    return prof


def profile_from_draws(trace_draws, density, **kw):
    """``profile`` started at the mean of sampling-space draws (n_chain, n_t, d) or (n, d), with their standard deviation as the
    grid scale (``TraceTuple.profile``)."""
    x = trace_draws
    if hasattr(x, 'is_cuda'):
        x = x.reshape(-1, x.shape[-1]).double()
        mean, sd = x.mean(dim=0).cpu().numpy(), x.std(dim=0).cpu().numpy()
    else:
        x = np.asarray(x, dtype=np.float64).reshape(-1, np.shape(x)[-1])
        mean, sd = x.mean(axis=0), x.std(axis=0, ddof=1)
    kw.setdefault('scale', sd)
    return profile(density, _start_sampling=mean, **kw)
