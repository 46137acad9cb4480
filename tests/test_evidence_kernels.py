"""The data-parallel kernels under the evidence estimators and the refit selection (bayesfast_amd/csrc/bfhip_sit.hip,
bfhip_refit.hip) against plain host restatements of the same operations: float64 / extended-precision sums with scipy's
special functions, math.fsum, mpmath, numpy's sort and search, and the oracle's C restatements.  Sizes straddle every tile,
grid-cap and split threshold of the launches; inputs include the special values each kernel has to pass through.

Every tolerance is derived from the conditioning of the operation at that input (the comment or docstring next to it
says how), in units of EPS = 2^-52, never picked to make a comparison pass.  Where the reference package has been built
into oracle/_ref, its own compiled ``_cubic`` and ``bridge`` are compared as well; only those extra comparisons skip
without it."""
import importlib
import math
import os
import warnings

import numpy as np
import pytest
from scipy.special import erfcx, logsumexp, ndtr, ndtri

EPS = np.finfo(np.float64).eps
TINY = 5e-324                     # one subnormal ulp: the absolute error of a result that underflowed


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _n_cu(ctx):
    import torch
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _reference():
    from oracle import reference
    if not reference.is_built():
        return None
    return reference.load()


# ---- host semantics of importance_weights (no GPU) ------------------------------------------------------------------

def test_host_importance_weights_follow_np_clip_on_special_values():
    """The host route is the reference's ``np.clip(w, 0, mean(w) * n**k)``: a NaN weight makes the cap NaN and with it
    every truncated weight; an infinite weight makes the cap infinite (nothing else is clipped); logp = -inf is a zero
    weight; k < 0 returns an unclipped copy."""
    from bayesfast_amd.core.refit import importance_weights
    lq = np.zeros(4)
    w, wt = importance_weights(np.array([0., np.nan, 1., -1.]), lq, 0.25)
    assert np.isnan(w[1]) and np.isfinite(np.delete(w, 1)).all()
    assert np.isnan(wt).all()
    w, wt = importance_weights(np.array([0., np.inf, 1., -np.inf]), lq, 0.)
    assert wt.tolist() == [1., np.inf, math.e, 0.]
    w, wt = importance_weights(np.array([0., np.nan, 1., -1.]), lq, -1.)
    assert wt is not w and np.array_equal(wt, w, equal_nan=True)
    w, wt = importance_weights(np.log([1., 1., 1., 5.]), lq, 0.)
    assert wt[:3].tolist() == [1.] * 3 and wt[3] == np.mean(w) < w[3]


# ---- bfhip_kde_cdf --------------------------------------------------------------------------------------------------
# out[j][i] = sum_k w[k] ndtr((pts[j][i] - data[j][k]) / h[j]).  The terms are non-negative, so the error of each value is
# bounded relative to the terms themselves:
#   * the summation: a thread adds ceil(ceil(n / n_split) / 256) terms in order, the block tree adds 8 levels, the combine
#     kernel n_split partials: at most DEPTH = that many additions, each off by EPS / 2 of the running sum (EPS of it here);
#   * erfc itself (ocml) and scipy's ndtr: a few ulp each, with the products 0.5 w and w ndtr: C_F = 8 EPS per term;
#   * the argument u = (x_k - p) / (h sqrt 2): rounded by both sides, |du / u| <= C_ARG EPS with C_ARG = 4 (device: the
#     constant, 1/h, the difference and the product; host: the difference, / h and ndtr's / sqrt 2).  It moves erfc(u) by
#     |d log erfc / du| |du| = 2 |u| / (sqrt(pi) erfcx(u)) C_ARG EPS relative -- about 2 u^2 C_ARG EPS in the upper tail of
#     u (deep-tail values of the cdf), nearly nothing where erfc(u) is close to 2.
# The host reference sums in extended precision (x87 80-bit: 11 more bits than float64), so its own summation error is
# below EPS / 2048 relative and is not budgeted.
KDE_C_F, KDE_C_ARG = 8., 4.


def _kde_split(ctx, n, m, d):
    """The data split of bfhip_kde_cdf's launch (bfhip_sit.hip): one per 16384 samples, at most enough groups to fill
    4 workgroups per CU."""
    tiles = (m + 7) // 8
    ns = (n + 16383) // 16384
    want = (4 * _n_cu(ctx) + tiles * d - 1) // (tiles * d)
    return max(1, min(ns, want)), ns > want


def _kde_ref(data, w, h, pts):
    """(cdf, bound / EPS without the summation term, sum of the terms, dcdf/dh * h) at every point, one data row."""
    cdf, sens, tot, dh = np.empty(pts.size), np.empty(pts.size), np.empty(pts.size), np.empty(pts.size)
    chunk = max(1, (1 << 22) // max(1, data.size))
    for i in range(0, pts.size, chunk):
        p = pts[i:i + chunk, None]
        t = w * ndtr((p - data) / h)
        u = (data - p) / (h * math.sqrt(2.))
        with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
            s = np.where(np.isfinite(erfcx(u)), 2. * np.abs(u) / (math.sqrt(math.pi) * erfcx(u)), 0.)
        cdf[i:i + chunk] = np.sum(t.astype(np.longdouble), axis=1)
        sens[i:i + chunk] = np.sum(t * (KDE_C_F + KDE_C_ARG * s), axis=1)
        tot[i:i + chunk] = np.sum(t, axis=1)
        z = (p - data) / h
        dh[i:i + chunk] = np.sum(w * np.exp(-0.5 * z * z) * np.abs(z), axis=1) / math.sqrt(2 * math.pi)
    return cdf, sens, tot, dh


def _kde_inputs(rng, n, d):
    """d rows of data with different location, scale and shape; non-normalised weights with zeros; a bandwidth per row."""
    loc = np.array([0., 3., -50., 1e3, 0.5, -2., 7.])[:d]
    scale = np.array([1., 0.01, 20., 3., 1e-3, 0.4, 5.])[:d]
    z = np.where(rng.uniform(size=(d, n)) < 0.3, rng.laplace(size=(d, n)), rng.normal(size=(d, n)) + 2.)
    data = loc[:, None] + scale[:, None] * z
    w = rng.uniform(0., 3., size=n)
    w[rng.uniform(size=n) < 0.15] = 0.
    w[0] = 1.25
    h = scale * np.array([0.3, 0.07, 1.1, 0.5, 0.02, 2., 0.15])[:d]
    return data, w, h


def _kde_points(data, h, m, rot):
    """m points per row from a pool of data points themselves, the middle, near tails and +-40 h beyond the data."""
    out = np.empty((data.shape[0], m))
    for j in range(data.shape[0]):
        x, hj = data[j], h[j]
        lo, hi = x.min(), x.max()
        pool = np.concatenate(([lo - 40 * hj, 0.5 * (lo + hi), hi + 40 * hj, lo, hi, lo - 8 * hj, hi + 8 * hj, np.median(x)],
                               x[:12], np.linspace(lo - 3 * hj, hi + 3 * hj, 21)))
        out[j] = np.resize(np.roll(pool, -(rot + 5 * j)), m)
    return out


def _kde_cases():
    ns = (1, 255, 257, 16384, 16385, 3 * 16384 + 7, 200003)
    ms = (1, 7, 8, 9, 41)
    cases = [(n, m, d) for i, n in enumerate(ns) for k, d in enumerate((1, 3, 7)) for m in (ms[(i + 2 * k) % 5],)]
    cases += [(16385, m, 3) for m in ms]
    cases.append((3 * 16384 + 7, 392, 7))   # 49 tiles x 7 rows: 4 splits clamped to fill the chip
    return cases


@pytest.mark.gpu
def test_kde_cdf_matches_an_extended_precision_sum_at_every_split():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    rng = np.random.default_rng(101)
    seen_split, seen_clamp = set(), False
    for case, (n, m, d) in enumerate(_kde_cases()):
        data, w, h = _kde_inputs(rng, n, d)
        pts = _kde_points(data, h, m, case)
        dd, wd, hd, pd = ctx.tensor(data), ctx.tensor(w), ctx.tensor(h), ctx.tensor(pts)
        out = torch.full((d, m), np.nan, dtype=torch.float64, device=ctx.device)
        again = torch.full_like(out, np.nan)
        for o in (out, again):
            _lib.check(ctx._lib.bfhip_kde_cdf(ctx.handle, d, n, _ptr(dd), _ptr(wd), _ptr(hd), m, _ptr(pd), _ptr(o)))
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint64), again.cpu().numpy().view(np.uint64)), (n, m, d)
        n_split, clamped = _kde_split(ctx, n, m, d)
        seen_split.add(n_split)
        seen_clamp |= clamped
        depth = -(-(-(-n // n_split)) // 256) + 8 + n_split
        for j in range(d):
            ref, sens, tot, _ = _kde_ref(data[j], w, h[j], pts[j])
            bound = EPS * (depth * tot + sens) + n * w.max() * TINY
            err = np.abs(got[j] - ref.astype(np.float64))
            assert np.all(err <= bound), (n, m, d, j, np.max(err / bound))
    assert max(seen_split) > 1 and (seen_clamp or _n_cu(ctx) < 86)
    print('splits', sorted(seen_split), 'clamped', seen_clamp)


@pytest.mark.gpu
def test_kde_cdf_deep_tail_and_fsum_spot_checks():
    """A few rows against math.fsum of the same float64 terms, and deep lower-tail points (every term ~1e-20 .. 1e-140)
    against mpmath at 40 digits on the exact double inputs, within the bound above (there the argument term dominates)."""
    import mpmath
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    rng = np.random.default_rng(7)
    n = 257
    data, w, h = _kde_inputs(rng, n, 1)
    lo = data[0].min()
    pts = np.array([[lo - 6 * h[0], lo - 10 * h[0], lo - 17 * h[0], lo - 25 * h[0], lo, np.median(data[0])]])
    dd, wd, hd, pd = ctx.tensor(data), ctx.tensor(w), ctx.tensor(h), ctx.tensor(pts)
    out = torch.empty_like(pd)
    _lib.check(ctx._lib.bfhip_kde_cdf(ctx.handle, 1, n, _ptr(dd), _ptr(wd), _ptr(hd), pts.shape[1], _ptr(pd), _ptr(out)))
    got = out.cpu().numpy()[0]
    ref, sens, tot, _ = _kde_ref(data[0], w, h[0], pts[0])
    bound = EPS * ((-(-n // 256) + 9) * tot + sens) + n * w.max() * TINY
    mpmath.mp.dps = 40
    for i, p in enumerate(pts[0]):
        exact = mpmath.fsum(mpmath.mpf(float(wk)) * mpmath.ncdf((mpmath.mpf(float(p)) - mpmath.mpf(float(xk))) / mpmath.mpf(float(h[0])))
                            for xk, wk in zip(data[0], w))
        assert 0 < got[i] and abs(got[i] - exact) <= bound[i], (i, got[i], exact, bound[i])
        terms = w * ndtr((p - data[0]) / h[0])
        assert abs(math.fsum(terms) - float(ref[i])) <= EPS * tot[i]


@pytest.mark.gpu
def test_kde_cdf_m_zero_is_a_no_op():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    a = ctx.tensor(np.ones(5))
    out = torch.full((5,), 7., dtype=torch.float64, device=ctx.device)
    _lib.check(ctx._lib.bfhip_kde_cdf(ctx.handle, 1, 5, _ptr(a), _ptr(a), _ptr(a), 0, _ptr(a), _ptr(out)))
    _lib.check(ctx._lib.bfhip_kde_cdf(ctx.handle, 1, 5, _ptr(a), _ptr(a), _ptr(a), 0, None, None))
    assert out.cpu().numpy().tolist() == [7.] * 5


# ---- bfhip_spline_build's knot values -------------------------------------------------------------------------------

H_REL = 64 * EPS


@pytest.mark.gpu
@pytest.mark.parametrize('weighted', [False, True])
def test_spline_build_knot_values_are_ndtri_of_the_host_cdf(weighted):
    """The device route of SIT._gaussianize builds every spline on the device (bandwidth, cdf sums, ndtri).  At the knots
    it returns, y_k must be ndtri of the host cdf with the host bandwidth (oracle.kde_bandwidth, the reference's formula):
    a wrong h or wrong sums fail here.  The cdf p_k is off by at most EPS (DEPTH + C_F + C_ARG 2 u^2 ...) relative, as
    for bfhip_kde_cdf (DEPTH = ceil(n / 1024) + 6 + 16: 1024 threads stride over the samples, a 64-lane butterfly, 16 wave
    sums in order).  The bandwidth is sqrt(weighted variance) * neff^(-1/5): sums of non-negative terms on both sides
    (torch's reduction trees, numpy's pairwise sum; depth < 64), so h differs by at most H_REL = 64 EPS relative, which
    moves the cdf by h |dp/dh| H_REL = sum w phi(z) |z| H_REL.  ndtri maps dp to dy = dp / phi(y), plus its own few ulp."""
    from bayesfast_amd.transforms import SIT
    from oracle import oracle as orc
    ctx = _ctx()
    rng = np.random.default_rng(33)
    n, d = 70000, 4
    y = np.stack([rng.laplace(size=n) * 2., rng.normal(size=n) * 0.05 + 3., rng.standard_t(4, size=n) * 10.,
                  np.where(rng.uniform(size=n) < 0.3, rng.normal(-6., 0.2, size=n), rng.normal(5., 1.5, size=n))], 1)
    sit = SIT(n_iter=1, random_generator=1)
    sit._weights = rng.uniform(0.2, 1., size=n) if weighted else np.ones(n)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        splines = sit._gaussianize(ctx.tensor(y)).splines
    wn = sit._weights / np.sum(sit._weights)
    depth = -(-n // 1024) + 6 + 16
    for j, sp in enumerate(splines):
        h = orc.kde_bandwidth(y[:, j], sit._weights)
        ref, sens, tot, dpdh = _kde_ref(y[:, j], wn, h, sp.x)
        p = ref.astype(np.float64)
        dp = EPS * (depth * tot + sens) + dpdh * H_REL
        yk = ndtri(p)
        phi = np.exp(-0.5 * yk * yk) / math.sqrt(2 * math.pi)
        tol = dp / phi + 4 * EPS * np.abs(yk)
        err = np.abs(sp.y - yk)
        assert np.all(err <= tol), (j, np.max(err / tol), int(np.argmax(err / tol)))


# ---- bfhip_spline_apply -----------------------------------------------------------------------------------------------

def _hermite(x, y, s):
    """A monotone piecewise cubic from knots, values and slopes, with the linear extrapolation rows (the layout of
    utils/cubic.py: m + 1 rows, highest order first)."""
    m = x.size
    c = np.zeros((m + 1, 4))
    c[0, 2:] = s[0], y[0]
    c[m, 2:] = s[-1], y[-1]
    for i in range(1, m):
        hh = x[i] - x[i - 1]
        dl = (y[i] - y[i - 1]) / hh
        c[i] = [(s[i - 1] + s[i] - 2 * dl) / hh**2, (3 * dl - 2 * s[i - 1] - s[i]) / hh, s[i - 1], y[i - 1]]
    return c


def _spline_set(fx):
    from bayesfast_amd.utils.spline import GaussianizingSpline
    out = [GaussianizingSpline.from_arrays(fx['sit.it0.d%d.x' % j], fx['sit.it0.d%d.y' % j], fx['sit.it0.d%d.c' % j]) for j in range(6)]
    x3, y3 = np.array([-1., 0.25, 2.]), np.array([-2., 0.5, 1.5])
    out.append(GaussianizingSpline.from_arrays(x3, y3, _hermite(x3, y3, np.array([1.5, 1.2, 0.3]))))
    x2, y2 = np.array([10., 10.5]), np.array([-0.25, 3.])
    out.append(GaussianizingSpline.from_arrays(x2, y2, _hermite(x2, y2, np.array([4., 8.]))))
    return out


def _spline_points(k):
    """Every knot, its float neighbours, interval midpoints, the ends, beyond them, +-1e300, +-inf, NaN (specials first)."""
    span = k[-1] - k[0]
    return np.concatenate(([np.inf, -np.inf, np.nan, 1e300, -1e300, k[0], k[-1], k[0] - span, k[-1] + span,
                            k[0] - 1e-3 * span, k[-1] + 1e-3 * span], k, np.nextafter(k, -np.inf), np.nextafter(k, np.inf),
                           0.5 * (k[:-1] + k[1:])))


def _cubic_terms(c, x, v, der):
    """Interval of every point (x[i-1] <= v < x[i]; 0 below, m at or above x[m-1]), the cubic's local coordinate, and the
    sum of the absolute values of its terms there (the scale of the rounding of one evaluation)."""
    m = x.size
    iv = np.searchsorted(x, v, side='right')
    base = np.where(iv == 0, x[0], x[np.clip(iv - 1, 0, m - 1)])
    t = v - base
    r = c[iv]
    lin = (iv == 0) | (iv == m)           # the linear extrapolation rows: only c2 and c3 are used
    with np.errstate(invalid='ignore', over='ignore'):
        if der:
            s = np.where(lin, np.abs(r[:, 2]), 3 * np.abs(r[:, 0]) * t * t + 2 * np.abs(r[:, 1] * t) + np.abs(r[:, 2]))
        else:
            s = np.where(lin, np.abs(r[:, 2] * t) + np.abs(r[:, 3]),
                         np.abs(r[:, 0] * t**3) + np.abs(r[:, 1] * t * t) + np.abs(r[:, 2] * t) + np.abs(r[:, 3]))
    return iv, t, s


def _host_cubic(r, t):
    return ((r[:, 0] * t + r[:, 1]) * t + r[:, 2]) * t + r[:, 3]


def _same_nonfinite(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isinf(a), a, 0), np.where(np.isinf(b), b, 0))


@pytest.mark.gpu
def test_spline_apply_matches_the_oracle_on_a_ragged_table():
    """Evaluate and derivative: the kernel is compiled with FP contraction, so every cubic may round differently from the
    oracle's; both are within 4 EPS of sum |terms| (six roundings of a four-term sum), so they agree to 8 EPS of it.
    Solve: both bisect until |f(t) - v| < 1e-10, possibly stopping at different steps, so the device result must be in the
    reference's knot interval, the host cubic at it must be within 1e-10 (+ its rounding, and the rounding of x + t,
    slope * EPS |x|) of the target, and it must be within twice that over the smaller of the two local slopes of the
    reference's answer.  The linear extrapolations are a few roundings of (v - c3) / c2 + x0 on both sides."""
    from bayesfast_amd.utils.spline import SplineTable
    from oracle import oracle as orc
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evidence.npz'))
    ctx = _ctx()
    sps = _spline_set(fx)
    ref_pkg = _reference()
    for n, cols in ((2, [6, 0, 7]), (36, [7, 1, 2, 3, 4, 5, 6]), (43, [5, 4, 7, 6, 3, 2]), (125001, [0, 1, 2, 3, 4, 5, 6, 7])):
        tab = SplineTable([sps[j] for j in cols], ctx)
        for mode in ('evaluate', 'derivative', 'solve'):
            src = [sps[j].y if mode == 'solve' else sps[j].x for j in cols]
            pts = np.stack([np.resize(np.roll(_spline_points(k), -(3 * i) if n > 2 else 0), n) for i, k in enumerate(src)], 1)
            got = tab.apply(mode, ctx.tensor(pts)).cpu().numpy()
            for i, j in enumerate(cols):
                s, v, g = sps[j], pts[:, i], got[:, i]
                ref = orc.spline_apply(mode, s.c, s.x, s.y, v)
                assert _same_nonfinite(g, ref), (n, mode, j)
                fin = np.isfinite(ref)
                if mode != 'solve':
                    _, _, size = _cubic_terms(s.c, s.x, v, mode == 'derivative')
                    assert np.all(np.abs(g[fin] - ref[fin]) <= 8 * EPS * size[fin]), (n, mode, j)
                else:
                    _check_solve(s, v, g, ref)
                if ref_pkg is not None and n > 2:
                    cub = importlib.import_module('bayesfast.utils._cubic')
                    r2, vc = np.empty_like(v), np.ascontiguousarray(v)
                    if mode == 'solve':
                        cub.solve(np.ascontiguousarray(s.c), s.x, s.y, vc, r2)
                        _check_solve(s, v, g, r2)
                    else:
                        getattr(cub, mode)(np.ascontiguousarray(s.c), s.x, vc, r2)
                        assert _same_nonfinite(g, r2)
                        _, _, size = _cubic_terms(s.c, s.x, v, mode == 'derivative')
                        assert np.all(np.abs(g[fin] - r2[fin]) <= 8 * EPS * size[fin]), (n, mode, j)


def _check_solve(s, v, g, ref):
    assert _same_nonfinite(g, ref)
    m = s.x.size
    iv = np.searchsorted(s.y, v, side='right')
    fin = np.isfinite(ref)
    inner = fin & (iv > 0) & (iv < m)
    outer = fin & ~inner
    # interior: the knot interval, the residual at the device's answer, the distance to the reference's
    k = iv[inner]
    lo, hi, vi, gi, ri = s.x[k - 1], s.x[k], v[inner], g[inner], ref[inner]
    assert np.all((lo <= gi) & (gi <= hi)) and np.all((lo <= ri) & (ri <= hi))
    rows = s.c[k]
    t = gi - lo
    res = np.abs(_host_cubic(rows, t) - vi)
    size = np.abs(rows[:, 0] * t**3) + np.abs(rows[:, 1] * t * t) + np.abs(rows[:, 2] * t) + np.abs(rows[:, 3])
    slope = lambda tt: np.abs((3 * rows[:, 0] * tt + 2 * rows[:, 1]) * tt + rows[:, 2])
    allow = 1e-10 + 8 * EPS * size + slope(t) * EPS * np.abs(gi)
    assert np.all(res <= allow), np.max(res / allow)
    smin = np.minimum(slope(t), slope(ri - lo))
    with np.errstate(divide='ignore'):
        dist = 2 * allow / smin + EPS * (np.abs(gi) + np.abs(ri))
    assert np.all(np.abs(gi - ri) <= dist), np.max(np.abs(gi - ri) / dist)
    # linear extrapolation: x0 + (v - c3) / c2 on both sides, a few roundings each
    r = np.where(iv[outer] == 0, 0, m)
    x0, c2, c3 = s.x[np.where(r == 0, 0, m - 1)], s.c[r, 2], s.c[r, 3]
    q = (v[outer] - c3) / c2
    tol = 2 * EPS * ((np.abs(v[outer]) + np.abs(c3)) / np.abs(c2) + np.abs(q) + np.abs(x0))
    assert np.all(np.abs(g[outer] - ref[outer]) <= tol)


# ---- bfhip_bridge_sums / bfhip_bridge_terms ---------------------------------------------------------------------------
BRIDGE_PAIRS = ((1, 257), (255, 256), (256, 1), (257, 131073), (131073, 131072), (131072, 3 * 131072 + 17),
                (3 * 131072 + 17, 255))
LOGRS = (0., 5., -5., 40., -40., 800., -800.)


def _log_sigmoid_lse(x):
    """log sum exp(x - logaddexp(x, 0)) without the cancellation of the reference's form: each term is -logaddexp(0, -x)
    (exact at both ends: +inf -> 0, -inf -> -inf), summed by scipy's logsumexp."""
    with np.errstate(invalid='ignore'):
        return logsumexp(-np.logaddexp(0., -x))


def _sums_tol(n, x):
    """Absolute bound on a device log-sum-exp of the log-sigmoid terms: each term's log is off by ~EPS (|x| + 2) (the
    log1p / exp of the kernel and of numpy), the sum of exp(t - max) by its depth -- ceil(n / (nb * 256)) + 8 + nb on the
    device with nb = min(ceil(n / 256), 512) blocks, log2(n) + 8 in scipy's pairwise sum -- relative, i.e. absolute in the
    log."""
    nb = min(-(-n // 256), 512)
    fin = np.abs(x[np.isfinite(x)])
    return EPS * (-(-n // (nb * 256)) + 8 + nb + math.log2(n) + 8 + 2 * (fin.max() if fin.size else 0.) + 4)


def _bridge_sums(ctx, a, b, logr):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ad, bd = ctx.tensor(a), ctx.tensor(b)
    out = torch.full((2,), 3., dtype=torch.float64, device=ctx.device)
    _lib.check(ctx._lib.bfhip_bridge_sums(ctx.handle, a.size, _ptr(ad), b.size, _ptr(bd), float(logr), _ptr(out)))
    return out.cpu().numpy()


@pytest.mark.gpu
def test_bridge_sums_match_the_log_sigmoid_sums():
    from oracle import oracle as orc
    ctx = _ctx()
    rng = np.random.default_rng(5)
    for na, nb in BRIDGE_PAIRS:
        a, b = rng.normal(-1., 4., size=na), rng.normal(1., 4., size=nb)
        for logr in LOGRS:
            got = _bridge_sums(ctx, a, b, logr)
            assert np.array_equal(got.view(np.uint64), _bridge_sums(ctx, a, b, logr).view(np.uint64))
            ref = (_log_sigmoid_lse(logr + a), _log_sigmoid_lse(-logr + b))
            for g, r, x in zip(got, ref, (logr + a, -logr + b)):
                assert abs(g - r) <= _sums_tol(x.size, x), (na, nb, logr, g, r)
            if abs(logr) <= 5:    # the reference's own formula, where it does not cancel (|x| < ~30)
                assert abs((got[0] - got[1]) - orc.bridge_score(logr, a, b)) <= _sums_tol(na, logr + a) + _sums_tol(nb, -logr + b)


@pytest.mark.gpu
def test_bridge_sums_against_mpmath_where_the_reference_form_cancels():
    """At |logr| = 40 and 800, x - logaddexp(x, 0) loses |x| EPS absolute (or all of a -4e-18 term); mpmath at 50 digits
    gives the exact value of the same sum of the exact double inputs."""
    import mpmath
    mpmath.mp.dps = 50
    ctx = _ctx()
    rng = np.random.default_rng(9)
    for n in (1, 255):
        a, b = rng.normal(0., 3., size=n), rng.normal(0., 3., size=n + 2)
        for logr in (40., -40., 800., -800.):
            got = _bridge_sums(ctx, a, b, logr)
            for g, s, arr in zip(got, (logr, -logr), (a, b)):
                x = [mpmath.mpf(float(s + v)) for v in arr]     # the kernel's rounded s + a_i, exactly
                exact = mpmath.log(mpmath.fsum(1 / (1 + mpmath.exp(-xi)) for xi in x))
                assert abs(g - float(exact)) <= _sums_tol(len(x), s + arr), (n, logr, g, exact)


@pytest.mark.gpu
def test_bridge_sums_special_entries():
    """-inf entries are zero terms; +inf is the limit log sigmoid(+inf) = 0 (the reference's x - logsumexp([x, 0]) is
    inf - inf = NaN there); a NaN entry makes its side NaN and leaves the other alone; all -inf gives -inf."""
    ctx = _ctx()
    rng = np.random.default_rng(13)
    for na, nb in ((257, 131073), (131073, 255)):
        a, b = rng.normal(size=na), rng.normal(size=nb)
        a[::7] = -np.inf
        got = _bridge_sums(ctx, a, b, 0.5)
        assert abs(got[0] - _log_sigmoid_lse(0.5 + a[np.isfinite(a)])) <= _sums_tol(na, a)
        a2 = a.copy()
        a2[na // 2] = np.inf
        got = _bridge_sums(ctx, a2, b, 0.5)
        assert abs(got[0] - _log_sigmoid_lse(0.5 + a2)) <= _sums_tol(na, a2)
        a3 = a.copy()
        a3[na - 1] = np.nan
        got = _bridge_sums(ctx, a3, b, 0.5)
        assert np.isnan(got[0]) and abs(got[1] - _log_sigmoid_lse(-0.5 + b)) <= _sums_tol(nb, b)
        got = _bridge_sums(ctx, np.full(na, -np.inf), np.full(nb, -np.inf), 3.)
        assert got.tolist() == [-np.inf, -np.inf]


def _terms_ref(lpp, lqp, lpq, lqq, logr):
    """evidence/bridge.py:50-55 as the reference writes it (two-row scipy logsumexp)."""
    n_p, n_q = lpp.size, lqq.size
    lp, lq = np.log(n_p / (n_p + n_q)), np.log(n_q / (n_p + n_q))
    with np.errstate(invalid='ignore', over='ignore'):
        f1 = np.exp(lpq - logr - logsumexp(np.array((lpq - logr + lp, lqq + lq)), axis=0))
        f2 = np.exp(lqp - logsumexp(np.array((lpp - logr + lp, lqp + lq)), axis=0))
    return f1, f2


def _terms_tol(ref, *logs):
    """exp turns an absolute error in its argument into the same relative error: the argument is a few sums and a
    logaddexp of the inputs, each rounded to EPS / 2 of its size, plus exp's own ulp on both sides: relative
    EPS (4 + 2 sum |input|), with one subnormal ulp where the result underflows."""
    size = sum(np.where(np.isfinite(x), np.abs(x), 0.) for x in logs)     # (a -inf input drops out of its logaddexp exactly)
    return EPS * (4 + 2 * size) * np.abs(ref) + 2 * TINY


def _bridge_terms(ctx, lpp, lqp, lpq, lqq, logr):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    d = [ctx.tensor(v) for v in (lpp, lqp, lpq, lqq)]
    f1 = torch.full((lqq.size,), 5., dtype=torch.float64, device=ctx.device)
    f2 = torch.full((lpp.size,), 5., dtype=torch.float64, device=ctx.device)
    _lib.check(ctx._lib.bfhip_bridge_terms(ctx.handle, lpp.size, _ptr(d[0]), _ptr(d[1]), lqq.size, _ptr(d[2]), _ptr(d[3]), float(logr),
                                           _ptr(f1), _ptr(f2)))
    return f1.cpu().numpy(), f2.cpu().numpy()


@pytest.mark.gpu
def test_bridge_terms_match_the_reference_formula():
    ctx = _ctx()
    rng = np.random.default_rng(17)
    for n_p, n_q in BRIDGE_PAIRS + ((3, 3),):
        lpp, lqp = rng.normal(-3., 4., size=n_p), rng.normal(-3., 4., size=n_p)
        lpq, lqq = rng.normal(-3., 4., size=n_q), rng.normal(-3., 4., size=n_q)
        if n_p >= 3 and n_q >= 3:   # zero terms, +inf, NaN, both -inf
            lpq[0], lqq[1], lpq[2], lqq[2] = -np.inf, -np.inf, np.inf, -np.inf
            lpp[0], lqp[1], lpp[2], lqp[2] = np.nan, -np.inf, -np.inf, -np.inf
        for logr in LOGRS:
            g1, g2 = _bridge_terms(ctx, lpp, lqp, lpq, lqq, logr)
            h1, h2 = _bridge_terms(ctx, lpp, lqp, lpq, lqq, logr)
            assert np.array_equal(g1.view(np.uint64), h1.view(np.uint64)) and np.array_equal(g2.view(np.uint64), h2.view(np.uint64))
            r1, r2 = _terms_ref(lpp, lqp, lpq, lqq, logr)
            lp, lq = np.log(n_p / (n_p + n_q)), np.log(n_q / (n_p + n_q))
            for g, r, logs in ((g1, r1, (lpq, lqq, logr, lp, lq)), (g2, r2, (lpp, lqp, logr, lp, lq))):
                assert _same_nonfinite(g, r), (n_p, n_q, logr)
                fin = np.isfinite(r)
                tol = _terms_tol(r, *logs)
                assert np.all(np.abs(g - r)[fin] <= tol[fin]), (n_p, n_q, logr, np.max((np.abs(g - r) / tol)[fin]))


@pytest.mark.gpu
@pytest.mark.parametrize('logz', [37.5, -12.])
def test_bridge_recovers_a_known_log_ratio(logz):
    """p = exp(logz) N(0, I_3) as 8 chains x 20000 steps, q = N(0.1, 1.15^2 I_3) with 150000 samples (beyond one grid of
    the sums kernel): the estimate is within 5 reported errors of logz (a 5-sigma statistical bound), and equal to the
    reference's bridge on the same arrays to 1e-9 (the secant runs on scores that differ by ~1e-13)."""
    from bayesfast_amd.evidence import bridge
    rng = np.random.default_rng(23)
    d, mu, sig = 3, 0.1, 1.15
    xp = rng.normal(size=(8, 20000, d))
    xq = mu + sig * rng.normal(size=(150000, d))
    lnorm = lambda x, m, s: np.sum(-0.5 * ((x - m) / s)**2 - np.log(s) - 0.5 * math.log(2 * math.pi), axis=-1)
    args = (logz + lnorm(xp, 0., 1.), logz + lnorm(xq, 0., 1.), lnorm(xp, mu, sig), lnorm(xq, mu, sig))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        logr, err = bridge(*args)
        assert 0 < err < 0.05 and abs(logr - logz) < 5 * err, (logr, err)
        ref = _reference()
        if ref is not None:
            lr, er = ref.evidence.bridge(*args)
            assert abs(logr - lr) < 1e-9 and abs(err - er) < 1e-9 * max(1., er), (logr, lr, err, er)


# ---- bfhip_importance_weights ------------------------------------------------------------------------------------------

def _iw_dev(ctx, lp, lq, k):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    a, b = ctx.tensor(lp), ctx.tensor(lq)
    w = torch.full_like(a, 9.)
    wt = torch.full_like(a, 9.)
    _lib.check(ctx._lib.bfhip_importance_weights(ctx.handle, lp.size, _ptr(a), _ptr(b), float(k), _ptr(w), _ptr(wt)))
    return w.cpu().numpy(), wt.cpu().numpy()


def _iw_tol(n, w, cap):
    """|device - host| for a truncated weight: 3 ulp of exp on either side (ocml's exp and numpy's are within ~1 ulp each),
    plus, for values at the cap, the rounding of the cap: the mean is a sum of non-negative weights, off by EPS per level
    of its depth (device: ceil(n / (nb * 256)) + 8 + nb with nb = min(ceil(n / 256), 256); numpy: log2(n) + 16 pairwise)
    and n**k by 2 ulp of pow on each side."""
    nb = min(-(-n // 256), 256)
    rel = EPS * (-(-n // (nb * 256)) + 8 + nb + math.log2(n) + 16 + 4)
    with np.errstate(invalid='ignore'):
        return 3 * np.spacing(np.abs(w)) + (rel * cap if np.isfinite(cap) else 0.)


@pytest.mark.gpu
def test_importance_weights_match_np_exp_and_np_clip():
    from bayesfast_amd.core.refit import importance_weights
    ctx = _ctx()
    rng = np.random.default_rng(29)
    for n in (1, 255, 256, 257, 65536, 65537, 200003):
        lp, lq = rng.normal(0., 2., size=n), rng.normal(0., 1., size=n)
        lp[: n // 3] += 3.                       # heavy weights that the cap clips
        for k in (-1., 0., 0.25, 1.):
            w, wt = _iw_dev(ctx, lp, lq, k)
            wr = np.exp(lp - lq)
            assert np.all(np.abs(w - wr) <= 3 * np.spacing(wr)), (n, k)
            if k < 0:
                assert np.array_equal(wt, w)
                continue
            cap = np.mean(wr) * n**k
            assert np.all(np.abs(wt - np.clip(wr, 0, cap)) <= _iw_tol(n, wr, cap)), (n, k)
            assert np.all(wt <= w) and (k > 0 or n == 1 or np.any(wt < w))
            # the public wrapper: device tensors against the host route on the same inputs
            dw, dwt = importance_weights(ctx.tensor(lp), ctx.tensor(lq), k)
            hw, hwt = importance_weights(lp, lq, k)
            assert np.array_equal(dw.cpu().numpy(), w) and np.array_equal(dwt.cpu().numpy(), wt)
            assert np.all(np.abs(wt - hwt) <= _iw_tol(n, hw, cap))


@pytest.mark.gpu
@pytest.mark.parametrize('n', [5, 255, 256, 257, 65537, 200003])
def test_importance_weights_special_values_follow_the_host_route(n):
    """logp = -inf is a zero weight; +inf an infinite one (so an infinite cap); one NaN makes the cap NaN, so np.clip --
    the host route and the reference -- makes every truncated weight NaN, and so must the kernel."""
    from bayesfast_amd.core.refit import importance_weights
    ctx = _ctx()
    rng = np.random.default_rng(31)
    lq = rng.normal(size=n)
    base = rng.normal(size=n)
    cases = []
    for specials in (((0, -np.inf), (3, -np.inf)), ((1, np.inf),), ((n - 1, np.nan),), ((2, np.nan), (4, np.inf), (0, -np.inf))):
        lp = base.copy()
        for i, v in specials:
            lp[i] = v
        cases.append(lp)
    for lp in cases:
        for k in (-1., 0., 0.25, 1.):
            hw, hwt = importance_weights(lp, lq, k)
            dw, dwt = (t.cpu().numpy() for t in importance_weights(ctx.tensor(lp), ctx.tensor(lq), k))
            assert _same_nonfinite(dw, hw) and _same_nonfinite(dwt, hwt), (n, k, lp[:5])
            fin, finw = np.isfinite(hwt), np.isfinite(hw)
            cap = np.mean(hw) * n**k
            assert np.all(np.abs(dwt[fin] - hwt[fin]) <= _iw_tol(n, hw, cap)[fin])
            assert np.all(np.abs(dw[finw] - hw[finw]) <= 3 * np.spacing(hw[finw]))


# ---- bfhip_sort_keys / bfhip_order_keys / bfhip_count_keys ---------------------------------------------------------------

def _key_inputs(rng, n):
    """Normals, heavy ties, +-0, +-inf, NaNs of both signs with payloads, subnormals and +-DBL_MAX."""
    nan_bits = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff4000000000abc], dtype=np.uint64)
    special = np.concatenate((nan_bits.view(np.float64), [0., -0., np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -1e-310,
                                                          np.finfo(np.float64).max, -np.finfo(np.float64).max]))
    a = rng.normal(size=n)
    ties = rng.uniform(size=n) < 0.4
    a[ties] = rng.choice([-1., 0.5, 2., -0., 1e-310], size=int(ties.sum()))
    pos = rng.choice(n, size=min(n, 3 * special.size), replace=False)
    a[pos] = np.resize(special, pos.size)
    return a


def _sort_dev(ctx, a):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ad = ctx.tensor(a)
    keys = torch.zeros(a.size, dtype=torch.int64, device=ctx.device)
    order = torch.zeros(a.size, dtype=torch.int64, device=ctx.device)
    ok = torch.zeros(a.size, dtype=torch.int64, device=ctx.device)
    _lib.check(ctx._lib.bfhip_sort_keys(ctx.handle, a.size, _ptr(ad), _ptr(keys), _ptr(order)))
    _lib.check(ctx._lib.bfhip_order_keys(ctx.handle, a.size, _ptr(ad), _ptr(ok)))
    return keys.cpu().numpy().view(np.uint64), order.cpu().numpy(), ok.cpu().numpy().view(np.uint64)


def _count_dev(ctx, keys, q, upper):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    kd = ctx.tensor(keys.view(np.int64)) if keys.size else None
    qd = ctx.tensor(q.view(np.int64))
    out = torch.full((q.size,), -7, dtype=torch.int64, device=ctx.device)
    _lib.check(ctx._lib.bfhip_count_keys(ctx.handle, keys.size, _ptr(kd), q.size, _ptr(qd), upper, _ptr(out)))
    return out.cpu().numpy()


def _queries(rng, keys, nq):
    """Below, equal to, between and above the keys (uint64), nq of them."""
    top = np.uint64(0xffffffffffffffff)
    pool = [np.array([0, 1, top, top - np.uint64(1)], dtype=np.uint64)]
    if keys.size:
        pool += [keys, keys + np.uint64(1), keys - np.uint64(1), np.array([keys[0], keys[-1]], dtype=np.uint64)]
    pool = np.concatenate(pool)
    return rng.choice(pool, size=nq)


@pytest.mark.gpu
def test_sort_order_and_count_keys_against_numpy():
    ctx = _ctx()
    rng = np.random.default_rng(37)
    for n in (1, 2, 255, 256, 257, 4097, 2**20 + 3):
        a = _key_inputs(rng, n)
        keys, order, ok = _sort_dev(ctx, a)
        assert np.array_equal(order, np.argsort(a, kind='stable')), n
        assert np.all(keys[1:] >= keys[:-1])
        assert np.array_equal(ok[order], keys)                    # order_keys: the sort's key per element
        s = a[order]
        same = (s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1]))
        assert np.array_equal(keys[1:] == keys[:-1], same)        # equal keys exactly for equal values (or two NaNs)
        for nq in (1, 127, 128, 129, 10000):
            q = _queries(rng, keys, nq)
            for upper, side in ((0, 'left'), (1, 'right')):
                assert np.array_equal(_count_dev(ctx, keys, q, upper), np.searchsorted(keys, q, side=side)), (n, nq, upper)
    for nq in (1, 129):
        q = _queries(rng, np.zeros(0, dtype=np.uint64), nq)
        for upper in (0, 1):
            assert not _count_dev(ctx, np.zeros(0, dtype=np.uint64), q, upper).any()


@pytest.mark.gpu
def test_signed_key_wrappers_against_torch():
    import torch
    from bayesfast_amd.core.refit import device_sort, _device_count
    ctx = _ctx()
    rng = np.random.default_rng(41)
    for n in (1, 257, 4097, 2**20 + 3):
        a = _key_inputs(rng, n)
        keys, order = device_sort(ctx.tensor(a))
        assert np.array_equal(order.cpu().numpy(), np.argsort(a, kind='stable'))
        assert bool((keys[1:] >= keys[:-1]).all())
        for nq in (1, 128, 10000):
            q = keys[torch.as_tensor(rng.integers(0, n, size=nq), device=ctx.device)]
            q = torch.cat((q, q + 1, q - 1, torch.tensor([-2**63, 2**63 - 1], dtype=torch.int64, device=ctx.device)))
            for upper in (False, True):
                assert torch.equal(_device_count(keys, q, upper), torch.searchsorted(keys, q, right=upper)), (n, nq, upper)


# ---- refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_data_kernels_refuse_bad_arguments_and_skip_empty_calls():
    """Bad sizes and null pointers are refused by the host-side checks, naming the function, before anything is
    launched; zero-size calls return without writing their outputs."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    a = torch.zeros(8, dtype=torch.float64, device=ctx.device)
    i32 = torch.tensor([0, 2], dtype=torch.int32, device=ctx.device)
    out = torch.full((8,), 7., dtype=torch.float64, device=ctx.device)
    i64 = torch.full((8,), 7, dtype=torch.int64, device=ctx.device)
    A, O, I, K, N = _ptr(a), _ptr(out), _ptr(i32), _ptr(i64), None
    bad = {
        'bfhip_kde_cdf': [(0, 4, A, A, A, 2, A, O), (1, 0, A, A, A, 2, A, O), (1, 4, A, A, A, -1, A, O), (1, 4, N, A, A, 2, A, O),
                          (1, 4, A, N, A, 2, A, O), (1, 4, A, A, N, 2, A, O), (1, 4, A, A, A, 2, N, O), (1, 4, A, A, A, 2, A, N),
                          (1, 2**31, A, A, A, 2, A, O)],
        'bfhip_spline_apply': [(-1, 2, 1, A, I, A, A, A, O), (3, 2, 1, A, I, A, A, A, O), (0, -1, 1, A, I, A, A, A, O),
                               (0, 2, 0, A, I, A, A, A, O), (0, 2, 1, N, I, A, A, A, O), (0, 2, 1, A, N, A, A, A, O),
                               (0, 2, 1, A, I, N, A, A, O), (0, 2, 1, A, I, A, N, A, O), (0, 2, 1, A, I, A, A, N, O),
                               (0, 2, 1, A, I, A, A, A, N)],
        'bfhip_bridge_sums': [(0, A, 4, A, 0., O), (4, A, 0, A, 0., O), (-1, A, 4, A, 0., O), (4, N, 4, A, 0., O),
                              (4, A, 4, N, 0., O), (4, A, 4, A, 0., N)],
        'bfhip_bridge_terms': [(0, A, A, 4, A, A, 0., O, O), (4, A, A, 0, A, A, 0., O, O)]
                              + [tuple(N if i == j else v for i, v in enumerate((4, A, A, 4, A, A, 0., O, O))) for j in (1, 2, 4, 5, 7, 8)],
        'bfhip_importance_weights': [(-1, A, A, 0.25, O, O)]
                                    + [tuple(N if i == j else v for i, v in enumerate((4, A, A, 0.25, O, O))) for j in (1, 2, 4, 5)],
        'bfhip_sort_keys': [(-1, A, K, K), (4, N, K, K), (4, A, N, K), (4, A, K, N)],
        'bfhip_order_keys': [(-1, A, K), (4, N, K), (4, A, N)],
        'bfhip_count_keys': [(-1, K, 4, K, 0, K), (4, K, -1, K, 0, K), (4, N, 4, K, 0, K), (4, K, 4, N, 0, K), (4, K, 4, K, 1, N)],
        # the FastICA iteration: (n, n_pad, d, y, partial), (d, nb, p, n, n_pad, partial, w, a, meas_k -- may be null),
        # (d, w1, w, resid, k, n_meas, wbuf, meas), (d, a, x, n_iter, work, resid)
        'bfhip_ica_tanh': [(0, 4, 2, O, O), (4, 3, 2, O, O), (4, 4, 0, O, O), (4, 4, 2, N, O), (4, 4, 2, O, N)],
        'bfhip_ica_assemble': [(0, 1, A, 4, 4, A, A, O, N), (2, 0, A, 4, 4, A, A, O, N), (2, 1, A, 0, 4, A, A, O, N), (2, 1, A, 4, 3, A, A, O, N)]
                              + [tuple(N if i == j else v for i, v in enumerate((2, 1, A, 4, 4, A, A, O, O))) for j in (2, 5, 6, 7)],
        'bfhip_ica_post': [(0, A, O, A, 0, 2, O, O), (2, A, O, A, -1, 2, O, O), (2, A, O, A, 2, 2, O, O)]
                          + [tuple(N if i == j else v for i, v in enumerate((2, A, O, A, 0, 2, O, O))) for j in (1, 2, 3, 6, 7)],
        'bfhip_polar_ns': [(0, A, O, 1, O, O), (1025, A, O, 1, O, O), (2, A, O, -1, O, O)]
                          + [tuple(N if i == j else v for i, v in enumerate((2, A, O, 1, O, O))) for j in (1, 2, 4, 5)],
    }
    for name, arg_sets in bad.items():
        f = getattr(ctx._lib, name)
        for args in arg_sets:
            with pytest.raises(ValueError, match=name):
                _lib.check(f(ctx.handle, *args))
    # zero-size calls: valid, and nothing is written
    empty = [('bfhip_kde_cdf', (1, 4, A, A, A, 0, A, O)), ('bfhip_spline_apply', (0, 0, 1, A, I, A, A, A, O)),
             ('bfhip_spline_apply', (2, 0, 1, N, I, A, A, A, N)), ('bfhip_importance_weights', (0, A, A, 0.25, O, O)),
             ('bfhip_importance_weights', (0, N, N, 0.25, N, N)), ('bfhip_sort_keys', (0, A, K, K)), ('bfhip_sort_keys', (0, N, N, N)),
             ('bfhip_order_keys', (0, A, K)), ('bfhip_count_keys', (4, K, 0, K, 0, K)), ('bfhip_count_keys', (0, N, 0, N, 1, N))]
    for name, args in empty:
        _lib.check(getattr(ctx._lib, name)(ctx.handle, *args))
    torch.cuda.synchronize(ctx.device)
    assert out.cpu().numpy().tolist() == [7.] * 8 and i64.cpu().numpy().tolist() == [7] * 8
    # the unsupported size of the sort is refused on the host too
    with pytest.raises(NotImplementedError, match='bfhip_sort_keys'):
        _lib.check(ctx._lib.bfhip_sort_keys(ctx.handle, 2**31, A, K, K))
