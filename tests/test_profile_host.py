"""Profiles of the density without a GPU: the masked Newton iteration and the grid line of the device kernels compiled for the host
(tests/profile_host: bfhip_hess.h, bfhip_profile.h with a team of one thread), and the ``Profile`` object's arithmetic.

Expected values come from closed forms, from the oracle (helpers/profile_cases.py: a constrained damped Newton iteration on the
oracle's original-space density composed with the transform) or, for the one bit-identity check, from the existing maximiser of
tests/hess_host -- never from the code under test."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, 'helpers'), os.path.join(HERE, 'hess_host'), os.path.join(HERE, 'profile_host')):
    if p not in sys.path:
        sys.path.insert(0, p)

import laplace_cases as lc  # noqa: E402
import profile_cases as pfc  # noqa: E402

SAMPLING, ORIGINAL = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (a) the header on the host -----------------------------------------------------------------------------------------------------
def test_gaussian_profile_is_the_closed_form():
    """correlated_gaussian_spec(5), no link, no transform: along every coordinate the profile is f_max - (v - mu_i)^2 / (2 Sigma_ii)
    (1e-10 relative), the free coordinates sit at the conditional mean mu + Sigma_.i (v - mu_i) / Sigma_ii (1e-8), and every point
    has status 0 after at most two accepted iterations (Newton's step on a quadratic is exact; the second one measures zero).  Both
    objectives: without a transform they are one function, bit for bit."""
    import profile_host
    from bayesfast_amd.workloads import correlated_gaussian_spec
    d = 5
    spec, cov = correlated_gaussian_spec(d)
    spec = dict(spec, link=None)
    sd = np.sqrt(np.diag(cov))
    # (the values stay inside the bound's ellipsoid, where the surrogate is the quadratic itself: asserted below)
    for i in range(d):
        fixed = np.zeros(d, dtype=bool)
        fixed[i] = True
        vals = np.array([[0., 0.5, 1., 1.5, 2.], [0., -0.5, -1., -1.5, -2.]]) * sd[i]
        res = profile_host.profile_lines(spec, fixed, i, np.zeros((2, d)), vals, objective=ORIGINAL, max_iter=50, xtol=1e-6)
        res0 = profile_host.profile_lines(spec, fixed, i, np.zeros((2, d)), vals, objective=SAMPLING, max_iter=50, xtol=1e-6)
        for key in ('x', 'logp', 'info'):
            assert np.array_equal(_bits(res[key]), _bits(res0[key]))
        want_f = -vals**2 / (2. * cov[i, i])
        want_x = cov[:, i][None, None, :] * (vals / cov[i, i])[:, :, None]
        assert np.all(lc.bound_ratio(spec, want_x.reshape(-1, d), True)[0] < 1.)
        assert np.all(np.abs(res['logp'] - want_f) <= 1e-10 * np.maximum(1., np.abs(want_f)))
        assert np.max(np.abs(res['x'] - want_x)) <= 1e-8
        assert np.all(res['info'][..., 1] == 0) and np.all(res['info'][..., 0] <= 2)
        assert np.array_equal(_bits(res['x'][..., i]), _bits(vals))


@pytest.mark.parametrize('n_fixed', [1, 2, 5])
def test_fixed_coordinates_keep_their_bits(n_fixed):
    """t2_spec(6, 'cubic') behind hard bounds: whatever the iteration does (it starts where -H is indefinite, so damped steps are
    taken), a fixed coordinate leaves with the bits it came in with -- a negative zero and a denormal among them."""
    import profile_host
    d = 6
    spec, x0 = lc.t2_spec(d, 'cubic')
    rng = np.random.default_rng(50 + n_fixed)
    for trial in range(4):
        idx = rng.choice(d, n_fixed, replace=False)
        fixed = np.zeros(d, dtype=bool)
        fixed[idx] = True
        start = x0 + 0.1 * rng.normal(size=d)
        start[idx[0]] = -0.
        if n_fixed > 1:
            start[idx[1]] = 4.9e-324
        for objective in (SAMPLING, ORIGINAL):
            res = profile_host.profile_lines(spec, fixed, -1, start, None, objective=objective)
            assert np.array_equal(_bits(res['x'][0, 0][fixed]), _bits(start[fixed]))
            assert res['info'][0, 0, 1] == 0 and res['info'][0, 0, 0] >= 1
            assert not np.any(res['x'][0, 0][~fixed] == start[~fixed])
            # walked: the walk coordinate takes the value's bits, the others of the mask keep the start's
            w = int(idx[-1])
            vals = np.array([[start[w] + 0.25, -0., start[w] - 0.5]])
            res = profile_host.profile_lines(spec, fixed, w, start, vals, objective=objective)
            for k in range(3):
                want = start.copy()
                want[w] = vals[0, k]
                assert np.array_equal(_bits(res['x'][0, k][fixed]), _bits(want[fixed]))


def test_all_fixed_evaluates_once():
    """No free coordinate: status 0, 0 iterations, no division by zero (the step measure is finite), the point untouched and the
    value equal to the evaluation's -- the oracle's, minus the Jacobian sum under the original objective."""
    import profile_host
    from oracle import oracle as orc
    d = 6
    spec, x0 = lc.t2_spec(d, 'cubic')
    pts = x0 + 0.3 * np.random.default_rng(4).normal(size=(5, d))
    f0 = orc.logp_and_grad(spec, pts, original_space=False)[0]
    for objective, want in ((SAMPLING, f0), (ORIGINAL, f0 - pfc.log_jacobian(spec, pts))):
        res = profile_host.profile_lines(spec, np.ones(d, dtype=bool), -1, pts, None, objective=objective)
        assert np.array_equal(_bits(res['x'][:, 0]), _bits(pts))
        assert np.all(res['info'][:, 0, 0] == 0) and np.all(res['info'][:, 0, 1] == 0)
        assert np.all(np.isfinite(res['info']))
        assert np.all(np.abs(res['logp'][:, 0] - want) <= 1e-12 * np.maximum(1., np.abs(want)))   # (relative, as the maximiser's value checks: to max(1, |f|))
        fo = profile_host.objective(spec, pts, objective)[0]
        assert np.array_equal(_bits(res['logp'][:, 0]), _bits(fo))
    # and walked with everything fixed: every value is one evaluation at the moved point
    vals = np.array([[0.1, 0.2, 0.3]])
    res = profile_host.profile_lines(spec, np.ones(d, dtype=bool), 2, pts[:1], vals, objective=ORIGINAL)
    moved = np.repeat(pts[:1], 3, axis=0)
    moved[:, 2] = vals[0]
    want = orc.logp_and_grad(spec, moved, original_space=False)[0] - pfc.log_jacobian(spec, moved)
    assert np.all(np.abs(res['logp'][0] - want) <= 1e-12 * np.maximum(1., np.abs(want)))
    assert np.all(res['info'][0, :, :2] == 0)


def test_empty_mask_is_the_existing_maximiser_bit_for_bit():
    """Empty mask, walk = -1, sampling objective on t2_spec(6, 'cubic'): x, logp and info of ``hess_host.maximize``, bit for bit."""
    import hess_host
    import profile_host
    d = 6
    spec, x0 = lc.t2_spec(d, 'cubic')
    starts = np.concatenate((x0[None], x0 + 0.5 * np.random.default_rng(8).normal(size=(5, d))))
    x, f, H, info = hess_host.maximize(spec, starts, 200, 1e-5)
    res = profile_host.profile_lines(spec, np.zeros(d, dtype=bool), -1, starts, None, objective=SAMPLING, max_iter=200, xtol=1e-5)
    assert np.all(info[:, 0] >= 2)
    assert np.array_equal(_bits(res['x'][:, 0]), _bits(x))
    assert np.array_equal(_bits(res['logp'][:, 0]), _bits(f))
    assert np.array_equal(_bits(res['info'][:, 0]), _bits(info))


def test_original_objective_is_the_oracle_chained_through_the_transform():
    """The original objective's value and gradient are the oracle's original-space ones chained through T (1e-11), inside and
    outside the decay ellipsoid -- where the sampling-space gradient carries the decay term without the Jacobian, the objective
    carries it with -- and its Hessian diagonal is the central difference of that gradient (h = 1e-4, fourth order: the
    truncation is below 1e-9 of the entries here; 1e-7 asked).  The sampling objective is the evaluation itself, bit for bit."""
    import hess_host
    import profile_host
    d = 6
    spec, x0 = lc.t2_spec(d, 'decay')
    rng = np.random.default_rng(5)
    pts = np.concatenate((x0 + 0.3 * rng.normal(size=(4, d)), -0.5 + 0.15 * rng.normal(size=(4, d))))
    rd = lc.bound_ratio(spec, pts, False)[1]
    assert np.any(rd > 1.05) and np.any(rd < 0.95) and np.all(np.abs(rd - 1.) > 0.05)
    fs, gs, hs = profile_host.objective(spec, pts, SAMPLING)
    f1, g1, H1 = hess_host.logp_grad_hess(spec, pts, False)
    assert np.array_equal(_bits(fs), _bits(f1)) and np.array_equal(_bits(gs), _bits(g1))
    assert np.array_equal(_bits(hs), _bits(np.einsum('nii->ni', H1)))
    fo, go, ho = profile_host.objective(spec, pts, ORIGINAL)
    fr, gr = pfc.objective(spec, pts)
    np.testing.assert_allclose(fo, fr, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(go, gr, rtol=1e-11, atol=1e-11 * np.max(np.abs(gr)))
    h = 1e-4
    for i in range(d):
        e = np.zeros(d)
        e[i] = h
        D = lambda s: (pfc.objective(spec, pts + s * e)[1][:, i] - pfc.objective(spec, pts - s * e)[1][:, i]) / (2. * s * h)
        fd = (4. * D(1.) - D(2.)) / 3.
        np.testing.assert_allclose(ho[:, i], fd, rtol=1e-7, atol=1e-7 * np.max(np.abs(ho)))


# offsets of a line's values from the maximum, in the sampling coordinates.  On t2_spec(6, 'decay') the reference optima of the lines
# below lie at 0.36 to 0.91 of the decay surface's radius for the first three and at 1.23 to 2.37 for the last two; between 0.45 and
# 1.2 the ramp holds the conditional maximum ON the surface (check_line asserts that no value is there)
LINE_OFFSETS = np.array([0., 0.3, 0.45, 1.2, 1.5])


@pytest.mark.parametrize('kind', ['cubic', 'decay'])
def test_original_objective_under_hard_bounds(kind):
    """t2_spec(6, kind): lines of the original objective with one, two and d - 1 fixed coordinates against the constrained Newton
    iteration on the oracle (profile_cases.reference_line); tolerances of the maximiser's tests at every value -- status 0,
    mean |x - x*| <= xtol over the free coordinates, the value to 1e-9 relative.  With the decay term the lines have optima inside
    the ellipsoid and, where the term is on, outside it (asserted); none on the surface itself (check_line asserts it)."""
    import profile_host
    d = 6
    spec, x0 = lc.t2_spec(d, kind)
    xtol = 1e-6
    none = np.zeros(d, dtype=bool)
    top = profile_host.profile_lines(spec, none, -1, x0, None, objective=ORIGINAL, max_iter=200, xtol=xtol)
    pfc.check_line(spec, {k: v[0] for k, v in top.items()}, none, -1, x0, None, xtol)
    xm = top['x'][0, 0]
    rng = np.random.default_rng(21)
    n_in = n_out = 0
    for fixed, walk in pfc.masks(d, rng):
        for sign in (1., -1.):
            vals = xm[walk] + sign * LINE_OFFSETS
            res = profile_host.profile_lines(spec, fixed, walk, xm, vals[None], objective=ORIGINAL, max_iter=200, xtol=xtol)
            n_it = pfc.check_line(spec, {k: v[0] for k, v in res.items()}, fixed, walk, xm, vals, xtol)
            assert np.all(n_it <= 8)
            if kind == 'decay':
                rd = lc.bound_ratio(spec, res['x'][0], False)[1]
                n_in, n_out = n_in + int(np.sum(rd < 1.)), n_out + int(np.sum(rd > 1.))
    assert kind != 'decay' or (n_in == 18 and n_out == 12)


def test_a_conditional_maximum_on_the_decay_kink_is_flagged():
    """The decay term is gamma max(beta_d^2 - alpha_2, 0): across its surface the gradient jumps, and for a range of values the ramp
    holds the conditional maximum ON the surface, where no gradient vanishes (the reference iteration alternates between the two
    sides: asserted).  Pinned here on t2_spec(6, 'decay'), coordinate 1 at 0.6 above the maximum: the device iteration ends there
    with status 3 (a short step that is still damped) on the surface to 1e-3 of its radius, with a finite value that is not below
    either side's reference iterate by more than 1e-5 relative (the reference's two points are 1e-3 apart in value), the fixed
    coordinate keeps its bits, and the line goes on: the next value, off the surface, meets the full tolerances."""
    import profile_host
    d = 6
    spec, x0 = lc.t2_spec(d, 'decay')
    xtol = 1e-6
    fixed = np.arange(d) == 1
    xm = pfc.conditional_max(spec, x0, np.zeros(d, dtype=bool))[0]
    vals = xm[1] + np.array([0.45, 0.6, 1.2])
    xr, fr, gr = pfc.reference_line(spec, fixed, 1, xm, vals)
    assert pfc.on_a_kink(spec, xr[1]) and gr[1] > 1e-3 and not pfc.on_a_kink(spec, xr[0]) and not pfc.on_a_kink(spec, xr[2])
    res = profile_host.profile_lines(spec, fixed, 1, xm, vals[None], objective=ORIGINAL, max_iter=200, xtol=xtol)
    x, f, info = res['x'][0], res['logp'][0], res['info'][0]
    print('on the kink: status %d, %d iterations, last step %.3g, lambda %.3g, radius ratio %.6f, value %.9g (reference iterate %.9g)'
          % (info[1, 1], info[1, 0], info[1, 2], info[1, 3], lc.bound_ratio(spec, x[1:2], False)[1][0], f[1], fr[1]))
    assert info[1, 1] == 3 and info[1, 3] > 0. and np.isfinite(f[1])
    assert abs(lc.bound_ratio(spec, x[1:2], False)[1][0] - 1.) <= 1e-3
    assert f[1] >= fr[1] - 1e-5 * max(1., abs(fr[1]))
    assert np.array_equal(_bits(x[:, 1]), _bits(vals))
    for k in (0, 2):
        assert info[k, 1] == 0 and np.sum(np.abs(x[k] - xr[k])) / (d - 1) <= xtol and abs(f[k] - fr[k]) <= 1e-9 * max(1., abs(fr[k]))


def test_line_edge_cases():
    """A NaN value ends the line (NaN and status 4 from there on, the columns before it untouched by it); a NaN start gives status
    2 in every column; walk = -1 with more than one value, a walk coordinate outside the mask or out of range and an unknown
    objective are refused."""
    import profile_host
    d = 6
    spec, x0 = lc.t2_spec(d, 'cubic')
    fixed = np.zeros(d, dtype=bool)
    fixed[[1, 4]] = True
    vals = x0[1] + np.array([[0., 0.2, 0.4, 0.6]])
    full = profile_host.profile_lines(spec, fixed, 1, x0, vals, objective=ORIGINAL)
    cut = vals.copy()
    cut[0, 2] = np.nan
    res = profile_host.profile_lines(spec, fixed, 1, x0, cut, objective=ORIGINAL)
    for key in ('x', 'logp', 'info'):
        assert np.array_equal(_bits(res[key][0, :2]), _bits(full[key][0, :2]))
    assert np.all(np.isnan(res['x'][0, 2:])) and np.all(np.isnan(res['logp'][0, 2:])) and np.all(res['info'][0, 2:, 1] == 4)
    bad = x0.copy()
    bad[0] = np.nan
    res = profile_host.profile_lines(spec, fixed, 1, bad, vals, objective=ORIGINAL)
    assert np.all(res['info'][0, :, 1] == 2) and np.all(res['info'][0, :, 0] == 0)
    with pytest.raises(ValueError):
        profile_host.profile_lines(spec, fixed, -1, x0, vals)
    with pytest.raises(ValueError):
        profile_host.profile_lines(spec, fixed, 0, x0, vals)
    with pytest.raises(ValueError):
        profile_host.profile_lines(spec, fixed, d, x0, vals)
    with pytest.raises(ValueError):
        profile_host.profile_lines(spec, fixed, 1, x0, vals, objective=2)


# ---- (b) the Profile object ---------------------------------------------------------------------------------------------------------
def _synthetic(values, delta):
    from bayesfast_amd.utils import Profile
    v = np.asarray(values, dtype=np.float64)
    return Profile(x_max=[0.], logp_max=0., params=[0], values={0: v}, logp={0: -0.5 * np.asarray(delta)}, x={0: v[:, None]},
                   status={0: np.zeros(v.size, dtype=int)}, n_iter={0: np.zeros(v.size, dtype=int)})


@pytest.mark.parametrize('grid', ['centred', 'off_centre', 'coarse'])
def test_interval_of_a_parabola_is_mu_plus_minus_sigma(grid):
    """delta = (v - mu)^2 / sigma^2: the signed root is a straight line, so the linear interpolation is exact -- mu +- sigma at
    68.27 % and mu +- 2 sigma at 95.45 % to 1e-12 (relative to sigma), whether or not mu is a grid point."""
    from scipy.stats import chi2
    mu, sigma = 0.7, 0.3
    v = {'centred': mu + sigma * np.linspace(-4., 4., 21), 'off_centre': mu + 0.013 + sigma * np.linspace(-4., 4., 21),
         'coarse': mu + sigma * np.array([-3.1, -0.4, 0.9, 2.6])}[grid]
    p = _synthetic(v, (v - mu)**2 / sigma**2)
    for n_sigma in (1., 2.):
        level = chi2.cdf(n_sigma**2, 1)
        iv = p.interval(0, level)
        assert iv.lower_reached and iv.upper_reached
        assert abs(iv.lower - (mu - n_sigma * sigma)) <= 1e-12 * sigma and abs(iv.upper - (mu + n_sigma * sigma)) <= 1e-12 * sigma
    assert np.array_equal(p.delta[0], (v - mu)**2 / sigma**2)


def test_interval_that_never_reaches_the_threshold_is_flagged():
    """A profile too flat on one side (and one cut short by not-run points): that side returns the grid's end and False."""
    v = np.linspace(-1., 1., 11)
    delta = np.where(v < 0., 0.2 * v**2, 9. * v**2)   # the left side ends at delta = 0.2 < 1
    iv = _synthetic(v, delta).interval(0)
    assert iv.lower == -1. and not iv.lower_reached
    from scipy.stats import chi2
    assert iv.upper_reached and abs(iv.upper - np.sqrt(chi2.ppf(0.6827, 1)) / 3.) <= 1e-12   # (delta = 9 v^2 reaches the quantile)
    delta = 9. * v**2
    delta[:3] = np.nan
    delta[3:5] = 0.01   # finite but below the threshold up to the last run point, v[3]
    iv = _synthetic(v, delta).interval(0)
    assert iv.lower == v[3] and not iv.lower_reached and iv.upper_reached


def test_levels2d_and_the_not_converged_count():
    """Two degrees of freedom: the chi-square quantile is -2 log(1 - p) (scipy's to 1e-12); n_not_converged counts every status but
    0 and 4 over the maximisation from x_0, the 1-D and the 2-D points."""
    from scipy.stats import chi2
    from bayesfast_amd.utils import Profile
    levels = (0.6827, 0.9545, 0.9973)
    np.testing.assert_allclose(Profile.levels2d(levels), chi2.ppf(levels, 2), rtol=1e-12)
    np.testing.assert_allclose(Profile.levels2d(), chi2.ppf((0.6827, 0.9545), 2), rtol=1e-12)
    p = _synthetic(np.arange(5.), np.arange(5.))
    p.status[0] = np.array([0, 1, 4, 3, 0])
    p.status2d[(0, 1)] = np.array([[0, 2], [4, 0]])
    assert p.n_not_converged == 3 and p.status_max == 0
    p.status_max = 3   # the maximisation from x_0 counts too
    assert p.n_not_converged == 4


# ---- (c) profile() on a stand-in device: the host build behind DeviceDensity's interface ------------------------------------------------
class _HostDevice:
    """What ``profile`` uses of a ``DeviceDensity`` of a scalar spec, answered by the host builds (profile_host, hess_host) and the
    NumPy transform of laplace_cases: the driver's grids, launches and bookkeeping run without a GPU."""

    def __init__(self, spec):
        self.spec, self.d = spec, int(spec['d'])
        self.launches = []

    def profile_lines(self, fixed, walk, x_start, values=None, objective='original', max_iter=50, xtol=1e-6):
        import profile_host
        import torch
        out = profile_host.profile_lines(self.spec, fixed, walk, x_start, values, objective={'sampling': 0, 'original': 1}[objective],
                                         max_iter=max_iter, xtol=xtol)
        self.launches.append(out['logp'].shape)
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def logp_grad_hess(self, x, original_space=False):
        import hess_host
        import torch
        f, g, H = hess_host.logp_grad_hess(self.spec, np.atleast_2d(x), original_space)
        return torch.as_tensor(f[0]), torch.from_numpy(g[0]), torch.from_numpy(H[0])

    def constraint(self, which, x):
        import torch
        return torch.from_numpy({'to_original': lc.to_original, 'from_original': lc.from_original}[which](self.spec, x))


def test_profile_driver_on_a_gaussian():
    """``profile`` on correlated_gaussian_spec(5) through the stand-in: three launches (maximum, 1-D, 2-D); delta[i] =
    (v - mu_i)^2 / Sigma_ii and delta2d the quadratic form of the 2 x 2 marginal covariance to 1e-8; the default scale is
    sqrt(Sigma_ii), so the default grid is mu +- 4 sigma with the maximum its centre; interval at the one-sigma level is
    mu +- sigma to 1e-6."""
    from scipy.stats import chi2
    from bayesfast_amd.utils import profile as profile_fn
    from bayesfast_amd.workloads import correlated_gaussian_spec
    d = 5
    spec, cov = correlated_gaussian_spec(d, fit_scale=3.)   # (a wide bound: mu +- 4 sigma with the conditional means stays inside)
    spec = dict(spec, link=None)
    dev = _HostDevice(spec)
    p = profile_fn(dev, x_0=0.3 * np.ones(d), pairs='all', n_grid=9)
    assert len(dev.launches) == 3 and dev.launches[0] == (1, 1) and dev.launches[1][0] == 2 * d and dev.launches[2][0] == 10 * 9 * 2
    assert p.n_not_converged == 0 and p.improved_at == []
    sd = np.sqrt(np.diag(cov))
    np.testing.assert_allclose(p.scale, sd, rtol=1e-10)
    for i in range(d):
        v = p.values[i]
        np.testing.assert_allclose(v, sd[i] * np.linspace(-4., 4., 9), atol=1e-9)
        pts = np.outer(v / cov[i, i], cov[:, i])
        assert np.all(lc.bound_ratio(spec, pts, True)[0] < 1.)   # (condition on the inputs: the quadratic itself, no extrapolation)
        assert np.max(np.abs(p.delta[i] - v**2 / cov[i, i])) <= 1e-8 * 16.
        np.testing.assert_allclose(p.x[i], pts, atol=1e-7)
        iv = p.interval(i, chi2.cdf(1., 1))
        assert abs(iv.lower + sd[i]) <= 1e-6 and abs(iv.upper - sd[i]) <= 1e-6 and iv.lower_reached and iv.upper_reached
    for i, j in p.pairs:
        vi, vj = p.values2d[(i, j)]
        P2 = np.linalg.inv(cov[np.ix_([i, j], [i, j])])
        want = P2[0, 0] * vi[:, None]**2 + 2. * P2[0, 1] * vi[:, None] * vj[None, :] + P2[1, 1] * vj[None, :]**2
        inside = want <= 20.   # (the corners of the 4 sigma box lie outside the bound's ellipsoid, where the surrogate extrapolates)
        assert inside.sum() >= 40
        assert np.max(np.abs(p.delta2d[(i, j)] - want)[inside]) <= 1e-8 * 20.


def test_profile_driver_behind_hard_bounds_and_a_local_maximum():
    """t2_spec(6, 'cubic') through the stand-in, explicit and default grids: every delta >= -1e-9, the centre's delta is 0 to 1e-9,
    the grid is in original units inside the bounds; an explicit grid is used as given.  And a start that is held at a worse point
    (max_iter = 0: the 'maximum' is x_0 itself) is found out: improved_at is not empty, logp_max is the best value seen and no delta
    is negative."""
    from bayesfast_amd.utils import profile
    d = 6
    spec, x0 = lc.t2_spec(d, 'cubic')
    dev = _HostDevice(spec)
    xo0 = lc.to_original(spec, x0)
    p = profile(dev, x_0=xo0, params=[0, 2, 5], pairs=[(0, 5)], n_grid=7, span=2., max_iter=100)
    assert p.n_not_converged == 0 and p.improved_at == []
    xr = pfc.conditional_max(spec, x0, np.zeros(d, dtype=bool))[0]
    np.testing.assert_allclose(p.x_max, lc.to_original(spec, xr), atol=1e-5)
    for i in p.params:
        assert np.all(p.delta[i] >= -1e-9) and abs(p.delta[i][3]) <= 1e-9 and abs(p.values[i][3] - p.x_max[i]) <= 1e-12
        assert np.all(p.values[i] > -3.) and np.all(p.values[i] < 5.) and np.all(np.diff(p.values[i]) > 0)
    assert np.all(p.delta2d[(0, 5)] >= -1e-9) and np.all(p.delta2d[(0, 5)].min(axis=1) >= p.delta[0] - 1e-9)
    g = {2: p.x_max[2] + np.array([-0.4, -0.1, 0.2, 0.6])}
    pg = profile(dev, x_0=xo0, params=[2], grid=g, max_iter=100)
    np.testing.assert_allclose(pg.values[2], g[2], rtol=1e-12)
    assert np.all(pg.delta[2] > 0) and pg.n_not_converged == 0
    fr = [pfc.reference_line(spec, np.arange(d) == 2, 2, xr, lc.from_original(spec, np.where(np.arange(d) == 2, v, p.x_max))[2:3])[1][0]
          for v in g[2]]
    np.testing.assert_allclose(pg.logp[2], fr, rtol=1e-9)
    # nothing iterates (max_iter = 0): the "maximum" is x_0 itself and every grid point stays where it starts, so some beat it
    bad = profile(dev, x_0=xo0, params=[0, 1], n_grid=5, max_iter=0, scale=np.ones(d))
    best = max(np.max(bad.logp[0]), np.max(bad.logp[1]))
    assert bad.improved_at and {w for w, f in bad.improved_at} <= {0, 1} and bad.logp_max == best
    assert bad.logp_max > float(dev.logp_grad_hess(x0)[0]) - float(pfc.log_jacobian(spec, x0))
    assert all(np.all(bad.delta[i] >= 0.) for i in (0, 1)) and bad.status_max == 1 and bad.n_not_converged == 11
    # with the pair, the best point seen is a 2-D one (both coordinates moved towards the maximum): x_max is that point, fetched from
    # the 2-D launch, and logp_max is the oracle's value there
    bad2 = profile(dev, x_0=xo0, params=[0, 1], pairs=[(0, 1)], n_grid=5, max_iter=0, scale=np.ones(d))
    assert bad2.logp_max == np.max(bad2.logp2d[(0, 1)]) > best and ((0, 1), bad2.logp_max) in bad2.improved_at
    assert np.all(bad2.delta2d[(0, 1)] >= 0.) and all(np.all(bad2.delta[i] >= 0.) for i in (0, 1))
    a, b = np.unravel_index(np.argmax(bad2.logp2d[(0, 1)]), (5, 5))
    assert bad2.x_max[0] == bad2.values[0][a] and bad2.x_max[1] == bad2.values[1][b] and np.array_equal(bad2.x_max[2:], xo0[2:])
    f_at = pfc.objective(spec, lc.from_original(spec, bad2.x_max))[0][0]
    assert abs(f_at - bad2.logp_max) <= 1e-12 * max(1., abs(f_at))


def test_abi_has_the_profile_calls():
    """The two exports are in the binding table with the header's argument counts, the constants agree with the header, and the
    version is at least 112."""
    import re
    from bayesfast_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'bfhip.h')).read()
    assert _lib.lib().bfhip_version() >= 112
    for name, n_arg in (('bfhip_profile_lines', 12), ('bfhip_pipeline_profile_lines', 13)):
        assert len(_lib.SYMBOLS[name][1]) == n_arg
        decl = re.search(r'int %s\(([^;]*)\);' % name, hdr).group(1)
        assert decl.count(',') + 1 == n_arg
    for key, value in (('SAMPLING', _lib.PROFILE_SAMPLING), ('ORIGINAL', _lib.PROFILE_ORIGINAL), ('NOT_RUN', _lib.PROFILE_NOT_RUN)):
        assert int(re.search(r'#define BFHIP_PROFILE_%s (\d+)' % key, hdr).group(1)) == value
    from bayesfast_amd.device import DeviceDensity
    assert DeviceDensity.MAXIMIZE_STATUS[_lib.PROFILE_NOT_RUN] == 'not run' and len(DeviceDensity.MAXIMIZE_STATUS) == 5
