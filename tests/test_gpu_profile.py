"""GPU: profiles of the device density along grid lines (bfhip_profile_lines, bfhip_pipeline_profile_lines) and the public
``profile`` / ``Profile`` built on them.

Every expected value comes from a closed form, from the CPU oracle (helpers/profile_cases.py: a constrained damped Newton iteration on
the oracle's original-space density composed with the transform) or, for the bit-identity checks, from the existing maximiser entry
points and from other launches of the same call -- never from the code under test alone."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import laplace_cases as lc  # noqa: E402
import pipeline_hess_cases as pc  # noqa: E402
import profile_cases as pfc  # noqa: E402


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(_bits(a[k][rows_a]), _bits(b[k][rows_b])) for k in ('x', 'logp', 'info'))


def _report(what, n_it):
    """The accepted Newton iterations per grid point of a checked line (continuation, no tangent predictor): printed, for the record."""
    print('%s: iterations per grid point mean %.2f, max %d' % (what, np.mean(n_it), np.max(n_it)))


# ---- 1: the lines against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 16, 64, 128])
def test_scalar_lines_reach_the_reference(ctx, d):
    """t2_spec(d) behind hard bounds (cubic terms from d = 16 on; 64 threads below d = 32, 256 above; 152 KB of LDS at d = 128):
    the maximum of the original objective, then a 3-value line for each of three masks (one, two and d - 1 fixed coordinates; at
    d = 2 one coordinate is free) against the constrained Newton iteration on the oracle.  Tolerances of the maximiser's tests:
    status 0, mean |x - x*| <= xtol over the free coordinates, the value to 1e-9 relative; fixed coordinates keep their bits."""
    from bayesfast_amd.device import DeviceDensity
    spec, x0 = lc.t2_spec(d, 'cubic' if d >= 16 else 'quadratic')
    dd = DeviceDensity(spec, ctx)
    xtol = 1e-6
    none = np.zeros(d, dtype=bool)
    top = _np(dd.profile_lines(none, -1, x0, None, objective='original', max_iter=200, xtol=xtol))
    pfc.check_line(spec, {k: v[0] for k, v in top.items()}, none, -1, x0, None, xtol)
    xm = top['x'][0, 0]
    cases = pfc.masks(d, np.random.default_rng(40 + d))
    fixed = np.array([m for m, w in cases])
    walk = np.array([w for m, w in cases])
    vals = xm[walk][:, None] + np.array([0.25, 0.5, 0.75])[None] * np.array([1., -1., 1.])[:, None]
    res = _np(dd.profile_lines(fixed, walk, np.repeat(xm[None], 3, axis=0), vals, objective='original', max_iter=200, xtol=xtol))
    for l in range(3):
        n_it = pfc.check_line(spec, {k: v[l] for k, v in res.items()}, fixed[l], int(walk[l]), xm, vals[l], xtol)
        _report('scalar d %d, %d fixed' % (d, fixed[l].sum()), n_it)


@pytest.mark.parametrize('gauss_newton', [False, True])
@pytest.mark.parametrize('shape', [(40, 9, 4), (100, 27, 9), (24, 70, 6), (40, 27, 27)])
def test_pipeline_lines_reach_the_reference(ctx, shape, gauss_newton):
    """maximiser_spec at the shapes where the kernels' paths differ (compressed outputs, several tiles, d > 64, the eight-chain
    layout), full and Gauss-Newton matrix, both objectives: the maximum, then a 5-value line along two different coordinates against
    the reference (same tolerances as the scalar lines); the returned value equals ``logp_and_grad`` at the returned point, minus
    the Jacobian sum under the original objective, to 1e-12 relative.
    The wide shape has 24 outputs and a prior on 35 of its 70 inputs: 59 conditions on 70 parameters, so the original-space density
    has a manifold of maxima (its value there is the perfect fit's, 0) and no reference POINT exists; only the log-Jacobian of the
    sampling objective makes the maximum unique.  A property of the inputs, asserted below: that shape's lines are held to the
    reference under the sampling objective only; under the original objective they are held to what needs no unique optimum (the
    perfect fit's value at the top, finite flagged results, the fixed coordinates' bits, the value against ``logp_and_grad``)."""
    from bayesfast_amd.device import DeviceDensity
    m, d, nq = shape
    spec, x0 = pc.maximiser_spec(m, d, nq)
    dd = DeviceDensity(spec, ctx)
    xtol = 1e-6
    none = np.zeros(d, dtype=bool)
    determined = m + int(np.count_nonzero(spec['prior']['prec_diag'])) >= d
    assert determined == (shape != (24, 70, 6))
    walk = np.array([1, d - 2])
    fixed = np.zeros((2, d), dtype=bool)
    fixed[0, 1] = fixed[1, d - 2] = fixed[1, 0] = True   # (the second line holds one more coordinate than it walks)
    for objective in ('sampling', 'original'):
        kw = dict(objective=objective, max_iter=200, xtol=xtol, gauss_newton=gauss_newton)
        original = objective == 'original'
        top = _np(dd.pipeline_profile_lines(none, -1, x0, None, **kw))
        unique = determined or not original
        if unique:
            pfc.check_line(spec, {k: v[0] for k, v in top.items()}, none, -1, x0, None, xtol, original)
        else:
            assert top['info'][0, 0, 1] in (0, 3) and abs(top['logp'][0, 0]) <= 1e-9   # (the perfect fit)
        xm = top['x'][0, 0]
        vals = xm[walk][:, None] + 0.15 * np.arange(5)[None] * np.array([1., -1.])[:, None]
        res = _np(dd.pipeline_profile_lines(fixed, walk, np.repeat(xm[None], 2, axis=0), vals, **kw))
        for l in range(2):
            if unique:
                n_it = pfc.check_line(spec, {k: v[l] for k, v in res.items()}, fixed[l], int(walk[l]), xm, vals[l], xtol, original)
                _report('pipeline %r gauss_newton %d %s' % (shape, gauss_newton, objective), n_it)
            else:   # what holds whether or not the optimum is unique: a run, finite line whose fixed coordinates keep their bits
                want = np.repeat(xm[None], 5, axis=0)
                want[:, walk[l]] = vals[l]
                assert np.array_equal(_bits(res['x'][l][:, fixed[l]]), _bits(want[:, fixed[l]]))
                assert np.all(np.isin(res['info'][l, :, 1], (0, 1, 3))) and np.all(np.isfinite(res['logp'][l])) and np.all(np.isfinite(res['x'][l]))
        # (relative as the maximiser's value checks are: to max(1, |f|); the perfect fit's value is 0)
        pts = res['x'].reshape(-1, d)
        f = dd.logp_and_grad(pts, False)[0].cpu().numpy() - (pfc.log_jacobian(spec, pts) if original else 0.)
        assert np.all(np.abs(res['logp'].ravel() - f) <= 1e-12 * np.maximum(1., np.abs(f)))


# ---- 2: bit identity with the maximiser ----------------------------------------------------------------------------------------------
def test_empty_mask_is_the_maximiser_bit_for_bit(ctx):
    """Empty mask, walk = -1, sampling objective: x, logp and info of ``maximize`` (d = 16 and 64: both block sizes) and of
    ``pipeline_maximize`` (full and Gauss-Newton), bit for bit."""
    from bayesfast_amd.device import DeviceDensity
    for d in (16, 64):
        spec, x0 = lc.t2_spec(d, 'cubic')
        starts = np.concatenate((x0[None], x0 + 0.3 * np.random.default_rng(d).normal(size=(6, d))))
        dd = DeviceDensity(spec, ctx)
        want = _np(dd.maximize(starts, max_iter=200, xtol=1e-5))
        got = _np(dd.profile_lines(np.zeros(d, dtype=bool), -1, starts, None, objective='sampling', max_iter=200, xtol=1e-5))
        assert np.all(want['info'][:, 0] >= 2)
        assert _same({k: got[k][:, 0] for k in got}, want)
    spec, x0 = pc.maximiser_spec(40, 9, 4)
    starts = x0 + 0.1 * np.random.default_rng(5).normal(size=(7, 9))
    dd = DeviceDensity(spec, ctx)
    for gn in (False, True):
        want = _np(dd.pipeline_maximize(starts, max_iter=200, xtol=1e-5, gauss_newton=gn))
        got = _np(dd.pipeline_profile_lines(np.zeros(9, dtype=bool), -1, starts, None, objective='sampling', max_iter=200, xtol=1e-5,
                                            gauss_newton=gn))
        assert np.all(want['info'][:, 0] >= 2)
        assert _same({k: got[k][:, 0] for k in got}, want)


# ---- 3: lines are independent ------------------------------------------------------------------------------------------------------
def test_lines_do_not_depend_on_the_launch(ctx):
    """600 lines of 4 values on the 9-input pipeline shape -- more than the grid's cap of two workgroups per CU, so workgroups walk
    over several lines: any 20 of them alone equal the launch's results bit for bit; a line whose start is NaN has status 2 in every
    column and a NaN-terminated line status 4 and NaN behind the terminator, with the values before it and every neighbour's bits
    unchanged."""
    from bayesfast_amd.device import DeviceDensity
    spec, x0 = pc.maximiser_spec(40, 9, 4)
    d, n, n_val = 9, 600, 4
    dd = DeviceDensity(spec, ctx)
    rng = np.random.default_rng(11)
    starts = x0 + 0.1 * rng.normal(size=(n, d))
    walk = rng.integers(0, d, size=n)
    fixed = np.zeros((n, d), dtype=bool)
    fixed[np.arange(n), walk] = True
    fixed[np.arange(n), (walk + 1 + rng.integers(0, d - 1, size=n)) % d] |= rng.random(n) < 0.5
    vals = starts[np.arange(n), walk][:, None] + 0.1 * np.arange(n_val)[None] * rng.choice([-1., 1.], size=n)[:, None]
    clean = _np(dd.pipeline_profile_lines(fixed, walk, starts, vals, max_iter=100, xtol=1e-6))
    assert not np.any(np.isin(clean['info'][..., 1], (2, 4))) and np.mean(clean['info'][..., 1] == 0) > 0.9   # (conditions on the inputs)
    bad_start, cut = 301, 555
    starts2, vals2 = starts.copy(), vals.copy()
    starts2[bad_start, (walk[bad_start] + 1) % d] = np.nan
    vals2[cut, 2] = np.nan
    res = _np(dd.pipeline_profile_lines(fixed, walk, starts2, vals2, max_iter=100, xtol=1e-6))
    others = np.setdiff1d(np.arange(n), [bad_start, cut])
    assert _same(res, clean, others, others)
    assert np.all(res['info'][bad_start, :, 1] == 2) and np.all(res['info'][bad_start, :, 0] == 0)
    assert _same(res, clean, (cut, slice(0, 2)), (cut, slice(0, 2)))
    assert np.all(res['info'][cut, 2:, 1] == 4) and np.all(np.isnan(res['logp'][cut, 2:])) and np.all(np.isnan(res['x'][cut, 2:]))
    rows = np.sort(rng.choice(n, 20, replace=False))
    rows[:3] = [0, bad_start, cut]
    sub = _np(dd.pipeline_profile_lines(fixed[rows], walk[rows], starts2[rows], vals2[rows], max_iter=100, xtol=1e-6))
    assert _same(sub, res, slice(None), rows)
    one = _np(dd.pipeline_profile_lines(fixed[599], int(walk[599]), starts2[599], vals2[599:600], max_iter=100, xtol=1e-6))
    assert _same(one, res, slice(None), slice(599, 600))


# ---- 4: the public interface -------------------------------------------------------------------------------------------------------
def test_profile_of_a_gaussian_is_the_closed_form(ctx):
    """A pipeline with linear outputs and no transform is a Gaussian posterior N(mu, Sigma) (profile_cases.linear_gaussian_spec,
    d = 9), so with ``pairs='all'``: delta[i] = (v - mu_i)^2 / Sigma_ii and delta2d = the quadratic form of the 2 x 2 marginal
    covariance, both to 1e-8; interval(i) at the one-sigma level chi2.cdf(1, 1) = mu_i +- sqrt(Sigma_ii) to 1e-6 (the default
    level, 0.6827, is that level rounded: its quantile is 1.0000217, which moves the ends by 1.1e-5 sigma, so it is held to its own
    quantile); n_not_converged == 0; no grid point beats the maximum."""
    from scipy.stats import chi2
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.utils import profile
    spec, mu, cov = pfc.linear_gaussian_spec(40, 9)
    d = 9
    dd = DeviceDensity(spec, ctx)
    p = profile(dd, x_0=mu + 0.2 * np.random.default_rng(2).normal(size=d), pairs='all', n_grid=11)
    assert p.n_not_converged == 0 and p.improved_at == [] and len(p.pairs) == 36
    np.testing.assert_allclose(p.x_max, mu, atol=1e-6)
    for i in range(d):
        v = p.values[i]
        assert v.size == 11 and np.all(np.diff(v) > 0)
        want = (v - mu[i])**2 / cov[i, i]
        assert np.max(np.abs(p.delta[i] - want)) <= 1e-8 * max(1., np.max(want))
        np.testing.assert_allclose(p.x[i], mu + np.outer((v - mu[i]) / cov[i, i], cov[:, i]), atol=1e-6)
        sd = np.sqrt(cov[i, i])
        iv = p.interval(i, level=chi2.cdf(1., 1))
        assert iv.lower_reached and iv.upper_reached and abs(iv.lower - (mu[i] - sd)) <= 1e-6 and abs(iv.upper - (mu[i] + sd)) <= 1e-6
        iv, q = p.interval(i), np.sqrt(chi2.ppf(0.6827, 1))
        assert abs(iv.lower - (mu[i] - q * sd)) <= 1e-6 and abs(iv.upper - (mu[i] + q * sd)) <= 1e-6
        _report('profile() gaussian 1-D', p.n_iter[i])
    for i, j in p.pairs:
        vi, vj = p.values2d[(i, j)]
        P2 = np.linalg.inv(cov[np.ix_([i, j], [i, j])])
        di, dj = (vi - mu[i])[:, None], (vj - mu[j])[None, :]
        want = P2[0, 0] * di**2 + 2. * P2[0, 1] * di * dj + P2[1, 1] * dj**2
        assert p.delta2d[(i, j)].shape == (11, 11) and np.all(p.status2d[(i, j)] == 0)
        assert np.max(np.abs(p.delta2d[(i, j)] - want)) <= 1e-8 * max(1., np.max(want))
    _report('profile() gaussian 2-D', np.concatenate([p.n_iter2d[q].ravel() for q in p.pairs]))


def test_profile_behind_the_transform_and_from_a_trace(ctx):
    """maximiser_spec as it is (hard bounds, input scales, prior): every delta >= -1e-9, delta at the centre grid point is 0 (to
    1e-9: the centre point is one more Newton step from the converged maximum), the grid is reported in original units around
    x_max; ``TraceTuple.profile`` on a short run (64 chains x 200 draws) returns intervals that contain x_max."""
    import bayesfast_amd as bfa
    from bayesfast_amd.utils import profile
    spec, x0 = pc.maximiser_spec(40, 9, 4)
    d = 9
    den = pfc.spec_density(spec, ctx)
    p = profile(den, x_0=lc.to_original(spec, x0), pairs=[(0, 3), (2, 7)], n_grid=9, span=3.)
    assert p.n_not_converged == 0
    lo, hi = spec['ranges'][:, 0], spec['ranges'][:, 1]
    xr = pfc.conditional_max(spec, x0, np.zeros(d, dtype=bool))[0]
    np.testing.assert_allclose(p.x_max, lc.to_original(spec, xr), atol=1e-5)
    for i in range(d):
        assert np.all(p.delta[i] >= -1e-9) and abs(p.delta[i][4]) <= 1e-9
        assert abs(p.values[i][4] - p.x_max[i]) <= 1e-12 and np.all(p.values[i] > lo[i]) and np.all(p.values[i] < hi[i])
    for q in p.pairs:
        assert np.all(p.delta2d[q] >= -1e-9) and np.all(p.status2d[q] == 0)
        # the 2-D profile's minimum over j at a fixed value of i is the 1-D profile of i (on the grid: not below it)
        assert np.all(p.delta2d[q].min(axis=1) >= p.delta[q[0]] - 1e-9)
    rng = np.random.default_rng(3)
    tt = bfa.sample(den, bfa.NTrace(n_chain=64, n_iter=250, n_warmup=50, x_0=lc.to_original(spec, x0 + 0.1 * rng.normal(size=(64, d))),
                                    random_generator=5), verbose=False)
    pt = tt.profile(den, n_grid=9)
    np.testing.assert_allclose(pt.x_max, p.x_max, atol=1e-5)
    for i in range(d):
        iv = pt.interval(i)
        assert iv.lower_reached and iv.upper_reached and iv.lower < pt.x_max[i] < iv.upper
        assert np.all(pt.delta[i] >= -1e-9)


def test_refusals(ctx):
    """The streamed form raises NotImplementedError (the lines and ``profile``); a walk coordinate outside the mask, walk = -1 with
    several values and an unknown objective raise ValueError; a scalar density passed to the pipeline call, and the reverse, raise
    as the maximiser's entry points do; the context stays usable."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.utils import profile
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec = pc.streamed_spec()
    d = spec['d']
    sd = DeviceDensity(spec, ctx)
    fixed = np.zeros(d, dtype=bool)
    fixed[3] = True
    with pytest.raises(NotImplementedError, match='streamed'):
        sd.pipeline_profile_lines(fixed, 3, np.zeros((1, d)), np.zeros((1, 2)))
    with pytest.raises(NotImplementedError, match='streamed'):
        profile(sd, params=[0])
    gspec = correlated_gaussian_spec(16)[0]
    gd = DeviceDensity(gspec, ctx)
    with pytest.raises(NotImplementedError, match='scalar surrogate density'):
        gd.pipeline_profile_lines(np.ones(16, dtype=bool), 3, np.zeros((1, 16)), np.zeros((1, 2)))
    mspec, x0 = pc.maximiser_spec(40, 9, 4)
    md = DeviceDensity(mspec, ctx)
    with pytest.raises(NotImplementedError, match='pipeline density'):
        md.profile_lines(np.ones(9, dtype=bool), 3, x0[None], np.zeros((1, 2)))
    fixed = np.zeros(9, dtype=bool)
    fixed[3] = True
    with pytest.raises(ValueError, match='not in the line'):
        md.pipeline_profile_lines(fixed, 4, x0[None], np.zeros((1, 2)))
    with pytest.raises(ValueError):
        md.pipeline_profile_lines(fixed, 9, x0[None], np.zeros((1, 2)))
    with pytest.raises(ValueError, match='n_val == 1'):
        md.pipeline_profile_lines(fixed, -1, x0[None], np.zeros((1, 2)))
    with pytest.raises(ValueError):
        md.pipeline_profile_lines(fixed, 3, x0[None], np.zeros((1, 2)), objective='neither')
    with pytest.raises(ValueError, match='not in the line'):
        gd.profile_lines(np.zeros(16, dtype=bool), 2, np.zeros((1, 16)), np.zeros((1, 2)))
    out = _np(md.pipeline_profile_lines(fixed, 3, x0[None], x0[3] + np.zeros((1, 1))))
    assert out['info'][0, 0, 1] == 0
