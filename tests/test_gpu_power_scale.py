"""Power-scaling sensitivity on the device (csrc/bfhip_pscale.h: ``bfhip_rw_weights``; csrc/bfhip_pscale.hip: ``bfhip_pscale_cjs``)
through ctypes and through ``bayesfast_amd.utils.power_scale`` / ``data_power_scale``, against the loop-written references of
helpers/power_scale_reference.py.

Sizes.  ``bfhip_rw_weights``: those of helpers/reweight_cases.py (1 .. 262145; tests/test_gpu_data_reweight.py says what each is for).
``bfhip_pscale_cjs``: n = 1 | 2 | 3 no bin, one, two; 255 .. 257 a workgroup's threads; TILE - 1 .. TILE + 1 a second tile of 2048
sorted positions; 256 TILE + 1 = 524289: 257 tiles, so that every one of the offsets kernel's 16 slices holds 16 tiles or more and the
finish kernel's slices walk 16 tiles each (the loop reference takes minutes there: the vector restatement of the cases, held to the
loop at the smaller sizes).

Tolerances.  Keys, rows, flags, NaN patterns, untouched columns and the exact zeros are exact.  Floating figures are held to 1e-9
relative, the project's figure for a device route against a loop reference; ten times what rounding alone does to the reference on
the cases' inputs (float64 against numpy.longdouble, on the CPU, by helpers/power_scale_cases.py; docs/EXPERIMENTS.md has the table)
is below it for every figure: ``ROUNDING`` in the cases, 4.7e-11 for cjs at the most.  Each test prints its figures before it asserts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, 'helpers')):
    if p not in sys.path:
        sys.path.insert(0, p)

import data_loo_reference as dr  # noqa: E402
import power_scale_cases as pc  # noqa: E402
import reweight_cases as rc  # noqa: E402
from power_scale_reference import ecdf_reference, power_scale_reference, weights_reference  # noqa: E402
from psis_reference import tail_size  # noqa: E402
from test_power_scale_host import assert_power_scale  # noqa: E402

RTOL = 1e-9
assert max(pc.ROUNDING.values()) < RTOL
TILE = 2048


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def series_of(l, ld, rng):
    """(n, ld) with -l's columns cycled through the first 16 slots, noise beyond"""
    series = rng.standard_normal((l.shape[0], ld))
    for j in range(16):
        series[:, j] = -l[:, j % l.shape[1]]
    return series


# ---- 1: bfhip_rw_weights ---------------------------------------------------------------------------------------------------------------
def run_weights(series, nb, lb, ld_u=16, finish=True):
    """``bfhip_ploo_moments``, ``bfhip_ploo_tail``, ``bfhip_rw_finish`` on one-parameter draws and ``bfhip_rw_weights`` on the same batch
    -> u (n, ld_u), wout (4, 16), rw_out; u and wout filled with -7 before."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    n, ld = series.shape
    s = ctx.tensor(series)
    lbd = None if lb is None else ctx.tensor(np.asarray(lb, dtype=np.float64))
    x = ctx.tensor(np.linspace(-1., 1., n).reshape(1, n, 1))
    centre = ctx.tensor(np.zeros(1))
    m1 = tail_size(n) + 1
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    rw = torch.full((_lib.RW_SUMS + 6, 16), -7., dtype=torch.float64, device=ctx.device)
    u = torch.full((n, ld_u), -7., dtype=torch.float64, device=ctx.device)
    wout = torch.full((_lib.RWW_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, m1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, m1), dtype=torch.int32, device=ctx.device)
    work = ctx.empty((int(lib.bfhip_ploo_work_bytes(n)),), dtype=torch.uint8)
    rww = ctx.empty((int(lib.bfhip_rw_work_bytes(n, 1)),), dtype=torch.uint8)
    head = (h, n, _ptr(s), ld, nb, _lib.PLOO_ELL, None, _ptr(lbd))
    _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), work.numel()))
    _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), work.numel()))
    if finish:
        _lib.check(lib.bfhip_rw_finish(*head, _ptr(keys), _ptr(rows), _ptr(out), _ptr(work), work.numel(), 1, n, n, 1, _ptr(x), 0, 0, 1,
                                       _ptr(centre), _ptr(rw), _ptr(rww), rww.numel()))
    _lib.check(lib.bfhip_rw_weights(*head, _ptr(keys), _ptr(rows), _ptr(out), _ptr(work), work.numel(), _ptr(u), ld_u, _ptr(wout)))
    return _np(u), _np(wout), _np(rw)


@pytest.mark.parametrize('n', rc.SIZES)
def test_rw_weights_match_the_reference(n):
    """u against exp(v) / sum of the reference, without weights and with weights that are -inf in most rows; zeros in the rows of zero
    weight; a column's weights byte-equal in every slot it is cycled through, at nb = 16, 15 and 1 with strides of 19, on a second run
    and without ``bfhip_rw_finish`` in between; khat and the flags are ``bfhip_rw_finish``'s on the same batch, bit for bit."""
    x, l, lw = rc.rw_inputs(n)
    k = l.shape[1]
    rng = np.random.default_rng(n)
    for weighted in (False, True):
        lb = dr.normalise(lw) if weighted else None
        keep = np.ones(n, dtype=bool) if lb is None else lb > -np.inf
        _, want = weights_reference(l, lw if weighted else None)
        u, wout, rw = run_weights(series_of(l, 16, rng), 16, lb)
        with np.errstate(all='ignore'):
            err = np.abs(u[:, :k] - want) / np.abs(want)
        print('n=%d w=%d largest relative error of u' % (n, weighted), np.nanmax(err[keep]) if np.isfinite(err[keep]).any() else np.nan, 'sums',
              u[:, :k].sum(axis=0), 'khat', wout[1, :k], 'flags', wout[2, :k])
        assert np.all(u[~keep] == 0.)
        # (with three rows of any weight at n = 25 the tail holds rows of none and the fit is NaN, in psis itself: flags 0, weights NaN)
        assert np.array_equal(np.isnan(u[:, :k]), np.isnan(want)), (n, weighted)
        fin = ~np.isnan(want)
        assert np.all(err[fin & keep[:, None]] <= RTOL)
        sums = u.sum(axis=0)
        assert np.all((np.abs(sums - 1.) < 1e-12) | np.isnan(sums)) and not np.any(u < 0.)
        for j in range(16):
            assert u[:, j].tobytes() == u[:, j % k].tobytes() and wout[:, j].tobytes() == wout[:, j % k].tobytes(), (n, weighted, j)
        assert wout[1].tobytes() == rw[1].tobytes() and wout[2].tobytes() == rw[5].tobytes(), (wout[1:3], rw[[1, 5]])
        assert np.all(wout[2] == (2. if n < 25 else 0.))
        again, wagain, _ = run_weights(series_of(l, 16, rng), 16, lb, finish=False)
        assert again.tobytes() == u.tobytes() and wagain.tobytes() == wout.tobytes(), (n, weighted, 'twice')
        for nb in (15, 1):
            got, wgot, _ = run_weights(series_of(l, 19, rng), nb, lb, ld_u=19)
            assert got[:, :nb].tobytes() == u[:, :nb].tobytes() and wgot[:, :nb].tobytes() == wout[:, :nb].tobytes(), (n, weighted, nb)
            assert np.all(got[:, nb:] == -7.) and np.all(wgot[:, nb:] == -7.)


def test_rw_weights_of_degenerate_columns():
    """n = 1000: a NaN ratio at non-zero weight (flag 1: NaN in the rows of the sample, 0 elsewhere), the same in a row of zero weight
    (ignored), a constant ratio (without weights u is 1 / n bit for bit), no row of non-zero weight (flag 4: all 0)."""
    n = 1000
    rng = np.random.default_rng(5)
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.8] = -np.inf
    lw[7], lw[11] = 0.1, -np.inf
    base = 0.4 * rng.standard_normal(n)
    cols = [base.copy() for _ in range(3)]
    cols[0][7] = np.nan
    cols[1][11] = np.nan
    l = np.stack(cols + [np.full(n, 0.25)], axis=1)
    lb = dr.normalise(lw)
    keep = lb > -np.inf
    series = np.zeros((n, 16))
    series[:, :4] = -l
    u, wout, _ = run_weights(series, 4, lb)
    _, want = weights_reference(l[:, 1:3], lw)
    print('flags', wout[2, :4], 'khat', wout[1, :4])
    assert wout[2, :4].tolist() == [1., 0., 0., 0.] and np.isnan(wout[1, 0]) and np.isnan(wout[0, 0])
    assert np.isnan(u[keep, 0]).all() and np.all(u[~keep, :4] == 0.)
    assert np.all(np.abs(u[:, 1:3] - want) <= RTOL * np.abs(want))
    flat, wflat, _ = run_weights(np.ascontiguousarray(series[:, 3:4]), 1, None, ld_u=1)
    assert np.all(flat[:, 0] == 1. / n) and wflat[0, 0] == float(n) and wflat[2, 0] == 2.
    none, wnone, _ = run_weights(series, 4, np.full(n, -np.inf))
    assert np.all(none[:, :4] == 0.) and np.all(wnone[2, :4] >= 4.) and np.isnan(wnone[:2, :4]).all()


# ---- 2: bfhip_pscale_cjs ---------------------------------------------------------------------------------------------------------------
def cjs_case(n, masked, seed=0):
    """x (n,) of both signs on a grid of about forty values (ties, across every tile edge), w (n,) normalised -- with ``masked`` zero in
    a third of the rows --, u (n, 8): one-hot on the first and on the last sorted position of the sample, zero on its lowest third, w
    itself, and four tilts whose log ratios spread by 0.01 to 0.5."""
    rng = np.random.default_rng(900 + n + seed)
    z = rng.standard_normal(n)
    x = (np.round(z * 6.) / 6. if n > 16 else z) * 3. - 1.   # (the smallest sizes keep their bins)
    w = rng.random(n) + 0.1
    if masked:
        w[rng.random(n) < 0.33] = 0.
        w[n // 2] = 1.
    w /= w.sum()
    live = np.flatnonzero(w)
    order = live[np.argsort(x[live], kind='stable')]
    u = np.zeros((n, 8))
    u[order[0], 0] = 1.
    u[order[-1], 1] = 1.
    low = w.copy()
    low[order[:max(1, len(order) // 3)]] = 0.
    u[:, 2] = low / low.sum() if low.sum() > 0 else w
    u[:, 3] = w
    for i, s in enumerate((0.01, 0.05, 0.2, 0.5)):
        t = w * np.exp(s * (z if i % 2 == 0 else -0.5 * z * z))
        u[:, 4 + i] = t / t.sum()
    return x, w, u


def run_cjs(x, w, u, nb=16, ld_u=16, slots=16):
    """The column buffer as ``bfhip_wstat_columns`` leaves it (NaN in the rows of zero weight), ``bfhip_diag_sort`` on its column 3,
    ``bfhip_wstat_moments`` on the weights and ``bfhip_pscale_cjs`` with u's columns cycled through the slots -> out (5, 16), -7 before."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    n = len(x)
    col = np.zeros((n, 16))
    col[:, 3] = np.where(w != 0, x, np.nan)
    ub = np.full((n, ld_u), -3.)
    for j in range(slots):
        ub[:, j] = u[:, j % u.shape[1]]
    cold, wd, ud = ctx.tensor(col), ctx.tensor(w), ctx.tensor(ub)
    keys, order = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int32)
    wsum = ctx.empty((4,))
    work = ctx.empty((max(_lib.WSTAT_WORK, _lib.pscale_work(n)),))
    out = torch.full((_lib.CJS_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    _lib.check(lib.bfhip_wstat_moments(h, n, None, _ptr(wd), _ptr(wsum), None, _ptr(work)))
    _lib.check(lib.bfhip_diag_sort(h, n, _ptr(cold), 3, _ptr(keys), _ptr(order)))
    _lib.check(lib.bfhip_pscale_cjs(h, n, _ptr(keys), _ptr(order), _ptr(wsum), _ptr(wd), _ptr(ud), ld_u, nb, _ptr(out), _ptr(work)))
    return _np(out)


def hold_cjs(out, ref, cols, label):
    for name, row in (('J', 0), ('bound', 1), ('cjs', 2), ('ks', 3)):
        g, r = out[row, cols], np.asarray(ref[name], dtype=np.float64)
        with np.errstate(all='ignore'):
            rel = np.abs(g / r - 1.)
            print(label, name, 'largest relative error', np.nanmax(rel) if np.isfinite(rel).any() else np.nan)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, name, g, r)
        ok = ~np.isnan(r)
        assert np.all(np.abs(g - r)[ok] <= RTOL * np.abs(r)[ok]), (label, name, g, r)


@pytest.mark.parametrize('n', [1, 2, 3, 255, 256, 257, TILE - 1, TILE, TILE + 1, 256 * TILE + 1])
def test_pscale_cjs_matches_the_reference(n):
    from bayesfast_amd import _lib
    assert _lib.PSCALE_TILE == TILE
    for masked in (False, True):
        x, w, u = cjs_case(n, masked)
        out = run_cjs(x, w, u)
        label = 'n=%d masked=%d' % (n, masked)
        vec = pc.ecdf_vector(x, w, u)
        hold_cjs(out, vec, list(range(8)), label + ' vector')
        if n <= TILE + 1:
            loops = [ecdf_reference(x, w, u[:, s]) for s in range(8)]
            hold_cjs(out, {k: np.array([r[k] for r in loops]) for k in ('J', 'bound', 'cjs', 'ks')}, list(range(8)), label + ' loop')
        flag = 2. if vec['bound'][0] == 0. else 0.   # (fewer than two draws in the sample, or all of them equal)
        assert np.all(out[4] == flag) and (flag == 0. or (w != 0).sum() < 3), out[4]
        if flag == 0.:
            assert out[0, 3] == 0. and out[2, 3] == 0. and out[3, 3] == 0.   # u is w: exact zeros
            assert np.all(out[2, [0, 1, 2, 4, 5, 6, 7]] > 0.)
        for j in range(16):
            assert out[:, j].tobytes() == out[:, j % 8].tobytes(), (label, j)
        assert run_cjs(x, w, u).tobytes() == out.tobytes(), (label, 'twice')
        if n in (3, 257, TILE + 1):
            for nb in (15, 1):
                for ld in (16, 19):
                    got = run_cjs(x, w, u, nb=nb, ld_u=ld)
                    assert got[:, :nb].tobytes() == out[:, :nb].tobytes(), (label, nb, ld)
                    assert np.all(got[:, nb:] == -7.)


def test_pscale_cjs_of_degenerate_parameters():
    """A non-finite draw in a row of the sample (flag 1: every figure NaN, in every column), the same in a row of zero weight
    (ignored), a constant parameter (flag 2: bound == 0, cjs and ks NaN), NaN weights in one column (that column alone)."""
    n = 600
    x, w, u = cjs_case(n, True)
    live = np.flatnonzero(w)
    dead = np.flatnonzero(w == 0)
    base = run_cjs(x, w, u)
    xd = x.copy()
    xd[dead[:3]] = [np.nan, np.inf, -np.inf]
    assert run_cjs(xd, w, u).tobytes() == base.tobytes()
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[live[5]] = bad
        out = run_cjs(xb, w, u)
        assert np.all(out[4] == 1.) and np.isnan(out[:4]).all(), (bad, out)
    out = run_cjs(np.full(n, 2.5), w, u)
    assert np.all(out[4] == 2.) and np.all(out[1] == 0.) and np.isnan(out[2:4]).all()
    un = u.copy()
    un[live, 5] = np.nan
    out = run_cjs(x, w, un)
    assert np.isnan(out[[0, 2, 3], 5]).all() and out[:, [0, 1, 2, 3, 4, 6, 7]].tobytes() == base[:, [0, 1, 2, 3, 4, 6, 7]].tobytes()


# ---- 3: power_scale: the device route against the host port and the reference -------------------------------------------------------------
def test_power_scale_device_route_matches_the_host_port():
    """(n_chain, n_draw, d) = (3, 130, 5) cut from a wider parent (neither stride is the tight one), C = 3 components by A = 7 powers
    (batches of 16 and 5), float64 and float32 draws, with weights and without; ``max_bytes=1`` (one batch per group) is byte-equal to
    the default; a scenario's figures do not depend on the batch or slot it lands in."""
    import torch
    from bayesfast_amd.utils import power_scale
    rng = np.random.default_rng(78)
    n_chain, n_draw, d = 3, 130, 5
    alphas = (0.6, 0.8, 0.95, 1.05, 1.2, 1.5, 0.9)
    parent = rng.standard_normal((n_chain, n_draw + 2, d + 3)) * 3. + 10.
    xs = parent[:, 2:, 1:d + 1]
    z = (xs.reshape(-1, d) - 10.) / 3.
    g = np.stack([-0.5 * (z[:, 0] - 0.4)**2, 0.6 * z[:, 1] - 0.2 * z[:, 2]**2, 0.3 * z[:, 3] + 1.], axis=1).reshape(n_chain, n_draw, 3)
    lw = 0.5 * rng.standard_normal((n_chain, n_draw))
    lw[0, :9] = -np.inf
    pd = torch.as_tensor(parent, device='cuda')
    view = pd[:, 2:, 1:d + 1]
    assert not view.is_contiguous()
    gd = torch.as_tensor(g, device='cuda')
    figs = ('cjs', 'ks', 'mean', 'sd', 'mcse_mean', 'khat', 'ess', 'log_evidence_ratio', 'sensitivity', 'mean_gradient', 'sd_gradient')
    n = n_chain * n_draw
    for weights in (None, lw):
        got = power_scale(view, gd, log_weights=weights, alphas=alphas, names=['prior', 'likelihood', 'other'])
        host = power_scale(xs, g, log_weights=weights, alphas=alphas, names=['prior', 'likelihood', 'other'])
        ref = power_scale_reference(xs.reshape(-1, d), g.reshape(-1, 3), None if weights is None else weights.reshape(-1), alphas)
        label = 'w=%d' % (weights is not None)
        assert_power_scale(got, ref, 'device against reference ' + label, n, floor_last=False)
        assert_power_scale(host, ref, 'host against reference ' + label, n, floor_last=False)
        assert got.diagnosis == host.diagnosis and got.n == n and np.array_equal(got.flags, host.flags)
        small = power_scale(view, gd, log_weights=weights, alphas=alphas, max_bytes=1)
        again = power_scale(view, gd, log_weights=None if weights is None else torch.as_tensor(weights, device='cuda'), alphas=alphas)
        one = power_scale(view, gd[:, :, 2:], log_weights=weights, alphas=(alphas[1], alphas[4]))   # component 2 alone, two powers
        for f in figs:
            assert getattr(small, f).tobytes() == getattr(got, f).tobytes(), ('max_bytes', f)
            assert getattr(again, f).tobytes() == getattr(got, f).tobytes(), ('again', f)
        for f in ('cjs', 'ks', 'mean', 'sd', 'mcse_mean', 'khat', 'ess', 'log_evidence_ratio'):
            assert getattr(one, f)[0, 0].tobytes() == getattr(got, f)[2, 1].tobytes(), ('alone', f)
            assert getattr(one, f)[0, 1].tobytes() == getattr(got, f)[2, 4].tobytes(), ('alone', f)
        assert 'largest sensitivity' in str(got)
    p32 = parent.astype(np.float32)
    got32 = power_scale(torch.as_tensor(p32, device='cuda')[:, 2:, 1:d + 1], gd, log_weights=lw, alphas=alphas)
    ref32 = power_scale_reference(p32[:, 2:, 1:d + 1].astype(np.float64).reshape(-1, d), g.reshape(-1, 3), lw.reshape(-1), alphas)
    assert_power_scale(got32, ref32, 'float32', n, floor_last=False)
    flat = power_scale(torch.as_tensor(xs.reshape(-1, d), device='cuda'), gd.reshape(-1, 3), log_weights=lw.reshape(-1), alphas=alphas)
    for f in figs:
        assert getattr(flat, f).tobytes() == getattr(got, f).tobytes(), ('flat', f)
    # a constant component without weights: u is w bit for bit
    const = power_scale(view, torch.full((n_chain, n_draw, 1), 0.75, dtype=torch.float64, device='cuda'), alphas=(0.9, 1.1))
    assert np.all(const.cjs == 0.) and np.all(const.ks == 0.) and np.all(const.flags == 2)


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', [3, 17])
def test_power_scale_of_a_pipeline_density(d, dense):
    """m = 21, 4 x 300 points on both sides of the bound, input scales, a prior on some inputs only, ``prior_each`` on and off;
    ``Chi2PipelineDensity.power_scale`` against the reference fed with the components restated in longdouble.  The likelihood component
    g = -r^T P r / 2, r = f - y, is held to dg = 4 (m + _acc_len) EPS (sum_j |(P r)_j| (sf_j + |y_j|) + sum_ij |r_i| |P_ij| |r_j| / 2),
    the bound tests/test_gpu_data_reweight.py uses for its linear ratio carried through the quadratic form; the prior's, d elementwise
    float64 operations, to 4 d EPS |g|.  A ratio is l = (alpha - 1) g, so abs_l = 10 max |alpha - 1| max dg as in that test's argument;
    a distance is to first order linear in l, so it is held to that over the smallest spread of l, relative.  The powers are set so
    that the likelihood's ratios spread by 0.2 and 0.4 over the draws.  ``predictive`` before and after is
    byte-equal: the surrogate's own device model is untouched."""
    from test_polymodel_kernels import restate_poly, random_poly, random_points, _acc_len, EPS, LD
    from test_gpu_predictive import _Fixed
    from bayesfast_amd import Chi2PipelineDensity
    ctx = _ctx()
    rng = np.random.default_rng(500 + d + dense)
    m, n_chain, n_draw = 21, 4, 300
    n = n_chain * n_draw
    poly = random_poly(rng, d, m, 'quad')
    pts = random_points(rng, poly, n, far=False)
    su = _Fixed.model(poly)
    lo, hi = rng.normal(size=d) - 3., rng.normal(size=d) + 3.
    su.input_scales = np.stack([lo, hi], 1)
    x_orig = lo + (hi - lo) * pts
    xs = (x_orig - lo) / (hi - lo)
    f, _, sf, _, info = restate_poly(poly, xs, jac=False)
    assert info['outside'].any() and (~info['outside']).any()
    y = (f[rng.integers(n)] + 0.3 * rng.normal(size=m)).astype(np.float64)
    bmat = rng.normal(size=(m, m))
    prec = (bmat @ bmat.T / m + 2. * np.eye(m)) if dense else None
    pdiag = None if dense else rng.uniform(0.5, 3., size=m)
    prior_mu = x_orig.mean(axis=0) + 0.5 * x_orig.std(axis=0) * rng.normal(size=d)
    prior_prec = np.where(np.arange(d) % 2 == 0, 1. / x_orig.var(axis=0), 0.)
    den = Chi2PipelineDensity(su, y, prec=prec, prec_diag=pdiag, prior_mu=prior_mu, prior_prec=prior_prec, logp0=3.)
    big_p = np.asarray(prec if dense else np.diag(pdiag), dtype=LD)
    r = f - np.asarray(y, dtype=LD)
    pr = r @ big_p.T
    g_like = -0.5 * np.einsum('ni,ni->n', r, pr)
    step = min(0.3, 0.2 / float(g_like.std()))   # the likelihood's log ratios spread by 0.2 and 0.4 over the draws, or less
    alphas = (1. - step, 1. + step, 1. - 2. * step)
    dg = 4 * (m + _acc_len(poly)) * EPS * (np.einsum('nj,nj->n', np.abs(pr), sf + np.abs(y)) + 0.5 * np.einsum('ni,ij,nj->n', np.abs(r), np.abs(big_p), np.abs(r)))
    each = -0.5 * np.asarray(prior_prec, dtype=LD) * (np.asarray(x_orig, dtype=LD) - np.asarray(prior_mu, dtype=LD))**2
    who = np.flatnonzero(prior_prec > 0)
    g_prior = each[:, who].sum(axis=1)
    dgp = 4 * d * EPS * np.abs(each[:, who]).sum(axis=1)
    dl = float(max(np.max(dg), np.max(dgp))) * max(abs(a - 1.) for a in alphas)
    x = ctx.tensor(x_orig.reshape(n_chain, n_draw, d))
    before = den.predictive(x, outputs=[0, 20])
    lw = 0.3 * rng.standard_normal((n_chain, n_draw))
    for prior_each in (False, True):
        comps = [g_like, g_prior] + ([each[:, i] for i in who] if prior_each else [])
        names = ['likelihood', 'prior'] + (['prior[%d]' % i for i in who] if prior_each else [])
        g = np.stack(comps, axis=1).astype(np.float64)
        spread = np.array([abs(a - 1.) * g[:, c].std() for c in range(g.shape[1]) for a in alphas])
        print('d=%d dense=%d each=%d: dl' % (d, dense, prior_each), dl, 'smallest spread of l', spread.min())
        for weights in (None, lw):
            ref = power_scale_reference(x_orig, g, None if weights is None else weights.reshape(-1), alphas)
            got = den.power_scale(x, log_weights=weights, alphas=alphas, prior_each=prior_each)
            assert got.names == names and got.n == n and got.cjs.shape == (len(names), 3, d) and len(got.diagnosis) == d
            assert_power_scale(got, ref, 'd=%d dense=%d each=%d w=%d' % (d, dense, prior_each, weights is not None), n,
                               abs_l=10. * dl, abs_cjs=10. * dl / spread.min(), floor_last=False)
    print(got)
    plain = Chi2PipelineDensity(su, y, prec=prec, prec_diag=pdiag)
    none = plain.power_scale(x, prior_each=True)
    assert none.names == ['likelihood'] and none.diagnosis is None and np.isfinite(none.sensitivity).all()
    after = den.predictive(x, outputs=[0, 20])
    for name in before.table.names:
        assert before.table[name].tobytes() == after.table[name].tobytes(), name
    assert _np(before.chi2).tobytes() == _np(after.chi2).tobytes()


# ---- 5: after sample() -----------------------------------------------------------------------------------------------------------------
def test_trace_power_scale_after_sample(monkeypatch):
    """d = 3, m = 5, 4 chains x 60 iterations with 20 of warm-up: ``tt.power_scale(density)`` is ``data_power_scale`` on the view
    ``_diag_input`` hands out, byte for byte, with ``since_iter`` and ``log_weights``; with two ranks it refuses and names gather()."""
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import data_power_scale
    rng = np.random.default_rng(6)
    d, m = 3, 5
    su = bfa.PolyModel('quadratic', input_size=d, output_size=m)
    xf = rng.normal(size=(4 * su.n_param, d))
    q = rng.normal(size=(m, d, d)) * 0.2
    a_lin = rng.normal(size=(d, m))
    model = lambda v: np.einsum('ni,kij,nj->nk', v, q, v) + v @ a_lin
    yf = model(xf)
    y = model(np.zeros((1, d)) + 0.1)[0]
    prior_mu, prior_prec = np.array([0.3, 0., -0.2]), np.array([2., 0., 30.])
    den = bfa.Chi2PipelineDensity(su, y, prec_diag=np.full(m, 4.), prior_mu=prior_mu, prior_prec=prior_prec)
    den.fit(xf, -0.5 * 4. * ((yf - y)**2).sum(axis=1) - 0.5 * (prior_prec * (xf - prior_mu)**2).sum(axis=1), y=yf)
    tt = bfa.sample(den, bfa.NTrace(n_chain=4, n_iter=60, n_warmup=20, x_0=rng.normal(size=(4, d)) * 0.1, random_generator=7),
                    verbose=False)
    figs = ('cjs', 'ks', 'mean', 'sd', 'mcse_mean', 'khat', 'ess', 'log_evidence_ratio', 'sensitivity', 'mean_gradient', 'sd_gradient')
    view = tt._diag_input(None, False, True, 'samples')
    assert tuple(view.shape) == (4, 40, d) and view.is_cuda
    got, want = tt.power_scale(den), data_power_scale(den, view)
    for f in figs:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    print(got)
    assert got.n == 160 and got.names == ['likelihood', 'prior'] and np.isfinite(got.sensitivity).all() and len(got.diagnosis) == d
    lw = 0.2 * rng.standard_normal((4, 30))
    got = tt.power_scale(den, since_iter=30, log_weights=lw, prior_each=True, alphas=(0.98, 1.02))
    want = data_power_scale(den, tt._diag_input(30, False, True, 'samples'), log_weights=lw, prior_each=True, alphas=(0.98, 1.02))
    assert got.n == 120 and got.names == ['likelihood', 'prior', 'prior[0]', 'prior[2]'] and got.cjs.shape == (4, 2, d)
    for f in figs:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='gather'):
        tt.power_scale(den)


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_and_the_model_usable():
    import torch
    from test_polymodel_kernels import random_poly, random_points
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel
    from bayesfast_amd.utils import power_scale
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    rng = np.random.default_rng(9)
    poly = random_poly(rng, 5, 4, 'quad')
    pts = ctx.tensor(random_points(rng, poly, 40))
    dm = DevicePolyModel(poly, ctx)
    f0 = dm.fun_and_jac(pts, jac=False)[0].clone()
    n = 100
    xh = rng.standard_normal(n)
    lh = 0.3 * xh[:, None] * np.ones((1, 16))
    series = ctx.tensor(-lh)
    m1 = tail_size(n) + 1
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    u = torch.full((n, 16), -7., dtype=torch.float64, device=ctx.device)
    wout = torch.full((_lib.RWW_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, m1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, m1), dtype=torch.int32, device=ctx.device)
    nbytes = int(lib.bfhip_ploo_work_bytes(n))
    work = ctx.empty((nbytes,), dtype=torch.uint8)
    head = (h, n, _ptr(series), 16, 16, _lib.PLOO_ELL, None, None)
    _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), nbytes))
    _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), nbytes))

    def weights(n=n, s=series, ld=16, nb=16, mode=_lib.PLOO_ELL, k=keys, r=rows, o=out, wk=work, wb=nbytes, uu=u, ldu=16, wo=wout):
        return lib.bfhip_rw_weights(h, n, _ptr(s), ld, nb, mode, None, None, _ptr(k), _ptr(r), _ptr(o), _ptr(wk), wb, _ptr(uu), ldu, _ptr(wo))

    cases = {'n = 0': dict(n=0), 'no series': dict(s=None), 'nb = 17': dict(nb=17), 'nb = 0': dict(nb=0), 'ld < nb': dict(ld=8), 'mode': dict(mode=2),
             'no keys': dict(k=None), 'no rows': dict(r=None), 'no out': dict(o=None), 'no work': dict(wk=None),
             'short work buffer': dict(wb=nbytes - 1), 'no u': dict(uu=None), 'ld_u < nb': dict(ldu=15), 'no wout': dict(wo=None)}
    for name, kw in cases.items():
        rcode = weights(**kw)
        assert rcode == -1, name
        with pytest.raises(ValueError):
            _lib.check(rcode)
    assert weights(n=2**31) == -4
    with pytest.raises(NotImplementedError):
        _lib.check(weights(n=2**31))

    # bfhip_pscale_cjs
    w = ctx.tensor(np.full(n, 1. / n))
    col = ctx.tensor(np.tile(xh[:, None], (1, 16)))
    skeys, order = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int32)
    wsum, cwork = ctx.empty((4,)), ctx.empty((max(_lib.WSTAT_WORK, _lib.pscale_work(n)),))
    cout = torch.full((_lib.CJS_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    _lib.check(lib.bfhip_wstat_moments(h, n, None, _ptr(w), _ptr(wsum), None, _ptr(cwork)))
    _lib.check(lib.bfhip_diag_sort(h, n, _ptr(col), 0, _ptr(skeys), _ptr(order)))

    def cjs(n=n, k=skeys, o=order, ws=wsum, ww=w, uu=u, ldu=16, nb=16, co=cout, wk=cwork):
        return lib.bfhip_pscale_cjs(h, n, _ptr(k), _ptr(o), _ptr(ws), _ptr(ww), _ptr(uu), ldu, nb, _ptr(co), _ptr(wk))

    cases = {'n = 0': dict(n=0), 'no keys': dict(k=None), 'no order': dict(o=None), 'no wsum': dict(ws=None), 'no w': dict(ww=None),
             'no u': dict(uu=None), 'ld_u < nb': dict(ldu=15), 'nb = 17': dict(nb=17, ldu=17), 'nb = 0': dict(nb=0), 'no out': dict(co=None),
             'no work': dict(wk=None)}
    for name, kw in cases.items():
        rcode = cjs(**kw)
        assert rcode == -1, name
        with pytest.raises(ValueError):
            _lib.check(rcode)
    assert cjs(n=2**31) == -4
    assert lib.bfhip_pscale_cjs(None, n, _ptr(skeys), _ptr(order), _ptr(wsum), _ptr(w), _ptr(u), 16, 16, _ptr(cout), _ptr(cwork)) == -1
    assert _lib.pscale_work(1) == 352 and _lib.pscale_work(TILE) == 352 and _lib.pscale_work(TILE + 1) == 704
    big = torch.zeros((1, 1), dtype=torch.float64, device=ctx.device).expand(2**31, 1)   # (a view: no memory behind it)
    with pytest.raises(NotImplementedError, match='2\\^31 - 1 draws'):
        power_scale(big, big)
    with pytest.raises(ValueError):
        power_scale(col, series[:, :0])
    with pytest.raises(ValueError, match='each side of 1'):
        power_scale(col, series, alphas=(1.01, 1.02))
    ctx.synchronize()
    assert bool((u == -7.).all()) and bool((wout == -7.).all()) and bool((cout == -7.).all())
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
    assert weights() == 0 and cjs() == 0
    ctx.synchronize()
    _, want = weights_reference(lh[:, :1])
    got = _np(u)
    assert np.all(np.abs(got[:, 3] - want[:, 0]) <= RTOL * want[:, 0])
    ref = ecdf_reference(xh, np.full(n, 1. / n), got[:, 3])
    co = _np(cout)
    print('after the refusals: cjs', co[2, 3], ref['cjs'], 'ks', co[3, 3], ref['ks'])
    assert abs(co[2, 3] - ref['cjs']) <= RTOL * ref['cjs'] and abs(co[3, 3] - ref['ks']) <= RTOL * ref['ks']
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)


# ---- 7: the conjugate normal model through the device route ----------------------------------------------------------------------------------
@pytest.mark.parametrize('par', list(pc.CONJUGATE))
def test_conjugate_normal_regimes_on_the_device(par):
    """The inputs and margins of tests/test_power_scale_host.py's test 3: 40 000 draws, the three diagnoses, each sensitivity within five
    standard deviations (over 8 seeds, measured on the host port) of the quadrature of the exact CDFs; and the host port's own values to
    1e-9."""
    import torch
    from bayesfast_amd.utils import power_scale
    want_diag, sd_prior, sd_like = pc.CONJUGATE[par]
    x, g = pc.conjugate_draws(*par, seed=100)
    got = power_scale(torch.as_tensor(x, device='cuda'), torch.as_tensor(g, device='cuda'), names=['prior', 'likelihood'])
    host = power_scale(x, g, names=['prior', 'likelihood'])
    quad = pc.conjugate_quadrature(*par, lo=x.min(), hi=x.max())
    ratio = got.sensitivity[:, 0] / np.array(quad)
    print(par, 'sensitivity', got.sensitivity[:, 0], 'host', host.sensitivity[:, 0], 'quadrature', quad, 'ratio', ratio, got.diagnosis)
    assert got.diagnosis == [want_diag]
    assert abs(ratio[0] - 1.) <= 5. * sd_prior and abs(ratio[1] - 1.) <= 5. * sd_like
    assert np.all(np.abs(got.sensitivity - host.sensitivity) <= RTOL * host.sensitivity)
    assert np.all(np.abs(got.cjs - host.cjs) <= RTOL * host.cjs) and np.all(np.abs(got.ks - host.ks) <= RTOL * host.ks)
