"""Pointwise PSIS-LOO and WAIC on the device (csrc/bfhip_ploo.h: ``bfhip_ploo_moments`` / ``_tail`` / ``_finish``) through ctypes and
through ``bayesfast_amd.utils.pointwise_loo`` / ``data_loo``, against NumPy's stable argsort and the loop-written reference of
helpers/data_loo_reference.py.

Sizes.  ``SIZES`` are those of test_gpu_psis.py (24 | 25 the smallest fitted tail, 224 .. 226 the crossing of the two tail-size rules,
255 .. 257 a workgroup's 256 threads and 16-row slices, 262145 the first size at which the 1024 workgroups of the strided reductions
stride).  The select's own edges: n = 4 | 5 | 9 | 10 is the tail size M = 0 | 1 | 1 | 2 (no candidate at all; one, in place; from
two on through the two segmented sorts); its workgroups own contiguous ranges of at least 256 rows, so 256 | 257 is one range | two
(144 + 113 rows: a ragged last range), and from 4096 x 256 = 1048576 rows on there are 4096 ranges that grow: 2^22 + 1 rows make 4081
ranges of 1040 rows (once, with two columns).  There is no candidate capacity: a column's list holds exactly M pairs.

Tolerances.  Keys, rows, n_tail, flags and NaN patterns are exact.  Floating figures are held to 1e-9 relative, the project's figure
for a device route against a loop reference; p_loo, a difference, to 1e-9 max(|lpd|, |elpd_loo|) absolute.  What rounding alone does
to the reference on these very inputs (float64 against numpy.longdouble, on the CPU; docs/EXPERIMENTS.md has the table) is in
``ROUNDING`` below with ten times the largest relative difference per figure; where that is below 1e-9 the figure keeps 1e-9.
Each test prints every figure before it asserts."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import data_loo_reference as dr  # noqa: E402
from psis_reference import tail_size  # noqa: E402

RTOL = 1e-9
SIZES = (1, 24, 25, 224, 225, 226, 255, 256, 257, 1000, 4097, 100003, 262145)
SELECT_SIZES = (1, 4, 5, 9, 10) + SIZES[1:]
FIGURES = ('lpd', 'p_waic', 'elpd_waic', 'elpd_loo', 'khat', 'sigma', 'ess_loo', 'pit')
# ten times the largest relative float64-against-longdouble difference of the reference over loo_case(n, weighted), n in SIZES,
# both weightings (elpd_loo 1.06e-12 at n = 100003, ess_loo 1.8e-13 at 262145, sigma 7.8e-14 at 25, khat 3.3e-14 at 4097, pit 2.9e-14,
# lpd 2.6e-14, p_waic 2.3e-14, elpd_waic 1.1e-14; p_loo 1.07e-12 of max(|lpd|, |elpd_loo|)): every one is below 1e-9, so RTOL holds
ROUNDING = dict(lpd=2.6e-13, p_waic=2.3e-13, elpd_waic=1.1e-13, elpd_loo=1.06e-11, khat=3.3e-13, sigma=7.8e-13, ess_loo=1.8e-12, pit=2.9e-13)


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_stages(series, nb, mode, c=None, lb=None, stages=3):
    """The stages as include/bfhip.h declares them on the (n, ld) array ``series`` -> out (16, 16), keys (16, M + 1), rows (16, M + 1)."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    n, ld = series.shape
    s = ctx.tensor(series)
    cd = None if c is None else ctx.tensor(np.asarray(c, dtype=np.float64))
    lbd = None if lb is None else ctx.tensor(np.asarray(lb, dtype=np.float64))
    m1 = tail_size(n) + 1
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, m1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, m1), dtype=torch.int32, device=ctx.device)
    work = ctx.empty((int(lib.bfhip_ploo_work_bytes(n)),), dtype=torch.uint8)
    head = (h, n, _ptr(s), ld, nb, mode, _ptr(cd), _ptr(lbd))
    _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), work.numel()))
    if stages > 1:
        _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), work.numel()))
    if stages > 2:
        _lib.check(lib.bfhip_ploo_finish(*head, _ptr(keys), _ptr(rows), _ptr(out), _ptr(work), work.numel()))
    return _np(out), _np(keys).view(np.uint64), _np(rows).view(np.uint32)


def shifted_ratios(ell, lb):
    """What the kernels sort by, operation for operation: (lb - ell) - max, -inf in a row of zero weight, NULL weights as 0."""
    with np.errstate(all='ignore'):
        r = (0. if lb is None else lb) - ell
        if lb is not None:
            r[lb == -np.inf] = -np.inf
        keep = np.ones(len(ell), dtype=bool) if lb is None else lb > -np.inf
        mx = np.fmax.reduce(np.concatenate([[-np.inf], r[keep]]))   # (fmax from -inf on: a NaN is passed over)
        return r - mx, mx


def select_columns(n, rng):
    """The patterns of the select test: smooth, ties across the cut (rounded to 0.05), all equal, +-0 at the top, a NaN, heavy ties."""
    t = rng.standard_normal(n)
    cols = [-0.5 * t * t - 0.9, np.round(-0.5 * t * t, 1) / 2., np.full(n, -1.25)]
    z = np.abs(rng.standard_normal(n))
    z[rng.random(n) < 0.4] = 0.
    z[rng.random(n) < 0.3] *= -1.          # (-0 among them)
    cols.append(np.where(z == 0, z, np.abs(z)))
    bad = -0.5 * rng.standard_normal(n)**2
    bad[n // 2] = np.nan
    cols.append(bad)
    cols.append(rng.integers(0, 3, size=n).astype(np.float64))
    return cols


# ---- 1: the select, exactly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SELECT_SIZES)
def test_tail_is_the_stable_argsort_tail(n):
    """Keys and rows of every column equal NumPy's stable argsort as integers: six patterns cycled through the 16 slots (so a column's
    result is byte-equal in any slot), at nb = 16, 15 and 1 and with a row stride of 19; without weights and with weights that are
    -inf in most rows (fewer rows of non-zero weight than the tail holds at some sizes, none at n = 1)."""
    from bayesfast_amd import _lib
    rng = np.random.default_rng(n)
    pats = select_columns(n, rng)
    lbw = rng.standard_normal(n)
    lbw[rng.random(n) < 0.85] = -np.inf
    for lb in (None, lbw):
        want = [dr.tail_reference(shifted_ratios(p, lb)[0]) for p in pats]
        for nb, ld in ((16, 16), (15, 16), (1, 16), (16, 19)):
            series = rng.standard_normal((n, ld))
            for j in range(16):
                series[:, j] = pats[j % len(pats)]
            out, keys, rows = run_stages(series, nb, _lib.PLOO_ELL, lb=lb, stages=2)
            for j in range(nb):
                wk, wr = want[j % len(pats)]
                mx = shifted_ratios(pats[j % len(pats)], lb)[1]
                assert out[10, j] == mx or (np.isnan(mx) and np.isnan(out[10, j])), (n, nb, ld, j)
                assert np.array_equal(keys[j], wk), (n, nb, ld, j, 'keys')
                assert np.array_equal(rows[j], wr), (n, nb, ld, j, 'rows')


def test_tail_at_four_million_rows():
    """n = 2^22 + 1, two columns filled (nb = 2, row stride 2): 4081 ranges of 1040 rows, M = 6145; one smooth column, one with ties."""
    from bayesfast_amd import _lib
    n = 2**22 + 1
    rng = np.random.default_rng(22)
    t = rng.standard_normal(n)
    series = np.stack([-0.5 * t * t, np.round(t, 2)], axis=1)
    out, keys, rows = run_stages(series, 2, _lib.PLOO_ELL, stages=2)
    for j in range(2):
        wk, wr = dr.tail_reference(shifted_ratios(series[:, j], None)[0])
        assert np.array_equal(keys[j], wk) and np.array_equal(rows[j], wr), j


# ---- 2: the columns against the reference ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loo_case(n, weighted):
    """z, c, ell = c - z^2 / 2 (the kernel's three operations) and the log weights of a case, with the reference of every column;
    three columns up to n = 4097, one beyond.  Column 0 is standard normal (khat near 0.5 x ...: a light tail), column 1 has a
    wider z (a heavier tail), column 2 a narrow one."""
    rng = np.random.default_rng(1000 + n + weighted)
    k = 3 if n <= 4097 else 1
    z = rng.standard_normal((n, k)) * np.array([1., 1.6, 0.5])[:k]
    c = np.array([-0.3, 0.4, 1.1])[:k]
    ell = c - 0.5 * (z * z)
    lw = None
    if weighted:
        lw = 0.7 * rng.standard_normal(n)
        lw[rng.random(n) < 0.1] = -np.inf
        if n == 1:
            lw[:] = 0.3
    ref = [dr.column_reference(ell[:, j], lw, z[:, j]) for j in range(k)]
    return z, c, ell, lw, ref


def assert_columns(got, ref, label, pit=True, waic_abs=0.):
    """got: dict of (k,) arrays; ref: list of dicts"""
    for j, r in enumerate(ref):
        with np.errstate(all='ignore'):
            for f in FIGURES:
                print(label, j, f, got[f][j], float(r[f]), abs(got[f][j] / np.float64(r[f]) - 1))
            print(label, j, 'p_loo', got['p_loo'][j], float(r['p_loo']), abs(got['p_loo'][j] - np.float64(r['p_loo'])))
        assert int(got['n_tail'][j]) == r['n_tail']
        for f in FIGURES:
            want = np.float64(r[f])
            if f == 'pit' and not pit:
                assert np.isnan(got[f][j])
            elif np.isnan(want) or np.isinf(want):
                assert np.array_equal(got[f][j], want, equal_nan=True), (label, j, f)
            else:
                assert abs(got[f][j] - want) <= max(RTOL, ROUNDING[f]) * abs(want) + (waic_abs if 'waic' in f else 0.), (label, j, f)
        want = np.float64(r['p_loo'])
        if np.isnan(want):
            assert np.isnan(got['p_loo'][j])
        else:
            assert abs(got['p_loo'][j] - want) <= RTOL * max(abs(np.float64(r['lpd'])), abs(np.float64(r['elpd_loo']))), (label, j)


def figures_of(out, k):
    with np.errstate(all='ignore'):
        p_waic = out[2] / (1. - out[12])
        return dict(lpd=out[0, :k], p_waic=p_waic[:k], elpd_waic=(out[0] - p_waic)[:k], elpd_loo=out[3, :k], p_loo=(out[0] - out[3])[:k],
                    khat=out[4, :k], sigma=out[5, :k], n_tail=out[6, :k], ess_loo=out[8, :k], pit=out[9, :k], flags=out[11, :k])


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_columns_match_the_reference_in_both_modes(n, weighted):
    from bayesfast_amd import _lib
    z, c, ell, lw, ref = loo_case(n, weighted)
    k = z.shape[1]
    lb = None if lw is None else dr.normalise(lw)
    series = np.zeros((n, 16))
    c16 = np.zeros(16)
    c16[:k] = c
    series[:, :k] = z
    got_z = figures_of(run_stages(series, k, _lib.PLOO_Z, c=c16, lb=lb)[0], k)
    assert_columns(got_z, ref, 'n=%d w=%d Z' % (n, weighted))
    series[:, :k] = ell
    got_e = figures_of(run_stages(series, k, _lib.PLOO_ELL, lb=lb)[0], k)
    assert_columns(got_e, ref, 'n=%d w=%d ELL' % (n, weighted), pit=False)
    for f in FIGURES[:-1] + ('p_loo', 'n_tail', 'flags'):   # the two modes see the same ell: the same bits
        assert got_z[f].tobytes() == got_e[f].tobytes(), f
    assert np.all(got_z['flags'] == (2. if n < 25 else 0.))


def test_pointwise_loo_device_route_matches_the_host_port_and_the_reference():
    """``pointwise_loo`` on a GPU (n_chain, n_draw, k) view with strides, k = 21 (batches of 16 and 5), float64 and float32, with
    weights; a column's figures do not depend on the batch or slot it lands in."""
    import torch
    from bayesfast_amd.utils import pointwise_loo
    rng = np.random.default_rng(77)
    n_chain, n_draw, k = 3, 130, 21
    t = rng.standard_normal((n_chain, n_draw + 2, k + 3))
    parent = -0.5 * t * t * rng.uniform(0.5, 2., size=k + 3)
    lw = 0.5 * rng.standard_normal((n_chain, n_draw))
    pd = torch.as_tensor(parent, device='cuda')
    view = pd[:, 2:, 1:k + 1]
    assert not view.is_contiguous()
    seen = parent[:, 2:, 1:k + 1].reshape(-1, k)
    got = pointwise_loo(view, log_weights=torch.as_tensor(lw, device='cuda'))
    ref = [dr.column_reference(seen[:, j], lw) for j in range(k)]
    cols = {f: getattr(got, f) for f in FIGURES + ('p_loo', 'n_tail')}
    assert_columns(cols, ref, 'view', pit=False)
    again = pointwise_loo(view, log_weights=torch.as_tensor(lw, device='cuda'))
    for f in cols:
        assert getattr(again, f).tobytes() == cols[f].tobytes(), f
    one = pointwise_loo(view[:, :, 17:18], log_weights=lw)      # column 17 alone: slot 0 of a batch of one
    for f in cols:
        assert getattr(one, f)[0].tobytes() == cols[f][17].tobytes(), f
    host = pointwise_loo(seen, log_weights=lw)
    for f in FIGURES[:-1]:
        np.testing.assert_allclose(getattr(host, f), cols[f], rtol=RTOL)
    assert got.n_khat_bad == host.n_khat_bad and got.outputs.tolist() == list(range(k))
    np.testing.assert_allclose(got.elpd_loo_total, host.elpd_loo_total, rtol=RTOL)
    p32 = parent.astype(np.float32)
    got32 = pointwise_loo(torch.as_tensor(p32, device='cuda')[:, 2:, 1:k + 1])
    ref32 = [dr.column_reference(p32[:, 2:, 1:k + 1].reshape(-1, k)[:, j].astype(np.float64)) for j in range(k)]
    assert_columns({f: getattr(got32, f) for f in cols}, ref32, 'float32', pit=False)


# ---- 3: degenerate input ----------------------------------------------------------------------------------------------------------------
def test_degenerate_columns():
    """One batch: a NaN, a +inf and a -inf ell at non-zero weight (every figure NaN), a NaN in a row of zero weight (ignored), a
    constant ell, ties across the cut; weights that are mostly zero.  Twice, byte for byte.  Without weights the constant column has
    a flat tail: khat = inf, nothing smoothed, p_loo = 0."""
    from bayesfast_amd import _lib
    n = 1000
    rng = np.random.default_rng(5)
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.8] = -np.inf
    lw[7] = 0.1
    lw[11] = -np.inf
    base = -0.5 * rng.standard_normal(n)**2
    cols = [base.copy() for _ in range(6)]
    cols[0][7] = np.nan
    cols[1][7] = np.inf
    cols[2][11] = np.nan
    cols[3] *= 2.
    const = np.full(n, -2.)
    cols[4] = np.round(base / 0.05) * 0.05
    cols[5][7] = -np.inf
    series = np.zeros((n, 16))
    for j, col in enumerate(cols):
        series[:, j] = col
    lb = dr.normalise(lw)
    ref = [dr.column_reference(col, lw) for col in cols]
    out = run_stages(series, 6, _lib.PLOO_ELL, lb=lb)[0]
    got = figures_of(out, 6)
    assert_columns(got, ref, 'degenerate', pit=False)
    assert got['flags'].tolist() == [1., 1., 0., 0., 0., 1.]
    assert np.isnan(got['khat'][0]) and np.isfinite(got['khat'][2])
    assert run_stages(series, 6, _lib.PLOO_ELL, lb=lb)[0][:12, :6].tobytes() == out[:12, :6].tobytes()
    series[:, 3] = const
    flat = figures_of(run_stages(series[:, 3:], 2, _lib.PLOO_ELL)[0], 2)
    # p_waic of a constant column is rounding alone: its mean is off by at most n EPS |ell|, the sum of squares by that squared
    assert_columns(flat, [dr.column_reference(const), dr.column_reference(cols[4])], 'flat, ties', pit=False, waic_abs=(n * 2.3e-16 * 2.)**2)
    assert flat['flags'].tolist() == [2., 0.] and np.isinf(flat['khat'][0]) and abs(flat['p_loo'][0]) < 1e-12
    none = run_stages(series, 6, _lib.PLOO_ELL, lb=np.full(n, -np.inf))[0]     # no row of non-zero weight
    assert np.all(none[11, :6] >= 4.) and np.isnan(none[[0, 3, 4, 8], :6]).all()


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', [3, 17])
def test_data_loo_of_a_pipeline_density(d, dense):
    """m = 21 (batches of 16 and 5), 4 x 300 points on both sides of the bound, input scales; ``data_loo`` against the reference fed
    with the restated z = W (y - f).  z is held to the residual model's own bound, 4 (m + _acc_len) EPS sum_j |W_ij| (|y_j| + sf_j), and
    that carries into ell as |z| dz; the figures are then held to RTOL plus the largest dell (every figure is 1-Lipschitz in a shift of
    ell up to the PSIS fit, whose sensitivity the same factor of ten covers).  ``predictive`` before and after is byte-equal: the
    surrogate's own device model came back."""
    import torch
    from test_polymodel_kernels import restate_poly, random_poly, random_points, _acc_len, EPS, LD
    from test_gpu_predictive import _Fixed
    from bayesfast_amd import Chi2PipelineDensity
    from bayesfast_amd.utils.data_loo import whitening_of
    ctx = _ctx()
    rng = np.random.default_rng(300 + d + dense)
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
    den = Chi2PipelineDensity(su, y, prec=prec, prec_diag=pdiag)
    x = ctx.tensor(x_orig.reshape(n_chain, n_draw, d))
    w, c = whitening_of(prec, pdiag)
    wl = np.asarray(w, dtype=LD)
    z = np.einsum('ij,nj->ni', wl, y.astype(LD) - f)
    dz = 4 * (m + _acc_len(poly)) * EPS * np.einsum('ij,nj->ni', np.abs(wl), np.abs(y.astype(LD)) + sf)
    dell = float(np.max(np.abs(z) * dz))
    print('largest dell', dell)
    before = den.predictive(x, outputs=[0, 20])
    lw = 0.3 * rng.standard_normal((n_chain, n_draw))
    for outputs, weights in ((None, None), ([1, 2, 3, 9, 10, 20], lw)):
        got = den.data_loo(x, outputs=outputs, log_weights=weights)
        idx = np.arange(m) if outputs is None else np.asarray(outputs)
        assert got.outputs.tolist() == idx.tolist() and got.n == n
        for j, i in enumerate(idx):
            zi = z[:, i].astype(np.float64)
            ref = dr.column_reference(c[i] - 0.5 * zi * zi, weights, zi)
            for fig in FIGURES:
                g, r = getattr(got, fig)[j], np.float64(ref[fig])
                print(d, dense, i, fig, g, r, abs(g / r - 1))
                scale = abs(r) if fig in ('khat', 'sigma', 'ess_loo', 'pit') else 1.
                assert abs(g - r) <= RTOL * abs(r) + 10. * dell * max(scale, 1.), (i, fig)
            assert got.n_tail[j] == ref['n_tail']
    after = den.predictive(x, outputs=[0, 20])
    for name in before.table.names:
        assert before.table[name].tobytes() == after.table[name].tobytes(), name
    assert _np(before.chi2).tobytes() == _np(after.chi2).tobytes()
    assert 'elpd_loo' in str(got)


# ---- 5: after sample() -----------------------------------------------------------------------------------------------------------------
def test_trace_data_loo_after_sample(monkeypatch):
    """d = 3, m = 5, 4 chains x 60 iterations with 20 of warm-up: ``tt.data_loo(density)`` is ``data_loo`` on the view ``_diag_input``
    hands out, byte for byte, with ``since_iter`` and ``log_weights``."""
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import data_loo
    rng = np.random.default_rng(6)
    d, m = 3, 5
    su = bfa.PolyModel('quadratic', input_size=d, output_size=m)
    xf = rng.normal(size=(4 * su.n_param, d))
    q = rng.normal(size=(m, d, d)) * 0.2
    a_lin = rng.normal(size=(d, m))
    model = lambda v: np.einsum('ni,kij,nj->nk', v, q, v) + v @ a_lin
    yf = model(xf)
    y = model(np.zeros((1, d)) + 0.1)[0]
    den = bfa.Chi2PipelineDensity(su, y, prec_diag=np.full(m, 4.))
    den.fit(xf, -0.5 * 4. * ((yf - y)**2).sum(axis=1), y=yf)
    tt = bfa.sample(den, bfa.NTrace(n_chain=4, n_iter=60, n_warmup=20, x_0=rng.normal(size=(4, d)) * 0.1, random_generator=7),
                    verbose=False)
    view = tt._diag_input(None, False, True, 'samples')
    assert tuple(view.shape) == (4, 40, d) and view.is_cuda
    got, want = tt.data_loo(den), data_loo(den, view)
    for f in FIGURES + ('p_loo',):
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    assert np.isfinite(got.elpd_loo).all() and np.all((got.pit > 0) & (got.pit < 1)) and got.n == 160
    lw = 0.2 * rng.standard_normal((4, 30))
    got = tt.data_loo(den, since_iter=30, log_weights=lw, outputs=[1, 2])
    want = data_loo(den, tt._diag_input(30, False, True, 'samples'), log_weights=lw, outputs=[1, 2])
    assert got.n == 120 and got.elpd_loo.tobytes() == want.elpd_loo.tobytes() and got.outputs.tolist() == [1, 2]
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='gather'):
        tt.data_loo(den)


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_and_the_model_usable():
    import torch
    from test_polymodel_kernels import random_poly, random_points
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    rng = np.random.default_rng(9)
    poly = random_poly(rng, 5, 4, 'quad')
    pts = ctx.tensor(random_points(rng, poly, 40))
    dm = DevicePolyModel(poly, ctx)
    f0 = dm.fun_and_jac(pts, jac=False)[0].clone()
    n = 100
    series = ctx.tensor(-0.5 * rng.standard_normal((n, 16))**2)
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, tail_size(n) + 1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, tail_size(n) + 1), dtype=torch.int32, device=ctx.device)
    nbytes = int(lib.bfhip_ploo_work_bytes(n))
    work = ctx.empty((nbytes,), dtype=torch.uint8)
    assert lib.bfhip_ploo_work_bytes(0) == 0 and lib.bfhip_ploo_work_bytes(2**31) == 0

    def calls(n=n, s=series, ld=16, nb=16, mode=_lib.PLOO_ELL, c=None, wb=nbytes):
        head = (h, n, _ptr(s), ld, nb, mode, _ptr(c), None)
        return (lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), wb),
                lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), wb),
                lib.bfhip_ploo_finish(*head, _ptr(keys), _ptr(rows), _ptr(out), _ptr(work), wb))

    cases = {'n = 0': dict(n=0), 'no series': dict(s=None), 'nb = 0': dict(nb=0), 'nb = 17': dict(nb=17), 'ld < nb': dict(ld=8),
             'mode': dict(mode=2), 'Z without c': dict(mode=_lib.PLOO_Z), 'short work buffer': dict(wb=nbytes - 1)}
    for name, kw in cases.items():
        for rc in calls(**kw):
            assert rc == -1, name
            with pytest.raises(ValueError):
                _lib.check(rc)
    for rc in calls(n=2**31):
        assert rc == -4
        with pytest.raises(NotImplementedError):
            _lib.check(rc)
    ctx.synchronize()
    assert bool((out == -7.).all())
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
    assert calls() == (0, 0, 0)
    ctx.synchronize()
    got = _np(out)
    ref = dr.column_reference(_np(series)[:, 3])
    assert abs(got[3, 3] - ref['elpd_loo']) <= RTOL * abs(ref['elpd_loo']) and abs(got[4, 3] - ref['khat']) <= RTOL * abs(ref['khat'])
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
