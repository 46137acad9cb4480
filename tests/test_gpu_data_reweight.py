"""The reweighted posterior on the device (csrc/bfhip_rw.h: ``bfhip_rw_finish`` after ``bfhip_ploo_moments`` and ``bfhip_ploo_tail``)
through ctypes and through ``bayesfast_amd.utils.reweight_moments`` / ``data_reweight``, against NumPy's stable argsort and the
loop-written reference of helpers/reweight_reference.py.

Sizes (helpers/reweight_cases.py).  n = 3 | 4 | 5: the matrix product's k-step of four rows (a ragged step, a full one, one row into
the next); 24 | 25 the first fitted tail; 255 .. 257 a workgroup's 256 threads (16 | 16 | 17 workgroups of the body pass, which take
16 rows each); 1000 and 4097 more of them; 12289 = 768 x 16 + 1, the first size at which the body pass's 768 workgroups stride; 262145
the first size at which the 1024 workgroups of the strided PLOO passes stride.  d = 7 | 8: 1 + 2 d = 15 | 17 features cross the edge of a tile of 16; d = 15 | 16: 1 + d = 16 |
17, the first-order block fills a tile; d = 27 is four tiles, one group of tiles; d = 128 (at n = 257) is 17 tiles in five groups.

Tolerances.  Keys, rows, n_tail, flags and NaN patterns are exact.  Floating figures are held to 1e-9 relative, the project's figure
for a device route against a loop reference -- a mean to 1e-9 sd_base, the log evidence ratio to 1e-9 max(1, |.|) -- or to ten times
what rounding alone does to the reference on these very inputs (float64 against numpy.longdouble, on the CPU, by
helpers/reweight_cases.py; docs/EXPERIMENTS.md has the table) where that is larger: ``ROUNDING`` below.  Each test prints every figure
before it asserts."""
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
import reweight_cases as rc  # noqa: E402
from psis_reference import tail_size  # noqa: E402
from reweight_reference import reweight_reference  # noqa: E402
from test_data_reweight_host import assert_against, K_FIGS, KD_FIGS  # noqa: E402

RTOL = 1e-9
# ten times the largest float64-against-longdouble difference of the reference over rc.rw_reference(n, weighted), n in rc.SIZES, both
# weightings, in the units the figure is held in (docs/EXPERIMENTS.md has the table): mean 1.7e-10 sd_base at n = 4097 (the offsets
# are up to 1e5 sd, and the reference sums x itself), mcse_mean 8.1e-12 at 4097, sd 2.3e-14 at 262145, khat 1.6e-13, ess 5.0e-14 and
# log_evidence_ratio 2.2e-14 at 262145, sigma 7.0e-15: only the mean's is above 1e-9, every other figure keeps RTOL
ROUNDING = dict(mean=1.7e-9, mcse_mean=8.1e-11, sd=2.3e-13, khat=1.6e-12, ess=5.0e-13, log_evidence_ratio=2.2e-13, sigma=7.0e-14)
RAW_FIGS = ('log_evidence_ratio', 'khat', 'sigma', 'ess', 'mean', 'sd', 'mcse_mean')


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def shifted_ratios(l, lb):
    """What the kernels sort by, operation for operation, for the series -l: (lb - (-l)) - max, -inf in a row of zero weight, NULL
    weights as 0."""
    with np.errstate(all='ignore'):
        r = (0. if lb is None else lb) - (-l)
        if lb is not None:
            r[lb == -np.inf] = -np.inf
        keep = np.ones(len(l), dtype=bool) if lb is None else lb > -np.inf
        mx = np.fmax.reduce(np.concatenate([[-np.inf], r[keep]]))
        return r - mx, mx


def run_rw(xt, series, nb, lb, centre, since=0):
    """The two PLOO stages and ``bfhip_rw_finish`` as include/bfhip.h declares them: xt a device tensor (n_chain, n_draw, d) read in
    place from draw ``since`` of every chain on, series (n, ld) holding -l -> rw_out (8 + 2 (1 + 2 d), 16), keys (16, M + 1), rows (16, M + 1), out (16, 16)."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    n, ld = series.shape
    n_chain, n_draw, d = int(xt.shape[0]), int(xt.shape[1]) - since, int(xt.shape[2])
    assert n_chain * n_draw == n
    s = ctx.tensor(series)
    lbd = None if lb is None else ctx.tensor(np.asarray(lb, dtype=np.float64))
    cd = ctx.tensor(np.asarray(centre, dtype=np.float64))
    m1 = tail_size(n) + 1
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    rw = torch.full((_lib.RW_SUMS + 2 * (1 + 2 * d), 16), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, m1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, m1), dtype=torch.int32, device=ctx.device)
    work = ctx.empty((int(lib.bfhip_ploo_work_bytes(n)),), dtype=torch.uint8)
    rww = ctx.empty((int(lib.bfhip_rw_work_bytes(n, d)),), dtype=torch.uint8)
    head = (h, n, _ptr(s), ld, nb, _lib.PLOO_ELL, None, _ptr(lbd))
    _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), work.numel()))
    _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), work.numel()))
    ldr = int(xt.stride(1)) if xt.shape[1] > 1 else d
    _lib.check(lib.bfhip_rw_finish(*head, _ptr(keys), _ptr(rows), _ptr(out), _ptr(work), work.numel(), n_chain, n_draw, int(xt.stride(0)),
                                   ldr, _ptr(xt), int(xt.dtype == torch.float32), since, d, _ptr(cd), _ptr(rw), _ptr(rww), rww.numel()))
    return _np(rw), _np(keys).view(np.uint64), _np(rows).view(np.uint32), _np(out)


def figures_of(rw, d, centre, n, weighted, cols):
    """The figures of the columns ``cols`` from the raw block, by the closed form: with D = sum w (x - c), mean = c + D,
    sum w (x - mean)^2 = sum w (x - c)^2 - D^2, sum w^2 (x - mean)^2 = sum w^2 (x - c)^2 - 2 D sum w^2 (x - c) + D^2 sum w^2."""
    nf, r0 = 1 + 2 * d, 8
    o = rw[:, cols]
    with np.errstate(all='ignore'):
        s1, s2 = o[r0], o[r0 + nf]
        e1, e2 = o[r0 + 1:r0 + 1 + d] / s1, o[r0 + 1 + d:r0 + nf] / s1
        q1, q2 = o[r0 + nf + 1:r0 + nf + 1 + d] / s1**2, o[r0 + nf + 1 + d:r0 + 2 * nf] / s1**2
        sw2 = s2 / s1**2
        mean = centre[:, None] + e1
        sd = np.sqrt((e2 - e1 * e1) / (1. - sw2))
        mcse = np.sqrt(q2 - 2. * e1 * q1 + e1 * e1 * sw2)
        ler = o[0] + (0. if weighted else -np.log(n))
    return dict(log_evidence_ratio=ler, khat=o[1], sigma=o[2], n_tail=o[3], ess=o[4], flags=o[5], mean=mean.T, sd=sd.T, mcse_mean=mcse.T)


def series_of(l, ld, rng):
    """(n, ld) with -l's columns cycled through the first 16 slots, noise beyond"""
    series = rng.standard_normal((l.shape[0], ld))
    for j in range(16):
        series[:, j] = -l[:, j % l.shape[1]]
    return series


def n_chain_of(n):
    return next(c for c in (5, 4, 3, 2, 1) if n % c == 0)


# ---- 1: bfhip_rw_finish against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', rc.SIZES)
def test_rw_finish_matches_the_reference(n):
    """Every d of the docstring at nb = 16 on contiguous float64 draws, without weights and with weights that are -inf in most rows
    (fewer rows of non-zero weight than the tail holds at some sizes); at d = 27 also nb = 15 and nb = 1 with a row stride of 19, the
    draws as a [:, since:] view of a wider parent with a chain stride, and float32 draws.  A column's figures are byte-equal in every
    slot it is cycled through, at any nb, and on a second run."""
    import torch
    ctx = _ctx()
    x, l, lw = rc.rw_inputs(n)
    k = l.shape[1]
    rng = np.random.default_rng(n)
    n_chain = n_chain_of(n)
    n_draw = n // n_chain
    for weighted in (False, True):
        ref = rc.rw_reference(n, weighted)
        lb = dr.normalise(lw) if weighted else None
        keep = np.ones(n, dtype=bool) if lb is None else lb > -np.inf
        want_tail = [dr.tail_reference(shifted_ratios(l[:, j], lb)[0]) for j in range(k)]
        for d in rc.dims_of(n):
            xd = np.ascontiguousarray(x[:, :d])
            centre = xd[keep].mean(axis=0) + 0.01 * xd[keep].std(axis=0)   # near the base mean, not on it
            sub = {f: (ref[f][:, :d] if np.ndim(ref[f]) == 2 else ref[f][:d] if f.endswith('_base') else ref[f]) for f in ref}
            xt = ctx.tensor(xd.reshape(n_chain, n_draw, d))
            rw, keys, rows, out = run_rw(xt, series_of(l, 16, rng), 16, lb, centre)
            for j in range(16):
                wk, wr = want_tail[j % k]
                assert np.array_equal(keys[j], wk) and np.array_equal(rows[j], wr), (n, weighted, d, j, 'tail')
                assert rw[:, j].tobytes() == rw[:, j % k].tobytes(), (n, weighted, d, j, 'slot')
            label = 'n=%d w=%d d=%d' % (n, weighted, d)
            assert_against(figures_of(rw, d, centre, n, weighted, list(range(k))), sub, label, extra=ROUNDING, figs=RAW_FIGS, base=False)
            if d != 27:
                continue
            again = run_rw(xt, series_of(l, 16, rng), 16, lb, centre)[0]
            assert again.tobytes() == rw.tobytes(), (n, weighted, 'twice')
            for nb in (15, 1):
                got = run_rw(xt, series_of(l, 19, rng), nb, lb, centre)[0]
                assert got[:, :nb].tobytes() == rw[:, :nb].tobytes(), (n, weighted, nb)
                assert np.all(got[:, nb:] == -7.)
            parent = rng.standard_normal((n_chain, n_draw + 2, d + 3))
            parent[:, 2:, 1:d + 1] = xd.reshape(n_chain, n_draw, d)
            view = torch.as_tensor(parent, device=ctx.device)[:, :, 1:d + 1]
            assert not view.is_contiguous()
            got = run_rw(view, series_of(l, 16, rng), 16, lb, centre, since=2)[0]
            assert got.tobytes() == rw.tobytes(), (n, weighted, 'view')
            x32 = xd.astype(np.float32)
            got = run_rw(torch.as_tensor(x32.reshape(n_chain, n_draw, d), device=ctx.device), series_of(l, 16, rng), 16, lb, centre)[0]
            ref32 = reweight_reference(x32.astype(np.float64), l[:, :1], lw if weighted else None) if n <= 4097 else None
            if ref32 is not None:
                assert_against(figures_of(got, d, centre, n, weighted, [0]), ref32, label + ' f32', extra=ROUNDING, figs=RAW_FIGS, base=False)
        flags = 4. if not keep.any() else 2. if n < 25 else 0.
        assert np.all(rw[5, :16] == flags), (n, weighted, rw[5])


# ---- 2: degenerate input ---------------------------------------------------------------------------------------------------------------
def test_degenerate_columns_and_draws():
    """One batch at n = 1000, d = 5: a NaN and a +inf ratio at non-zero weight (the scenario is NaN, flag 1), a NaN ratio and a NaN draw
    in a row of zero weight (ignored), a constant ratio, ties across the cut; a NaN and an inf draw at non-zero weight take their
    parameter in every scenario and nothing else; no row of non-zero weight is flag 4."""
    n, d = 1000, 5
    rng = np.random.default_rng(5)
    ctx = _ctx()
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.8] = -np.inf
    lw[7], lw[11] = 0.1, -np.inf
    x = rng.standard_normal((n, d)) * np.array([1., 3., 0.1, 20., 1.]) + np.array([0., 5., -2., 100., 1.])
    base = 0.5 * x[:, 0] - 0.3 * (x[:, 1] - 5.) / 3.
    cols = [base.copy() for _ in range(6)]
    cols[0][7] = np.nan
    cols[1][7] = np.inf
    cols[2][11] = np.nan
    cols[3] = np.full(n, 0.25)
    cols[4] = np.round(base / 0.05) * 0.05
    cols[5][7] = -np.inf
    l = np.stack(cols, axis=1)
    x[11, 2] = np.nan
    lb = dr.normalise(lw)
    keep = lb > -np.inf
    centre = x[keep].mean(axis=0)
    series = np.zeros((n, 16))
    series[:, :6] = -l
    for bad_draws in (False, True):
        if bad_draws:
            x[7, 3], x[np.flatnonzero(keep)[5], 4] = np.nan, np.inf
        ref = reweight_reference(x, l, lw)
        rw = run_rw(ctx.tensor(x.reshape(4, 250, d)), series, 6, lb, centre)[0]
        got = figures_of(rw, d, centre, n, True, list(range(6)))
        with np.errstate(all='ignore'):   # a parameter with a non-finite draw: whatever the sums hold, it is not a number
            for f in ('mean', 'sd', 'mcse_mean'):
                got[f] = np.where(np.isfinite(got['mean']) & np.isfinite(got['sd']), got[f], np.nan)
        assert_against(got, ref, 'degenerate %d' % bad_draws, figs=RAW_FIGS, base=False)
        assert got['flags'].tolist() == [1., 1., 0., 0., 0., 1.]
        assert np.isnan(got['khat'][0]) and np.isfinite(got['khat'][2]) and np.isfinite(got['mean'][2, :3]).all()
        if bad_draws:
            assert np.isnan(got['mean'][2:5, 3:]).all() and np.isfinite(got['log_evidence_ratio'][2:5]).all()
    x = rng.standard_normal((n, d))
    flat = run_rw(ctx.tensor(x.reshape(1, n, d)), np.ascontiguousarray(series[:, 3:]), 2, None, x.mean(axis=0))[0]
    got = figures_of(flat, d, x.mean(axis=0), n, False, [0, 1])
    print('constant ratio', got['log_evidence_ratio'][0], got['khat'][0], got['mean'][0] - x.mean(axis=0), got['sd'][0] / x.std(axis=0, ddof=1) - 1)
    assert got['flags'].tolist() == [2., 0.] and np.isinf(got['khat'][0]) and abs(got['log_evidence_ratio'][0] - 0.25) < 1e-12
    assert np.all(np.abs(got['mean'][0] - x.mean(axis=0)) < 1e-12) and np.all(np.abs(got['sd'][0] / x.std(axis=0, ddof=1) - 1) < 1e-12)
    none = run_rw(ctx.tensor(x.reshape(1, n, d)), series, 6, np.full(n, -np.inf), centre)[0]
    assert np.all(none[5, :6] >= 4.) and np.isnan(none[[0, 1, 4], :6]).all() and np.isnan(none[8:, :6]).all()


# ---- 3: reweight_moments: the device route against the host port ----------------------------------------------------------------------------
def test_reweight_moments_device_route_matches_the_host_port():
    """(n_chain, n_draw, d) = (3, 130, 5) cut from a wider parent (neither stride is the tight one), K = 21 (batches of 16 and 5),
    float64 and float32 draws, with weights and without; a scenario's figures do not depend on the batch or slot it lands in."""
    import torch
    from bayesfast_amd.utils import reweight_moments
    rng = np.random.default_rng(77)
    n_chain, n_draw, d, k = 3, 130, 5, 21
    parent = rng.standard_normal((n_chain, n_draw + 2, d + 3)) * 3. + 10.
    xs = parent[:, 2:, 1:d + 1]
    z = (xs.reshape(-1, d) - 10.) / 3.
    dirs = rng.standard_normal((k, d)) * np.linspace(0.02, 0.4, k)[:, None]
    l = (z @ dirs.T + rng.normal(size=k)).reshape(n_chain, n_draw, k)
    lw = 0.5 * rng.standard_normal((n_chain, n_draw))
    lw[0, :9] = -np.inf
    pd = torch.as_tensor(parent, device='cuda')
    view = pd[:, 2:, 1:d + 1]
    assert not view.is_contiguous()
    ld = torch.as_tensor(l, device='cuda')
    names = K_FIGS + KD_FIGS + ('mean_base', 'sd_base', 'n_tail', 'flags')
    for weights in (None, lw):
        got = reweight_moments(view, ld, log_weights=weights)
        host = reweight_moments(xs, l, log_weights=weights)
        assert_against(got, {f: getattr(host, f) for f in names}, 'device against host w=%d' % (weights is not None))
        ref = reweight_reference(xs.reshape(-1, d), l.reshape(-1, k)[:, 15:18], weights)
        sel = {f: (getattr(got, f)[15:18] if f not in ('mean_base', 'sd_base') else getattr(got, f)) for f in names}
        assert_against(sel, ref, 'device against reference w=%d' % (weights is not None))
        again = reweight_moments(view, ld, log_weights=None if weights is None else torch.as_tensor(weights, device='cuda'))
        one = reweight_moments(view, ld[:, :, 17:18], log_weights=weights)       # scenario 17 alone: slot 0 of a batch of one
        for f in K_FIGS + KD_FIGS:
            assert getattr(again, f).tobytes() == getattr(got, f).tobytes(), f
            assert getattr(one, f)[0].tobytes() == getattr(got, f)[17].tobytes(), f
        assert got.n == n_chain * n_draw and got.n_khat_bad == host.n_khat_bad and 'worst: scenario' in str(got)
    p32 = parent.astype(np.float32)
    got32 = reweight_moments(torch.as_tensor(p32, device='cuda')[:, 2:, 1:d + 1], ld, log_weights=lw)
    host32 = reweight_moments(p32[:, 2:, 1:d + 1].astype(np.float64), l, log_weights=lw)
    assert_against(got32, {f: getattr(host32, f) for f in names}, 'float32')
    flat = reweight_moments(torch.as_tensor(xs.reshape(-1, d), device='cuda'), ld.reshape(-1, k), log_weights=lw.reshape(-1))
    for f in K_FIGS + KD_FIGS:
        assert getattr(flat, f).tobytes() == getattr(got, f).tobytes(), f


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', [3, 17])
def test_data_reweight_of_a_pipeline_density(d, dense):
    """m = 21, K = 33 data vectors (batches of 16, 16 and 1; with chunk_bytes = 1 three derived models), 4 x 300 points on both sides of
    the bound, input scales; ``data_reweight`` against the reference fed with l = A f + b restated in longdouble.  l is held to the
    derived model's own bound dl = 4 (m + _acc_len) EPS (sum_j |A_kj| sf_j + |b_k|); every figure is 1-Lipschitz in a shift of l in the
    units it is held in (a weight moves by its relative dl, a mean by that times E|x - mean| <= sd) up to the PSIS fit, whose
    sensitivity the same factor of ten covers, as tests/test_gpu_data_loo.py argues it for ell: RTOL plus ten times the largest dl.
    ``predictive`` before and after is byte-equal: the surrogate's own device model came back."""
    from test_polymodel_kernels import restate_poly, random_poly, random_points, _acc_len, EPS, LD
    from test_gpu_predictive import _Fixed
    from bayesfast_amd import Chi2PipelineDensity
    from bayesfast_amd.utils.reweight import ratio_coefficients
    ctx = _ctx()
    rng = np.random.default_rng(300 + d + dense)
    m, n_chain, n_draw, big_k = 21, 4, 300, 33
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
    # data vectors whose ratios spread by 0 (y itself) to about 0.6 over the draws
    dy = rng.normal(size=(big_k, m))
    a1, _ = ratio_coefficients(y, y + dy, prec, pdiag)
    dy *= (np.linspace(0., 0.6, big_k) / (np.asarray(f, dtype=np.float64) @ a1.T).std(axis=0))[:, None]
    y_new = y + dy
    a, b = ratio_coefficients(y, y_new, prec, pdiag)
    al = np.asarray(a, dtype=LD)
    l = (np.einsum('km,nm->nk', al, f) + np.asarray(b, dtype=LD)).astype(np.float64)
    dl_all = 4 * (m + _acc_len(poly)) * EPS * (np.einsum('km,nm->nk', np.abs(al), sf) + np.abs(b))
    dl = float(np.max(dl_all))
    print('largest dl', dl, 'spread of l', l.std(axis=0)[[0, 16, 32]])
    x = ctx.tensor(x_orig.reshape(n_chain, n_draw, d))
    before = den.predictive(x, outputs=[0, 20])
    lw = 0.3 * rng.standard_normal((n_chain, n_draw))
    lr = _np(den.data_log_ratio(x, y_new)).reshape(n, big_k)
    with np.errstate(all='ignore'):
        print('data_log_ratio: largest error / its bound', np.nanmax(np.abs(lr - l) / dl_all))
    assert lr.shape == (n, big_k) and np.all(np.abs(lr - l) <= dl_all) and np.all(lr[:, 0] == 0.)
    for weights in (None, lw):
        ref = reweight_reference(x_orig, l, weights)
        got = den.data_reweight(x, y_new, log_weights=weights)
        assert got.n == n and got.mean.shape == (big_k, d)
        assert_against(got, ref, 'd=%d dense=%d w=%d' % (d, dense, weights is not None), abs_l=10. * dl)
        # three derived models of 16, 16 and 1 outputs (the polymodel kernel's last bit of an output depends on the model it sits in)
        small = den.data_reweight(x, y_new, log_weights=weights, chunk_bytes=1)
        assert_against(small, ref, 'd=%d dense=%d w=%d, in chunks' % (d, dense, weights is not None), abs_l=10. * dl)
    one = den.data_reweight(x, y_new[0])    # the data itself: the base table and a ratio of 0
    assert one.flags.tolist() == [2] and one.log_evidence_ratio[0] == 0. and np.all(np.abs(one.shift[0]) < 1e-12)
    after = den.predictive(x, outputs=[0, 20])
    for name in before.table.names:
        assert before.table[name].tobytes() == after.table[name].tobytes(), name
    assert _np(before.chi2).tobytes() == _np(after.chi2).tobytes()
    assert 'khat' in str(got)


# ---- 5: after sample() -----------------------------------------------------------------------------------------------------------------
def test_trace_data_reweight_after_sample(monkeypatch):
    """d = 3, m = 5, 4 chains x 60 iterations with 20 of warm-up: ``tt.data_reweight(density, y_new)`` is ``data_reweight`` on the view
    ``_diag_input`` hands out, byte for byte, with ``since_iter`` and ``log_weights``; a data vector moved towards larger outputs
    moves the posterior."""
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import data_reweight
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
    y_new = np.stack([y, y + 0.1, y - 0.05 * np.arange(m)])
    view = tt._diag_input(None, False, True, 'samples')
    assert tuple(view.shape) == (4, 40, d) and view.is_cuda
    got, want = tt.data_reweight(den, y_new), data_reweight(den, view, y_new)
    for f in K_FIGS + KD_FIGS:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    print(got)
    assert got.n == 160 and got.log_evidence_ratio[0] == 0. and np.isfinite(got.mean).all() and np.all(got.shift[1] != 0.)
    lw = 0.2 * rng.standard_normal((4, 30))
    got = tt.data_reweight(den, y_new[1], since_iter=30, log_weights=lw)
    want = data_reweight(den, tt._diag_input(30, False, True, 'samples'), y_new[1], log_weights=lw)
    assert got.n == 120 and got.mean.tobytes() == want.mean.tobytes() and got.mean.shape == (1, d)
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='gather'):
        tt.data_reweight(den, y_new)


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_and_the_model_usable():
    import torch
    from test_polymodel_kernels import random_poly, random_points
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel
    from bayesfast_amd.utils import reweight_moments
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    rng = np.random.default_rng(9)
    poly = random_poly(rng, 5, 4, 'quad')
    pts = ctx.tensor(random_points(rng, poly, 40))
    dm = DevicePolyModel(poly, ctx)
    f0 = dm.fun_and_jac(pts, jac=False)[0].clone()
    n, d = 100, 5
    xh = rng.standard_normal((n, d))
    lh = 0.3 * xh[:, :1] * np.ones((1, 16))
    x, series, centre = ctx.tensor(xh), ctx.tensor(-lh), ctx.tensor(xh.mean(axis=0))
    m1 = tail_size(n) + 1
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    rw = torch.full((_lib.RW_SUMS + 2 * (1 + 2 * d), 16), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, m1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, m1), dtype=torch.int32, device=ctx.device)
    nbytes, rbytes = int(lib.bfhip_ploo_work_bytes(n)), int(lib.bfhip_rw_work_bytes(n, d))
    work, rww = ctx.empty((nbytes,), dtype=torch.uint8), ctx.empty((rbytes,), dtype=torch.uint8)
    assert lib.bfhip_rw_work_bytes(0, d) == 0 and lib.bfhip_rw_work_bytes(2**31, d) == 0 and lib.bfhip_rw_work_bytes(n, 0) == 0
    assert lib.bfhip_rw_work_bytes(n, _lib.MAX_DIM + 1) == 0 and lib.bfhip_rw_work_bytes(n, _lib.MAX_DIM) > 0
    head = (h, n, _ptr(series), 16, 16, _lib.PLOO_ELL, None, None)
    _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), nbytes))
    _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), nbytes))

    def call(n=n, s=series, ld=16, nb=16, mode=_lib.PLOO_ELL, wb=nbytes, n_chain=1, n_draw=n, ldr=d, xp=x, dd=d, c=centre, o=rw, rb=rbytes):
        return lib.bfhip_rw_finish(h, n, _ptr(s), ld, nb, mode, None, None, _ptr(keys), _ptr(rows), _ptr(out), _ptr(work), wb, n_chain,
                                   n_draw, n_draw * ldr, ldr, _ptr(xp), 0, 0, dd, _ptr(c), _ptr(o), _ptr(rww), rb)

    cases = {'n = 0': dict(n=0, n_draw=0), 'no series': dict(s=None), 'nb = 17': dict(nb=17), 'ld < nb': dict(ld=8), 'mode': dict(mode=2),
             'short work buffer': dict(wb=nbytes - 1), 'chains x draws != n': dict(n_chain=3), 'no draws': dict(xp=None), 'd = 0': dict(dd=0),
             'd = 129': dict(dd=129), 'ldr < d': dict(ldr=d - 1), 'no centre': dict(c=None), 'no out': dict(o=None),
             'short own work buffer': dict(rb=rbytes - 1)}
    for name, kw in cases.items():
        rcode = call(**kw)
        assert rcode == -1, name
        with pytest.raises(ValueError):
            _lib.check(rcode)
    assert call(n=2**31, n_draw=2**31) == -4
    with pytest.raises(NotImplementedError):
        _lib.check(call(n=2**31, n_draw=2**31))
    big = torch.zeros((1, 1), dtype=torch.float64, device=ctx.device).expand(2**31, 1)   # (a view: no memory behind it)
    with pytest.raises(NotImplementedError, match='2\\^31 - 1 draws'):
        reweight_moments(big, big)
    with pytest.raises(ValueError):
        reweight_moments(x, series[:, :0])
    ctx.synchronize()
    assert bool((rw == -7.).all())
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
    assert call() == 0
    ctx.synchronize()
    got = figures_of(_np(rw), d, xh.mean(axis=0), n, False, [3])
    ref = reweight_reference(xh, lh[:, :1])
    assert_against(got, ref, 'after the refusals', figs=RAW_FIGS, base=False)
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
