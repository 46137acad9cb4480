"""The host side of the reweighted posterior (bayesfast_amd/utils/reweight.py, ``device.linear_dense``): no GPU.

1. ``linear_dense``: the derived K-output model, restated in longdouble from its own dense arrays, equals A f + b of the restated
   parent within 4 (m + _acc_len) EPS (sum_j |A_kj| sf_j + |b_k|), the bound tests/test_gpu_data_loo.py uses for z: the derived
   coefficients are m-term float64 sums of the parent's, every term of the parent's majorant sf carries its share.
2. The host port of ``reweight_moments`` against the loop-written reference of helpers/reweight_reference.py: 1e-9 relative, the
   project's figure for a route against a loop reference; a mean, which may sit at 0, to 1e-9 sd_base absolute, a shift to 1e-9
   absolute (it is the mean in units of sd_base), the log evidence ratio, a logarithm that may be 0, to 1e-9 max(1, |.|).
3. A closed form: linear surrogate, Gaussian prior, exact Gaussian posterior and evidence.
4. Degenerate input and refusals.
Every test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, 'helpers')):
    if p not in sys.path:
        sys.path.insert(0, p)

from reweight_reference import reweight_reference  # noqa: E402
from bayesfast_amd.utils.reweight import reweight_moments, data_reweight, Reweighted, ratio_coefficients  # noqa: E402

RTOL = 1e-9
K_FIGS = ('log_evidence_ratio', 'khat', 'sigma', 'ess')
KD_FIGS = ('mean', 'sd', 'mcse_mean', 'shift', 'shift_mcse')


def spec_from_dense(dense):
    """The dense arrays of ``polymodel_dense_from_poly`` as a poly_spec of at most four configs on all outputs."""
    d, m = int(dense['d']), int(dense['m'])
    outs = np.arange(m)
    cfgs = [dict(order='linear', input_mask=np.arange(d), output_mask=outs, coef=np.concatenate([dense['c0'][:, None], dense['lin']], axis=1))]
    if dense['quad'] is not None:
        cfgs.append(dict(order='quadratic', input_mask=np.arange(d), output_mask=outs, coef=dense['quad']))
    if len(dense['mask2']):
        cfgs.append(dict(order='cubic-2', input_mask=np.asarray(dense['mask2'], dtype=np.int64), output_mask=outs, coef=dense['cub2']))
    if len(dense['mask3']):
        cfgs.append(dict(order='cubic-3', input_mask=np.asarray(dense['mask3'], dtype=np.int64), output_mask=outs, coef=dense['cub3']))
    spec = dict(input_size=d, output_size=m, use_bound=bool(dense['use_bound']), configs=cfgs)
    if dense['use_bound']:
        spec.update(mu=dense['mu'], hess=dense['hess'], alpha=dense['alpha'], f_mu=dense['f_mu'])
    return spec


# ---- 1: linear_dense -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['quad', 'cubic'])
@pytest.mark.parametrize('d', [3, 17])
def test_linear_dense_is_a_times_f_plus_b(d, kind):
    from test_polymodel_kernels import restate_poly, random_poly, random_points, _acc_len, EPS, LD
    from bayesfast_amd.device import polymodel_dense_from_poly, linear_dense, residual_dense
    rng = np.random.default_rng(40 + d + len(kind))
    m, big_k, n = 21, 5, 60
    poly = random_poly(rng, d, m, kind)
    pts = random_points(rng, poly, n, far=False)
    f, _, sf, _, info = restate_poly(poly, pts, jac=False)
    assert info['outside'].any() and (~info['outside']).any()
    a, b = rng.normal(size=(big_k, m)), rng.normal(size=big_k) * 3.
    a[1] = 0.
    b[1] = 0.
    dense = polymodel_dense_from_poly(poly)
    before = {k: np.array(v) for k, v in dense.items() if isinstance(v, np.ndarray)}
    got = linear_dense(dense, a, b)
    for k, v in before.items():   # the parent's arrays are left alone
        assert np.array_equal(dense[k], v), k
    assert got['m'] == big_k and got['d'] == d and got['use_bound'] == dense['use_bound']
    for k in ('mu', 'hess', 'alpha', 'mask2', 'mask3'):
        assert np.array_equal(got[k], dense[k]), k
    g, _, _, _, _ = restate_poly(spec_from_dense(got), pts, jac=False)
    al = np.asarray(a, dtype=LD)
    want = np.einsum('km,nm->nk', al, f) + np.asarray(b, dtype=LD)
    tol = 4 * (m + _acc_len(poly)) * EPS * (np.einsum('km,nm->nk', np.abs(al), sf) + np.abs(b))
    err = np.abs(g - want)
    with np.errstate(all='ignore'):
        print(d, kind, 'largest error / bound', float(np.nanmax(err / tol)), 'largest bound / |value|', float(np.max(tol / np.maximum(np.abs(want), 1e-300))))
    assert np.all(err <= tol)
    assert np.all(g[:, 1] == 0)     # A_k = 0, b_k = 0: the ratio of the data vector to itself is 0 exactly
    # residual_dense is the case A = -W, b = W y, and stays as it is
    w, y = rng.normal(size=(m, m)), rng.normal(size=m)
    rd, ld = residual_dense(dense, y, w), linear_dense(dense, -w, w @ y)
    for k in ('lin', 'quad', 'cub2', 'cub3'):
        assert (rd[k] is None and ld[k] is None) or np.array_equal(rd[k], ld[k]), k
    np.testing.assert_allclose(rd['c0'], ld['c0'], rtol=0, atol=1e-12 * np.abs(w).sum())
    with pytest.raises(ValueError):
        linear_dense(dense, a[:, :-1], b)
    with pytest.raises(ValueError):
        linear_dense(dense, a, b[:-1])


# ---- 2: the host port against the reference ------------------------------------------------------------------------------------------------
def host_case(n, big_k, weighted, seed=0):
    """d = 3 draws with different scales and offsets, K ratios linear-plus-quadratic in the draws with shifts of 0 .. 0.8 sd (so that
    khat runs from small to large), log weights that are -inf in a tenth of the rows."""
    rng = np.random.default_rng(7000 + 10 * n + big_k + weighted + seed)
    d = 3
    z = rng.standard_normal((n, d))
    x = z * np.array([1., 0.02, 30.]) + np.array([0.5, -4., 1e3])
    dirs = rng.standard_normal((big_k, d))
    dirs *= (np.linspace(0., 0.8, big_k) / np.sqrt((dirs * dirs).sum(axis=1)))[:, None]
    l = z @ dirs.T + 0.05 * (z[:, :1]**2) * np.linspace(-1., 1., big_k)[None, :] + rng.normal(size=big_k)[None, :]
    lw = None
    if weighted:
        lw = 0.7 * rng.standard_normal(n)
        lw[rng.random(n) < 0.1] = -np.inf
        if n < 5:
            lw[0] = 0.3
    return x, l, lw


def assert_against(got, ref, label, rtol=RTOL, abs_l=0., k_sel=None, extra=None, figs=None, base=True):
    """got a ``Reweighted`` (or a dict of arrays), ref the reference's dict.  ``abs_l``: what is known of the error of the ratios fed
    to the two (0 where both got the same numbers); ``extra``: per-figure relative bounds that replace rtol where they are larger; ``figs``: the figures to hold
    (default all); ``base=False``: ``got`` has no base table."""
    get = (lambda f: getattr(got, f)) if not isinstance(got, dict) else (lambda f: got[f])
    extra = extra or {}
    ks = range(len(ref['khat'])) if k_sel is None else k_sel
    sdb = np.asarray(ref['sd_base'], dtype=np.float64)
    mscale = lambda r: np.where(np.isfinite(sdb) & (sdb > 0), np.abs(sdb), np.abs(r))   # (one draw has no sd: its mean is held relatively)
    for f in ('mean_base', 'sd_base') if base else ():
        g, r = get(f), np.asarray(ref[f], dtype=np.float64)
        print(label, f, 'largest |got - want|', np.nanmax(np.abs(g - r)) if np.isfinite(r).any() else np.nan)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, f)
        ok = ~np.isnan(r)
        with np.errstate(all='ignore'):
            err = np.abs(g - r)
        assert np.all(err[ok] <= max(rtol, extra.get(f, 0.)) * (mscale(r)[ok] if f == 'mean_base' else np.abs(r[ok]))), (label, f)
    for j, k in enumerate(ks):
        assert int(get('n_tail')[j]) == int(ref['n_tail'][k]) and int(get('flags')[j]) == int(ref['flags'][k]), (label, k, 'n_tail, flags')
        for f in (K_FIGS + KD_FIGS if figs is None else figs):
            g, r = np.atleast_1d(get(f)[j]), np.atleast_1d(np.asarray(ref[f][k], dtype=np.float64))
            with np.errstate(all='ignore'):
                print(label, k, f, 'largest |got - want|', np.nanmax(np.abs(g - r)) if np.isfinite(r).any() else np.nan, 'of', np.nanmax(np.abs(r)) if np.isfinite(r).any() else np.nan)
            assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r)), (label, k, f)
            ok = np.isfinite(r)
            tol = max(rtol, extra.get(f, 0.))
            if f == 'mean':
                bound = (tol + abs_l) * mscale(r)
            elif f == 'shift':
                bound = tol + abs_l + 0. * r
            elif f == 'log_evidence_ratio':
                bound = tol * np.maximum(1., np.abs(r)) + abs_l
            else:
                bound = (tol + abs_l) * np.abs(r) + (abs_l if f in ('khat',) else 0.)
            with np.errstate(all='ignore'):
                err = np.abs(g - r)
            assert np.all(err[ok] <= bound[ok]), (label, k, f, g, r)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('big_k', [1, 17])
@pytest.mark.parametrize('n', [1, 4, 5, 24, 25, 257, 1000])
def test_host_port_matches_the_reference(n, big_k, weighted):
    x, l, lw = host_case(n, big_k, weighted)
    got = reweight_moments(x, l, log_weights=lw)
    ref = reweight_reference(x, l, lw)
    assert isinstance(got, Reweighted) and got.n == n and got.mean.shape == (big_k, 3) and got.khat.shape == (big_k,)
    assert_against(got, ref, 'n=%d K=%d w=%d' % (n, big_k, weighted))
    if n >= 25:
        assert np.isfinite(got.khat).all() and np.all(got.flags == 0)
    else:
        assert np.isinf(got.khat).all() and np.all(got.flags == 2)
    # (n_chain, n_draw, d) input, torch CPU tensors: the same numbers
    if n == 1000:
        import torch
        again = reweight_moments(torch.as_tensor(x.reshape(4, 250, 3)), torch.as_tensor(l.reshape(4, 250, big_k)),
                                 log_weights=None if lw is None else lw.reshape(4, 250))
        for f in K_FIGS + KD_FIGS:
            assert getattr(again, f).tobytes() == getattr(got, f).tobytes(), f
        assert 'worst: scenario' in str(got)


# ---- 3: a closed form ------------------------------------------------------------------------------------------------------------------
def closed_form(seed):
    """f(x) = G x + g0 with d = 4, m = 12, a dense precision, a diagonal Gaussian prior: posterior and evidence are Gaussian.  20000
    independent draws from the exact posterior; the data moved so that the posterior mean of parameter 0 moves by 0.5 and by 1.0 base
    sd.  |mean - exact| <= 5 mcse_mean, khat < 0.5, sd within 5 %, the log evidence ratio to 0.02.  Seeds 1 to 3 of this very set-up,
    on the CPU: errors of at most 1.57 | 1.21 | 1.65 mcse, khat (0.17, 0.36) | (0.15, 0.36) | (0.22, 0.52), sd within 2.3 | 2.3 | 4.9 %,
    evidence-ratio errors of at most 0.015 | 0.007 | 0.010; seed 3 is over the khat bound at the full sd of shift, which is the
    method's limit and no fault of the code.  The test fixes seed 2."""
    rng = np.random.default_rng(seed)
    d, m, n = 4, 12, 20000
    g_mat, g0 = rng.normal(size=(m, d)), rng.normal(size=m)
    bm = rng.normal(size=(m, m))
    prec = bm @ bm.T / m + np.eye(m)
    mu0, s0 = rng.normal(size=d), rng.uniform(1., 2., size=d)
    y = g_mat @ rng.normal(size=d) + g0 + np.linalg.solve(np.linalg.cholesky(prec).T, rng.normal(size=m))
    lam = g_mat.T @ prec @ g_mat + np.diag(1. / s0**2)
    cov = np.linalg.inv(lam)
    post = lambda yy: cov @ (g_mat.T @ prec @ (yy - g0) + mu0 / s0**2)
    mean, sd = post(y), np.sqrt(np.diag(cov))
    y_new = []
    for s in (0.5, 1.0):
        target = np.zeros(d)
        target[0] = s * sd[0]
        y_new.append(y + g_mat @ np.linalg.solve(g_mat.T @ prec @ g_mat, lam @ target))
    y_new = np.array(y_new)
    for k in range(2):
        np.testing.assert_allclose(post(y_new[k]) - mean, [(0.5, 1.0)[k] * sd[0], 0., 0., 0.], atol=1e-10)
    cy = np.linalg.inv(prec) + (g_mat * s0**2) @ g_mat.T
    logev = lambda yy: -0.5 * (yy - g0 - g_mat @ mu0) @ np.linalg.solve(cy, yy - g0 - g_mat @ mu0)
    x = mean + rng.standard_normal((n, d)) @ np.linalg.cholesky(cov).T
    a, b = ratio_coefficients(y, y_new, prec=prec)
    l = (x @ g_mat.T + g0) @ a.T + b
    direct = np.array([[-0.5 * (f - yk) @ prec @ (f - yk) + 0.5 * (f - y) @ prec @ (f - y) for yk in y_new] for f in (x[:5] @ g_mat.T + g0)])
    np.testing.assert_allclose(l[:5], direct, rtol=1e-10, atol=1e-10)
    got = reweight_moments(x, l)
    print(got)
    for k in range(2):
        err = (got.mean[k] - post(y_new[k])) / got.mcse_mean[k]
        ev = got.log_evidence_ratio[k] - (logev(y_new[k]) - logev(y))
        print(k, 'error / mcse', err, 'khat', got.khat[k], 'sd / sd_base', got.sd[k] / got.sd_base, 'evidence-ratio error', ev, 'shift', got.shift[k])
    return got, np.array([post(yk) for yk in y_new]), np.array([logev(yk) - logev(y) for yk in y_new])


def test_linear_gaussian_closed_form():
    got, exact_mean, exact_ratio = closed_form(2)
    for k in range(2):
        assert np.all(np.abs(got.mean[k] - exact_mean[k]) <= 5. * got.mcse_mean[k])
        assert got.khat[k] < 0.5
        assert np.all(np.abs(got.sd[k] / got.sd_base - 1.) <= 0.05)
        assert abs(got.log_evidence_ratio[k] - exact_ratio[k]) <= 0.02
    assert got.n_khat_bad == 0
    rng = np.random.default_rng(5)
    m, y, y_new = 12, rng.normal(size=12), rng.normal(size=(2, 12))
    # the diagonal form of the coefficients
    pd = rng.uniform(0.5, 2., size=m)
    a1, b1 = ratio_coefficients(y, y_new[0], prec_diag=pd)
    a2, b2 = ratio_coefficients(y, y_new[:1], prec=np.diag(pd))
    np.testing.assert_allclose(a1, a2, rtol=1e-14)
    np.testing.assert_allclose(b1, b2, rtol=1e-13)


# ---- 4: degenerate input and refusals -----------------------------------------------------------------------------------------------------
def test_degenerate_input():
    n, d = 400, 3
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, d)) + 2.
    l = 0.4 * x[:, :1] * np.array([[0., 1., 1., 1., 1.]]) + np.array([[0., 0.3, 0.3, 0.3, 0.3]])
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.2] = -np.inf
    lw[7], lw[11] = 0.1, -np.inf
    # y_new == y: the ratio is 0 in every row; without weights the tail has no spread: the base table and a ratio of 0
    got = reweight_moments(x, l)
    print(got.khat, got.flags, got.log_evidence_ratio, got.shift[0])
    assert np.isinf(got.khat[0]) and got.flags[0] == 2 and got.log_evidence_ratio[0] == 0.
    np.testing.assert_allclose(got.mean[0], got.mean_base, rtol=0, atol=1e-13)
    np.testing.assert_allclose(got.sd[0], got.sd_base, rtol=1e-12)
    np.testing.assert_allclose(got.mean_base, x.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(got.sd_base, x.std(axis=0, ddof=1), rtol=1e-13)
    assert np.all(np.abs(got.shift[0]) < 1e-12) and got.shift[1, 0] > 0.2
    # a NaN draw in a row of zero weight is ignored; in a row of non-zero weight it takes its parameter in every scenario
    x2 = x.copy()
    x2[11, 1] = np.nan
    a, b = reweight_moments(x2, l, log_weights=lw), reweight_moments(x, l, log_weights=lw)
    for f in K_FIGS + KD_FIGS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    x2[7, 2] = np.inf
    a = reweight_moments(x2, l, log_weights=lw)
    ref = reweight_reference(x2, l, lw)
    assert_against(a, ref, 'bad draw')
    assert np.isnan(a.mean[:, 2]).all() and np.isnan(a.sd_base[2]) and np.isfinite(a.mean[:, :2]).all() and np.isfinite(a.khat).all()
    # a non-finite ratio in a row of non-zero weight takes its scenario; in a row of zero weight it is ignored
    l2 = l.copy()
    l2[11, 1], l2[7, 2], l2[7, 3] = np.nan, np.nan, np.inf
    a = reweight_moments(x, l2, log_weights=lw)
    assert_against(a, reweight_reference(x, l2, lw), 'bad ratio')
    assert a.flags.tolist() == [0, 0, 1, 1, 0] and np.isnan(a.mean[2]).all() and np.isnan(a.khat[3]) and np.isfinite(a.mean[1]).all()
    assert a.mean[1].tobytes() == b.mean[1].tobytes()
    # no row of non-zero weight
    a = reweight_moments(x, l, log_weights=np.full(n, -np.inf))
    assert np.all(a.flags == 4) and np.isnan(a.mean).all() and np.isnan(a.khat).all() and np.isnan(a.mean_base).all()
    assert a.n_tail.tolist() == [60] * 5
    # shapes
    for bad in (lambda: reweight_moments(x, l[:-1]), lambda: reweight_moments(x, l[:, 0]), lambda: reweight_moments(x[:, 0], l),
                lambda: reweight_moments(x, l, log_weights=lw[:-1]), lambda: reweight_moments(x[:0], l[:0])):
        with pytest.raises(ValueError):
            bad()


def test_refusals(monkeypatch):
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import data_reweight as exported, reweight_moments as rm, Reweighted as rw
    assert exported is data_reweight and rm is reweight_moments and rw is Reweighted
    from bayesfast_amd import utils
    for name in ('reweight_moments', 'data_reweight', 'Reweighted'):
        assert name in utils.__all__ and name in bfa.__all__ and getattr(bfa, name) is getattr(utils, name)
    su = bfa.PolyModel('quadratic', input_size=2, output_size=3)
    den = bfa.Chi2PipelineDensity(su, np.zeros(3), prec_diag=np.ones(3))
    x = np.zeros((10, 2))
    with pytest.raises(NotImplementedError, match='GPU tensor'):
        data_reweight(den, x, np.ones(3))
    with pytest.raises(NotImplementedError, match='GPU tensor'):
        den.data_reweight(x, np.ones(3))
    with pytest.raises(NotImplementedError, match='GPU tensor'):
        den.data_log_ratio(x, np.ones(3))
    with pytest.raises(ValueError, match='Chi2PipelineDensity'):
        data_reweight(su, x, np.ones(3))
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='gather'):
        data_reweight(den, x, np.ones(3))
    for bad in (np.ones(4), np.ones((2, 4)), np.ones((1, 2, 3))):
        with pytest.raises(ValueError):
            ratio_coefficients(np.zeros(3), bad, prec_diag=np.ones(3))
    assert hasattr(bfa.TraceTuple, 'data_reweight')


def test_rows_of_zero_weight_in_the_tail_stay_out_of_the_table():
    """With fewer than n_tail + 1 rows of non-zero weight ``psis`` hands smoothed weight to rows of zero
    weight: ess and the evidence ratio are ``psis``'s, the table's weights are normalised over the rows of the sample -- moving every
    draw by a constant moves the means by that constant and nothing else."""
    from bayesfast_amd.utils.psis import psis
    for n, live in ((100, 18), (257, 46)):   # n_tail = 20 | 49: the tail and its cut hold 3 | 4 rows of zero weight
        x, l, lw = host_case(n, 3, True)
        lw = 0.7 * np.random.default_rng(n).standard_normal(n)
        lw[np.random.default_rng(n + 1).permutation(n)[live:]] = -np.inf
        got, ref = reweight_moments(x, l, log_weights=lw), reweight_reference(x, l, lw)
        assert_against(got, ref, 'n=%d' % n)
        ps = psis(lw - np.log(np.exp(lw - lw.max()).sum()) - lw.max() + l[:, 1])
        dead = np.exp(ps.log_weights[lw == -np.inf]).sum()
        print(n, 'weight on rows of zero weight', dead, 'ess', got.ess[1], ps.ess)
        assert dead > 0 and abs(got.ess[1] / ps.ess - 1) < 1e-12 and abs(got.khat[1] - ps.khat) < 1e-12
        moved = reweight_moments(x + 1000., l, log_weights=lw)
        print(n, 'moved: largest change of a mean / sd_base', np.max(np.abs(moved.mean - 1000. - got.mean) / got.sd_base))
        assert np.all(np.abs(moved.mean - 1000. - got.mean) <= 1e-9 * got.sd_base) and np.all(np.abs(moved.sd / got.sd - 1.) <= 1e-9)
