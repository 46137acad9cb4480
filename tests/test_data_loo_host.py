"""The host side of pointwise PSIS-LOO and WAIC (bayesfast_amd/utils/data_loo.py, device.residual_dense): no GPU.

- the host port against the loop-written reference of helpers/data_loo_reference.py, 1e-9 relative (two float64 routes of the same
  formulas; what rounding alone does to them is in tests/test_gpu_data_loo.py's docstring);
- the closed form on a linear-Gaussian model, where log p(y_i | y_-i) is exact from the marginal of y;
- the residual model against the extended-precision restatement of tests/test_polymodel_kernels.py;
- the interface."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import data_loo_reference as dr  # noqa: E402

RTOL = 1e-9
FIGURES = ('lpd', 'p_waic', 'elpd_waic', 'elpd_loo', 'p_loo', 'khat', 'sigma', 'ess_loo', 'pit')


def _compare(got, refs, label, waic_abs=0.):
    for j, r in enumerate(refs):
        assert int(got.n_tail[j]) == r['n_tail']
        for f in FIGURES:
            g, w = getattr(got, f)[j], np.float64(r[f])
            if not np.isfinite(w):
                assert np.array_equal(g, w, equal_nan=True), (label, j, f, g, w)
            elif f == 'p_loo':
                assert abs(g - w) <= RTOL * max(abs(np.float64(r['lpd'])), abs(np.float64(r['elpd_loo']))), (label, j, f, g, w)
            else:
                assert abs(g - w) <= RTOL * abs(w) + (waic_abs if 'waic' in f else 0.), (label, j, f, g, w)


# ---- 1: the host port against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('n', [1, 24, 25, 224, 225, 226, 1000, 4097])
def test_host_port_matches_the_reference(n, k):
    from bayesfast_amd.utils import pointwise_loo
    rng = np.random.default_rng(10 * n + k)
    z = rng.standard_normal((n, k)) * np.array([1., 1.6, 0.5])[:k]
    ell = np.array([-0.3, 0.4, 1.1])[:k] - 0.5 * z * z
    lw = 0.7 * rng.standard_normal(n)
    sparse = np.where(rng.random(n) < 0.8, -np.inf, lw)
    sparse[0] = 0.
    for label, w in (('plain', None), ('weights', lw), ('mostly zero', sparse)):
        got = pointwise_loo(ell, log_weights=w, z=z)
        _compare(got, [dr.column_reference(ell[:, j], w, z[:, j]) for j in range(k)], '%s n=%d' % (label, n))
        assert got.n == n and got.outputs.tolist() == list(range(k))
    got3 = pointwise_loo(ell.reshape(1, n, k), z=z.reshape(1, n, k))          # (n_chain, n_draw, k)
    assert got3.elpd_loo.tobytes() == pointwise_loo(ell, z=z).elpd_loo.tobytes()


def test_host_port_special_columns():
    """A NaN in a row of zero weight is ignored; a NaN, a +inf and a -inf ell at non-zero weight make the column NaN; a flat tail has
    khat = inf and unsmoothed weights; ties across the cut (ell rounded to 0.05)."""
    from bayesfast_amd.utils import pointwise_loo
    n = 1000
    rng = np.random.default_rng(5)
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.5] = -np.inf
    lw[7], lw[11] = 0.1, -np.inf
    base = -0.5 * rng.standard_normal(n)**2
    cols = [base.copy() for _ in range(6)]
    cols[0][7] = np.nan
    cols[1][7] = np.inf
    cols[2][11] = np.nan
    cols[3] *= 2.
    const = np.full(n, -2.)
    cols[4] = np.round(base / 0.05) * 0.05
    cols[5][7] = -np.inf
    ell = np.stack(cols, axis=1)
    got = pointwise_loo(ell, log_weights=lw)
    _compare(got, [dr.column_reference(c, lw) for c in cols], 'special')
    assert np.isnan(got.elpd_loo[[0, 1, 5]]).all() and np.isfinite(got.elpd_loo[[2, 3, 4]]).all()
    assert np.isnan(got.pit).all() and np.isnan(got.elpd_loo_total)
    ell[:, 3] = const
    plain = pointwise_loo(ell[:, 3:5])                                       # without weights the constant column's tail is flat
    # p_waic of a constant column is rounding alone: its mean is off by at most n EPS |ell|, the sum of squares by that squared
    _compare(plain, [dr.column_reference(const), dr.column_reference(cols[4])], 'flat, ties', waic_abs=(n * 2.3e-16 * 2.)**2)
    assert np.isinf(plain.khat[0]) and plain.khat[0] > 0 and abs(plain.p_loo[0]) < 1e-12 and plain.n_khat_bad >= 1


# ---- 2: the closed form -------------------------------------------------------------------------------------------------------------------
def linear_gaussian(seed, dense, n=40000, m=48, d=3):
    """y = A theta + e, e ~ N(0, Sigma), theta ~ N(0, 4 I), one point shifted by 1.5 sigma; n exact posterior draws.  Returns
    ell (n, m), z (n, m) and the exact log p(y_i | y_-i) and pit from the marginal y ~ N(0, Sigma + 4 A A^T)."""
    from scipy.special import ndtr
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, d))
    if dense:
        l = np.eye(m) + 0.05 * rng.standard_normal((m, m))
        sigma = l @ l.T / 4.
    else:
        sigma = np.diag(rng.uniform(0.1, 0.5, size=m))
    theta = 2. * rng.standard_normal(d)
    y = a @ theta + np.linalg.cholesky(sigma) @ rng.standard_normal(m)
    y[m // 2] += 1.5 * np.sqrt(sigma[m // 2, m // 2])
    p = np.linalg.inv(sigma)
    post_prec = a.T @ p @ a + np.eye(d) / 4.
    post_cov = np.linalg.inv(post_prec)
    mean = post_cov @ (a.T @ p @ y)
    draws = mean + rng.standard_normal((n, d)) @ np.linalg.cholesky(post_cov).T
    dg = np.diag(p)
    w = p / np.sqrt(dg)[:, None]
    z = (y - draws @ a.T) @ w.T
    ell = 0.5 * np.log(dg / (2. * np.pi)) - 0.5 * z * z
    k = np.linalg.inv(sigma + 4. * a @ a.T)
    ky, kd = k @ y, np.diag(k)
    return ell, z, 0.5 * np.log(kd / (2. * np.pi)) - 0.5 * ky * ky / kd, ndtr(ky / np.sqrt(kd))


# twice the largest per-point error of the host port over the seeds 0 .. 19 (Monte-Carlo error of 40 000 draws), measured on the CPU:
# diagonal: |elpd_loo - exact| up to ELPD_SEEN[0], |pit - exact| up to PIT_SEEN[0]; dense: ELPD_SEEN[1], PIT_SEEN[1]
ELPD_SEEN = (0.0213, 0.0203)
PIT_SEEN = (0.00202, 0.00232)


@pytest.mark.parametrize('dense', [False, True])
def test_closed_form_on_a_linear_gaussian_model(dense):
    """m = 48, d = 3, 40 000 exact posterior draws, seed 100 (not one of the 20 the bounds were measured on).  Every point has
    khat < 0.7 (the largest over the 20 seeds was 0.565 diagonal, 0.550 dense); per point |elpd_loo - exact| and |pit - exact| stay
    within twice the largest error seen over those seeds: diagonal 2 x 0.0213 and 2 x 0.00202, dense 2 x 0.0203 and 2 x 0.00232
    (docs/EXPERIMENTS.md).  p_loo_total and p_waic_total are printed."""
    from bayesfast_amd.utils import pointwise_loo
    ell, z, exact, pit = linear_gaussian(100, dense)
    got = pointwise_loo(ell, z=z)
    e_err, p_err = np.max(np.abs(got.elpd_loo - exact)), np.max(np.abs(got.pit - pit))
    print('dense' if dense else 'diagonal', 'largest khat', got.khat.max(), 'elpd error', e_err, 'pit error', p_err, 'p_loo_total',
          got.p_loo_total, 'p_waic_total', got.p_waic_total)
    assert got.khat.max() < 0.7 and got.n_khat_bad == 0
    assert e_err <= 2. * ELPD_SEEN[int(dense)]
    assert p_err <= 2. * PIT_SEEN[int(dense)]


# ---- 3: the residual model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', [3, 17])
@pytest.mark.parametrize('kind', ['linear', 'quad', 'cubic'])
def test_residual_model_is_the_whitened_residual(kind, d, dense):
    """The restatement of the residual description equals W (y - f) of the restated original, inside, outside and far outside the
    bound, within 4 (m + _acc_len(poly)) EPS sum_j |W_ij| (|y_j| + sf_j): the forward bound of the float64 contraction that builds
    the coefficients (m terms per coefficient, each coefficient then in a term of the restatement's own sums)."""
    from test_polymodel_kernels import restate_poly, random_poly, random_points, _acc_len, EPS, LD
    from bayesfast_amd.device import polymodel_dense_from_poly, residual_dense, polymodel_desc_from_dense
    from bayesfast_amd.utils.data_loo import whitening_of
    rng = np.random.default_rng(1000 * d + 10 * len(kind) + dense)
    m = 21
    poly = random_poly(rng, d, m, kind)
    x = random_points(rng, poly, 48)
    f, _, sf, _, info = restate_poly(poly, x, jac=False)
    if kind != 'linear':
        assert info['outside'].any() and (~info['outside']).any() and np.max(info['beta']) > 400 * float(poly['alpha'])
    y = rng.normal(size=m)
    bmat = rng.normal(size=(m, m))
    prec = bmat @ bmat.T / m + 0.5 * np.eye(m) if dense else None
    pdiag = None if dense else rng.uniform(0.2, 3., size=m)
    w, c = whitening_of(prec, pdiag)
    np.testing.assert_allclose(c, 0.5 * np.log((np.diag(prec) if dense else pdiag) / (2 * np.pi)), rtol=1e-15)
    dense_arrays = polymodel_dense_from_poly(poly)
    res = residual_dense(dense_arrays, y, w)
    ds, keep = polymodel_desc_from_dense(res)
    assert ds.m == m and ds.d == d and ds.use_bound == (0 if kind == 'linear' else 1)
    # the residual description as a poly spec of full masks, for the restatement
    full = np.arange(d)
    cfgs = [dict(order='linear', input_mask=full, output_mask=np.arange(m), coef=np.concatenate([res['c0'][:, None], res['lin']], axis=1))]
    if res['quad'] is not None:
        cfgs.append(dict(order='quadratic', input_mask=full, output_mask=np.arange(m), coef=res['quad']))
    if res['mask2'].size:
        cfgs.append(dict(order='cubic-2', input_mask=res['mask2'], output_mask=np.arange(m), coef=res['cub2']))
    if res['mask3'].size:
        cfgs.append(dict(order='cubic-3', input_mask=res['mask3'], output_mask=np.arange(m), coef=res['cub3']))
    rpoly = dict(input_size=d, output_size=m, use_bound=res['use_bound'], configs=cfgs)
    if res['use_bound']:
        rpoly.update(mu=res['mu'], hess=res['hess'], alpha=res['alpha'], f_mu=res['f_mu'])
    elif 'mu' in poly:
        rpoly.update(mu=poly['mu'], hess=poly['hess'], alpha=poly['alpha'], f_mu=np.zeros(m), use_bound=True)   # (ignored: all linear)
    zr = restate_poly(rpoly, x, jac=False)[0]
    wl = np.asarray(w, dtype=LD)
    want = np.einsum('ij,nj->ni', wl, y.astype(LD) - f)
    tol = 4 * (m + _acc_len(poly)) * EPS * np.einsum('ij,nj->ni', np.abs(wl), np.abs(y.astype(LD)) + sf)
    err = np.abs(zr - want)
    print(kind, d, dense, 'largest error / tolerance', float(np.max(err / tol)))
    assert np.all(err <= tol)


# ---- 4: the interface ---------------------------------------------------------------------------------------------------------------------
def test_interface(monkeypatch):
    import bayesfast_amd as bfa
    from bayesfast_amd import _lib, parallel, utils
    from bayesfast_amd.utils import DataLOO, data_loo, pointwise_loo
    for name in ('data_loo', 'pointwise_loo', 'DataLOO'):
        assert name in utils.__all__ and name in bfa.__all__ and getattr(bfa, name) is getattr(utils, name)
    _lib.build()
    assert _lib.lib().bfhip_version() >= 111
    rng = np.random.default_rng(3)
    ell = -0.5 * rng.standard_normal((500, 4))**2
    a, b = pointwise_loo(ell), pointwise_loo(ell - 0.1 * rng.random(4))
    diff, se = a.compare(b)
    d_i = a.elpd_loo - b.elpd_loo
    assert diff == d_i.sum() and se == np.sqrt(4 * d_i.var(ddof=1)) and diff > 0
    assert a.compare(a) == (0., 0.)
    with pytest.raises(ValueError):
        a.compare(pointwise_loo(ell[:, :3]))
    with pytest.raises(ValueError):
        a.compare(None)
    assert a.elpd_loo_total == a.elpd_loo.sum() and a.se_elpd_loo == np.sqrt(4 * a.elpd_loo.var(ddof=1))
    assert a.p_loo_total == a.p_loo.sum() and a.elpd_waic_total == a.elpd_waic.sum() and a.p_waic_total == a.p_waic.sum()
    assert 'elpd_loo' in str(a) and 'khat' in repr(a)
    for bad in (ell[:, 0], ell.reshape(5, 10, 10, 4), ell[:0], ell[:, :0]):
        with pytest.raises(ValueError):
            pointwise_loo(bad)
    with pytest.raises(ValueError):
        pointwise_loo(ell, log_weights=np.zeros(499))
    with pytest.raises(ValueError):
        pointwise_loo(ell, z=ell[:, :3])
    su = bfa.PolyModel('linear', input_size=2, output_size=3)
    den = bfa.Chi2PipelineDensity(su, np.zeros(3), prec_diag=np.ones(3))
    with pytest.raises(NotImplementedError):
        data_loo(den, np.zeros((10, 2)))
    with pytest.raises(NotImplementedError):
        den.data_loo(np.zeros((10, 2)))
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='gather'):
        data_loo(den, np.zeros((10, 2)))
