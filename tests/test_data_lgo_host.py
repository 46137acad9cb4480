"""The host side of leave-group-out cross-validation (bayesfast_amd/utils/data_lgo.py): no GPU.

- ``group_whitening_of`` against an independent derivation, the conditional Gaussian from the covariance (mean f_B + Sigma_B,-B
  Sigma_-B,-B^-1 (y - f)_-B, Schur-complement covariance) through ``scipy.stats.multivariate_normal.logpdf``, 1e-10 relative; singleton
  groups against ``data_loo.whitening_of``;
- the host port against the loop-written reference of helpers/lgo_reference.py, 1e-9 relative (``ROUNDING`` below: what rounding
  alone does to the reference on these inputs stays under that);
- the closed form on a linear-Gaussian model, where log p(y_B | y_-B) is exact from the marginal of y;
- the argument checks.

ROUNDING.  helpers/lgo_reference.py in float64 against itself in numpy.longdouble on the inputs of
``test_host_port_matches_the_reference`` (every n, every weighting, the four columns), largest relative difference per figure, times
ten (docs/EXPERIMENTS.md has the table): every entry is below 1e-9, so RTOL holds for every figure."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import data_loo_reference as dr  # noqa: E402
import lgo_reference as lr  # noqa: E402
from lgo_cases import RTOL, FIGURES, chi2_case, compare  # noqa: E402

EPS = 2.0**-52
SIZES = (1, 24, 25, 224, 225, 226, 1000, 4097)
WEIGHTINGS = ('plain', 'weights', 'mostly zero')
# ten times the largest relative difference between the float64 and the longdouble reference over SIZES x WEIGHTINGS x four columns
ROUNDING = dict(lpd=7.3e-14, p_waic=2.3e-14, elpd_waic=1.8e-14, elpd_lgo=3.8e-13, p_lgo=3.9e-13, khat=1e-13, sigma=1.3e-13, ess_lgo=1.9e-13,
                chi2_base=2.8e-14, chi2_lgo=6.9e-14, ppp_base=4.9e-14, ppp_lgo=7.2e-13)


# ---- 1: the whitening ----------------------------------------------------------------------------------------------------------------
def precision(dense, m=12, seed=3):
    rng = np.random.default_rng(seed)
    if dense:
        l = np.eye(m) + 0.3 * rng.standard_normal((m, m))
        return l @ l.T
    return np.diag(rng.uniform(0.5, 4., size=m))


GROUPS12 = ([3], [5, 6], [0, 4, 9], [1, 2, 7, 8, 10, 11])


@pytest.mark.parametrize('dense', [False, True])
def test_whitening_against_the_conditional_gaussian(dense):
    from bayesfast_amd.utils import group_whitening_of
    p = precision(dense)
    rng = np.random.default_rng(11)
    y, f = rng.standard_normal(12), rng.standard_normal(12)
    kw = dict(prec=p) if dense else dict(prec_diag=np.diag(p))
    a, const, sizes, colg = group_whitening_of(groups=GROUPS12, **kw)
    assert a.shape == (12, 12) and sizes.tolist() == [1, 2, 3, 6] and colg.tolist() == [0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3]
    z = a @ (y - f)
    for k, g in enumerate(GROUPS12):
        ell = const[k] - 0.5 * np.sum(z[colg == k]**2)
        want = lr.whiten_reference(p, y, f, g)
        assert abs(ell - want) <= 1e-10 * abs(want), (dense, k, ell, want)


@pytest.mark.parametrize('dense', [False, True])
def test_singleton_groups_are_whitening_of(dense):
    """For b = 1 both routes take one square root of P_ii and divide row i of P by it: L_B = sqrt(P_ii) has condition number 1, so the
    two Cholesky paths (LAPACK's 1 x 1 factor and a triangular solve here, numpy's sqrt and a division there) differ by at most the
    roundings of a square root and a division, 2 EPS relative per entry of W; a b x b block would allow b EPS cond(P_BB).  c_i is
    log(sqrt(P_ii)) - log(2 pi) / 2 here and log(P_ii / 2 pi) / 2 there: three roundings of terms of size at most |log P_ii| + log 2 pi."""
    from bayesfast_amd.utils import group_whitening_of
    from bayesfast_amd.utils.data_loo import whitening_of
    p = precision(dense)
    kw = dict(prec=p) if dense else dict(prec_diag=np.diag(p))
    a, const, sizes, colg = group_whitening_of(groups=[[i] for i in range(12)], **kw)
    w, c = whitening_of(**kw)
    assert np.all(np.abs(a - w) <= 2. * EPS * np.abs(w))
    assert np.all(np.abs(const - c) <= 3. * EPS * (np.abs(np.log(np.diag(p))) + np.log(2. * np.pi)))
    assert sizes.tolist() == [1] * 12 and colg.tolist() == list(range(12))


# ---- 2: the host port against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_host_port_matches_the_reference(n):
    from bayesfast_amd.utils import grouped_loo
    for weighting in WEIGHTINGS:
        q, dof, const, lw = chi2_case(n, weighting)
        got = grouped_loo(q, dof, const, log_weights=lw)
        refs = [lr.group_reference(q[:, j], dof[j], const[j], lw) for j in range(q.shape[1])]
        compare(got, refs, '%s n=%d' % (weighting, n), ROUNDING)
        assert got.n == n and got.size.tolist() == [1, 2, 17, 457]
    q, dof, const, _ = chi2_case(n, 'plain')
    got3 = grouped_loo(q.reshape(1, n, -1), dof, const)          # (n_chain, n_draw, K)
    assert got3.ppp_lgo.tobytes() == grouped_loo(q, dof, const).ppp_lgo.tobytes()


@pytest.mark.parametrize('n', [25, 1000])
def test_singleton_groups_give_pointwise_loo(n):
    from bayesfast_amd.utils import grouped_loo, pointwise_loo
    rng = np.random.default_rng(n)
    z = rng.standard_normal((n, 3)) * np.array([1., 1.6, 0.5])
    c = np.array([-0.3, 0.4, 1.1])
    lw = 0.7 * rng.standard_normal(n)
    for w in (None, lw):
        got = grouped_loo(z * z, np.ones(3), c, log_weights=w)
        loo = pointwise_loo(c - 0.5 * (z * z), log_weights=w)
        for f, g in (('lpd', 'lpd'), ('p_waic', 'p_waic'), ('elpd_waic', 'elpd_waic'), ('elpd_lgo', 'elpd_loo'), ('p_lgo', 'p_loo'),
                     ('khat', 'khat'), ('sigma', 'sigma'), ('ess_lgo', 'ess_loo')):
            assert np.all(np.abs(getattr(got, f) - getattr(loo, g)) <= RTOL * np.abs(getattr(loo, g))), (f, n)
        assert np.array_equal(got.n_tail, loo.n_tail)
        # for one point the survival function of z^2 is the two-sided tail of z
        from scipy.special import ndtr
        refs = [lr.group_reference(z[:, j]**2, 1., c[j], w) for j in range(3)]
        two_sided = np.array([sum(np.exp(dr.normalise(w)[s] if w is not None else -np.log(n)) * 2. * ndtr(-abs(z[s, j])) for s in range(n))
                              for j in range(3)])
        assert np.all(np.abs(got.ppp_base - two_sided) <= RTOL * two_sided)
        compare(got, refs, 'singletons n=%d' % n)


def test_host_port_special_columns():
    """A NaN in a row of zero weight is ignored; a NaN and a +inf q (ell = -inf) at non-zero weight make the column NaN; a constant
    column has a flat tail, khat = inf and unsmoothed weights; ties across the cut (q rounded to 0.1)."""
    from bayesfast_amd.utils import grouped_loo
    n = 1000
    rng = np.random.default_rng(5)
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.5] = -np.inf
    lw[7], lw[11] = 0.1, -np.inf
    base = rng.chisquare(3, size=n)
    cols = [base.copy() for _ in range(5)]
    cols[0][7] = np.nan
    cols[1][7] = np.inf
    cols[2][11] = np.nan
    cols[3] *= 2.
    cols[4] = np.round(base / 0.1) * 0.1
    q = np.stack(cols, axis=1)
    dof, const = np.full(5, 3.), np.full(5, -1.5)
    got = grouped_loo(q, dof, const, log_weights=lw)
    compare(got, [lr.group_reference(c, 3., -1.5, lw) for c in cols], 'special')
    assert np.isnan(got.elpd_lgo[[0, 1]]).all() and np.isnan(got.ppp_lgo[[0, 1]]).all() and np.isnan(got.chi2_base[[0, 1]]).all()
    assert np.isfinite(got.elpd_lgo[[2, 3, 4]]).all() and np.isfinite(got.ppp_lgo[[2, 3, 4]]).all()
    assert np.isnan(got.elpd_lgo_total)
    flat = np.full((n, 1), 4.)
    plain = grouped_loo(np.concatenate([flat, q[:, 4:5]], axis=1), dof[:2], const[:2])   # without weights the constant column's tail is flat
    # p_waic of a constant column is rounding alone: its mean is off by at most n EPS |ell|, the sum of squares by that squared
    compare(plain, [lr.group_reference(flat[:, 0], 3., -1.5), lr.group_reference(cols[4], 3., -1.5)], 'flat, ties',
            waic_abs=(n * 2.3e-16 * 3.5)**2)
    assert np.isinf(plain.khat[0]) and plain.khat[0] > 0 and abs(plain.p_lgo[0]) < 1e-12 and plain.n_khat_bad >= 1
    assert abs(plain.chi2_lgo[0] - 4.) < 1e-12 and abs(plain.ppp_lgo[0] - lr.survival(3., 4.)) < 1e-12
    empty = grouped_loo(q[:, 3:4], dof[:1], const[:1], log_weights=np.full(n, -np.inf))   # no row of non-zero weight
    assert all(np.isnan(getattr(empty, f)[0]) for f in FIGURES)


# ---- 3: the closed form --------------------------------------------------------------------------------------------------------------
GROUPS48 = ([5], [10, 11], [14, 15, 16], [20, 21, 22, 23], [33, 34, 35, 36, 37, 38, 39, 40], [2, 19, 44])


def linear_gaussian_groups(seed, dense, n=40000, m=48, d=3):
    """test_data_loo_host.py's model: y = A theta + e, e ~ N(0, Sigma), theta ~ N(0, 4 I), one point shifted by 1.5 sigma; n exact
    posterior draws.  Returns q (n, K), the sizes, c_B, the exact log p(y_B | y_-B) from the marginal y ~ N(0, K^-1), K = (Sigma +
    4 A A^T)^-1, and for every group the mean of Q over n exact draws from the posterior given y_-B alone."""
    from bayesfast_amd.utils import group_whitening_of
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

    def posterior_draws(rows):
        pr = np.linalg.inv(sigma[np.ix_(rows, rows)])
        cov = np.linalg.inv(a[rows].T @ pr @ a[rows] + np.eye(d) / 4.)
        mean = cov @ (a[rows].T @ pr @ y[rows])
        return mean + rng.standard_normal((n, d)) @ np.linalg.cholesky(cov).T

    w, const, sizes, colg = group_whitening_of(prec=p, groups=GROUPS48) if dense else group_whitening_of(prec_diag=np.diag(p), groups=GROUPS48)
    chi2 = lambda draws, k: (((y - draws @ a.T) @ w[colg == k].T)**2).sum(axis=1)
    full = posterior_draws(np.arange(m))
    q = np.stack([chi2(full, k) for k in range(len(GROUPS48))], axis=1)
    kk = np.linalg.inv(sigma + 4. * a @ a.T)
    ky = kk @ y
    exact, ppp = [], []
    for k, g in enumerate(GROUPS48):
        kbb = kk[np.ix_(g, g)]
        exact.append(-0.5 * len(g) * np.log(2. * np.pi) + 0.5 * np.linalg.slogdet(kbb)[1] - 0.5 * ky[g] @ np.linalg.solve(kbb, ky[g]))
        rest = np.setdiff1d(np.arange(m), g)
        ppp.append(lr.survival(len(g), chi2(posterior_draws(rest), k)).mean())
    return q, sizes, const, np.array(exact), np.array(ppp)


# twice the largest per-group error of the host port over the seeds 0 .. 19 (Monte-Carlo error of 40 000 draws), measured on the CPU:
# diagonal: |elpd_lgo - exact| up to ELPD_SEEN[0], |ppp_lgo - exact| up to PPP_SEEN[0]; dense: ELPD_SEEN[1], PPP_SEEN[1]
ELPD_SEEN = (0.0137, 0.0206)
PPP_SEEN = (0.00590, 0.00433)


@pytest.mark.parametrize('dense', [False, True])
def test_closed_form_on_a_linear_gaussian_model(dense):
    """m = 48, d = 3, 40 000 exact posterior draws, seed 100 (not one of the 20 the bounds were measured on); groups of 1, 2, 3, 4 and
    8 adjacent points and one of 3 scattered points.  Every group has khat < 0.7 (the largest over the 20 seeds was 0.644 diagonal,
    0.619 dense); per group |elpd_lgo - exact| and |ppp_lgo - exact| stay within twice the largest error seen over those seeds:
    diagonal 2 x 0.0137 and 2 x 0.00590, dense 2 x 0.0206 and 2 x 0.00433 (docs/EXPERIMENTS.md).  A group of 16 is deliberately not in
    the set: its khat passes 0.7 on some seeds.  The group of 8 is outputs 33 .. 40: khat is a property of the rows of A that the block
    holds, and a block of 8 at outputs 28 .. 35 carries the posterior at some of the 20 seeds (khat 0.95 at seed 14, dense), which is
    the method's honest answer there and no test of its figures."""
    from bayesfast_amd.utils import grouped_loo
    q, sizes, const, exact, ppp = linear_gaussian_groups(100, dense)
    got = grouped_loo(q, sizes, const)
    e_err, p_err = np.max(np.abs(got.elpd_lgo - exact)), np.max(np.abs(got.ppp_lgo - ppp))
    print('dense' if dense else 'diagonal', 'largest khat', got.khat.max(), 'elpd error', e_err, 'ppp error', p_err, 'ppp_lgo', got.ppp_lgo,
          'ppp_base', got.ppp_base)
    assert got.khat.max() < 0.7 and got.n_khat_bad == 0
    assert e_err <= 2. * ELPD_SEEN[int(dense)]
    assert p_err <= 2. * PPP_SEEN[int(dense)]


# ---- 4: the arguments ------------------------------------------------------------------------------------------------------------------
def test_group_arguments():
    from bayesfast_amd.utils import group_whitening_of, grouped_loo, DataLGO
    p = precision(True)
    for bad in ([[0, 1], [1, 2]],            # overlapping
                [[0, 1], []],                # empty
                [[2, 1]],                    # unsorted
                [[1, 1]],                    # not unique
                [[0, 12]], [[-1, 3]],        # out of range
                [], None, 'ab', [[0.5, 1.]], 3,
                np.zeros(11, dtype=np.int64),          # a label array of the wrong length
                np.full(12, -2), np.full(12, -1)):     # labels below -1; no group at all
        with pytest.raises(ValueError):
            group_whitening_of(prec=p, groups=bad)
    with pytest.raises(ValueError):
        group_whitening_of(prec=p, prec_diag=np.ones(12), groups=[[0]])
    with pytest.raises(ValueError):
        group_whitening_of(groups=[[0]])
    labels = np.full(12, -1)
    for k, g in enumerate(GROUPS12[:3]):
        labels[g] = 2 * k + 1                 # (the groups are the labels in ascending order, whatever their values)
    by_list = group_whitening_of(prec=p, groups=[list(g) for g in GROUPS12[:3]])
    by_tuple = group_whitening_of(prec=p, groups=tuple(np.array(g) for g in GROUPS12[:3]))
    by_label = group_whitening_of(prec=p, groups=labels)
    for u, v, t in zip(by_list, by_label, by_tuple):
        assert np.array_equal(u, v) and np.array_equal(u, t)
    q = np.random.default_rng(0).chisquare(2, size=(50, 2))
    for kw in (dict(dof=[2.]), dict(dof=[2., 0.]), dict(dof=[2., 2.], const=[0.]), dict(dof=[2., 2.], log_weights=np.zeros(49))):
        with pytest.raises(ValueError):
            grouped_loo(q, **kw)
    with pytest.raises(ValueError):
        grouped_loo(q[:, 0], [2.])
    one, two = grouped_loo(q, [2., 2.]), grouped_loo(q[:, :1], [2.])
    assert isinstance(one, DataLGO) and one.compare(one) == (0., 0.) and 'DataLGO: 2 groups' in str(one)
    with pytest.raises(ValueError):
        one.compare(two)
    import bayesfast_amd
    from bayesfast_amd.core.density import Chi2PipelineDensity
    from bayesfast_amd.samplers.sample_trace import TraceTuple
    assert bayesfast_amd.data_lgo is bayesfast_amd.utils.data_lgo and hasattr(Chi2PipelineDensity, 'data_lgo') and hasattr(TraceTuple, 'data_lgo')
    with pytest.raises(NotImplementedError):
        bayesfast_amd.data_lgo(object(), np.zeros((4, 2)), [[0]])   # host draws
