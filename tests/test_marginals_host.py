"""The host port of ``bayesfast_amd.utils.marginals`` against the Python-integer reference of helpers/marginals_reference.py, against
``np.histogram`` / ``np.histogram2d`` on inputs that keep clear of the edges, its properties, special values, errors and the
``Marginals`` object.  Every integer is compared with ==."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import marginals_reference as mr  # noqa: E402

from bayesfast_amd.utils import marginals, Marginals  # noqa: E402
from bayesfast_amd.utils.marginals import weight_shift  # noqa: E402

SHAPES = [(1, 1), (2, 2), (257, 3), (1000, 17), (7, 33, 5)]
BINS = (1, 2, 3, 64, 100, 1024)
BINS2D = (1, 2, 3, 64, 100, 128)


def draws(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) * (1. + np.arange(shape[-1])) + np.arange(shape[-1])


def weights_of(kind, shape, seed):
    rng = np.random.default_rng(seed + 1)
    if kind is None:
        return None
    w = rng.gamma(0.3, size=shape)
    if kind == 'zeros':
        w[rng.random(shape) < 0.9] = 0.
        w.reshape(-1)[0] = 1.
    elif kind == 'dominant':
        w.reshape(-1)[w.size // 2] = 50. * w.sum() + 1.
    return w


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', [None, 'gamma', 'zeros', 'dominant'])
def test_host_port_against_the_reference(shape, kind):
    x = draws(shape, sum(shape))
    w = weights_of(kind, shape[:-1], sum(shape))
    # the bin counts rotate over the shapes and kinds: every one of them meets every shape class over the grid
    k = SHAPES.index(shape) + [None, 'gamma', 'zeros', 'dominant'].index(kind)
    for step in range(2):
        bins, bins2d = BINS[(k + 3 * step) % 6], BINS2D[(k + 3 * step + 1) % 6]
        pairs = 'all' if shape[-1] <= 5 else [(0, 1), (16, 3), (2, 2), (0, 1)]
        ref = mr.reference(x, weights=w, bins=bins, bins2d=bins2d, pairs=pairs, loops=np.prod(shape) < 3000)
        got = marginals(x, weights=w, bins=bins, bins2d=bins2d, pairs=pairs)
        mr.assert_equal(got, ref, (shape, kind, bins, bins2d))
        assert (got.mass1d.sum(axis=1, dtype=np.uint64) + got.outside.sum(axis=1, dtype=np.uint64) == np.uint64(got.total)).all()


@pytest.mark.parametrize('bins', BINS)
def test_every_bin_count_and_the_vectorised_reference(bins):
    """Every 1-D and 2-D bin count on one input with given ranges that cut draws off; and the reference's vectorised path against
    its own loops."""
    bins2d = BINS2D[BINS.index(bins)]
    x = draws((400, 3), bins)
    w = weights_of('gamma', (400,), bins)
    ranges = [(-1., 1.5), (-2., 3.), (0.1, 0.7)]
    a, b = (mr.reference(x, weights=w, bins=bins, bins2d=bins2d, ranges=ranges, loops=l) for l in (True, False))
    for k in ('mass1d', 'outside', 'mass2d', 'levels1d', 'levels2d'):
        assert np.array_equal(a[k], b[k]), k
    got = marginals(x, weights=w, bins=bins, bins2d=bins2d, ranges=ranges)
    mr.assert_equal(got, a, bins)
    assert got.outside[:, :2].any() and not got.outside[:, 2].any()
    lw = marginals(x, log_weights=np.log(w) + 3., bins=bins, bins2d=bins2d, ranges=ranges)
    mr.assert_equal(lw, mr.reference(x, log_weights=np.log(w) + 3., bins=bins, bins2d=bins2d, ranges=ranges), (bins, 'log'))


def centre_jitter(rng, n, lo, hi, bins):
    """n values at bin centres plus a jitter below a quarter of the width."""
    width = (hi - lo) / bins
    return lo + (rng.integers(0, bins, size=n) + 0.5 + rng.uniform(-0.24, 0.24, size=n)) * width


@pytest.mark.parametrize('bins', (1, 2, 3, 7, 64, 100, 128, 1000))
def test_against_numpy_histograms(bins):
    rng = np.random.default_rng(bins)
    n = 1001
    ranges = [(-3., 3.), (0.1, 0.7), (-1e-3, 5e6), (1e8, 1e8 + 1)]
    x = np.stack([centre_jitter(rng, n, lo, hi, bins) for lo, hi in ranges], axis=1)
    b2 = min(bins, 128)
    x2 = np.stack([centre_jitter(rng, n, lo, hi, b2) for lo, hi in ranges], axis=1)
    wi = rng.integers(0, 9, size=n).astype(np.float64)
    wi[0] = 8.        # the largest weight is a power of two: w' = w / 8 is dyadic and q = w 2^(k - 3)
    unit = 1 << (weight_shift(n) - 3)
    for w, scale in ((None, 1), (wi, unit)):
        got = marginals(x, weights=w, bins=bins, pairs=None, ranges=ranges)
        got2 = marginals(x2, weights=w, bins2d=b2, ranges=ranges)
        assert got.total == (n if w is None else int(wi.sum()) * unit) and not got.outside.any()
        for c, (lo, hi) in enumerate(ranges):
            h = np.histogram(x[:, c], bins=bins, range=(lo, hi), weights=w)[0]
            assert np.array_equal(got.mass1d[c], h.astype(np.uint64) * np.uint64(scale)), (c, bins)
        for p, (i, j) in enumerate(got2.pairs):
            h = np.histogram2d(x2[:, i], x2[:, j], bins=b2, range=(ranges[i], ranges[j]), weights=w)[0]
            assert np.array_equal(got2.mass2d[p], h.astype(np.uint64) * np.uint64(scale)), (i, j, bins)


def test_properties():
    rng = np.random.default_rng(5)
    n, d = 3000, 4
    x = draws((n, d), 5)
    w = rng.gamma(0.3, size=n)
    k = weight_shift(n)
    assert [weight_shift(v) for v in (1, 2, 3, 1000, 2**31 - 1)] == [62, 61, 60, 52, 31] == [mr.shift(v) for v in (1, 2, 3, 1000, 2**31 - 1)]
    for v in (1, 1000, 6 * 10**6, 2**31 - 1):
        assert v << weight_shift(v) <= 1 << 62
    m = marginals(x, weights=w, probs=(0.25, 0.5, 0.68, 0.95, 1.))
    # conservation, the lower bound of the total (the largest weight is 2^k exactly) and the truncation bound
    assert (m.mass1d.sum(axis=1, dtype=np.uint64) + m.outside.sum(axis=1, dtype=np.uint64) == np.uint64(m.total)).all()
    assert 1 << k <= m.total <= 1 << 62
    exact = sum(Fraction(float(v)) / Fraction(float(w.max())) for v in w)     # sum w' without rounding of the sum
    wp = [Fraction(float(v / w.max())) for v in w]                          # the rounded quotients that are quantised
    lost = sum(wp) - Fraction(m.total, 1 << k)
    assert 0 <= lost < Fraction(n, 1 << k)
    assert abs(float(exact - sum(wp))) < n * 2.**-52
    # bins add: two row blocks with the ranges, the maximum and the draw count of the whole
    from bayesfast_amd.utils.marginals import _HostPasses, marginals_sharded, _check_options
    opts = _check_options(d, 64, 64, m.ranges, None, 'all', (0.68,))
    parts = []
    for sl in (slice(0, 1100), slice(1100, n)):
        ps = _HostPasses(x[sl], w[sl], 'lin')
        ps.quantise(w.max(), k)
        parts.append(ps.hist(m.ranges[:, 0], m.ranges[:, 1], 64, 64, opts[4]).numpy().view(np.uint64))
    whole = _HostPasses(x, w, 'lin')
    whole.quantise(w.max(), k)
    assert np.array_equal(parts[0] + parts[1], whole.hist(m.ranges[:, 0], m.ranges[:, 1], 64, 64, opts[4]).numpy().view(np.uint64))
    assert np.array_equal((parts[0] + parts[1])[:d * 64].reshape(d, 64), m.mass1d)
    # levels: not increasing in p, invariant under a permutation of the bins, p = 1 gives the smallest bin that holds mass
    assert (np.diff(m.levels1d.astype(np.float64), axis=0) <= 0).all() and (np.diff(m.levels2d.astype(np.float64), axis=0) <= 0).all()
    from bayesfast_amd.utils.marginals import _levels_host
    h = m.mass2d.reshape(len(m.pairs), -1)
    perm = rng.permutation(h.shape[1])
    assert np.array_equal(_levels_host(h, m.probs)[0], _levels_host(h[:, perm], m.probs)[0])
    assert np.array_equal(_levels_host(h, m.probs)[0], m.levels2d)
    assert m.levels1d[-1, 0] == m.mass1d[0][m.mass1d[0] > 0].min()
    # ties: the sorted and the threshold formulation agree
    tied = np.array([[5, 5, 5, 3, 3, 1, 0, 0, 7, 7]], dtype=np.uint64)
    for p in (0.25, 0.3, 0.5, 0.68, 0.95, 1.):
        assert _levels_host(tied, [p])[0][0, 0] == mr.level([int(v) for v in tied[0]], p)
    assert [int(_levels_host(tied, [p])[0][0, 0]) for p in (0.25, 0.39, 0.8, 0.97, 1.)] == [7, 5, 5, 3, 1]
    assert _levels_host(np.zeros((1, 9), dtype=np.uint64), [0.5])[0][0, 0] == 0
    # the order of the draws does not matter
    order = rng.permutation(n)
    m2 = marginals(x[order], weights=w[order], probs=(0.25, 0.5, 0.68, 0.95, 1.))
    assert np.array_equal(m.mass2d, m2.mass2d) and np.array_equal(m.mass1d, m2.mass1d) and m.total == m2.total
    assert np.array_equal(m.edges, m2.edges)


def test_special_values():
    rng = np.random.default_rng(8)
    n, d = 300, 8
    x = draws((n, d), 8)
    w = rng.gamma(0.5, size=n)
    w[[5, 6, 7]] = 0.
    lo, hi = -2., 2.5
    x[:, 0] = np.clip(x[:, 0], -1., 1.)
    x[0, 0], x[1, 0], x[2, 0], x[3, 0] = lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    x[10, 1], x[11, 1], x[12, 1] = np.nan, np.inf, -np.inf       # non-finite draws of non-zero weight
    x[5, 2], x[6, 2], x[7, 2] = np.nan, np.inf, -np.inf          # non-finite (and extreme) draws of zero weight: not part of the sample
    x[5, 3] = 1e300
    x[:, 4] = 0.1                                                # a constant column
    x[7, 4] = -1.
    x[:, 5] = np.nan                                             # no finite value
    x[3, 5] = np.inf
    x[:, 6] = -0.
    ranges = np.array([(lo, hi)] * d)
    ref = mr.reference(x, weights=w, ranges=ranges, bins=7, bins2d=5, loops=True)
    got = marginals(x, weights=w, ranges=ranges, bins=7, bins2d=5)
    mr.assert_equal(got, ref, 'given')
    q = ref['q']
    assert got.mass1d[0, 0] >= q[0] and got.mass1d[0, -1] >= q[1] and got.outside[0].tolist() == [q[2], q[3], 0]
    assert got.outside[1, 2] == q[10] + q[11] + q[12] and got.outside[2, 2] == 0
    assert got.outside[5, 2] == got.total and not got.mass1d[5].any()
    ref = mr.reference(x, weights=w, bins=7, bins2d=5, loops=True)
    got = marginals(x, weights=w, bins=7, bins2d=5)
    mr.assert_equal(got, ref, 'default')
    assert not got.outside[:, :2].any()
    assert got.ranges[4].tolist() == [-0.4, 0.6] and got.ranges[6].tolist() == [-0.5, 0.5] and np.isnan(got.ranges[5]).all()
    assert np.isnan(got.edges[5]).all() and not got.mass1d[5].any() and got.levels1d[0, 5] == 0
    assert got.ranges[3, 1] < 1e300 and np.isfinite(got.ranges[2]).all()
    assert got.mass1d[4, 3] == got.total         # the constant sits in the middle bin of 7
    # -inf log weights are zero weights; a negative, NaN or +inf weight, or none above zero, makes every float output NaN
    lw = np.log(np.where(w > 0, w, 1.))
    lw[w == 0] = -np.inf
    a, b = marginals(x, log_weights=lw, bins=7, bins2d=5), mr.reference(x, log_weights=lw, bins=7, bins2d=5, loops=True)
    mr.assert_equal(a, b, '-inf')
    assert a.total == got.total or abs(a.total - got.total) <= 2 * n     # (exp(log w) is w up to rounding)
    for bad in (dict(weights=-w), dict(weights=np.where(np.arange(n) == 9, np.nan, w)), dict(weights=np.where(np.arange(n) == 9, np.inf, w)),
                dict(weights=np.zeros(n)), dict(log_weights=np.full(n, -np.inf)), dict(log_weights=np.where(np.arange(n) == 9, np.inf, lw)),
                dict(log_weights=np.where(np.arange(n) == 9, np.nan, lw))):
        r = marginals(x, bins=7, bins2d=5, **bad)
        mr.assert_equal(r, mr.reference(x, bins=7, bins2d=5, levels=False, **bad), list(bad))
        assert r.total == 0 and np.isnan(r.edges).all() and np.isnan(r.density1d(0)).all() and np.isnan(r.density2d(0, 1)).all()
        assert np.isnan(r.level_density1d(0)).all() and np.isnan(r.level_density2d(0, 1)).all() and np.isnan(r.ranges).all()


def test_value_errors():
    x = draws((50, 3), 1)
    w = np.ones(50)
    with pytest.raises(ValueError):
        marginals(x, log_weights=w, weights=w)
    assert marginals(x).total == 50        # neither is allowed
    for bad in (dict(weights=w[:49]), dict(weights=np.ones((50, 1, 1))), dict(bins=0), dict(bins=1025), dict(bins2d=0), dict(bins2d=129),
                dict(ranges=[(0, 1)] * 2), dict(ranges=[(0, 1), (1, 1), (0, 1)]), dict(ranges=[(0, 1), (2, 1), (0, 1)]),
                dict(ranges=[(0, 1), (0, np.inf), (0, 1)]), dict(ranges=[(0, 1), (np.nan, 1), (0, 1)]), dict(probs=(0., 0.5)),
                dict(probs=(0.5, 1.01)), dict(probs=()), dict(params=[0, 3]), dict(pairs=[(0, 3)]), dict(pairs='some')):
        with pytest.raises(ValueError):
            marginals(x, **bad)
    with pytest.raises(ValueError):
        marginals(x[0])
    with pytest.raises(ValueError):
        marginals(x[:0])
    with pytest.raises(ValueError):
        marginals(np.zeros((2, 70000)), bins2d=128)      # more than 2^31 - 1 bins in all
    # params select and order columns; pairs are positions in params
    m = marginals(x, params=[2, 0], pairs=[(0, 1)], bins=8, bins2d=4)
    full = marginals(x, pairs=[(2, 0)], bins=8, bins2d=4)
    assert np.array_equal(m.mass1d, full.mass1d[[2, 0]]) and np.array_equal(m.mass2d, full.mass2d) and m.params.tolist() == [2, 0]
    import torch
    t = marginals(torch.as_tensor(x), weights=torch.as_tensor(w), bins=8, bins2d=4)      # a CPU tensor takes the host port
    assert np.array_equal(t.mass2d, marginals(x, weights=w, bins=8, bins2d=4).mass2d)


def test_the_marginals_object():
    rng = np.random.default_rng(3)
    n = 20000
    x = np.stack([np.where(rng.random(n) < 0.5, -3., 3.) + 0.5 * rng.standard_normal(n), rng.standard_normal(n)], axis=1)
    w = rng.gamma(2., size=n)
    ranges = [(-4.5, 4.5), (-1., 1.)]
    m = marginals(x, weights=w, ranges=ranges, bins=40, bins2d=20)
    assert isinstance(m, Marginals) and repr(m).startswith('Marginals(n_param=2, bins=40, n_pair=1, bins2d=20, total=')
    inside = (m.total - m.outside.sum(axis=1).astype(object)) / m.total
    for i in range(2):
        width = (ranges[i][1] - ranges[i][0]) / 40
        np.testing.assert_allclose(m.density1d(i).sum() * width, float(inside[i]), rtol=1e-12)
    area = (9. / 20) * (2. / 20)
    np.testing.assert_allclose(m.density2d(0, 1).sum() * area, int(m.mass2d.sum()) / m.total, rtol=1e-12)
    # (follow-on float arithmetic: a few roundings)
    np.testing.assert_allclose(m.level_density2d(0, 1) * (m.total * area), m.levels2d[:, 0].astype(np.float64), rtol=1e-14)
    np.testing.assert_allclose(m.level_density1d(0) * (m.total * 9. / 40), m.levels1d[:, 0].astype(np.float64), rtol=1e-14)
    assert (m.density1d(0) >= m.level_density1d(0)[0]).sum() == (m.mass1d[0] >= m.levels1d[0, 0]).sum()
    runs = m.interval(0, 0.68)
    assert len(runs) == 2 and runs[0][1] < 0 < runs[1][0] and -4.5 <= runs[0][0] and runs[1][1] <= 4.5
    coarse = marginals(x, weights=w, ranges=[(-4.5, 4.5), (-4., 4.)], bins=8, pairs=None)      # a Gaussian in 8 bins: one run
    assert coarse.interval(1, 0.68) == [[-1., 1.]] and len(coarse.interval(0, 0.68)) == 2
    covered = sum(int(m.mass1d[0][(m.edges[0, :-1] >= a - 1e-9) & (m.edges[0, 1:] <= b + 1e-9)].sum()) for a, b in runs)
    assert covered >= 0.68 * int(m.mass1d[0].sum())
    with pytest.raises(ValueError):
        m.interval(0, 0.5)
    with pytest.raises(KeyError):
        m.density2d(1, 0)
