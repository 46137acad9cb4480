"""The device route of ``bayesfast_amd.utils.marginals`` (csrc/bfhip_marg.hip) against the Python-integer reference of
helpers/marginals_reference.py and against the host port, every integer with ==.

Sizes.  The column passes walk 16 rows per workgroup and step (17 is the first n with two steps); the elementwise kernels and the
levels take 256 elements per workgroup (255 | 256 | 257); a row tile of the pair kernel is 16384 / ld rows, ld the padded number
of parameters: 1024 rows at d <= 16, 512 at d <= 32, 256 at d <= 64 (first n past them: 1025, 513, 257); a row chunk of the pair
kernel is 8 bins2d^2 rows rounded up to tiles (32768 at 64 bins: 32769 is the first n with two chunks; 100003 has four) until
there are 1024 chunks, after which the chunks grow (1048577 at d <= 16 and few bins); the 1-D histogram takes 4096 rows per
workgroup (4097) up to 512 workgroups (2097153: they stride); the extent pass has at most 1024 workgroups of 16 rows (16385) and the
quantisation 1024 of 256 (262145).  d = 17 and 33 give pairs across batches of 16 parameters.

``weights=`` results equal the host port bit for bit.  With ``log_weights=`` the device's exp and NumPy's may differ in the last
place: each bin is held to |q_dev - q_ref| <= 2^-50 q_ref + (rows in that bin): two 1-ulp functions plus one truncation per row."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import marginals_reference as mr  # noqa: E402

FIELDS = ('mass1d', 'mass2d', 'outside', 'levels1d', 'levels2d', 'edges', 'edges2d', 'ranges')
# n: (d, bins, bins2d, weights)
GRID = {1: (1, 1, 1, None), 2: (2, 2, 2, 'gamma'), 17: (3, 3, 3, 'zeros'), 63: (16, 64, 2, 'gamma'), 64: (17, 100, 3, 'dominant'),
        65: (33, 1024, 1, None), 255: (3, 64, 64, 'gamma'), 256: (2, 100, 100, 'zeros'), 257: (33, 3, 3, 'gamma'),
        513: (17, 2, 128, None), 1025: (2, 1, 128, 'gamma'), 2047: (3, 1024, 64, 'dominant'), 2048: (16, 7, 3, None),
        2049: (17, 64, 3, 'gamma'), 4097: (1, 1024, 1, 'gamma'), 16385: (3, 64, 100, 'zeros'), 32769: (3, 3, 64, 'gamma'),
        100003: (3, 64, 64, 'gamma')}


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _i64(n, fill=0):
    import torch
    return torch.full((n,), fill, dtype=torch.int64, device='cuda')


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def draws(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * (1. + np.arange(d)) + np.arange(d)


def weights_of(kind, n, seed):
    rng = np.random.default_rng(seed + 1)
    if kind is None:
        return None
    w = rng.gamma(0.3, size=n)
    if kind == 'zeros':
        w[rng.random(n) < 0.9] = 0.
        w[0] = 1.
    elif kind == 'dominant':
        w[n // 2] = 50. * w.sum() + 1.
    return w


def pairs_of(d, bins2d):
    if d <= 3 or bins2d <= 3:
        return 'all'
    return [(0, d - 1), (3, 5), (d - 1, 1)]


@functools.lru_cache(maxsize=None)
def grid_case(n):
    d, bins, bins2d, kind = GRID[n]
    x, w = draws(n, d, n), weights_of(kind, n, n)
    return x, w, mr.reference(x, weights=w, bins=bins, bins2d=bins2d, pairs=pairs_of(d, bins2d))


def same(a, b):
    return a.total == b.total and all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in FIELDS)


@pytest.mark.parametrize('n', sorted(GRID))
def test_device_against_the_reference_and_the_host_port(n):
    from bayesfast_amd.utils import marginals
    d, bins, bins2d, kind = GRID[n]
    x, w, ref = grid_case(n)
    opt = dict(bins=bins, bins2d=bins2d, pairs=pairs_of(d, bins2d))
    got = marginals(_dev(x), weights=None if w is None else _dev(w), **opt)
    mr.assert_equal(got, ref, (n, d, bins, bins2d, kind))
    assert same(got, marginals(x, weights=w, **opt))
    assert (got.mass1d.sum(axis=1, dtype=np.uint64) + got.outside.sum(axis=1, dtype=np.uint64) == np.uint64(got.total)).all()


@pytest.mark.parametrize('n', (262145, 1048577, 2097153))
def test_large_sizes_past_the_grid_limits(n):
    """d = 2, few bins, whole-number weights with the largest 8 (w' dyadic: q = w 2^(k - 3)), against integer ``np.bincount``."""
    from bayesfast_amd.utils import marginals
    from bayesfast_amd.utils.marginals import weight_shift
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 2))
    wi = rng.integers(0, 9, size=n)
    wi[n - 1] = 8
    ranges = [(-1.5, 2.), (-3., 0.5)]
    unit = 1 << (weight_shift(n) - 3)
    xd = _dev(x)
    for w, scale in ((None, 1), (wi, unit)):
        got = marginals(xd, weights=None if w is None else _dev(w.astype(np.float64)), bins=5, bins2d=2, ranges=ranges)
        wt = np.ones(n, dtype=np.int64) if w is None else w
        s1 = [mr.slots(x[:, c], *ranges[c], 5 / (ranges[c][1] - ranges[c][0]), 5) for c in range(2)]
        s2 = [mr.slots(x[:, c], *ranges[c], 2 / (ranges[c][1] - ranges[c][0]), 2) for c in range(2)]
        for c in range(2):
            row = np.bincount(s1[c], weights=wt, minlength=8).astype(np.uint64) * np.uint64(scale)     # (sums below 2^53: exact)
            assert np.array_equal(got.mass1d[c], row[:5]) and np.array_equal(got.outside[c], row[5:]), (n, c)
        ok = (s2[0] < 2) & (s2[1] < 2)
        want = np.bincount(s2[0][ok] * 2 + s2[1][ok], weights=wt[ok], minlength=4).astype(np.uint64) * np.uint64(scale)
        assert np.array_equal(got.mass2d.reshape(-1), want), n
        assert got.total == int(wt.sum()) * scale
    # default ranges: the extent pass beyond its grid
    x[n - 3, 0], x[n - 2, 1] = -77., 99.
    got = marginals(_dev(x), bins=5, pairs=None)
    assert got.ranges.tolist() == [[-77., x[:, 0].max()], [x[:, 1].min(), 99.]]


# ---- through ctypes --------------------------------------------------------------------------------------------------------------------
def _series(x):
    """(n, 16) series buffer of x (n, d <= 16), unused columns zero."""
    buf = np.zeros((x.shape[0], 16))
    buf[:, :x.shape[1]] = x
    return _dev(buf)


def test_add_to_contract_pairs_with_repeats_and_levels_through_ctypes():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context, _ptr
    ctx = get_context()
    lib, h = ctx._lib, ctx.handle
    rng = np.random.default_rng(11)
    n, d, B, B2 = 3001, 5, 9, 6
    x = draws(n, d, 11)
    qn = rng.integers(0, 1 << 40, size=n).astype(np.int64)
    qn[rng.random(n) < 0.2] = 0
    lo, hi = np.full(16, -2.), np.full(16, 3.)
    inv, inv2 = B / (hi - lo), B2 / (hi - lo)
    buf, q = _series(x), _dev(qn)
    c = [_dev(v) for v in (lo, hi, inv, inv2)]
    ql = [int(v) for v in qn]
    m1, out, m2 = mr.histograms(x, ql, lo, hi, B, B2, [(0, 1), (4, 2), (0, 1), (3, 3), (1, 0)])
    pairs = _dev(np.array([(0, 1), (4, 2), (0, 1), (3, 3), (1, 0)], dtype=np.int32))
    # 1-D: one call; two calls on row blocks; a non-zero buffer is added to
    one, o_one = _i64(16 * B), _i64(48)
    _lib.check(lib.bfhip_marg_hist1d(h, n, _ptr(buf), _ptr(q), _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), d, B, _ptr(one), _ptr(o_one)))
    two, o_two = _i64(16 * B, 5), _i64(48, 7)
    cut = 1234
    _lib.check(lib.bfhip_marg_hist1d(h, cut, _ptr(buf), _ptr(q), _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), d, B, _ptr(two), _ptr(o_two)))
    _lib.check(lib.bfhip_marg_hist1d(h, n - cut, _ptr(buf[cut:]), _ptr(q[cut:]), _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), d, B, _ptr(two),
                                     _ptr(o_two)))
    want1 = np.zeros((16, B), dtype=np.uint64)
    want1[:d] = np.array(m1, dtype=np.uint64)
    want_o = np.zeros((16, 3), dtype=np.uint64)
    want_o[:d] = np.array(out, dtype=np.uint64)
    assert np.array_equal(_u64(one).reshape(16, B), want1) and np.array_equal(_u64(o_one).reshape(16, 3), want_o)
    assert np.array_equal(_u64(two).reshape(16, B), want1 + np.uint64(5)) and np.array_equal(_u64(o_two).reshape(16, 3), want_o + np.uint64(7))
    # indices at a column offset of a wider matrix; nothing else is written
    ld = 32
    idx = torch.full((n, ld), 77, dtype=torch.uint8, device='cuda')
    _lib.check(lib.bfhip_marg_index(h, n, _ptr(buf), _ptr(c[0]), _ptr(c[1]), _ptr(c[3]), d, B2, _ptr(idx), ld, 16))
    got = idx.cpu().numpy()
    s2 = np.stack([mr.slots(x[:, k], -2., 3., inv2[0], B2) for k in range(d)], axis=1)
    assert np.array_equal(got[:, 16:16 + d], np.where(s2 < B2, s2, 255).astype(np.uint8))
    assert (got[:, :16] == 77).all() and (got[:, 16 + d:] == 77).all()
    # 2-D: repeats and (i, i); two calls on row blocks equal one; a non-zero buffer is added to
    pairs16 = pairs + 16
    nb2 = 5 * B2 * B2
    one2, two2 = _i64(nb2), _i64(nb2, 3)
    _lib.check(lib.bfhip_marg_hist2d(h, n, _ptr(idx), ld, _ptr(pairs16), 5, _ptr(q), B2, _ptr(one2)))
    cut = 1536      # (a multiple of 16 rows keeps the second block's index rows 16-byte aligned)
    _lib.check(lib.bfhip_marg_hist2d(h, cut, _ptr(idx), ld, _ptr(pairs16), 5, _ptr(q), B2, _ptr(two2)))
    _lib.check(lib.bfhip_marg_hist2d(h, n - cut, _ptr(idx[cut:]), ld, _ptr(pairs16), 5, _ptr(q[cut:]), B2, _ptr(two2)))
    want2 = np.array(m2, dtype=np.uint64).reshape(-1)
    assert np.array_equal(_u64(one2), want2) and np.array_equal(_u64(two2), want2 + np.uint64(3))
    assert np.array_equal(want2[:B2 * B2], want2[2 * B2 * B2:3 * B2 * B2])                       # the repeated pair
    assert np.array_equal(want2[:B2 * B2].reshape(B2, B2).T, want2[4 * B2 * B2:].reshape(B2, B2))   # (1, 0) is (0, 1) transposed
    diag = want2[3 * B2 * B2:4 * B2 * B2].reshape(B2, B2)
    assert diag.sum() == np.diag(diag).sum() > 0
    # a pair with a column outside the matrix adds nothing; without q every row counts once
    stray = _dev(np.array([(0, ld), (-1, 3), (16, 17)], dtype=np.int32))
    cnt = _i64(3 * B2 * B2)
    _lib.check(lib.bfhip_marg_hist2d(h, n, _ptr(idx), ld, _ptr(stray), 3, None, B2, _ptr(cnt)))
    cn = _u64(cnt).reshape(3, -1)
    ok = (s2[:, 0] < B2) & (s2[:, 1] < B2)
    assert not cn[:2].any() and np.array_equal(cn[2], np.bincount(s2[ok, 0] * B2 + s2[ok, 1], minlength=B2 * B2).astype(np.uint64))
    # argument errors before anything is launched
    assert lib.bfhip_marg_hist2d(h, n, _ptr(idx), 48, _ptr(pairs), 5, _ptr(q), B2, _ptr(one2)) == -1
    assert lib.bfhip_marg_hist2d(h, n, _ptr(idx), ld, _ptr(pairs), 5, _ptr(q), 129, _ptr(one2)) == -1
    assert lib.bfhip_marg_hist1d(h, n, _ptr(buf), _ptr(q), _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), d, 1025, _ptr(one), _ptr(o_one)) == -1
    assert lib.bfhip_marg_index(h, n, _ptr(buf), _ptr(c[0]), _ptr(c[1]), _ptr(c[3]), d, B2, _ptr(idx), ld, 28) == -1
    # levels: a hand-written histogram with ties, an all-zero one, one bin, and a long one
    hists = np.zeros((4, 300), dtype=np.int64)
    hists[0, :10] = [5, 5, 5, 3, 3, 1, 0, 0, 7, 7]
    hists[2, 299] = 1 << 61
    hists[3] = rng.integers(0, 1 << 50, size=300)
    hists[3, 100:140] = hists[3, 7]
    probs = np.array([0.25, 0.39, 0.8, 0.97, 1.])
    lv, tot = _i64(4 * 5, -1), _i64(4, -1)
    hists_d, probs_d = _dev(hists), _dev(probs)
    _lib.check(lib.bfhip_marg_levels(h, 4, 300, _ptr(hists_d), 5, _ptr(probs_d), _ptr(lv), _ptr(tot)))
    lv, tot = _u64(lv).reshape(4, 5), _u64(tot)
    assert lv[0].tolist() == [7, 5, 5, 3, 1] and not lv[1].any() and (lv[2] == np.uint64(1 << 61)).all()
    assert tot.tolist() == [int(v) for v in hists.sum(axis=1)]
    assert lv[3].tolist() == [mr.level([int(v) for v in hists[3]], p) for p in probs]
    # quantise: the flag counts what cannot be a weight, and is added to
    wp = np.array([0., 1., 0.5, 2.**-40, -0.25, np.nan, 1.5, np.inf, 0.75])
    qq, flag, wp_d = _i64(9, -1), _i64(1, 10), _dev(wp)
    _lib.check(lib.bfhip_marg_quantise(h, 9, _ptr(wp_d), 40, _ptr(qq), _ptr(flag)))
    assert _u64(qq).tolist() == [0, 1 << 40, 1 << 39, 1, 0, 0, 0, 0, 3 << 38] and int(flag.item()) == 14
    _lib.check(lib.bfhip_marg_quantise(h, 9, None, 62, _ptr(qq), _ptr(flag)))
    assert _u64(qq).tolist() == [1] * 9 and int(flag.item()) == 14
    assert lib.bfhip_marg_quantise(h, 9, None, 63, _ptr(qq), _ptr(flag)) == -1


def test_contention_one_bin_and_the_diagonal():
    """100003 draws in one bin of one pair: a lost update shows as a count below n.  Then all of them on the diagonal."""
    from bayesfast_amd.utils import marginals
    n = 100003
    x = np.full((n, 2), 0.25)
    got = marginals(_dev(x), bins=64, bins2d=64)
    assert got.mass2d[0, 32, 32] == n == got.mass2d.sum() and got.mass1d[:, 32].tolist() == [n, n] and got.total == n
    w = np.full(n, 3.)
    got = marginals(_dev(x), weights=_dev(w), bins=64, bins2d=128)
    assert got.mass2d[0, 64, 64] == got.total == n << (62 - 17) and got.levels2d[:, 0].tolist() == [got.total] * 2
    rng = np.random.default_rng(1)
    x[:, 0] = rng.standard_normal(n)
    x[:, 1] = x[:, 0]
    w = rng.gamma(0.3, size=n)
    got = marginals(_dev(x), weights=_dev(w), bins=64, bins2d=64)
    assert np.array_equal(np.diag(got.mass2d[0]), got.mass1d[0]) and got.mass2d.sum(dtype=np.uint64) == got.total
    assert same(got, marginals(x, weights=w, bins=64, bins2d=64))


def test_float32_views_strides_and_batch_independence():
    import torch
    from bayesfast_amd.utils import marginals
    rng = np.random.default_rng(4)
    x = _dev(rng.standard_normal((12, 500, 20)))
    v = x[:, 137:]
    lw = rng.standard_normal((12, 363))
    w = _dev(np.exp(lw))
    opt = dict(bins=50, bins2d=10, pairs=[(0, 19), (17, 3), (5, 6)])
    assert not v.is_contiguous()
    a = marginals(v, weights=w, **opt)
    assert same(a, marginals(v.contiguous(), weights=w, **opt)) and same(a, marginals(v, weights=w.reshape(-1), **opt))
    assert same(a, marginals(v.cpu().numpy(), weights=np.exp(lw), **opt))
    # float32 is read as float64
    x32 = v.to(torch.float32)
    assert same(marginals(x32, weights=w, **opt), marginals(x32.cpu().numpy().astype(np.float64), weights=np.exp(lw), **opt))
    # input the column kernel cannot read in place: a last axis that is not contiguous, float16
    t = x.permute(0, 2, 1)[:, :, :100]
    assert t.stride(2) != 1
    assert same(marginals(t, weights=w[:, :20], **opt), marginals(t.contiguous(), weights=w[:, :20], **opt))
    h16 = x[:4, :200, :18].to(torch.float16)
    o16 = dict(bins=50, bins2d=10, pairs=[(0, 17), (16, 3)])
    assert same(marginals(h16, **o16), marginals(h16.cpu().numpy().astype(np.float64), **o16))
    # a parameter's histograms do not depend on the batch or the column it lands in; params selects columns
    y = rng.standard_normal((3000, 40))
    wy = rng.gamma(0.5, size=3000)
    perm = rng.permutation(40)
    pr = [(0, 39), (3, 20), (17, 16)]
    inv = np.argsort(perm)
    s0 = marginals(_dev(y), weights=_dev(wy), bins=33, bins2d=7, pairs=pr)
    s1 = marginals(_dev(y[:, perm]), weights=_dev(wy), bins=33, bins2d=7, pairs=[(inv[i], inv[j]) for i, j in pr])
    assert np.array_equal(s0.mass1d[perm], s1.mass1d) and np.array_equal(s0.mass2d, s1.mass2d) and np.array_equal(s0.edges[perm], s1.edges)
    assert np.array_equal(s0.levels1d[:, perm], s1.levels1d) and np.array_equal(s0.levels2d, s1.levels2d)
    s2 = marginals(_dev(y), weights=_dev(wy), bins=33, bins2d=7, params=[39, 0, 20, 3], pairs=[(1, 0), (3, 2)])
    assert np.array_equal(s2.mass1d, s0.mass1d[[39, 0, 20, 3]]) and np.array_equal(s2.mass2d, s0.mass2d[:2])
    # twice the same bits
    assert same(s0, marginals(_dev(y), weights=_dev(wy), bins=33, bins2d=7, pairs=pr))


def test_special_values():
    from bayesfast_amd.utils import marginals
    rng = np.random.default_rng(8)
    n, d = 300, 19
    x = draws(n, d, 8)
    w = rng.gamma(0.5, size=n)
    w[[5, 6, 7]] = 0.
    lo, hi = -2., 2.5
    x[:, 0] = np.clip(x[:, 0], -1., 1.)
    x[0, 0], x[1, 0], x[2, 0], x[3, 0] = lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    x[10, 1], x[11, 1], x[12, 1] = np.nan, np.inf, -np.inf       # non-finite draws of non-zero weight
    x[5, 2], x[6, 2], x[7, 2] = np.nan, np.inf, -np.inf          # non-finite (and extreme) draws of zero weight
    x[5, 17] = 1e300
    x[:, 4] = 0.1                                                # a constant column
    x[7, 4] = -1.
    x[:, 18] = np.nan                                            # no finite value
    x[3, 18] = np.inf
    x[:, 6] = -0.
    ranges = np.array([(lo, hi)] * d)
    pairs = [(0, 1), (2, 17), (4, 18), (6, 0), (1, 18)]
    for rg in (ranges, None):
        ref = mr.reference(x, weights=w, ranges=rg, bins=7, bins2d=5, pairs=pairs)
        got = marginals(_dev(x), weights=_dev(w), ranges=rg, bins=7, bins2d=5, pairs=pairs)
        mr.assert_equal(got, ref, rg is None)
        assert same(got, marginals(x, weights=w, ranges=rg, bins=7, bins2d=5, pairs=pairs))
    q = ref['q']
    assert got.ranges[4].tolist() == [-0.4, 0.6] and got.ranges[6].tolist() == [-0.5, 0.5] and np.isnan(got.ranges[18]).all()
    assert got.outside[18, 2] == got.total and not got.mass1d[18].any() and got.outside[1, 2] == q[10] + q[11] + q[12]
    assert got.ranges[17, 1] < 1e300 and not got.outside[2].any()
    lw = np.log(np.where(w > 0, w, 1.))
    lw[w == 0] = -np.inf
    a = marginals(_dev(x), log_weights=_dev(lw), bins=7, bins2d=5, pairs=pairs)
    assert np.array_equal(a.ranges, got.ranges, equal_nan=True) and not a.outside[2].any() and a.total > 0
    for bad in (dict(weights=-w), dict(weights=np.where(np.arange(n) == 9, np.nan, w)), dict(weights=np.where(np.arange(n) == 9, np.inf, w)),
                dict(weights=np.zeros(n)), dict(log_weights=np.full(n, -np.inf)), dict(log_weights=np.where(np.arange(n) == 9, np.inf, lw)),
                dict(log_weights=np.where(np.arange(n) == 9, np.nan, lw))):
        r = marginals(_dev(x), bins=7, bins2d=5, pairs=pairs, **{k: _dev(v) for k, v in bad.items()})
        mr.assert_equal(r, dict(bad=True), list(bad))
        assert np.isnan(r.density1d(0)).all() and np.isnan(r.density2d(0, 1)).all() and np.isnan(r.ranges).all()
    with pytest.raises(ValueError):
        marginals(_dev(x), weights=_dev(w[:299]))
    with pytest.raises(ValueError):
        marginals(_dev(x), weights=_dev(w), log_weights=_dev(lw))
    with pytest.raises(ValueError):
        marginals(_dev(x), bins2d=129)


def test_log_weights_within_two_ulps_and_a_truncation_per_row():
    from bayesfast_amd.utils import marginals
    rng = np.random.default_rng(12)
    n, d = 20011, 3
    x = draws(n, d, 12)
    lw = 2. * rng.standard_normal(n)
    lw[:7] = -np.inf
    opt = dict(bins=64, bins2d=16)
    dev, ref = marginals(_dev(x), log_weights=_dev(lw), **opt), marginals(x, log_weights=lw, **opt)
    assert np.array_equal(dev.ranges, ref.ranges)
    rows = marginals(x[7:], ranges=ref.ranges, **opt)      # the rows of every bin, among those that have a weight
    worst = 0.
    for k in ('mass1d', 'mass2d'):
        a, b, r = (getattr(m, k).astype(object) for m in (dev, ref, rows))
        diff, bound = abs(a - b), b * 2.**-50 + r
        ratio = float(np.max(diff / np.maximum(bound, 1)))
        print(k, 'largest |q_dev - q_ref|', diff.max(), 'of', b.max(), 'largest ratio to the bound', ratio)
        worst = max(worst, ratio)
        assert (diff <= bound).all(), k
    print('largest ratio', worst)
    assert abs(dev.total - ref.total) <= ref.total * 2.**-50 + n


def test_trace_marginals_after_sample():
    """16 chains x 40 draws x 4-d: the device route on the chains where sample() left them equals the host port on
    tt.get(flatten=False)."""
    import bayesfast_amd as bfa
    from bayesfast_amd.utils import marginals
    d = 4
    rng = np.random.default_rng(2)
    su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
    den = bfa.SurrogateDensity(su, input_scales=np.stack([np.full(d, -8.), np.full(d, 9.)], 1))
    xf = rng.standard_normal((4 * su.n_param, d)) * 1.5
    den.fit(xf, -0.5 * (xf**2).sum(axis=1))
    tt = bfa.sample(den, bfa.NTrace(n_chain=16, n_iter=60, n_warmup=20, x_0=rng.standard_normal((16, d)), random_generator=7),
                    verbose=False)
    assert tt.device('samples').is_cuda
    for kw in (dict(), dict(original_space=False), dict(since_iter=31), dict(include_warmup=True)):
        x = tt.get(flatten=False, **kw)
        assert x.shape[0] == 16 and x.shape[2] == d
        for opt in (dict(), dict(bins=10, bins2d=5, pairs=[(3, 0)], probs=(0.5,)), dict(ranges=[(-1., 1.)] * d, params=None)):
            assert same(tt.marginals(**kw, **opt), marginals(x, **opt)), (kw, opt)
        w = np.exp(0.1 * (x**2).sum(axis=2))
        got = tt.marginals(np.log(w), bins=12, bins2d=6, **kw)
        ref = marginals(x, log_weights=np.log(w), bins=12, bins2d=6)
        rows = marginals(x, bins=12, bins2d=6, ranges=ref.ranges)
        for k in ('mass1d', 'mass2d'):
            a, b, r = (getattr(m, k).astype(object) for m in (got, ref, rows))
            assert (abs(a - b) <= b * 2.**-50 + r).all(), (kw, k)
    with pytest.raises(ValueError):
        tt.marginals(since_iter=59)
    with pytest.raises(TypeError):
        tt.marginals(return_type='logp')
