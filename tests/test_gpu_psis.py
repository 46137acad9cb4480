"""The device route of ``bayesfast_amd.utils.psis`` (csrc/bfhip_psis.hip) against the loop-written reference of
helpers/psis_reference.py: Pareto-smoothed importance weights over the sizes at which the tail rule and the reductions change
shape, their properties, the weighted table over the shape grid with gamma, mostly-zero and dominated weights, float32 and strided
input, special columns and batch independence, the running sum of the permuted weights through ctypes at its level boundaries, and
``TraceTuple.weighted_summary`` after ``sample()``.

Sizes of ``psis``: 24 | 25 is the smallest fitted tail, 224 .. 226 the crossing of the two tail-size rules; a workgroup of the
two-level reductions spans 256 values (257 is the first size with two) and the 1024 workgroups of the first level span 262144
before they stride (262145).  The running sum works in tiles of 2048 sorted positions, and the one workgroup that scans the tile
sums takes 256 of them at a time: boundaries at 2048 | 2049 and 524288 | 524289.

Tolerances: 1e-9 relative throughout, the project's figure for the device against a loop reference.  For khat, sigma and
log_mean_weight the profile likelihoods multiply rounding by the tail size M; what rounding alone does was measured on these very
inputs (``gaussian_pair(S, scale, seed=S)``, scale 0.8 and 1.2, every S below from 25 on) by running the reference once in float64
and once in numpy.longdouble on the CPU.  The largest relative differences: khat 1.4e-11 and sigma 1.5e-11 (S = 262145, scale 1.2),
log_mean_weight 1.0e-10 (S = 100003, scale 0.8, where the value itself is -6.3e-5: 7e-15 absolute), ess 3.3e-14, log_weights 4.5e-15
(docs/EXPERIMENTS.md has the table).  Ten times those is 1.4e-10, 1.5e-10 and 1.0e-9, so the tolerance stays at the 1e-9 it started
from.  One input has a figure of its own: the ratios with ties (S = 4097, rounded to 0.05) have log_mean_weight = -7.8e-7, the two
runs of the reference differ by 3.54e-8 of it (2.8e-14 absolute: two units in the last place of the 8.5 that cancels), and the device
was seen 3.63e-8 from the float64 run; that figure of that input is held to ten times the reference's own difference, 3.54e-7.
Each test prints every figure before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import psis_reference as pr  # noqa: E402

RTOL = 1e-9
SIZES = (1, 24, 25, 224, 225, 226, 255, 256, 257, 1000, 4097, 100003, 262145)
TABLE_SHAPES = [(1, 3), (2, 2), (255, 1), (256, 17), (257, 16), (7, 333, 5), (65537, 2)]


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


@functools.lru_cache(maxsize=None)
def psis_case(s, scale):
    logp, logq, _ = pr.gaussian_pair(s, scale, seed=s)
    return logp, logq, pr.psis_reference(logp - logq)


def assert_psis(got, ref, label='', rtol_lmw=RTOL):
    lw = got.log_weights.cpu().numpy().reshape(-1)
    b = np.asarray(ref['log_weights'], dtype=np.float64)
    with np.errstate(all='ignore'):
        for k in ('khat', 'sigma', 'log_mean_weight', 'ess'):
            print(label, k, getattr(got, k), float(ref[k]), abs(np.float64(getattr(got, k)) / np.float64(ref[k]) - 1))
        print(label, 'log_weights', np.nanmax(np.abs(lw / b - 1)) if np.isfinite(b).any() else np.nan)
    assert got.n_tail == ref['n_tail']
    for k in ('khat', 'sigma', 'log_mean_weight', 'ess'):
        a, r = getattr(got, k), float(ref[k])
        assert np.isnan(a) == np.isnan(r), (k, a, r)
        if not np.isnan(r):
            np.testing.assert_allclose(a, r, rtol=rtol_lmw if k == 'log_mean_weight' else RTOL, atol=0, err_msg=k)
    assert np.array_equal(np.isnan(lw), np.isnan(b))
    np.testing.assert_allclose(lw, b, rtol=RTOL, atol=0)


def assert_table(got, ref, label=''):
    for k in got.names:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        with np.errstate(all='ignore'):
            print(label, k, np.nanmax(np.abs(a / b - 1)) if np.isfinite(b).any() else np.nan)
    for k in got.names:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, k
        assert np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=0, err_msg=k)


def same_bytes(a, b):
    return a.names == b.names and all(a[k].tobytes() == b[k].tobytes() for k in a.names)


def table_case(shape, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * (1. + np.arange(shape[-1])) + np.arange(shape[-1])
    w = rng.gamma(0.7, size=shape[:-1])
    if kind == 'zeros':
        w[rng.random(shape[:-1]) < 0.9] = 0.
        w.reshape(-1)[0] = 1.
    elif kind == 'dominant':
        w.reshape(-1)[w.size // 2] = 50. * w.sum()
    return x, w


@pytest.mark.parametrize('s', SIZES)
def test_psis_against_the_reference(s):
    from bayesfast_amd.utils import psis
    for scale in (0.8, 1.2):
        logp, logq, ref = psis_case(s, scale)
        got = psis(_dev(logp), _dev(logq))
        assert got.log_weights.is_cuda and got.log_weights.shape == (s,)
        assert_psis(got, ref, (s, scale))
        assert (got.khat == np.inf) == (s < 25)


def test_psis_properties():
    import torch
    from bayesfast_amd.utils import psis
    from bayesfast_amd.evidence import psis as psis_ev
    assert psis_ev is psis
    s = 4097
    logp, logq, ref = psis_case(s, 0.8)
    got = psis(_dev(logp), _dev(logq))
    lw_in, lw = logp - logq, got.log_weights.cpu().numpy()
    # the smoothed values land where their ratios were: the order of the input survives, and below the tail only a constant is taken off
    order = np.argsort(lw_in, kind='stable')
    assert np.all(np.diff(lw[order]) >= 0)
    body = order[:s - got.n_tail]
    np.testing.assert_allclose(lw[body] - lw[body[0]], lw_in[body] - lw_in[body[0]], rtol=1e-9, atol=1e-12)
    tail = order[s - got.n_tail:]
    moved = np.abs((lw[tail] - lw[body[0]]) - (lw_in[tail] - lw_in[body[0]]))
    assert np.sum(moved > 1e-3) > got.n_tail // 2   # the tail was smoothed (its largest value may sit at the cap, unmoved)
    assert abs(torch.logsumexp(got.log_weights, 0).item()) < 1e-12
    # the ratio alone, any shape; bitwise the same as the pair (IEEE subtraction) and over two calls
    one = psis(_dev(lw_in).reshape(17, 241))
    assert one.log_weights.shape == (17, 241)
    assert one.log_weights.reshape(-1).cpu().numpy().tobytes() == lw.tobytes()
    again = psis(_dev(logp), _dev(logq))
    assert again.log_weights.cpu().numpy().tobytes() == lw.tobytes()
    assert all(getattr(again, k) == getattr(got, k) == getattr(one, k) for k in ('khat', 'sigma', 'n_tail', 'log_mean_weight', 'ess'))
    # heavy ties in the tail: ratios rounded to 0.05
    tied = np.round(lw_in / 0.05) * 0.05
    ref_t = pr.psis_reference(tied)
    assert np.isfinite(ref_t['khat']) and len(np.unique(np.sort(tied)[-ref_t['n_tail']:])) < ref_t['n_tail'] // 3
    # (log_mean_weight of this input is -7.8e-7, what is left when the maximum 8.5 cancels: the float64 reference itself is 3.54e-8 relative,
    # 2.8e-14 absolute, from its numpy.longdouble run, so this one figure gets ten times that; every other figure keeps 1e-9)
    assert_psis(psis(_dev(tied)), ref_t, 'ties', rtol_lmw=3.54e-7)
    # float32 ratios are read as float64
    assert_psis(psis(_dev(lw_in.astype(np.float32))), pr.psis_reference(lw_in.astype(np.float32)), 'f32')


def test_psis_degenerate_input():
    from bayesfast_amd.utils import psis
    rng = np.random.default_rng(0)
    cases = [np.full(100, -3.), rng.standard_normal(400), rng.standard_normal(400), rng.standard_normal(400), np.zeros(1)]
    cases[1][17] = -np.inf
    cases[2][3] = np.nan
    cases[3][399] = np.inf
    for i, lw in enumerate(cases):
        ref = pr.psis_reference(lw)
        got = psis(_dev(lw))
        assert_psis(got, ref, i)
    assert psis(_dev(cases[0])).khat == np.inf
    r = psis(_dev(cases[1]))
    assert r.log_weights[17].item() == -np.inf and np.isfinite(r.khat)
    for lw in cases[2:4]:
        r = psis(_dev(lw))
        assert bool(r.log_weights.isnan().all()) and np.isnan([r.khat, r.sigma, r.log_mean_weight, r.ess]).all()
    with pytest.raises(ValueError):
        psis(_dev(np.zeros(5)), _dev(np.zeros(4)))


@pytest.mark.parametrize('shape', TABLE_SHAPES)
def test_table_against_the_reference(shape):
    from bayesfast_amd.utils import weighted_summary
    kinds = ('gamma',) if shape[0] > 1000 else ('gamma', 'zeros', 'dominant')   # (the loop reference is slow at the largest size)
    for kind in kinds:
        x, w = table_case(shape, kind, seed=sum(shape))
        ref = pr.table_reference(x, weights=w)
        assert (ref['margin'] >= 1e-9).all()
        got = weighted_summary(_dev(x), weights=_dev(w))
        assert got.names == ('mean', 'sd', 'q5', 'q50', 'q95', 'mcse_mean', 'ess', 'ess_kish')
        assert_table(got, ref, (shape, kind))
        if kind == 'gamma':
            assert_table(weighted_summary(_dev(x), log_weights=_dev(np.log(w).reshape(-1) - 2.)), ref, (shape, 'log'))
            x32 = x.astype(np.float32)
            ref32 = pr.table_reference(x32, weights=w)
            assert (ref32['margin'] >= 1e-9).all()
            assert_table(weighted_summary(_dev(x32), weights=w), ref32, (shape, 'f32'))


def test_table_special_columns():
    from bayesfast_amd.utils import weighted_summary
    x, w = table_case((300, 19), 'gamma', seed=3)
    w[[5, 6, 7]] = 0.
    x[:, 1] = 0.1                # constants whose weighted sum is not the constant
    x[:, 17] = -0.
    x[10, 2] = np.nan            # non-finite draws of non-zero weight
    x[11, 3] = np.inf
    x[299, 18] = -np.inf
    x[5, 4] = np.nan             # non-finite draws of zero weight: not part of the sample
    x[6, 4] = -np.inf
    x[7, 16] = np.inf
    x[:, 5] = 2.5
    x[7, 5] = -1.                # constant among the rows that count
    ref = pr.table_reference(x, weights=w, probs=(0.025, 0.5))
    assert (ref['margin'][[0, 4, 6, 16]] >= 1e-9).all()
    got = weighted_summary(_dev(x), weights=_dev(w), probs=(0.025, 0.5))
    assert got.names[2:4] == ('q2.5', 'q50')
    assert_table(got, ref)
    assert all(np.isnan(got[k][[2, 3, 18]]).all() for k in got.names)
    assert all(np.isfinite(got[k][[0, 4, 6, 16]]).all() for k in got.names)
    for c, v in ((1, 0.1), (5, 2.5), (17, 0.)):
        assert got['mean'][c] == v and got['q2.5'][c] == v and got['sd'][c] == 0. and np.isnan(got['mcse_mean'][c])
    w1 = np.zeros(300)
    w1[20] = 4.                  # one weight equal to 1 after normalisation
    one = weighted_summary(_dev(x), weights=_dev(w1))
    assert one['mean'][0] == x[20, 0] and one['q95'][6] == x[20, 6] and np.isnan(one['sd'][0]) and np.isnan(one['mcse_mean'][0])
    assert_table(one, pr.table_reference(x, weights=w1))
    neg = weighted_summary(_dev(x), weights=_dev(-w))
    assert all(np.isnan(neg[k]).all() for k in neg.names)
    with pytest.raises(ValueError):
        weighted_summary(_dev(x), weights=_dev(w[:299]))
    with pytest.raises(ValueError):
        weighted_summary(_dev(x))


def test_table_strided_view_repeatability_and_batch_independence():
    import torch
    from bayesfast_amd.utils import weighted_summary
    rng = np.random.default_rng(4)
    x = _dev(rng.standard_normal((12, 500, 20)))
    v = x[:, 137:]
    lw = _dev(rng.standard_normal((12, 363)))
    assert not v.is_contiguous()
    a, b = weighted_summary(v, log_weights=lw), weighted_summary(v.contiguous(), log_weights=lw)
    assert same_bytes(a, b) and same_bytes(a, weighted_summary(v, log_weights=lw.reshape(-1)))
    ref = pr.table_reference(v.cpu().numpy(), log_weights=lw.cpu().numpy())
    assert (ref['margin'] >= 1e-9).all()
    assert_table(a, ref)
    # input the column kernel cannot read in place is converted batch by batch: a last axis that is not contiguous, float16
    t = x.permute(0, 2, 1)[:, :, :363]
    assert t.stride(2) != 1
    assert same_bytes(weighted_summary(t, log_weights=lw[:, :20].repeat(1, 1)), weighted_summary(t.contiguous(), log_weights=lw[:, :20]))
    h16 = x[:4, :200, :18].to(torch.float16)
    ref16 = pr.table_reference(h16.cpu().numpy(), log_weights=lw[:4, :200].cpu().numpy())
    assert (ref16['margin'] >= 1e-9).all()
    assert_table(weighted_summary(h16, log_weights=lw[:4, :200]), ref16)
    # a parameter's figures do not depend on the batch or the column it lands in
    y = rng.standard_normal((3000, 40))
    y[5::7, 3] = y[4:-1:7, 3]    # some ties
    wy = rng.gamma(0.5, size=3000)
    perm = rng.permutation(40)
    s0, s1 = weighted_summary(_dev(y), weights=_dev(wy)), weighted_summary(_dev(y[:, perm]), weights=_dev(wy))
    for k in s0.names:
        assert s0[k][perm].tobytes() == s1[k].tobytes(), k


@pytest.mark.parametrize('n', (1, 255, 256, 257, 2048, 2049, 524288, 524289))
def test_cumweights_is_the_running_sum_of_the_permuted_weights(n):
    """Whole-number weights: every partial sum is exact, whatever its grouping, so the comparison is for equality."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context, _ptr
    rng = np.random.default_rng(n)
    w = rng.integers(0, 1000, size=n).astype(np.float64)
    order = rng.permutation(n).astype(np.uint32)
    ctx = get_context()
    w_d, o_d = _dev(w), _dev(order.view(np.int32))
    cum = torch.full((n + 1,), -7., dtype=torch.float64, device='cuda')
    work = torch.empty(((n + _lib.WSTAT_TILE - 1) // _lib.WSTAT_TILE,), dtype=torch.float64, device='cuda')
    _lib.check(ctx._lib.bfhip_wstat_cumweights(ctx.handle, n, _ptr(o_d), _ptr(w_d), _ptr(cum), _ptr(work)))
    got = cum.cpu().numpy()
    assert got[n] == -7.   # nothing is written past the end
    assert np.array_equal(got[:n], np.cumsum(w[order]))
    assert ctx._lib.bfhip_wstat_cumweights(ctx.handle, 0, _ptr(o_d), _ptr(w_d), _ptr(cum), _ptr(work)) == -1
    assert ctx._lib.bfhip_wstat_cumweights(ctx.handle, n, None, _ptr(w_d), _ptr(cum), _ptr(work)) == -1


def test_trace_weighted_summary_after_sample(monkeypatch):
    """16 chains x 40 draws x 4-d: the device route on the chains where sample() left them against the host port on
    tt.get(flatten=False), with the weights of a wider Gaussian than the sampled one."""
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import psis, weighted_summary
    d = 4
    rng = np.random.default_rng(2)
    su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
    den = bfa.SurrogateDensity(su, input_scales=np.stack([np.full(d, -8.), np.full(d, 9.)], 1))
    xf = rng.standard_normal((4 * su.n_param, d)) * 1.5
    den.fit(xf, -0.5 * (xf**2).sum(axis=1))
    tt = bfa.sample(den, bfa.NTrace(n_chain=16, n_iter=60, n_warmup=20, x_0=rng.standard_normal((16, d)), random_generator=7),
                    verbose=False)
    for kw in (dict(), dict(original_space=False), dict(since_iter=31), dict(include_warmup=True)):
        x = tt.get(flatten=False, **kw)
        assert x.shape[0] == 16 and x.shape[2] == d
        lw = 0.1 * (x**2).sum(axis=2)    # towards N(0, 1.25 I)
        r = psis(lw)
        want = weighted_summary(x, log_weights=r.log_weights, probs=(0.1, 0.5, 0.9))
        ref = pr.table_reference(x, log_weights=r.log_weights, probs=(0.1, 0.5, 0.9))
        assert (ref['margin'] >= 1e-9).all(), kw
        for lw_in in (r.log_weights, _dev(r.log_weights).reshape(-1)):
            got = tt.weighted_summary(lw_in, probs=(0.1, 0.5, 0.9), **kw)
            assert_table(got, want, kw)
            assert_table(got, ref, kw)
    assert tt.get(flatten=False).shape == (16, 40, d)
    with pytest.raises(ValueError):
        tt.weighted_summary(np.zeros((16, 1)), since_iter=59)
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r'gather\(\)'):
        tt.weighted_summary(np.zeros((16, 40)))
