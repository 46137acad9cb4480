"""The device route of the convergence diagnostics (csrc/bfhip_diag.hip through utils/diagnostics.py) against the loop-written
reference of helpers/diag_reference.py: the shape grid, ties, constant and non-finite parameters, float32 input, strided views,
repeatability and independence of the batch, ``TraceTuple.summary`` after ``sample()``, and the full 4096 x 1000 x 64 size."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import diag_reference as dr  # noqa: E402

GRID = [(4, 100, 3), (2, 8, 2), (7, 333, 5), (64, 1000, 16), (16, 63, 130), (256, 501, 20)]
RTOL = 1e-9
EXTRA = ('rhat', 'rhat_split', 'ess_bulk', 'ess_tail', 'ess_mean')


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def assert_table(got, ref, names=None):
    for k in (names or getattr(got, 'names', None) or tuple(got)):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, k
        assert np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=0, err_msg=k)


def single_calls(x):
    from bayesfast_amd.utils import rhat, ess
    return {'rhat': rhat(x), 'rhat_split': rhat(x, 'split'), 'ess_bulk': ess(x), 'ess_tail': ess(x, 'tail'), 'ess_mean': ess(x, 'mean')}


def same_bytes(a, b):
    return a.names == b.names and all(a[k].tobytes() == b[k].tobytes() for k in a.names)


@pytest.mark.parametrize('shape', GRID)
def test_shape_grid(shape):
    from bayesfast_amd.utils import summary
    x = dr.ar1(shape, seed=sum(shape))
    ref = dr.reference(x)
    assert (ref['margin'] >= 1e-9).all()
    got = summary(_dev(x))
    for k in got.names:
        print(shape, k, np.max(np.abs(got[k] / ref[k] - 1)))
    assert_table(got, ref)
    assert_table(single_calls(_dev(x)), ref, EXTRA)
    if shape[0] * shape[1] * shape[2] < 500000:
        x32 = x.astype(np.float32)
        ref32 = dr.reference(x32)
        assert (ref32['margin'] >= 1e-9).all()
        assert_table(summary(_dev(x32)), ref32)


def test_ties_constant_and_non_finite():
    from bayesfast_amd.utils import summary
    x = dr.ar1((7, 333, 5), seed=351)
    x[:, 1::2] = x[:, 0:332:2]   # every second draw repeats the previous one exactly
    ref = dr.reference(x)
    assert (ref['margin'] >= 1e-9).all()
    assert_table(summary(_dev(x)), ref)
    assert_table(single_calls(_dev(x)), ref, EXTRA)
    y = dr.ar1((4, 100, 19), seed=9)
    y[:, :, 1] = 1.5
    y[:, :, 17] = -0.
    y[:, :, 5] = 0.1      # constants whose sum of n copies is not n times the constant
    y[:, :, 6] = 0.001
    y[2, 17, 2] = np.nan
    y[0, 60, 3] = np.inf
    y[3, 99, 18] = -np.inf
    ref = dr.reference(y)
    got = summary(_dev(y))
    assert_table(got, ref)
    assert_table(single_calls(_dev(y)), ref, EXTRA)
    assert got['mean'][1] == 1.5 and got['sd'][1] == 0. and got['q95'][1] == 1.5 and np.isnan(got['rhat'][1])
    for v in single_calls(_dev(y)).values():   # the calls that sort nothing see the constants too
        assert np.isnan(v[[1, 5, 6, 17]]).all() and np.isfinite(v[[0, 4, 16]]).all()
    assert np.array_equal(got['mean'][[5, 6]], [0.1, 0.001]) and np.array_equal(got['sd'][[5, 6]], [0., 0.])
    y32 = y.astype(np.float32)
    assert_table(summary(_dev(y32)), dr.reference(y32))
    assert all(np.isnan(got[k][[2, 3, 18]]).all() for k in got.names)
    assert all(np.isfinite(got[k][[0, 4, 16]]).all() for k in got.names)
    other = summary(_dev(y), probs=(0.025, 0.975), prob=(0.1, 0.5, 0.9))
    assert other.names[2:4] == ('q2.5', 'q97.5')
    assert_table(other, dr.reference(y, probs=(0.025, 0.975), prob=(0.1, 0.5, 0.9)))
    with pytest.raises(ValueError):
        summary(_dev(y[:, :3]))
    with pytest.raises(ValueError):
        summary(_dev(y[0, :, 0]))


def test_strided_view_repeatability_and_batch_independence():
    from bayesfast_amd.utils import summary
    x = _dev(dr.ar1((40, 1500, 20), seed=4))
    v = x[:, 137:]   # an odd number of draws: the split starts one row further on
    assert not v.is_contiguous()
    a, b = summary(v), summary(v.contiguous())
    assert same_bytes(a, b) and same_bytes(a, summary(v))
    assert_table(a, dr.reference(v.cpu().numpy()))
    # input the column kernel cannot read in place is converted batch by batch: a last axis that is not contiguous, float16
    t = x.permute(0, 2, 1)[:, :, :40]   # (40, 20, 40) with stride 1 along time
    assert t.stride(2) != 1
    assert same_bytes(summary(t), summary(t.contiguous()))
    import torch
    h16 = x[:8, :200, :18].to(torch.float16)
    assert_table(summary(h16), dr.reference(h16.cpu().numpy()))
    y = dr.ar1((12, 400, 40), seed=6)
    y[:, 5::7, 3] = y[:, 4:-1:7, 3]   # some ties
    perm = np.random.default_rng(1).permutation(40)
    s0, s1 = summary(_dev(y)), summary(_dev(y[:, :, perm]))
    for k in s0.names:
        assert s0[k][perm].tobytes() == s1[k].tobytes(), k
    assert_table(s0, dr.reference(y))


def test_trace_summary_after_sample():
    """64 chains x 600 x 16-d on a correlated Gaussian behind input scales (two spaces): tt.summary against the reference on
    tt.get(flatten=False), in both spaces and for logp; mean and sd within 5 mcse_mean of the target's (5 standard errors over 32
    figures can fail by chance on some seeds: with random_generator=7 the largest are 3.1 for a mean and 3.9 for an sd)."""
    import bayesfast_amd as bfa
    from bayesfast_amd.workloads import correlated_gaussian_spec
    d = 16
    _, cov = correlated_gaussian_spec(d)
    prec = np.linalg.inv(cov)
    rng = np.random.default_rng(2)
    su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
    den = bfa.SurrogateDensity(su, input_scales=np.stack([np.full(d, -8.), np.full(d, 9.)], 1))
    xf = rng.multivariate_normal(np.zeros(d), cov * 2.25, size=4 * su.n_param)
    den.fit(xf, -0.5 * np.einsum('ij,jk,ik->i', xf, prec, xf))
    tt = bfa.sample(den, bfa.NTrace(n_chain=64, n_iter=600, n_warmup=200, x_0=rng.multivariate_normal(np.zeros(d), cov, size=64),
                                    random_generator=7), verbose=False)
    cases = [dict(), dict(original_space=False), dict(since_iter=251), dict(include_warmup=True), dict(return_type='logp'),
             dict(return_type='logp', original_space=False, since_iter=150)]
    for kw in cases:
        ref = dr.reference(tt.get(flatten=False, **kw))
        assert (ref['margin'] >= 1e-9).all(), kw
        assert_table(tt.summary(**kw), ref)
        assert_table({'rhat': tt.rhat(**kw), 'rhat_split': tt.rhat(method='split', **kw), 'ess_bulk': tt.ess(**kw),
                      'ess_tail': tt.ess(method='tail', **kw), 'ess_mean': tt.ess(method='mean', **kw)}, ref, EXTRA)
    s = tt.summary()
    sd = np.sqrt(np.diag(cov))
    print('mean / mcse', s['mean'] / s['mcse_mean'], 'sd / mcse', (s['sd'] - sd) / s['mcse_mean'], 'rhat', s['rhat'])
    assert np.all(np.abs(s['mean']) < 5 * s['mcse_mean']) and np.all(np.abs(s['sd'] - sd) < 5 * s['mcse_mean'])
    assert np.all(s['rhat'] < 1.05)
    with pytest.raises(ValueError):
        tt.summary(since_iter=599)
    with pytest.raises(ValueError):
        tt.rhat(return_type='all')


def test_full_size():
    """4096 x 1000 x 64 iid normal draws generated on the device: finite, R-hat within 0.01 of 1, and three parameters against the
    reference on their columns alone."""
    import torch
    from bayesfast_amd.utils import summary
    g = torch.Generator(device='cuda').manual_seed(13)
    x = torch.randn((4096, 1000, 64), generator=g, device='cuda', dtype=torch.float64)
    s = summary(x)
    for k in s.names:
        assert s[k].shape == (64,) and np.isfinite(s[k]).all(), k
    assert np.all(np.abs(s['rhat'] - 1) < 0.01)
    assert np.all(s['ess_bulk'] > 0.9 * 4096000) and np.all(np.abs(s['mean']) < 5 * s['mcse_mean'])
    for k in np.random.default_rng(17).choice(64, size=3, replace=False):
        ref = dr.reference(x[:, :, int(k)].cpu().numpy())
        assert (ref['margin'] >= 1e-9).all()
        assert_table({n: s[n][k:k + 1] for n in s.names}, ref)
