"""Gaussianized importance sampling (GIS) and Gaussianized harmonic mean (GHM), and the two plain estimators under them,
``importance`` and ``harmonic``, against the reference's own results (tests/golden/evidence_is_hm.npz,
make_golden_is_hm.py).  CPU: the argument errors raised before any device call, with the reference's messages.  GPU (marked):
``bfhip_logmeanexp_stats`` against a NumPy restatement at the grid's edge sizes and on special values, the fixture's values and
warnings, the known log-evidence of a Gaussian surrogate and of the 16-d funnel, and the device route against the host route."""
import os
import warnings

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- CPU: argument checks ----------------------------------------------------------------------------------------------

def test_public_names():
    import bayesfast_amd as bfa
    from bayesfast_amd import evidence
    for name in ('importance', 'harmonic', 'GIS', 'GHM'):
        assert getattr(bfa, name) is getattr(evidence, name)
        assert name in bfa.__all__ and name in evidence.__all__


@pytest.mark.parametrize('which', ['importance', 'harmonic'])
def test_estimators_refuse_wrong_dimension_and_shape(which):
    from bayesfast_amd import evidence
    f = getattr(evidence, which)
    names = ('logp_q', 'logq_q') if which == 'importance' else ('logp_p', 'logq_p')
    checked = names[1] if which == 'importance' else names[0]   # the reference checks the dimension of this one
    with pytest.raises(ValueError, match=r'^dim of {} should be 1 or 2, instead of 3\.$'.format(checked)):
        f(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match=r'^dim of {} should be 1 or 2, instead of 0\.$'.format(checked)):
        f(1., 2.)
    with pytest.raises(ValueError, match=r'^shape of {}, \(5,\), is different from shape of {}, \(6,\)\.$'.format(*names)):
        f(np.zeros(5), np.zeros(6))
    with pytest.raises(ValueError, match=r'^shape of {}, \(2, 3\), is different from shape of {}, \(6,\)\.$'.format(*names)):
        f(np.zeros((2, 3)), np.zeros(6))
    with pytest.raises(ValueError, match='invalid value for the inputs'):
        f(['a', 'b'], [1., 2.])
    with pytest.raises(ValueError, match='empty'):   # (the reference returns NaN here)
        f(np.zeros(0), np.zeros(0))


def test_gis_argument_errors():
    from bayesfast_amd import GIS, SIT
    for bad in (0, -3, 'x'):
        with pytest.raises(ValueError, match=r'^invalid value for n_q\.$'):
            GIS(n_q=bad)
    for bad in (0., -0.5, 'x'):
        with pytest.raises(ValueError, match=r'^invalid value for f_call\.$'):
            GIS(f_call=bad)
    for bad in (3, 'sit', [1]):
        with pytest.raises(ValueError, match=r'^invalid value for sit\.$'):
            GIS(sit=bad)
    g = GIS(sit=SIT(n_iter=2), n_q=100, f_call=None)
    assert g.n_q == 100 and g.f_call is None and g.sit.n_iter == 2
    assert GIS(sit=dict(n_iter=3)).sit.n_iter == 3 and GIS().f_call == 0.05
    x = np.random.default_rng(0).normal(size=(50, 3))
    with pytest.raises(ValueError, match=r'^logp should be callable\.$'):
        GIS()(x, None)
    with pytest.raises(ValueError, match=r'^logp should be callable\.$'):
        GIS()(x, np.zeros(50))
    with pytest.raises(ValueError, match=r'^invalid value for x_p\.$'):
        GIS()(np.zeros(50), lambda v: v[..., 0])
    with pytest.raises(ValueError, match=r'^invalid value for x_p\.$'):
        GIS()(np.zeros((2, 3, 4, 5)), lambda v: v[..., 0])
    with pytest.raises(ValueError, match=r'^invalid shape for x_p\.$'):
        GIS()(np.zeros((50, 1)), lambda v: v[..., 0])
    with pytest.raises(ValueError, match=r'^invalid shape for x_p\.$'):
        GIS()(np.zeros((1, 1, 4)), lambda v: v[..., 0])


def test_ghm_argument_errors():
    from bayesfast_amd import GHM
    for bad in (3, 'sit', [1]):
        with pytest.raises(ValueError, match=r'^invalid value for sit\.$'):
            GHM(sit=bad)
    assert GHM(sit=dict(n_iter=3)).sit.n_iter == 3
    x = np.random.default_rng(0).normal(size=(50, 3))
    msg = r'^you gave me neither the correct logp_p nor a callable logp function\.$'
    with pytest.raises(ValueError, match=msg):
        GHM()(x)
    with pytest.raises(ValueError, match=msg):
        GHM()(x, np.zeros(50))   # logp not callable
    with pytest.warns(RuntimeWarning, match='seems not correct'):
        with pytest.raises(ValueError, match=msg):
            GHM()(x, None, np.zeros(49))
    with pytest.warns(RuntimeWarning, match='seems not correct'):
        with pytest.raises(ValueError, match=msg):
            GHM()(x.reshape(5, 10, 3), logp_p=np.zeros(50))   # (chain, iteration) samples want logp_p of shape (5, 10)
    with pytest.raises(ValueError, match=r'^invalid value for x_p\.$'):
        GHM()(np.zeros(50), logp_p=np.zeros(50))
    with pytest.raises(ValueError, match=r'^invalid shape for x_p\.$'):
        GHM()(np.zeros((50, 1)), logp_p=np.zeros(50))


# ---- GPU: the reduction kernel ---------------------------------------------------------------------------------------

def _numpy_stats(x, y):
    """What importance.py:26-28 / harmonic.py:27-31 compute: L = log mean exp(x - y), the normalised terms and their moments."""
    from scipy.special import logsumexp
    t = x - y
    with np.errstate(invalid='ignore', over='ignore'):
        L = logsumexp(t, b=1. / t.size)
        f = np.exp(t - L)
        return L, np.mean(f), np.var(f), f


def _device_stats(x, y, terms=True):
    from bayesfast_amd.device import get_context
    from bayesfast_amd.evidence.importance import _logmeanexp_stats
    ctx = get_context()
    L, m, v, f = _logmeanexp_stats(ctx, ctx.tensor(x), ctx.tensor(y), want_terms=terms)
    return L, m, v, (f.cpu().numpy() if terms else None)


_SIZES = (1, 255, 256, 257, 131072 + 3, 512 * 256 * 3 + 17)


@pytest.mark.gpu
@pytest.mark.parametrize('n', _SIZES)
def test_logmeanexp_stats_matches_numpy(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n) * 3. + 1.
    y = rng.normal(size=n)
    if n > 3:
        x[rng.choice(n, max(1, n // 100), replace=False)] = -np.inf   # zero weights
    L0, m0, v0, f0 = _numpy_stats(x, y)
    L, m, v, f = _device_stats(x, y)
    assert abs(L - L0) < 1e-12 * max(1., abs(L0))
    assert abs(m - m0) < 1e-12 * abs(m0)
    assert abs(v - v0) <= 1e-10 * v0 + (1e-300 if n == 1 else 0.)
    np.testing.assert_allclose(f, f0, rtol=1e-13, atol=0.)
    assert np.array_equal(f == 0., np.isneginf(x))
    # deterministic: two calls are bitwise equal, and a device tensor gives what the array gives
    again = _device_stats(x, y)
    assert (L, m, v) == again[:3] and np.array_equal(f, again[3])
    assert _device_stats(x, y, terms=False)[:3] == (L, m, v)
    from bayesfast_amd import importance, harmonic
    from bayesfast_amd.device import get_context
    ctx = get_context()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert importance(x, y) == importance(ctx.tensor(x), ctx.tensor(y)) == importance(ctx.tensor(x), y)
    if n > 1:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert harmonic(-x, -y) == harmonic(ctx.tensor(-x), ctx.tensor(-y))


@pytest.mark.gpu
@pytest.mark.parametrize('n', _SIZES)
def test_logmeanexp_stats_special_values(n):
    from bayesfast_amd import importance
    rng = np.random.default_rng(100 + n)
    y = rng.integers(-40, 40, size=n) * 0.25
    # all t equal (x - y is exact here): every term is 1, the variance exactly 0, and so is importance's error
    x = y + 2.5
    L, m, v, f = _device_stats(x, y)
    assert L == 2.5 and m == 1. and v == 0. and np.all(f == 1.)
    logr, err = importance(x, y)
    assert logr == 2.5 and err == 0.
    # a NaN anywhere propagates to all three outputs
    x = rng.normal(size=n)
    x[n // 2] = np.nan
    L, m, v, _ = _device_stats(x, y)
    assert np.isnan(L) and np.isnan(m) and np.isnan(v)
    # every t = -inf: L = -inf, the moments NaN (scipy's logsumexp and numpy's var), no error
    x = np.full(n, -np.inf)
    L, m, v, f = _device_stats(x, y)
    L0, m0, v0, _ = _numpy_stats(x, y)
    assert L == L0 == -np.inf and np.isnan(m) and np.isnan(v) and np.isnan(m0) and np.isnan(v0) and np.isnan(f).all()


@pytest.mark.gpu
def test_logmeanexp_stats_refuses_bad_arguments():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context, _ptr
    ctx = get_context()
    a = torch.zeros(4, dtype=torch.float64, device=ctx.device)
    out = torch.zeros(3, dtype=torch.float64, device=ctx.device)
    f = ctx._lib.bfhip_logmeanexp_stats
    for args in ((0, _ptr(a), _ptr(a), _ptr(out)), (-1, _ptr(a), _ptr(a), _ptr(out)), (4, None, _ptr(a), _ptr(out)),
                 (4, _ptr(a), None, _ptr(out)), (4, _ptr(a), _ptr(a), None)):
        with pytest.raises(ValueError, match='bfhip_logmeanexp_stats'):
            _lib.check(f(ctx.handle, *args, None))
    _lib.check(f(ctx.handle, 4, _ptr(a), _ptr(a), _ptr(out), None))
    assert out.cpu().numpy().tolist() == [0., 1., 0.]


# ---- GPU: the estimators against the reference -------------------------------------------------------------------------

@pytest.mark.gpu
def test_importance_and_harmonic_match_the_reference():
    from bayesfast_amd import importance, harmonic
    from bayesfast_amd.device import get_context
    fx = np.load(os.path.join(G, 'evidence_is_hm.npz'))
    ctx = get_context()
    seen = set()
    for name in fx['cases']:
        name = str(name)
        f = importance if name.startswith('is_') else harmonic
        a, b = fx[name + '.a'].astype(np.float64), fx[name + '.b'].astype(np.float64)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            logr, err = f(a, b)
        msgs = [str(m.message) for m in w if m.category is RuntimeWarning]
        assert abs(logr - fx[name + '.logr']) < 1e-12, name
        assert abs(err - fx[name + '.err']) < 1e-10 * fx[name + '.err'], name
        assert any('larger than 0.25' in m for m in msgs) == bool(fx[name + '.w_large']), (name, msgs)
        assert any('more than 25%' in m for m in msgs) == bool(fx[name + '.w_tau']), (name, msgs)
        assert len(msgs) == int(fx[name + '.w_large']) + int(fx[name + '.w_tau']), (name, msgs)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert f(ctx.tensor(a), ctx.tensor(b)) == (logr, err), name   # device tensors: the same values
        seen.add((name[:2], bool(fx[name + '.w_large']), bool(fx[name + '.w_tau']), a.ndim, bool(np.isneginf(a).any())))
    # the fixture has what the cases are for: both dimensions, both warnings, -inf entries
    assert {(k, nd) for k, _, _, nd, _ in seen} == {('is', 1), ('is', 2), ('hm', 1), ('hm', 2)}
    assert any(s[1] for s in seen if s[0] == 'is') and any(s[1] for s in seen if s[0] == 'hm')
    assert any(s[2] for s in seen) and any(s[4] for s in seen)
    with pytest.warns(RuntimeWarning, match='larger than 0.25'):
        importance(fx['is_heavy.a'].astype(np.float64), fx['is_heavy.b'].astype(np.float64))
    with pytest.warns(RuntimeWarning, match='more than 25%'):
        harmonic(fx['hm_offset.a'].astype(np.float64), fx['hm_offset.b'].astype(np.float64))


# ---- GPU: GIS and GHM ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def gaussian_trace():
    """test_evidence.py:test_sample_then_gbs_end_to_end_on_a_gaussian_surrogate's setting: a quadratic surrogate of an
    unnormalised 12-d Gaussian sampled with NUTS; log Z = c0 + d/2 log(2 pi) + 1/2 log det Sigma."""
    import bayesfast_amd as bfa
    from bayesfast_amd.workloads import correlated_gaussian_spec
    d = 12
    _, cov = correlated_gaussian_spec(d)
    prec = np.linalg.inv(cov)
    c0 = -3.5
    rng = np.random.default_rng(7)
    su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
    den = bfa.SurrogateDensity(su)
    xf = rng.normal(size=(4 * su.n_param, d)) @ np.linalg.cholesky(cov).T * 1.6
    den.fit(xf, c0 - 0.5 * np.einsum('ij,jk,ik->i', xf, prec, xf))
    tt = bfa.sample(den, {'n_chain': 16, 'n_iter': 1500, 'n_warmup': 500, 'random_generator': 4}, verbose=False)
    exact = c0 + 0.5 * d * np.log(2 * np.pi) + 0.5 * np.linalg.slogdet(cov)[1]
    return tt, den, exact


def _quiet(f, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return f(*args, **kwargs)


@pytest.mark.gpu
def test_gis_recovers_the_gaussian_evidence_on_the_device_route(gaussian_trace, monkeypatch):
    import bayesfast_amd as bfa
    from bayesfast_amd.core.density import SurrogateDensity
    from bayesfast_amd.transforms.sit import SIT
    tt, den, exact = gaussian_trace
    # the device route: no host-side logp, draws or logq (they would raise here)
    with monkeypatch.context() as mp:
        for cls, name in ((SurrogateDensity, 'logp_and_grad'), (SIT, 'sample'), (SIT, 'logq')):
            mp.setattr(cls, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError('host route taken')))
        logz, err = _quiet(bfa.GIS(sit=dict(random_generator=5), n_q=12000), tt, den.logp)
    assert 0. < err < 0.1
    assert abs(logz - exact) < 3. * err + 0.02, (logz, err, exact)
    # the host route -- the same TraceTuple with logp wrapped so that it is just a callable, or the samples as an array -- is the
    # same estimate: same SIT (same seeds), same draws, log-densities to summation order
    logz_h, err_h = _quiet(bfa.GIS(sit=dict(random_generator=5), n_q=12000), tt, lambda x: den.logp(x))
    logz_a, err_a = _quiet(bfa.GIS(sit=dict(random_generator=5), n_q=12000), tt.get(flatten=False), den.logp)
    assert abs(logz - logz_h) < 1e-9 and abs(err - err_h) < 1e-9 * err
    assert abs(logz_a - logz_h) < 1e-9 and abs(err_a - err_h) < 1e-9 * err
    # logp_p is accepted and ignored (evidence/gaussianized.py:224); f_call sizes n_q from the TraceTuple's density calls
    logz_k, _ = _quiet(bfa.GIS(sit=dict(random_generator=5), n_q=12000), tt, den.logp, logp_p=np.zeros(3))
    assert logz_k == logz
    g = bfa.GIS(sit=dict(random_generator=5), f_call=0.05)
    logz_f, err_f = _quiet(g, tt, den.logp)
    assert abs(logz_f - exact) < 3. * err_f + 0.02, (logz_f, err_f, exact)


@pytest.mark.gpu
def test_ghm_recovers_the_gaussian_evidence_on_both_routes(gaussian_trace):
    import bayesfast_amd as bfa
    tt, den, exact = gaussian_trace
    logz, err = _quiet(bfa.GHM(sit=dict(random_generator=5)), tt, den.logp)
    assert 0. < err < 0.1
    assert abs(logz - exact) < 0.1, (logz, err, exact)
    logz_h, err_h = _quiet(bfa.GHM(sit=dict(random_generator=5)), tt, lambda x: den.logp(x))
    logz_a, err_a = _quiet(bfa.GHM(sit=dict(random_generator=5)), tt.get(flatten=False), den.logp)
    assert abs(logz - logz_h) < 1e-9 and abs(err - err_h) < 1e-9 * err
    assert abs(logz_a - logz_h) < 1e-9 and abs(err_a - err_h) < 1e-9 * err
    # logp_p given (evidence/gaussianized.py:257-265): used when its shape fits -- without a logp too --, recomputed with the
    # reference's warning when it does not
    lp = tt.get(return_type='logp', flatten=False)
    logz_k, _ = _quiet(bfa.GHM(sit=dict(random_generator=5)), tt, den.logp, logp_p=lp)
    assert abs(logz_k - logz) < 1e-6
    logz_n, _ = _quiet(bfa.GHM(sit=dict(random_generator=5)), tt, logp_p=lp)
    assert logz_n == logz_k
    logz_nh, _ = _quiet(bfa.GHM(sit=dict(random_generator=5)), tt.get(flatten=False), logp_p=lp)
    assert abs(logz_nh - logz_n) < 1e-9
    with pytest.warns(RuntimeWarning, match='seems not correct'):
        logz_w, _ = bfa.GHM(sit=dict(random_generator=5))(tt, den.logp, logp_p=lp[:, :-1])
    assert abs(logz_w - logz) < 1e-9
    with pytest.warns(RuntimeWarning, match='seems not correct'):
        with pytest.raises(ValueError, match='neither the correct logp_p nor a callable logp'):
            bfa.GHM(sit=dict(random_generator=5))(tt, logp_p=lp[:, :-1])


@pytest.mark.gpu
def test_gis_recovers_the_16d_funnel_evidence():
    """test_evidence.py:test_gbs_recovers_the_16d_funnel_evidence with GIS: fiducial logZ = -63.4988,
    exact posterior draws (8 x 1500) for the NUTS chains."""
    from bayesfast_amd import GIS
    D, a, b = 16, 1., 0.5
    const = np.log(8.) + (D - 1) * np.log(60.)

    def logp(x):
        n = x.shape[-1]
        return (-0.5 * x[..., 0]**2 / a**2 - 0.5 * np.sum(x[..., 1:]**2, axis=-1) * np.exp(-2 * b * x[..., 0])
                - 0.5 * np.log(2 * np.pi * a**2) - 0.5 * (n - 1) * np.log(2 * np.pi) - (n - 1) * b * x[..., 0] - const)

    rng = np.random.default_rng(16)
    x0 = rng.normal(size=(8, 1500)) * a
    xs = np.concatenate((x0[..., None], rng.normal(size=(8, 1500, D - 1)) * np.exp(b * x0)[..., None]), -1)
    logz, err = _quiet(GIS(sit=dict(random_generator=5), n_q=12000), xs, logp)
    assert 0. < err < 0.2
    assert abs(logz - (-63.4988)) < 3. * err + 0.05, (logz, err)
