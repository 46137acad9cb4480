"""GPU parity of the pipeline density's STREAMED form (bfhip_pld.h: pld_eval_stream_q8): surrogates whose monomials, with Phi, W
and the gradient table, do not fit one workgroup's LDS run in chunks of monomials -- the stand-alone evaluation
(bf_pld_logp_grad_kernel<8, E, true>) and the fused sampler (bf_sampler_kernel<W, ..., 11, FULLM>) against the CPU oracle on
shared xoshiro streams, and against the resident form where both run (bfhip_debug_set('pld_stream', 1))."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240917

# (m, d, nq, transform): a full quadratic at d = 64 behind the box transform (2,145 monomials), a quadratic in 64 of 128 inputs
# (2,209), and more outputs than monomials at d = 128 (339 monomials: the Householder compression, then still streamed)
SHAPES = [(457, 64, 64, True), (120, 128, 64, False), (400, 128, 20, True)]


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


_SPECS = {}


def _spec(m, d, nq, transform):
    from bayesfast_amd.workloads import random_pipeline_spec
    key = (m, d, nq, transform)
    if key not in _SPECS:
        _SPECS[key] = random_pipeline_spec(m, d, nq, seed=m + d, transform=transform)
    return _SPECS[key]


def _to_su(spec, x):
    """The surrogate's input for sampler-space points: the logistic map of random_pipeline_spec's box, then its input scaling."""
    xo = x
    if spec.get('ranges') is not None:
        rg = np.asarray(spec['ranges'])
        xo = rg[:, 0] + (rg[:, 1] - rg[:, 0]) / (1. + np.exp(-x))
    if spec.get('su_lo') is not None:
        xo = (xo - spec['su_lo']) / spec['su_diff']
    return xo


def _points(spec, transform, n, seed):
    rng = np.random.default_rng(seed)
    scale = np.repeat([0.15, 0.6, 2.5] if transform else [0.05, 0.2, 1.], (n + 2) // 3)[:n, None]
    return (0. if transform else 0.5) + rng.normal(size=(n, spec['d'])) * scale


@pytest.mark.parametrize('m,d,nq,transform', SHAPES)
def test_streamed_logp_and_grad_against_the_oracle(ctx, m, d, nq, transform):
    """Evaluation inside and outside the bound's ellipsoid; before the streamed form these shapes were refused at upload."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd import _lib
    from oracle import oracle as orc
    spec = _spec(m, d, nq, transform)
    dd = DeviceDensity(spec, ctx)
    x = _points(spec, transform, 21, m)
    lp, g = dd.logp_and_grad(x)
    assert _lib.last_kernel() == 'bf_pld_logp_grad_kernel<8, %d, true>' % (2 if d > 64 else 1)
    lpo, go = orc.logp_and_grad(spec, x)
    np.testing.assert_allclose(lp.cpu().numpy(), lpo, rtol=1e-10, atol=1e-8)
    np.testing.assert_allclose(g.cpu().numpy(), go, rtol=1e-9, atol=1e-7)
    xm = _to_su(spec, x) - spec['poly']['mu']
    b = np.sqrt(np.einsum('ij,jk,ik->i', xm, spec['poly']['hess'], xm))
    assert (b > spec['poly']['alpha']).any() and (b < spec['poly']['alpha']).any()


def test_streamed_leapfrog_step_matches_the_oracle(ctx):
    import torch
    from bayesfast_amd.device import DeviceDensity
    from oracle import oracle as orc
    spec = _spec(*SHAPES[0])
    dd = DeviceDensity(spec, ctx)
    rng = np.random.default_rng(8)
    n, d = 13, spec['d']
    q, p = rng.normal(size=(n, d)) * 0.3, rng.normal(size=(n, d))
    var_b, eps_b = rng.uniform(0.5, 2., size=(n, d)), rng.uniform(-0.05, 0.05, size=n)
    _, g = orc.logp_and_grad(spec, q)
    T = lambda a: ctx.tensor(np.atleast_2d(a).copy(), torch.float64)
    tq, tp, tg = T(q), T(p), T(g)
    v = ctx.empty(tq.shape)
    logp, energy = dd.leapfrog(ctx.tensor(eps_b), T(var_b), tq, tp, tg, velocity=v)
    for i in range(0, n, 3):
        r = orc.leapfrog(spec, var_b[i], eps_b[i], q[i], p[i], g[i])
        np.testing.assert_allclose(tq[i].cpu().numpy(), r['q'], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(tp[i].cpu().numpy(), r['p'], rtol=1e-9, atol=1e-8)
        np.testing.assert_allclose(tg[i].cpu().numpy(), r['grad'], rtol=1e-9, atol=1e-7)
        np.testing.assert_allclose(v[i].cpu().numpy(), r['v'], rtol=1e-9, atol=1e-8)
        np.testing.assert_allclose(logp[i].item(), r['logp'], rtol=1e-10, atol=1e-8)
        np.testing.assert_allclose(energy[i].item(), r['energy'], rtol=1e-10, atol=1e-8)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]])
def test_streamed_nuts_against_the_oracle(ctx, shape):
    """A short NUTS run (max_treedepth 6) in the fused sampler, a few chains against the oracle on their xoshiro streams: tree
    depth, size and divergence exactly, positions to 1e-8 on the first iterations."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    from oracle import oracle as orc
    spec = _spec(*shape)
    d = spec['d']
    x0 = np.random.default_rng(3).normal(size=(9, d)) * 0.1
    dc = DeviceChains(DeviceDensity(spec, ctx), x0, seed=SEED)
    n_iter, n_warmup = 6, 4
    s, st = dc.run(n_iter, 'NUTS', n_warmup=n_warmup, max_treedepth=6)
    assert ', 11, 0>' in _lib.last_kernel(), _lib.last_kernel()
    s, st = s.cpu().numpy(), st.cpu().numpy()
    assert dc.total_leapfrog == int(st[:, :, _lib.NSTATS.index('tree_size')].sum())
    for i in (0, 8):
        so, sto = orc.nuts_run(spec, orc.Chain(x0[i]), orc.make_rng('xoshiro', seed=SEED, stream=i), n_iter, n_warmup, max_treedepth=6)
        for f in ('tree_depth', 'tree_size', 'diverging'):
            assert np.array_equal(st[i, :, _lib.NSTATS.index(f)], sto[f]), (i, f, st[i, :, _lib.NSTATS.index(f)], sto[f])
        np.testing.assert_allclose(s[i, :3], so[:3], rtol=1e-8, atol=1e-8)


def test_streamed_hmc_resume_and_full_rank_metric(ctx):
    """HMC against the oracle, a NUTS run cut into two launches equal to one launch, and the full-rank metric
    (bf_sampler_kernel<8, true, false, 11, 1>) against the oracle -- on the compressed d = 128 shape."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    from oracle import oracle as orc
    spec = _spec(*SHAPES[2])
    d = spec['d']
    x0 = np.random.default_rng(12).normal(size=(5, d)) * 0.1
    dc = DeviceChains(DeviceDensity(spec, ctx), x0, seed=SEED)
    s, st = dc.run(6, 'HMC', n_warmup=4, n_int_step=6)
    assert ', 11, 0>' in _lib.last_kernel()
    s, st = s.cpu().numpy(), st.cpu().numpy()
    for i in (0, 4):
        so, sto = orc.hmc_run(spec, orc.Chain(x0[i]), orc.make_rng('xoshiro', seed=SEED, stream=i), 6, 4, n_int_step=6)
        for f in ('accepted', 'diverging'):
            assert np.array_equal(st[i, :, _lib.HSTATS.index(f)], sto[f]), (i, f)
        np.testing.assert_allclose(s[i, :4], so[:4], rtol=1e-8, atol=1e-8)
    a = DeviceChains(DeviceDensity(spec, ctx), x0, seed=3)
    s1, _ = a.run(8, 'NUTS', n_warmup=5, max_treedepth=6)
    b = DeviceChains(DeviceDensity(spec, ctx), x0, seed=3)
    s2a, _ = b.run(3, 'NUTS', n_warmup=5, max_treedepth=6)
    s2b, _ = b.run(5, 'NUTS', n_warmup=5, max_treedepth=6)
    assert np.array_equal(s1.cpu().numpy(), np.concatenate([s2a.cpu().numpy(), s2b.cpu().numpy()], 1))
    dc = DeviceChains(DeviceDensity(spec, ctx), x0[:2], seed=SEED, metric='full')
    s, st = dc.run(5, 'NUTS', n_warmup=3, max_treedepth=6)
    assert ', 11, 1>' in _lib.last_kernel(), _lib.last_kernel()
    s, st = s.cpu().numpy(), st.cpu().numpy()
    for i in range(2):
        so, sto = orc.nuts_run(spec, orc.Chain(x0[i], metric='full'), orc.make_rng('xoshiro', seed=SEED, stream=i), 5, 3, max_treedepth=6)
        for f in ('tree_depth', 'tree_size', 'diverging'):
            assert np.array_equal(st[i, :, _lib.NSTATS.index(f)], sto[f]), (i, f)
        np.testing.assert_allclose(s[i, :3], so[:3], rtol=1e-8, atol=1e-8)


def _des_a():
    import os
    import sys
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    if g not in sys.path:
        sys.path.insert(0, g)
    from specio import rebuild_pipeline_des
    return rebuild_pipeline_des(np.load(os.path.join(g, 'pipeline_des.npz')), 'a')


@pytest.mark.parametrize('which', ['des_a', 'd128'])
def test_forced_streamed_form_equals_the_resident_form(ctx, which):
    """pld_stream = 1 on shapes the resident form holds (the DES fixture; 100 outputs at d = 128): the same tree statistics as the
    resident form, and logp, gradient and positions to rounding (GEMM2 sums over K in another order)."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import random_pipeline_spec
    from bayesfast_amd import _lib
    spec = _des_a() if which == 'des_a' else random_pipeline_spec(100, 128, 9, seed=228, transform=True)
    d = spec['d']
    rng = np.random.default_rng(4)
    x = rng.normal(size=(19, d)) * 0.4
    x0 = rng.normal(size=(11, d)) * (0.4 if which == 'des_a' else 0.1)
    out = {}
    try:
        for forced in (0, 1):
            _lib.debug_set('pld_stream', forced)
            dd = DeviceDensity(spec, ctx)
            lp, g = dd.logp_and_grad(x)
            kern = _lib.last_kernel()
            dc = DeviceChains(dd, x0, seed=SEED)
            s, st = dc.run(10, 'NUTS', n_warmup=6)
            out[forced] = (lp.cpu().numpy(), g.cpu().numpy(), s.cpu().numpy(), st.cpu().numpy(), kern, _lib.last_kernel())
    finally:
        _lib.debug_set('pld_stream', 0)
    assert out[1][4].endswith('true>') and ', 11, 0>' in out[1][5], out[1][4:]
    assert ', 11, ' not in out[0][5]
    np.testing.assert_allclose(out[1][0], out[0][0], rtol=1e-12, atol=1e-10)
    np.testing.assert_allclose(out[1][1], out[0][1], rtol=1e-10, atol=1e-9)
    for f in ('tree_depth', 'tree_size', 'diverging'):
        k = _lib.NSTATS.index(f)
        assert np.array_equal(out[1][3][:, :, k], out[0][3][:, :, k]), f
    np.testing.assert_allclose(out[1][2], out[0][2], rtol=1e-8, atol=1e-8)
    k = _lib.NSTATS.index('logp')
    np.testing.assert_allclose(out[1][3][:, :, k], out[0][3][:, :, k], rtol=1e-10, atol=1e-8)


def test_streamed_refusals(ctx):
    """Tempered NUTS does not run the streamed form (NotImplementedError, nothing launched); min(m, nf) above the streamed form's
    register-held row tiles is refused at upload with its numbers."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import random_pipeline_spec
    spec = _spec(*SHAPES[1])
    d = spec['d']
    dc = DeviceChains(DeviceDensity(spec, ctx), np.zeros((3, d)) + 0.5, seed=1)
    with pytest.raises(NotImplementedError, match='streamed'):
        dc.run_tempered(2, np.full(d, 0.5), np.eye(d) * 0.01, n_warmup=1)
    with pytest.raises(NotImplementedError, match='1024'):
        DeviceDensity(random_pipeline_spec(1100, 64, 64, seed=1, transform=False), ctx)


def test_sample_on_a_fitted_457_output_quadratic_at_48_inputs(ctx):
    """End to end through the package API: a 457-output full quadratic PolyModel at d = 48 (1,225 monomials) fitted on 2P
    Sobol-normal points, Chi2PipelineDensity on it, ``sample()`` with 4096 chains; the posterior mean sits on the data's
    solution, and the tree sizes agree with the depths."""
    import bayesfast_amd as bfa
    from bayesfast_amd.workloads import sobol_normal
    from bayesfast_amd import _lib
    d, m = 48, 457
    rng = np.random.default_rng(17)
    A, c = rng.normal(size=(m, d)), rng.normal(size=m)
    Q = rng.normal(size=(m, d, d)) * 0.02
    model = lambda x: c + x @ A.T + np.einsum('nj,ojk,nk->no', x, Q, x)
    x_true = 0.3 * rng.normal(size=d)
    sigma = 0.5
    su = bfa.PolyModel('quadratic', input_size=d, output_size=m)
    den = bfa.Chi2PipelineDensity(su, model(x_true[None])[0], prec_diag=np.full(m, sigma ** -2))
    x_fit = sobol_normal(2 * su.n_param, d, seed=SEED)
    y_fit = model(x_fit)
    den.fit(x_fit, -0.5 * np.sum((y_fit - model(x_true[None])) ** 2, 1) / sigma ** 2, y=y_fit)
    n_chain, n_iter, n_warmup = 4096, 40, 25
    x0 = x_true + 0.01 * rng.normal(size=(n_chain, d))
    tt = bfa.sample(den, dict(n_chain=n_chain, n_iter=n_iter, n_warmup=n_warmup, x_0=x0, random_generator=7), verbose=False)
    assert ', 11, 0>' in _lib.last_kernel(), _lib.last_kernel()
    so = tt.get(flatten=True)
    assert so.shape == (n_chain * (n_iter - n_warmup), d) and np.isfinite(so).all()
    sig = so.std(0)
    assert np.all(np.abs(so.mean(0) - x_true) < 0.2 * sig + 1e-3), (so.mean(0) - x_true, sig)
    st = tt.device('stats').cpu().numpy()
    ts, td = st[:, :, _lib.NSTATS.index('tree_size')], st[:, :, _lib.NSTATS.index('tree_depth')]
    assert (ts >= 1).all() and (ts <= 2 ** td - 1).all() and (ts >= 2 ** (td - 1)).all()
