"""The Gaussian mixture on the device: ``bfhip_gmm_step`` (csrc/bfhip_gmm.h) through ctypes and ``utils.gmm.gmm_step``, ``gmm`` on
device tensors and ``TraceTuple.gmm``, against the host port (``_step_host``).  Expected values are never the device's.

The bound of one pass is derived in tests/helpers/gmm_cases.py: |dev - host| <= eps (64 (1 + E) + n) sum |terms|.
Every comparison prints the largest ratio to it before it asserts.

Shapes: n in {1, 15, 17, 255, 257, 4099} (a tile is 16 rows, a workgroup of the E kernel 64, a part at least 256; 4099 rows are 16
parts of 256 and a last one of 3), d in {1, 3, 4, 5, 16, 17, 27, 64, 65, 128} (k-step classes 1, 2, 4, 8, 16, 24, 32 of the E kernel;
1, 2, 4, 5 and 8 column blocks of the moment kernel, on both sides of its split at 32 columns), K in {1, 2, 3, 16, 17, 32} (a lane
takes every sixteenth component).  The rows live in a matrix three columns wider (NaN there), the responsibilities in one a column
wider."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

from gmm_cases import mixture, step_case, step_bounds   # noqa: E402

pytestmark = pytest.mark.gpu

# the largest difference between the device and the host route of the weights, means, covariances and the 30 log likelihoods after
# 30 iterations, measured on an MI355X (docs/EXPERIMENTS.md), by the number of parameters; the tests assert 100 times it
MEASURED_EM_DIFF = {3: 6.31e-14, 27: 2.84e-14}


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context()


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return _ctx().tensor(np.ascontiguousarray(a, dtype=np.float64))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_step(c, logw, stats=True, logpdf=True, resp=True, pad=3, rpad=1, x=None):
    """``bfhip_gmm_step`` itself, with ldx = d + pad and ldr = k + rpad: (stats, logpdf, resp) as arrays."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    x = c['x'] if x is None else x
    n, d = x.shape
    k = c['mean'].shape[0]
    wide = np.full((n, d + pad), np.nan)
    wide[:, :d] = x
    xd = _dev(wide)
    st = ctx.empty((k * (1 + d + d * d) + 2,)) if stats else None
    lp = ctx.empty((n,)) if logpdf else None
    r = torch.full((n, k + rpad), -7., dtype=torch.float64, device=xd.device) if resp else None
    nb = ctx._lib.bfhip_gmm_work_bytes(n, d, k)
    assert nb > 0
    work = ctx.empty((nb,), dtype=torch.uint8)
    keep = [_dev(c[key]) for key in ('centre', 'mean', 'whiten', 'logc')]
    lw = None if logw is None else _dev(logw)
    _lib.check(ctx._lib.bfhip_gmm_step(ctx.handle, d, k, n, _p(xd), d + pad, _p(lw), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]),
                                       _p(st), _p(lp), _p(r), k + rpad, _p(work), nb))
    torch.cuda.synchronize()
    if resp:
        assert bool((r[:, k:] == -7.).all()), 'a write past the k columns of resp'
    return (None if st is None else _np(st)), (None if lp is None else _np(lp)), (None if r is None else _np(r[:, :k]))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


SHAPES = [(1, 1, 1), (15, 3, 2), (17, 4, 3), (255, 5, 16), (257, 16, 17), (4099, 17, 2), (257, 27, 3), (255, 64, 2), (17, 65, 3),
          (15, 128, 1), (257, 1, 32), (4099, 128, 32)]


@pytest.mark.parametrize('n,d,K', SHAPES)
def test_step_against_host(n, d, K):
    from bayesfast_amd.utils.gmm import _step_host
    for weights in (True, False):
        c = step_case(n, d, K, seed=2, weights=weights)
        hst, hlp, hr = _step_host(c['x'], c['logw'], c['centre'], c['mean'], c['whiten'], c['logc'])
        f, fst = step_bounds(c['x'], c['logw'], c['centre'], c['mean'], c['whiten'], c['logc'], hlp, hr)
        st, lp, r = raw_step(c, c['logw'])
        print('n %d d %d K %d weights %s: ratios to the bound: logpdf %.3g resp %.3g stats %.3g' % (
            n, d, K, weights, np.abs(lp - hlp).max() / f, np.abs(r - hr).max() / f, (np.abs(st - hst) / np.maximum(fst, 1e-300)).max()))
        assert np.all(np.abs(lp - hlp) <= f) and np.all(np.abs(r - hr) <= f)
        assert np.all(np.abs(st - hst) <= fst)
        # each output alone: the same bits
        assert same(raw_step(c, c['logw'], True, False, False)[0], st)
        assert same(raw_step(c, c['logw'], False, True, False)[1], lp)
        assert same(raw_step(c, c['logw'], False, False, True)[2], r)
        s2 = st[K * (1 + d):-2].reshape(K, d, d)
        assert np.array_equal(s2, s2.swapaxes(1, 2))


def test_wrapper_and_views():
    """``gmm_step`` on device tensors is the same call: a strided view of a wider matrix goes in as it is."""
    from bayesfast_amd.utils import gmm_step
    c = step_case(300, 5, 3, seed=3)
    st, lp, r = raw_step(c, c['logw'])
    wide = _dev(np.hstack([c['x'], np.full((300, 2), np.nan)]))
    out = gmm_step(wide[:, :5], _dev(c['logw']), _dev(c['centre']), _dev(c['mean']), _dev(c['whiten']), _dev(c['logc']))
    assert all(o.is_cuda for o in out)
    assert same(_np(out[0]), st) and same(_np(out[1]), lp) and same(_np(out[2]), r)
    only = gmm_step(wide[:, :5], None, _dev(c['centre']), _dev(c['mean']), _dev(c['whiten']), _dev(c['logc']), stats=False, resp=False)
    assert only[0] is None and only[2] is None and same(_np(only[1]), lp)
    with pytest.raises(ValueError):
        gmm_step(wide[:, :5].to('cuda').float(), None, _dev(c['centre']), _dev(c['mean']), _dev(c['whiten']), _dev(c['logc']))
    with pytest.raises(ValueError):
        gmm_step(wide[:, :5], None, _dev(c['centre']), _dev(c['mean'][:, :4]), _dev(c['whiten']), _dev(c['logc']))


def test_bitwise_properties():
    n, d, K = 1500, 27, 3
    c = step_case(n, d, K, seed=4)
    st, lp, r = raw_step(c, c['logw'])
    st2, lp2, r2 = raw_step(c, c['logw'])
    assert same(st, st2) and same(lp, lp2) and same(r, r2)
    s2 = st[K * (1 + d):-2].reshape(K, d, d)
    assert np.array_equal(s2, s2.swapaxes(1, 2))
    # rows 5..20 alone, and at an offset view of the same matrix
    _, lpa, ra = raw_step(c, None, stats=False, x=c['x'][5:21])
    assert same(lpa, lp[5:21]) and same(ra, r[5:21])
    from bayesfast_amd.utils import gmm_step
    xd = _dev(np.hstack([c['x'], np.zeros((n, 1))]))
    par = [_dev(c[key]) for key in ('centre', 'mean', 'whiten', 'logc')]
    _, lpv, rv = gmm_step(xd[5:21, :d], None, *par, stats=False)
    assert same(_np(lpv), lp[5:21]) and same(_np(rv), r[5:21])
    _, lpv, rv = gmm_step(xd[1001:1003, :d], None, *par, stats=False)
    assert same(_np(lpv), lp[1001:1003]) and same(_np(rv), r[1001:1003])


def test_value_rules():
    n, d, K = 700, 6, 3
    c = step_case(n, d, K, seed=5)
    st, lp, r = raw_step(c, c['logw'])
    # a NaN row of weight -inf leaves stats bit-identical
    lw = c['logw'].copy()
    lw[341] = -np.inf
    x0, xn = c['x'].copy(), c['x'].copy()
    x0[341] = 0.
    xn[341] = np.nan
    s0, lp0, r0 = raw_step(c, lw, x=x0)
    sn, lpn, rn = raw_step(c, lw, x=xn)
    assert np.array_equal(s0, sn) and np.isfinite(sn).all()
    assert np.isnan(lpn[341]) and np.isnan(rn[341]).all()
    assert np.array_equal(np.delete(lpn, 341), np.delete(lp0, 341)) and np.array_equal(np.delete(rn, 341, axis=0), np.delete(r0, 341, axis=0))
    for v in (np.nan, np.inf):
        lb = c['logw'].copy()
        lb[699] = v
        sb, lpb, rb = raw_step(c, lb)
        assert np.isnan(sb).all() and np.array_equal(lpb, lp) and np.array_equal(rb, r), v
        xb = c['x'].copy()
        xb[400, 2] = v
        sb, lpb, rb = raw_step(c, c['logw'], x=xb)
        assert np.isnan(sb).all() and np.isnan(lpb[400]) and np.isnan(rb[400]).all(), v
        assert np.array_equal(np.delete(lpb, 400), np.delete(lp, 400))
    # a query at distance 1e4
    far = np.full((1, d), 1e4 / np.sqrt(d))
    _, lpf, rf = raw_step(c, None, stats=False, x=far)
    assert np.isfinite(lpf[0]) and lpf[0] < -1e6 and abs(rf[0].sum() - 1.) <= 4 * np.finfo(float).eps


def test_refusals():
    """None of these launches a kernel; the context works afterwards."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    L = ctx._lib
    z = _dev(np.zeros((4, 129)))
    par = _dev(np.zeros(129 * 129 * 2))
    out, work = ctx.empty((4 * 40,)), ctx.empty((1 << 20,), dtype=torch.uint8)

    def call(d=3, k=2, n=4, ldx=None, ldr=None, wb=None, x=z, stats=out, lp=None, resp=None):
        return L.bfhip_gmm_step(ctx.handle, d, k, n, _p(x), d if ldx is None else ldx, None, _p(par), _p(par), _p(par), _p(par), _p(stats),
                                _p(lp), _p(resp), k if ldr is None else ldr, _p(work), work.numel() if wb is None else wb)
    assert call() == 0
    rc = call(d=129)
    assert rc == -4 and b'BFHIP_MAX_DIM' in L.bfhip_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert call(k=33) == -4 and b'k = 33' in L.bfhip_last_error()
    assert call(n=2**31) == -4
    assert call(ldx=2) == -1 and b'ldx = 2' in L.bfhip_last_error()
    assert call(ldr=1, resp=out) == -1 and b'ldr = 1' in L.bfhip_last_error()
    need = L.bfhip_gmm_work_bytes(4, 3, 2)
    assert call(wb=need) == 0 and call(wb=need - 1) == -1 and b'work buffer' in L.bfhip_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(wb=need - 1))
    assert call(stats=None) == -1 and b'all NULL' in L.bfhip_last_error()
    off = C.c_void_p(work.data_ptr() + 8)
    rc = L.bfhip_gmm_step(ctx.handle, 3, 2, 4, _p(z), 3, None, _p(par), _p(par), _p(par), _p(par), _p(out), None, None, 2, off, work.numel() - 8)
    assert rc == -1 and b'aligned' in L.bfhip_last_error()
    assert call(x=None) == -1 and call(n=0) == -1 and call(d=0) == -1 and call(k=0) == -1
    torch.cuda.synchronize()
    c = step_case(20, 3, 2, seed=6)
    from bayesfast_amd.utils.gmm import _step_host
    hst = _step_host(c['x'], c['logw'], c['centre'], c['mean'], c['whiten'], c['logc'])[0]
    assert np.allclose(raw_step(c, c['logw'])[0], hst, rtol=1e-12, atol=1e-15)


def _em_case(d):
    if d == 3:
        x, _ = mixture(0, 6., 4000, 3)
        return x, dict()
    x, _ = mixture(1, 4., 5000, 27)
    m0 = np.zeros((2, 27))
    m0[1, 0] = 4.
    m0 += np.random.default_rng(5).standard_normal((2, 27)) * 0.3
    return x, dict(means_init=m0)


@pytest.mark.parametrize('d', [3, 27])
def test_gmm_device_against_host(d):
    from bayesfast_amd.utils import gmm
    x, kw = _em_case(d)
    host = gmm(x, 2, seed=0, tol=0., max_iter=30, **kw)
    dev = gmm(_dev(x), 2, seed=0, tol=0., max_iter=30, **kw)
    assert dev.weights.is_cuda and dev.means.is_cuda and dev.covariances.is_cuda
    assert dev.n_iter == host.n_iter == 30 and dev.n_collapsed == host.n_collapsed == 0 and dev.neff == host.neff
    diff = max(np.abs(_np(dev.weights) - host.weights).max(), np.abs(_np(dev.means) - host.means).max(),
               np.abs(_np(dev.covariances) - host.covariances).max(), np.abs(dev.history - host.history).max())
    print('d %d: largest difference device - host of weights, means, covariances and the 30 log likelihoods: %.3g' % (d, diff))
    assert diff <= 100. * MEASURED_EM_DIFF[d]
    rh = host.responsibilities()
    sure = rh.max(axis=1) > 0.5 + 1e-9
    lab = dev.labels()
    assert lab.is_cuda and sure.sum() > 0.99 * x.shape[0] and np.array_equal(_np(lab)[sure], host.labels()[sure])
    # the fitted mixture as a density on the device: points may be arrays or tensors
    q = x[::97]
    lp = dev.logpdf(q)
    assert lp.is_cuda and np.abs(_np(lp) - host.logpdf(q)).max() <= 1e-9 and same(_np(dev.logpdf(_dev(q))), _np(lp))
    s = dev.resample(1000, seed=2)
    assert s.is_cuda and s.shape == (1000, d) and bool((s == dev.resample(1000, seed=2)).all())
    # a second fit: the same bits
    again = gmm(_dev(x), 2, seed=0, tol=0., max_iter=30, **kw)
    assert same(_np(again.means), _np(dev.means)) and same(again.history, dev.history)


def test_gmm_device_selection_and_weights():
    """A sequence of component counts and log weights on the device route pick what the host route picks."""
    from bayesfast_amd.utils import gmm
    x, _ = mixture(2, 6., 4000, 3)
    lw = -0.05 * (x**2).sum(axis=1)
    host = gmm(x, (1, 2, 3), log_weights=lw, max_iter=64)
    dev = gmm(_dev(x), (1, 2, 3), log_weights=_dev(lw), max_iter=64)
    print(dev, host)
    assert dev.n_components == host.n_components == 2 and dev.converged and host.converged
    # the host looks at the log likelihood after every iteration, the device every 8: it stops at the next multiple of 8
    assert dev.n_iter == -(-host.n_iter // 8) * 8
    assert np.allclose(dev.bic_path, host.bic_path, rtol=1e-6) and abs(dev.neff - host.neff) <= 1e-9 * host.neff
    same_count = gmm(x, 2, log_weights=lw, tol=0., max_iter=dev.n_iter)
    assert np.abs(_np(dev.means) - same_count.means).max() <= 1e-8 and abs(dev.log_likelihood - same_count.log_likelihood) <= 1e-10


@pytest.fixture(scope='module')
def short_run():
    import bayesfast_amd as bfa
    d = 4
    rng = np.random.default_rng(7)
    su = bfa.PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(alpha_p=150.))
    den = bfa.SurrogateDensity(su, input_scales=np.stack([np.full(d, -8.), np.full(d, 9.)], 1))
    xf = rng.standard_normal((4 * su.n_param, d)) * 1.5
    den.fit(xf, -0.5 * (xf**2).sum(axis=1))
    return bfa.sample(den, bfa.NTrace(n_chain=64, n_iter=70, n_warmup=20, x_0=rng.standard_normal((64, d)), random_generator=7), verbose=False)


def test_trace_gmm(short_run, monkeypatch):
    tt = short_run
    assert tt.device('samples').is_cuda
    # one component is the mean and covariance of the selected draws: the selection arguments pick what get() picks
    for sel in (dict(), dict(since_iter=30), dict(include_warmup=True), dict(original_space=False)):
        x = tt.get(flatten=True, **sel)
        g = tt.gmm(1, max_iter=2, reg_covar=0., **sel)
        assert g.means.is_cuda and g.n == x.shape[0] and g.d == 4
        mu = x.mean(axis=0)
        assert np.abs(_np(g.means[0]) - mu).max() <= 1e-12 and np.abs(_np(g.covariances[0]) - np.cov(x.T, bias=True)).max() <= 1e-12
        assert g.chain_share.shape == (64, 1) and np.array_equal(g.chain_component, np.zeros(64, dtype=np.int64)) and not g.chain_split.any()
    x = tt.get(flatten=True)
    g = tt.gmm(1, params=[2, 0], max_iter=2)
    assert g.d == 2 and np.abs(_np(g.means[0]) - x[:, [2, 0]].mean(axis=0)).max() <= 1e-12
    lw = -0.1 * (x**2).sum(axis=1)
    g = tt.gmm(2, log_weights=lw.reshape(64, 50), tol=0., max_iter=16)
    from bayesfast_amd.utils import gmm
    h = gmm(x, 2, log_weights=lw, tol=0., max_iter=16)
    assert np.abs(_np(g.means) - h.means).max() <= 1e-8
    # chain_share is the weighted mean responsibility of a chain's draws: computed here from the host fit's responsibilities
    w = np.exp(lw).reshape(64, 50, 1)
    share = (w * h.responsibilities().reshape(64, 50, 2)).sum(axis=1) / w.sum(axis=1)
    assert g.chain_share.shape == (64, 2) and np.abs(g.chain_share - share).max() <= 1e-8
    assert np.abs(g.chain_share.sum(axis=1) - 1.).max() <= 1e-12
    plain = tt.gmm(2, tol=0., max_iter=16)
    hp = gmm(x, 2, tol=0., max_iter=16)
    assert np.abs(plain.chain_share - hp.responsibilities().reshape(64, 50, 2).mean(axis=1)).max() <= 1e-8
    assert np.abs(plain.chain_share.sum(axis=1) - 1.).max() <= 1e-12
    assert np.array_equal(g.chain_component, g.chain_share.argmax(axis=1)) and np.array_equal(g.chain_split, g.chain_share.max(axis=1) < 0.9)
    from bayesfast_amd import parallel
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='ALL chains'):
        tt.gmm(2)
