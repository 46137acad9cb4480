"""bfhip_health_chains (csrc/bfhip_health.hip) called directly and held to the plain ``np.longdouble`` reference of
helpers/health_reference.py (integers ==, doubles to 1e-12 relative: the two-pass error is at most about n 2^-53 = 4.6e-13 at
n <= 4096, and the tolerance is that doubled); its independence of the launch (a chain alone, in a batch, at another index: the same
bits); the device route of ``sampler_health`` against the host port; and one real run through ``sample()``.

Every table goes in as a view of a longer one (row0 > 0, a chain stride beyond its rows) with NaN everywhere outside the selected
rows, and every output is a slice of a larger buffer filled with a sentinel that has to survive outside the documented size."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import health_reference as hr  # noqa: E402
from trace_cases import same  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS = (2, 3, 63, 64, 65, 255, 256, 257, 1000)
N_CHAIN = (1, 5, 257)
ROW0, TAIL = 3, 2                  # rows of the longer table before and after the selected ones
GUARD = 64
SENTINEL = 0x7FF8DEADBEEF1234      # as int64 and, read as a float64, a quiet NaN with a payload of its own
MAX_TD = 10


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _place(ctx, st):
    """st (C, n, 11) as rows ROW0 .. ROW0 + n of a (C, ROW0 + n + TAIL, 11) device table of NaN -> (whole, view)."""
    import torch
    c, n = st.shape[:2]
    whole = np.full((c, ROW0 + n + TAIL, 11), np.nan)
    whole[:, ROW0:ROW0 + n] = st
    whole = torch.as_tensor(whole, device=ctx.device)
    return whole, whole[:, ROW0:ROW0 + n]


def _launch(ctx, view, n_chain, sampler, max_td=MAX_TD, chain0=0):
    """chains chain0 .. chain0 + n_chain of the device view -> (itab (n_chain, I_N) int64, ftab (n_chain, F_N) float64)"""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    n = int(view.shape[1])
    assert view.stride(2) == 1 and view.stride(1) == 11 and view.stride(0) > 11 * n
    oi = torch.full((n_chain * _lib.HEALTH_I_N + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=ctx.device)
    of = torch.full((n_chain * _lib.HEALTH_F_N + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=ctx.device)
    first = view[chain0:]
    _lib.check(ctx._lib.bfhip_health_chains(ctx.handle, n_chain, n, int(view.stride(0)), _ptr(first), int(sampler == 'HMC'), max_td,
                                            _ptr(oi[GUARD:]), _ptr(of[GUARD:])))
    oi, of = oi.cpu().numpy(), of.cpu().numpy()
    for o in (oi, of):
        assert np.all(o[:GUARD] == SENTINEL) and np.all(o[-GUARD:] == SENTINEL), 'written outside the table'
    return (oi[GUARD:-GUARD].reshape(n_chain, _lib.HEALTH_I_N).copy(),
            of[GUARD:-GUARD].view(np.float64).reshape(n_chain, _lib.HEALTH_F_N).copy())


def _split(itab, ftab):
    from bayesfast_amd import _lib
    k = len(_lib.HEALTH_I)
    return ({name: itab[:, j] for j, name in enumerate(_lib.HEALTH_I)}, itab[:, k:], {name: ftab[:, j] for j, name in enumerate(_lib.HEALTH_F)})


_TABLES = {}


def _table(sampler, n):
    """257 chains of n rows, their reference, and the device view: made once per (sampler, n) and left unchanged."""
    if (sampler, n) not in _TABLES:
        rng = np.random.default_rng(1000 * (sampler == 'HMC') + n)
        st = hr.random_table(rng, max(N_CHAIN), n, sampler)
        if sampler == 'NUTS':      # the ends of the depth range and the largest tree, wherever the draw did not put them
            st[0, 0, 2], st[0, 0, 3] = 0, 1
            st[0, n - 1, 2], st[0, n - 1, 3] = 12, 4095
        _TABLES[(sampler, n)] = (st, hr.reference(st, sampler, MAX_TD), _place(_ctx(), st))
    return _TABLES[(sampler, n)]


@pytest.mark.parametrize('sampler', ['NUTS', 'HMC'])
@pytest.mark.parametrize('n', N_ROWS)
def test_kernel_against_longdouble_reference(sampler, n):
    ctx = _ctx()
    st, ref, (whole, view) = _table(sampler, n)
    for n_chain in N_CHAIN:
        itab, ftab = _launch(ctx, view, n_chain, sampler)
        hr.assert_matches(*_split(itab, ftab), {k: v[:n_chain] for k, v in ref.items()}, where=(sampler, n, n_chain))
    if sampler == 'NUTS':
        assert ref['max_tree_size'][0] == 4095 and ref['depth_hist'][0, 0] >= 1 and ref['depth_hist'][0, 12] >= 1
        # another limit: the count moves, nothing else does
        it3, ft3 = _launch(ctx, view, 5, sampler, max_td=3)
        assert np.array_equal(it3[:, 1], (st[:5, :, 2] >= 3).sum(axis=1)) and same(np.delete(it3, 1, axis=1), np.delete(itab[:5], 1, axis=1))
        assert same(ft3, ftab[:5])


def test_argument_errors():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    st = torch.zeros((2, 4, 11), dtype=torch.float64, device=ctx.device)
    oi = torch.zeros((2, _lib.HEALTH_I_N), dtype=torch.int64, device=ctx.device)
    of = torch.zeros((2, _lib.HEALTH_F_N), dtype=torch.float64, device=ctx.device)
    f = ctx._lib.bfhip_health_chains
    good = [ctx.handle, 2, 4, 44, _ptr(st), 0, 10, _ptr(oi), _ptr(of)]
    assert f(*good) == 0
    for pos, bad in ((1, 0), (2, 1), (3, 43), (4, None), (5, 2), (6, 0), (6, 13), (7, None), (8, None)):
        args = list(good)
        args[pos] = bad
        assert f(*args) == -1, (pos, bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize('sampler', ['NUTS', 'HMC'])
def test_a_chain_has_the_same_bits_alone_in_a_batch_and_at_another_index(sampler):
    import torch
    ctx = _ctx()
    for n in (65, 1000):
        st, _, (whole, view) = _table(sampler, n)
        batch = _launch(ctx, view, 257, sampler)
        again = _launch(ctx, view, 257, sampler)
        assert same(batch[0], again[0]) and same(batch[1], again[1])
        for c in (0, 3, 256):
            alone = _launch(ctx, view, 1, sampler, chain0=c)
            assert same(alone[0][0], batch[0][c]) and same(alone[1][0], batch[1][c]), (n, c)
        some = _launch(ctx, view, 5, sampler, chain0=100)
        assert same(some[0], batch[0][100:105]) and same(some[1], batch[1][100:105])
        # chains 3 and 256 change places
        other = whole.clone()
        other[3], other[256] = whole[256], whole[3]
        moved = _launch(ctx, other[:, ROW0:ROW0 + n], 257, sampler)
        perm = np.arange(257)
        perm[3], perm[256] = 256, 3
        assert same(moved[0], batch[0][perm]) and same(moved[1], batch[1][perm])
    torch.cuda.synchronize()


def test_a_nan_energy_stays_in_its_chain():
    ctx = _ctx()
    for sampler in ('NUTS', 'HMC'):
        st, _, (whole, view) = _table(sampler, 257)
        clean = _launch(ctx, view, 5, sampler)
        dirty = whole.clone()
        dirty[2, ROW0 + 256, 1] = float('nan')
        itab, ftab = _launch(ctx, dirty[:, ROW0:ROW0 + 257], 5, sampler)
        keep = [0, 1, 3, 4]
        assert same(itab[keep], clean[0][keep]) and same(ftab[keep], clean[1][keep])
        assert itab[2, 5] == 1 and same(np.delete(itab[2], 5), np.delete(clean[0][2], 5))
        assert np.isnan(ftab[2, 1:6]).all() and same(ftab[2, [0, 6]], clean[1][2, [0, 6]])
        # an infinite logp as well; and a constant energy: bfmi is NaN, the rest is not
        dirty = whole.clone()
        dirty[1, ROW0, 0] = float('-inf')
        dirty[3, :, 1] = 520.1
        itab, ftab = _launch(ctx, dirty[:, ROW0:ROW0 + 257], 5, sampler)
        assert itab[1, 5] == 1 and np.isnan(ftab[1, 1:6]).all()
        assert np.isnan(ftab[3, 5]) and ftab[3, 3] == pytest.approx(520.1, rel=1e-14) and abs(ftab[3, 4]) < 1e-20 and itab[3, 5] == 0
        assert same(ftab[[0, 2, 4]], clean[1][[0, 2, 4]])


@pytest.mark.parametrize('sampler', ['NUTS', 'HMC'])
def test_device_route_equals_host_port(sampler):
    import torch
    from bayesfast_amd.utils import sampler_health
    ctx = _ctx()
    rng = np.random.default_rng(8)
    n_all, since, d = 300, 43, 5
    st = hr.random_table(rng, 12, n_all, sampler)
    x = 2. + rng.standard_normal((12, n_all, d)) * (1. + np.arange(d))
    x[7], st[7, :, 0] = x[7, :1], st[7, 0, 0]          # a frozen chain: stuck on both routes
    st_d, x_d = torch.as_tensor(st, device=ctx.device), torch.as_tensor(x, device=ctx.device)
    for lo in (0, since):
        v_st, v_x = st_d[:, lo:], x_d[:, lo:]
        assert lo == 0 or not (v_st.is_contiguous() or v_x.is_contiguous())
        dev = sampler_health(v_st, v_x, sampler=sampler, max_treedepth=7)
        host = sampler_health(st[:, lo:], x[:, lo:], sampler=sampler, max_treedepth=7)
        for k in hr.INTS + ('depth_hist_chain', 'depth_hist', 'divergent', 'saturated', 'low_bfmi', 'stuck', 'errored', 'flagged'):
            assert same(getattr(dev, k), getattr(host, k)), k
        assert dev.stuck[7] and dev.n_moved[7] == 0
        live = np.arange(12) != 7      # (the frozen chain's variances are rounding noise about 0 on either route: no relative error)
        for k in hr.FLOATS + ('chain_mean', 'chain_var'):
            a, b = getattr(dev, k), getattr(host, k)
            rows = live if k in ('logp_var', 'chain_var') else slice(None)
            assert np.all(np.abs(a[rows] - b[rows]) <= 1e-12 * np.abs(b[rows])), (k, np.abs(a[rows] / b[rows] - 1).max())
        for h in (dev, host):
            assert np.all(h.chain_var[7] <= 1e-25) and h.logp_var[7] <= 1e-20
        hr.assert_matches({k: getattr(dev, k)[live] for k in hr.INTS}, dev.depth_hist_chain[live], {k: getattr(dev, k)[live] for k in hr.FLOATS},
                          {k: v[live] for k, v in hr.reference(st[:, lo:], sampler, 7).items()}, where=(sampler, lo))
        assert np.allclose(dev.chain_z[live], host.chain_z[live], rtol=1e-9, atol=1e-9) and np.allclose(dev.logp_z, host.logp_z, rtol=1e-9, atol=1e-9)
    # the statistics alone; and where the divergences are, on the device, against the host port
    assert sampler_health(st_d[:, since:], sampler=sampler).chain_mean is None
    got, want = dev.where(x_d[:, since:]), host.where(x[:, since:])
    assert got.n_divergent == want.n_divergent == dev.n_divergent_total > 0
    assert np.allclose(got.shift, want.shift, rtol=1e-9, atol=1e-12)
    for k in ('mean', 'sd', 'q50'):
        assert np.allclose(got.summary[k], want.summary[k], rtol=1e-9, atol=1e-12), k


def test_one_real_run():
    """32 chains x 4-d Gaussian surrogate, max_treedepth = 2 and a small fixed step: every tree after the warm-up runs to the limit
    (3 leaves)."""
    import bayesfast_amd as bfa
    from bayesfast_amd.utils import summary
    d, n_chain = 4, 32
    rng = np.random.default_rng(4)
    su = bfa.PolyModel('quadratic', input_size=d, output_size=1)
    den = bfa.SurrogateDensity(su)
    xf = rng.standard_normal((8 * su.n_param, d)) * 1.5
    den.fit(xf, -0.5 * (xf**2).sum(axis=1))
    tt = bfa.sample(den, bfa.NTrace(n_chain=n_chain, n_iter=60, n_warmup=20, x_0=rng.standard_normal((n_chain, d)), random_generator=3,
                                    step_size=0.01, adapt_step_size=False, max_treedepth=2), verbose=False)
    size, depth, div = tt.stat('tree_size')[:, 20:], tt.stat('tree_depth')[:, 20:], tt.stat('diverging')[:, 20:]
    assert (size == 3).all() and (depth == 2).all()             # a saturated tree of depth 2 has 3 leaves
    h = tt.health()
    assert h.n_chain == n_chain and h.n_rows == 40 and h.max_treedepth == 2 and h.sampler == 'NUTS'
    assert np.array_equal(h.n_max_treedepth, (depth >= 2).sum(axis=1)) and np.array_equal(h.n_leapfrog, size.sum(axis=1).astype(np.int64))
    assert np.array_equal(h.n_divergent, (div != 0).sum(axis=1)) and h.n_leapfrog_total == 3 * 40 * n_chain
    assert h.saturated.all() and h.share_max_treedepth == 1. and h.depth_hist[2] == 40 * n_chain and not h.errored.any()
    assert any('tree depth' in w for w in h.warnings())
    assert np.allclose(h.logp_mean, tt.stat('logp')[:, 20:].mean(axis=1), rtol=1e-12)
    assert np.allclose(h.chain_mean, tt.get(flatten=False).mean(axis=1), rtol=1e-10, atol=1e-12)
    hw = tt.health(include_warmup=True, original_space=False)
    assert hw.n_rows == 60 and np.array_equal(hw.n_leapfrog, tt.stat('tree_size').sum(axis=1).astype(np.int64))
    idx = np.arange(0, n_chain, 2)
    half = tt.select_chains(idx)
    assert half.n_chain == 16 and half.device('samples').is_cuda and half._chains is None
    import torch
    sliced = tt.device('samples_original').index_select(0, torch.as_tensor(idx, device=tt.device('samples').device))[:, 20:]
    assert same(half.summary(), summary(sliced))
    assert same(half.get(flatten=False), tt.get(flatten=False)[idx])
    assert same(half.health().n_leapfrog, h.n_leapfrog[idx]) and same(half.health().bfmi, h.bfmi[idx])
