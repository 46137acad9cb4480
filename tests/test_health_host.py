"""``bayesfast_amd.utils.sampler_health`` on the host: the host port against a brute-force ``np.longdouble`` reference (integers ==,
doubles to 1e-12 relative: the two-pass error is at most about n 2^-53 = 4.6e-13 at n <= 4096, and the tolerance is that doubled; the
inputs have |mean| / sd <= 1e3); what the flags mean on planted cases; ``TraceTuple.select_chains`` and ``SamplerHealth.where`` on
host parts.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import health_reference as hr  # noqa: E402
from trace_cases import same  # noqa: E402

from bayesfast_amd import _lib  # noqa: E402
from bayesfast_amd.utils import sampler_health, divergent_summary, weighted_summary, SamplerHealth  # noqa: E402


def _parts(h):
    return ({k: getattr(h, k) for k in hr.INTS}, h.depth_hist_chain, {k: getattr(h, k) for k in hr.FLOATS})


def test_tables_agree_with_the_library():
    assert hr.NSTATS == _lib.NSTATS and hr.HSTATS == _lib.HSTATS and hr.MAX_TREEDEPTH == _lib.MAX_TREEDEPTH
    assert hr.INTS == _lib.HEALTH_I and hr.FLOATS == _lib.HEALTH_F
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'bfhip.h')).read()
    for j, k in enumerate(_lib.HEALTH_I):
        assert 'BFHIP_HEALTH_I_' + k.upper() in hdr
    for k in _lib.HEALTH_F:
        assert 'BFHIP_HEALTH_F_' + k.upper() in hdr
    assert _lib.HEALTH_I_N == 20 and _lib.HEALTH_F_N == 7


@pytest.mark.parametrize('sampler', ['NUTS', 'HMC'])
@pytest.mark.parametrize('n', [2, 3, 64, 65, 257])
def test_host_port_against_longdouble_reference(sampler, n):
    rng = np.random.default_rng(100 + n)
    st = hr.random_table(rng, 7, n, sampler)
    x = 3. + rng.standard_normal((7, n, 4))
    for max_td in (10, 3):
        h = sampler_health(st, x, sampler=sampler, max_treedepth=max_td)
        assert isinstance(h, SamplerHealth) and h.sampler == sampler and h.n_rows == n and h.n_chain == 7
        hr.assert_matches(*_parts(h), hr.reference(st, sampler, max_td), where=(sampler, n, max_td))
    # the draws' moments, the totals and the shares
    xl = x.astype(np.longdouble)
    m = xl.sum(axis=1) / n
    v = ((xl - m[:, None])**2).sum(axis=1) / (n - 1)
    assert np.abs(h.chain_mean - m).max() <= 1e-12 * np.abs(m).max() and (np.abs(h.chain_var - v) <= 1e-12 * v).all()
    assert h.n_divergent_total == h.n_divergent.sum() and h.share_divergent == h.n_divergent_total / (7 * n)
    assert h.share_max_treedepth == h.n_max_treedepth.sum() / (7 * n) and h.n_leapfrog_total == h.n_leapfrog.sum()
    assert np.array_equal(h.depth_hist, h.depth_hist_chain.sum(axis=0))
    if sampler == 'NUTS':
        assert h.depth_hist.sum() == 7 * n and (h.n_accepted == 0).all()
    else:
        assert h.depth_hist.sum() == 0 and (h.n_max_treedepth == 0).all()
    # a CPU tensor is the host port too; TNUTS is read as NUTS
    import torch
    assert same(vars(sampler_health(torch.as_tensor(st), torch.as_tensor(x), sampler=sampler, max_treedepth=3))['bfmi'], h.bfmi)
    if sampler == 'NUTS':
        assert same(sampler_health(st, sampler='TNUTS', max_treedepth=3).bfmi, h.bfmi)


def test_a_chain_does_not_depend_on_the_chains_beside_it():
    rng = np.random.default_rng(3)
    st, x = hr.random_table(rng, 9, 65, 'NUTS'), rng.standard_normal((9, 65, 3))
    h = sampler_health(st, x)
    part = sampler_health(st[4:6], x[4:6])
    for k in hr.INTS + hr.FLOATS + ('chain_mean', 'chain_var', 'depth_hist_chain'):
        assert same(getattr(part, k), getattr(h, k)[4:6]), k


def test_argument_checks():
    st = np.zeros((3, 5, 11))
    for bad in (dict(stats=st[:, :, :10]), dict(stats=st[:, :1]), dict(stats=st, samples=np.zeros((3, 4, 2))),
                dict(stats=st, max_treedepth=0), dict(stats=st, max_treedepth=13), dict(stats=st, sampler='MALA')):
        with pytest.raises(ValueError):
            sampler_health(**bad)


# ---- semantics -----------------------------------------------------------------------------------------------------------------------
def _null(seed=3, n_chain=64, n=200, d=5):
    """iid and AR(1) draws, iid energies, no divergence, trees below the limit"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_chain, n, d))
    for i in range(1, n):   # the last two parameters: AR(1), rho = 0.5, unit variance
        x[:, i, 3:] = 0.5 * x[:, i - 1, 3:] + np.sqrt(0.75) * x[:, i, 3:]
    st = np.zeros((n_chain, n, 11))
    st[:, :, 0] = -0.5 * (x**2).sum(axis=2)
    st[:, :, 1] = 10. + rng.standard_normal((n_chain, n))
    st[:, :, 2], st[:, :, 3], st[:, :, 4], st[:, :, 5] = 3, 7, 0.8, 0.3
    return st, x, rng


def test_null_case_flags_nothing():
    st, x, _ = _null()
    h = sampler_health(st, x)
    assert h.ok and not h.flagged.any() and h.warnings() == []
    # (and by a margin: half of z_max, twice var_ratio_min)
    assert np.abs(h.chain_z).max() < 4 and h.var_ratio.min() > 0.2 and h.logp_z.min() > -4
    assert abs(h.bfmi_median - 2.) < 0.2 and h.bfmi_min > 1.2
    assert 'flagged 0 of 64' in str(h)


def test_bfmi_of_iid_and_of_ar1_energies():
    rng = np.random.default_rng(2)
    n = 5000
    st = np.zeros((8, n, 11))
    st[:, :, 0] = rng.standard_normal((8, n))
    e = rng.standard_normal((8, n))
    st[:4, :, 1] = e[:4]
    ar = e[4:].copy()
    for i in range(1, n):
        ar[:, i] = 0.95 * ar[:, i - 1] + np.sqrt(1. - 0.95**2) * e[4:, i]
    st[4:, :, 1] = ar
    h = sampler_health(st)
    assert (np.abs(h.bfmi[:4] - 2.) < 0.15).all() and not h.low_bfmi[:4].any()       # E (dE)^2 / var E = 2 (1 - rho)
    assert (np.abs(h.bfmi[4:] - 0.1) < 0.04).all() and h.low_bfmi[4:].all()
    assert not h.ok and any('E-BFMI' in w and 'chains 4, 5, 6, 7' in w for w in h.warnings())
    assert not sampler_health(st, bfmi_min=0.05).low_bfmi.any()


def test_stuck_chains():
    st, x, _ = _null()
    x[5] = x[5, :1]                                            # frozen: every draw the first
    st[5, :, 0], st[5, :, 1] = st[5, 0, 0], st[5, 0, 1]
    x[40, :, 2] += 20. * x[:, :, 2].mean(axis=1).std()         # 20 between-chain sd away in one parameter
    h = sampler_health(st, x)
    assert np.array_equal(np.flatnonzero(h.stuck), [5, 40]) and np.array_equal(np.flatnonzero(h.flagged), [5, 40])
    assert abs(h.chain_z[40, 2]) > 8 and h.n_moved[5] == 0 and h.var_ratio[5].max() < 1e-20 and np.isnan(h.bfmi[5]) and not h.low_bfmi[5]
    assert any('stuck' in w and 'chains 5, 40' in w for w in h.warnings())
    # a chain that moves a quarter as far as the others: its variance is a sixteenth
    st, x, _ = _null()
    x[7] = x[7].mean(axis=0) + (x[7] - x[7].mean(axis=0)) / 4.
    h = sampler_health(st, x)
    assert np.array_equal(np.flatnonzero(h.stuck), [7]) and h.var_ratio[7].max() < 0.2
    assert not sampler_health(st, x, var_ratio_min=0.02).stuck.any()
    # a chain sitting in a region of much lower density shows in logp alone
    st, x, _ = _null()
    st[9, :, 0] -= 40.
    h = sampler_health(st)
    assert h.chain_z is None and h.var_ratio is None and np.array_equal(np.flatnonzero(h.stuck), [9]) and h.logp_z[9] < -8


def test_nan_energy_is_errored_and_stays_in_its_row():
    st, x, _ = _null()
    clean = sampler_health(st, x)
    st[2, 17, 1] = np.nan
    h = sampler_health(st, x)
    assert np.array_equal(np.flatnonzero(h.errored), [2]) and h.n_nonfinite[2] == 1 and not h.ok
    for k in ('logp_mean', 'logp_var', 'energy_mean', 'energy_var', 'bfmi'):
        assert np.isnan(getattr(h, k)[2])
        assert same(np.delete(getattr(h, k), 2), np.delete(getattr(clean, k), 2)), k
    for k in hr.INTS + ('mean_accept', 'step_size', 'chain_mean', 'chain_var'):
        if k != 'n_nonfinite':
            assert same(getattr(h, k), getattr(clean, k)), k
    assert any('not finite' in w for w in h.warnings())
    st[3, 0, 0] = -np.inf
    assert np.array_equal(np.flatnonzero(sampler_health(st, x).errored), [2, 3])


def test_fewer_than_eight_chains():
    st, x, _ = _null(n_chain=7)
    x[1], st[1, :, 0] = x[1, :1], st[1, 0, 0]
    h = sampler_health(st, x)
    assert np.isnan(h.chain_z).all() and np.isnan(h.logp_z).all() and h.chain_z.shape == (7, 5)
    assert np.array_equal(np.flatnonzero(h.stuck), [1])        # the constant-chain test alone
    assert np.isfinite(h.var_ratio[0]).all()


def test_divergent_and_saturated_warnings():
    st, x, _ = _null()
    st[3, 5:9, 10] = 1.
    st[60, 100, 10] = 1.
    st[8, :, 2] = 10
    h = sampler_health(st, x)
    assert h.n_divergent_total == 5 and np.array_equal(np.flatnonzero(h.divergent), [3, 60])
    assert np.array_equal(np.flatnonzero(h.saturated), [8]) and h.n_max_treedepth[8] == 200 and h.depth_hist[10] == 200
    w = h.warnings()
    assert len(w) == 2 and '5 of 12800' in w[0] and 'divergence' in w[0] and 'chains 3, 60' in w[0]
    assert 'tree depth' in w[1] and '200 of 12800' in w[1]
    assert sampler_health(st, x, max_treedepth=12).saturated.sum() == 0


# ---- where() and select_chains -------------------------------------------------------------------------------------------------------
def _trace(st, x, warmup=20):
    from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple
    n_chain, n = st.shape[:2]
    return TraceTuple(NTrace(n_chain=n_chain, n_iter=n, n_warmup=warmup, max_treedepth=6), x, st, 10. * x + 1., st[:, :, 0] - 1.)


def test_where_is_the_weighted_summary_of_the_divergent_rows():
    st, x, rng = _null()
    tt = _trace(st, x)
    assert tt.health().where(tt) is None and divergent_summary(x, st) is None
    mask = rng.uniform(size=st.shape[:2]) < 0.03
    mask[:, :20] = False
    st[:, :, 10] = mask
    x[mask] += 1.5
    tt = _trace(st, x)
    for sel in (dict(), dict(since_iter=50), dict(original_space=False)):
        h = tt.health(**sel)
        xs = tt.get(flatten=False, **sel)
        w = mask[:, sel.get('since_iter', 20):].astype(np.float64)
        got = h.where(tt)
        assert got.n_divergent == int(w.sum()) == h.n_divergent_total
        assert same(got.summary, weighted_summary(xs, weights=w))
        flat = xs.reshape(-1, 5)
        want = (flat[w.reshape(-1) > 0].mean(axis=0) - flat.mean(axis=0)) / flat.std(axis=0, ddof=1)
        assert np.allclose(got.shift, want, rtol=1e-9, atol=0) and (got.shift > 1.).all()
        assert same(h.where(xs), got) and same(divergent_summary(xs, st[:, sel.get('since_iter', 20):]), got)


def test_trace_health_selects_as_the_other_readers():
    st, x, _ = _null()
    st[4, 3, 10] = 1.                                           # a divergence in the warm-up
    st[:, :, 2] = 6
    tt = _trace(st, x)
    assert 'health' not in tt.READERS and tt.SAMPLER_READERS == ('health',)
    h = tt.health()
    assert h.n_rows == 180 and h.n_divergent_total == 0 and h.saturated.all() and h.max_treedepth == 6
    assert same(vars(h)['bfmi'], sampler_health(st[:, 20:], 10. * x[:, 20:] + 1., max_treedepth=6).bfmi)
    assert same(h.chain_mean, sampler_health(st[:, 20:], 10. * x[:, 20:] + 1.).chain_mean)
    assert tt.health(include_warmup=True).n_divergent_total == 1 and tt.health(since_iter=3).n_divergent[4] == 1
    assert same(tt.health(original_space=False).chain_mean, sampler_health(st[:, 20:], x[:, 20:]).chain_mean)
    assert tt.health(bfmi_min=5.).low_bfmi.all()
    with pytest.raises(ValueError, match='since_iter is too large. Nothing to return.'):
        tt.health(since_iter=199)
    info = {}
    tt.health(stats=info)
    assert info == dict(collectives=0, wire_bytes=0)


def test_select_chains(monkeypatch):
    from bayesfast_amd import parallel
    st, x, _ = _null()
    x[5] = x[5, :1]
    tt = _trace(st, x)
    h = tt.health()
    good = tt.select_chains(~h.flagged)
    keep = np.flatnonzero(~h.flagged)
    assert keep.size == 63 and good.n_chain == len(good) == 63 and tt.n_chain == 64 and good._chains is None
    assert good.sampler == 'NUTS' and good.n_warmup == 20 and good.i_iter == 200
    for kw in (dict(), dict(original_space=False), dict(return_type='logp'), dict(since_iter=0)):
        assert same(good.get(flatten=False, **kw), np.ascontiguousarray(tt.get(flatten=False, **kw)[keep]))
    assert same(good.stat('tree_size'), tt.stat('tree_size')[keep])
    assert good.health().ok
    from bayesfast_amd.utils import summary
    assert same(good.summary(), summary(tt.get(flatten=False)[keep]))
    idx = tt.select_chains([3, -1, 3])
    assert same(idx.get(flatten=False), tt.get(flatten=False)[[3, 63, 3]])
    import torch
    tensors = _trace(torch.as_tensor(st), torch.as_tensor(x)).select_chains(keep)
    assert same(tensors.get(flatten=False), good.get(flatten=False))
    with pytest.raises(ValueError):
        tt.select_chains(np.zeros(64, dtype=bool))
    with pytest.raises(ValueError):
        tt.select_chains(np.ones(63, dtype=bool))
    with pytest.raises(IndexError):
        tt.select_chains([64])
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r'gather\(\)'):
        tt.select_chains(keep)


def test_seam_forwards_health():
    from oracle import reference
    if not reference.is_built():
        pytest.skip('needs the reference built into oracle/_ref by build()')
    from bayesfast_amd import integrate
    st, x, _ = _null()
    st[3, 50, 10] = 1.
    inner = _trace(st, x)
    tt = integrate.reference_classes(reference.load()).TraceTuple(inner, None)
    assert tt.health.__doc__ == type(inner).health.__doc__
    for sel in (dict(), dict(since_iter=60, bfmi_min=5.)):
        a, b = tt.health(**sel), inner.health(**sel)
        for k in hr.INTS + hr.FLOATS + ('chain_mean', 'chain_z', 'flagged'):
            assert same(getattr(a, k), getattr(b, k)), k
    assert tt.health().n_divergent_total == 1
