"""The full-rank metric's wave routines (csrc/bfhip_metric.h) at every block edge, held to tests/helpers/metric_reference.py (itself
pinned to the oracle on the CPU by tests/test_metric_host.py).

A  bf_chol_rows and bf_chol_publish through bfhip_metric_init_full at every dimension around a block edge (blocks of 16 or 8
   columns, one or two elements per lane): the factor bit for bit and against a high-precision backward bound; failing pivots.
B  the matrix state the sampler kernels leave behind (FG, BG, COV, CHOL, CHOL_ROWS, the means, the counters), replayed bit for bit
   from each chain's own samples: bf_welford_cov, the window roll, update_window > 1, the tempered driver.
C  the momentum draw (bf_solve_lt) and the velocities (bf_velocity_full*) through one or two leapfrog steps against the oracle;
   the two kernel forms (FULLM = 1 and 2) and launch cuts leave every bit alone.

Not covered here: "the reference keeps its previous factor" after a failed pivot DURING adaptation.  A Welford covariance with the
10 I prior is always positive definite, so that branch cannot be reached with valid inputs; the failed-pivot path of bf_chol_rows is
covered through part A only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))

import metric_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = mr.ONE_STEP_SEED
COV, CHOL, CHOL_ROWS, FG, BG, WORK = range(6)   # BF_MAT_*: the slots of a chain's matrices
SENTINEL = -777.25


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _same(a, b):
    return np.array_equal(mr.bits(a), mr.bits(b))


# ---- A: bfhip_metric_init_full ---------------------------------------------------------------------------------------------------

def _metric_init(ctx, d, cov0, initial_weight, n_chain=3, n_alloc=4):
    """bfhip_metric_init_full for n_chain of n_alloc allocated chains -> (mat (n_alloc, 6, d, d), sc (n_alloc, SC_N)) on the host"""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    mat = torch.full((n_alloc, _lib.MAT_N, d, d), SENTINEL, dtype=torch.float64, device=ctx.device)
    sc = torch.zeros((n_alloc, _lib.SC_N), dtype=torch.float64, device=ctx.device)
    c0 = None if cov0 is None else ctx.tensor(np.ascontiguousarray(cov0), torch.float64)
    _lib.check(ctx._lib.bfhip_metric_init_full(ctx.handle, n_chain, d, _ptr(c0), float(initial_weight), _ptr(sc), _ptr(mat)))
    ctx.synchronize()
    return mat.cpu().numpy(), sc.cpu().numpy()


def _check_inputs_written(mat, sc, cov0, w, n_chain):
    """COV, FG, BG of the initialised chains; nothing of the chains beyond them"""
    d = cov0.shape[0]
    for c in range(n_chain):
        assert _same(mat[c, COV], cov0.T), c
        assert _same(mat[c, FG], (cov0 * w).T), c
        assert _same(mat[c, BG], np.eye(d) * 10.), c
    assert np.all(mat[n_chain:] == SENTINEL) and np.all(sc[n_chain:] == 0.)


@pytest.mark.parametrize('d', mr.CHOL_DIMS)
def test_init_factorises_bit_for_bit_at_every_block_edge(ctx, d):
    from bayesfast_amd import _lib
    err = _lib.SC_FIELDS.index('error')
    w = 7.
    factors = {}
    for name, cov0 in mr.chol_matrices(d):
        L, j_fail = mr.chol_columns(cov0)
        assert j_fail is None
        mat, sc = _metric_init(ctx, d, cov0, w)
        _check_inputs_written(mat, sc, cov0, w, 3)
        assert np.all(sc[:3, err] == 0.)
        for c in range(3):
            assert _same(mat[c, CHOL], L.T), (d, name, c, np.argwhere(mr.bits(mat[c, CHOL]) != mr.bits(L.T))[:4])
            assert _same(mat[c, CHOL_ROWS], L), (d, name, c, np.argwhere(mr.bits(mat[c, CHOL_ROWS]) != mr.bits(L))[:4])
            assert _same(mat[c, CHOL_ROWS], mat[c, CHOL].T)
            assert mr.meets_backward_bound(cov0, mat[c, CHOL_ROWS]), (d, name, c)   # the device's factor, independently
        factors[name] = mat[0, CHOL]
    assert _same(factors['dense'], factors['dense_upper_junk'])   # only the lower triangle is read
    # cov0 = NULL: the identity
    mat, sc = _metric_init(ctx, d, None, w)
    _check_inputs_written(mat, sc, np.eye(d), w, 3)
    for c in range(3):
        assert _same(mat[c, CHOL], np.eye(d)) and _same(mat[c, CHOL_ROWS], np.eye(d)) and sc[c, err] == 0.


@pytest.mark.parametrize('d', mr.FAIL_DIMS)
def test_init_reports_a_failing_pivot_and_publishes_nothing(ctx, d):
    from bayesfast_amd import _lib
    err = _lib.SC_FIELDS.index('error')
    cases = mr.fail_cases(d)
    assert len(cases) == 4 + (d > 16) + (d > 66)
    for name, a, j_star in cases:
        assert mr.chol_columns(a)[1] == j_star, (d, name)   # the reference fails exactly there (also tests/test_metric_host.py)
        mat, sc = _metric_init(ctx, d, a, 10.)
        assert np.all(sc[:3, err] == 3.), (d, name, sc[:, err])
        assert np.all(mat[:3, CHOL] == SENTINEL) and np.all(mat[:3, CHOL_ROWS] == SENTINEL), (d, name)
        _check_inputs_written(mat, sc, a, 10., 3)


# ---- B: the sampler kernels' matrix state, replayed from their own samples -------------------------------------------------------------

N_ITER, N_WARMUP, ADAPT_WINDOW = 20, 18, 5
# (adapt_window = 5: the windows roll with samples 5 and 15 and the window doubles to 10 and to 20)
ROLLED_TWICE = (15, 20)   # prev_update, adapt_window after the warm-up


def _check_against_replay(dc, samples, x0, cov0, update_window, initial_weight, tag):
    """every chain's matrices, means and counters against the replay of ITS OWN warm-up samples, bit for bit"""
    mat = dc.mat.cpu().numpy()
    fld = {k: dc.field(k).cpu().numpy() for k in ('fg_mean', 'bg_mean', 'fg_n', 'bg_n', 'n_samples', 'prev_update', 'adapt_window')}
    d = x0.shape[1]
    for i in range(x0.shape[0]):
        rp = mr.FullMetricReplay(d, cov0, initial_weight=initial_weight, adapt_window=ADAPT_WINDOW, update_window=update_window,
                                 initial_mean=x0[i])
        rp.feed(samples[i, :N_WARMUP])
        assert rp.n_failed == 0 and rp.n_roll == 2 and rp.state()[3:] == ROLLED_TWICE
        got = tuple(float(fld[k][i]) for k in ('fg_n', 'bg_n', 'n_samples', 'prev_update', 'adapt_window'))
        assert got == tuple(float(v) for v in rp.state()), (tag, i, got, rp.state())
        assert got[3:] == ROLLED_TWICE   # the device's own counters: two rolls, the window doubled
        for name, slot, want in (('FG', FG, rp.fg.T), ('BG', BG, rp.bg.T), ('COV', COV, rp.cov.T), ('CHOL', CHOL, rp.chol.T),
                                 ('CHOL_ROWS', CHOL_ROWS, rp.chol)):
            assert _same(mat[i, slot], want), (tag, i, name, np.argwhere(mr.bits(mat[i, slot]) != mr.bits(want))[:4])
        assert _same(fld['fg_mean'][i], rp.fg_mean), (tag, i, 'fg_mean')
        assert _same(fld['bg_mean'][i], rp.bg_mean), (tag, i, 'bg_mean')
        assert mr.meets_backward_bound(rp.cov, mat[i, CHOL_ROWS])


def _x0(d, n_chain=3):
    return np.random.default_rng(8000 + d).normal(size=(n_chain, d)) * 0.5


_B_CASES = [(17, 'NUTS', 1, False), (40, 'NUTS', 1, False), (40, 'NUTS', 3, False), (64, 'NUTS', 1, False), (65, 'NUTS', 1, False),
            (65, 'HMC', 1, False), (100, 'NUTS', 1, False), (127, 'NUTS', 1, False), (127, 'NUTS', 3, False),
            (65, 'NUTS', 1, True), (100, 'NUTS', 1, True)]


@pytest.mark.parametrize('d,sampler,update_window,dense', _B_CASES)
def test_sampler_matrix_state_equals_the_replay_of_its_samples(ctx, d, sampler, update_window, dense):
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import correlated_gaussian_spec
    from bayesfast_amd import _lib
    spec, _ = correlated_gaussian_spec(d)
    x0 = _x0(d)
    cov0 = mr.dense_cov0(d, lo=-1., hi=1.) if dense else None
    w = 6. if dense else 10.
    dc = DeviceChains(DeviceDensity(spec, ctx), x0, seed=SEED, metric='full' if cov0 is None else cov0, initial_weight=w,
                      adapt_window=ADAPT_WINDOW)
    s, st = dc.run(N_ITER, sampler, n_warmup=N_WARMUP, max_treedepth=4, n_int_step=4, update_window=update_window)
    s, st = s.cpu().numpy(), st.cpu().numpy()
    warm = st[:, :, (_lib.NSTATS if sampler == 'NUTS' else _lib.HSTATS).index('warmup')]
    assert warm[:, :N_WARMUP].all() and not warm[:, N_WARMUP:].any() and np.isfinite(s).all()   # every warm-up sample is output
    assert ', 0, 1>' in _lib.last_kernel(), _lib.last_kernel()
    _check_against_replay(dc, s, x0, cov0, update_window, w, (d, sampler, update_window, dense))


@pytest.mark.parametrize('d,update_window', [(12, 1), (70, 1), (70, 3)])
def test_tempered_matrix_state_equals_the_replay_of_its_samples(ctx, d, update_window):
    """the tempered chain driver (bfhip_tnuts_chain.h) calls the same helpers through tn_each"""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, _ = correlated_gaussian_spec(d)
    x0 = _x0(d) * 0.6
    u0 = np.random.default_rng(d).normal(size=x0.shape[0])
    dc = DeviceChains(DeviceDensity(spec, ctx), x0, seed=SEED, metric='full', adapt_window=ADAPT_WINDOW)
    s, st, stt = dc.run_tempered(N_ITER, np.zeros(d), np.eye(d) * 1.5, logxi=0.2, u_0=u0, n_warmup=N_WARMUP, max_treedepth=4,
                                 update_window=update_window)
    s = s.cpu().numpy()
    assert np.isfinite(s).all()
    _check_against_replay(dc, s, x0, None, update_window, 10., ('tempered', d, update_window))


# ---- C: momentum draw, velocities, the two kernel forms, launch cuts -------------------------------------------------------------

def _run_dict(dc, n, sampler, **kw):
    from bayesfast_amd import _lib
    s, st = dc.run(n, sampler, **kw)
    st = st.cpu().numpy()
    names = _lib.NSTATS if sampler == 'NUTS' else _lib.HSTATS
    return s.cpu().numpy(), {k: st[:, :, i] for i, k in enumerate(names)}


@pytest.mark.parametrize('d', mr.ONE_STEP_DIMS)
def test_one_and_two_steps_with_a_dense_fixed_metric_match_oracle(ctx, d):
    """One momentum draw through CHOL_ROWS and one or two leapfrog steps through COV per iteration, from a dense and badly scaled
    covariance, in both kernel forms: a wrong row of the factor's row-major copy or a wrong column of a tail loop moves the first
    position by far more than 1e-9 (tests/test_metric_host.py shows the comparison failing on a 1e-6 change of one element)."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    case = mr.one_step_case(d)
    dens = DeviceDensity(case['spec'], ctx)
    for sampler, kw in mr.ONE_STEP_RUNS:
        want = mr.oracle_one_step(case, sampler, kw)
        assert mr.every_chain_moves(case, want[0], want[1], sampler)
        try:
            for form in (2, 1):
                _lib.debug_set('no_vel_ahead', int(form == 1))
                dc = DeviceChains(dens, case['x0'], seed=SEED, step_size=case['step_size'], metric=case['cov0'])
                got = _run_dict(dc, mr.ONE_STEP_ITERS, sampler, n_warmup=0, adapt_step_size=False, adapt_metric=False, **kw)
                assert ', 0, %d>' % form in _lib.last_kernel(), _lib.last_kernel()
                mr.one_step_compare(got, want, sampler)
                assert mr.every_chain_moves(case, got[0], got[1], sampler)
        finally:
            _lib.debug_set('no_vel_ahead', 0)


@pytest.mark.parametrize('d', [8, 64, 100])
def test_velocity_ahead_form_changes_no_bit(ctx, d):
    """bfhip_tune.h lists no_vel_ahead among the choices that give the same results: FULLM = 2 (bf_velocity_full2, the next step's
    velocity taken with this one's) against FULLM = 1, with a fixed metric and after an adaptive warm-up."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import correlated_gaussian_spec
    from bayesfast_amd import _lib
    spec, _ = correlated_gaussian_spec(d)
    dens = DeviceDensity(spec, ctx)
    x0 = _x0(d)
    cov0 = mr.dense_cov0(d, lo=-0.5, hi=0.5)
    fixed, adaptive = {}, {}
    try:
        for off in (1, 0):
            _lib.debug_set('no_vel_ahead', off)
            dc = DeviceChains(dens, x0, seed=SEED, metric=cov0)
            fixed[off] = _run_dict(dc, 10, 'NUTS', n_warmup=6, max_treedepth=4, adapt_metric=False)
            assert ', 0, %d>' % (1 if off else 2) in _lib.last_kernel(), _lib.last_kernel()
            # adaptive: a launch that adapts (form 1 always), then one that starts after the warm-up (form 2 unless switched off)
            dc = DeviceChains(dens, x0, seed=SEED, metric='full', adapt_window=ADAPT_WINDOW)
            a = _run_dict(dc, 8, 'NUTS', n_warmup=8, max_treedepth=4)
            assert ', 0, 1>' in _lib.last_kernel(), _lib.last_kernel()
            b = _run_dict(dc, 6, 'NUTS', n_warmup=8, max_treedepth=4)
            assert ', 0, %d>' % (1 if off else 2) in _lib.last_kernel(), _lib.last_kernel()
            adaptive[off] = (a, b, dc.mat.cpu().numpy())
    finally:
        _lib.debug_set('no_vel_ahead', 0)
    assert _same(fixed[0][0], fixed[1][0])
    for f in fixed[0][1]:
        assert _same(fixed[0][1][f], fixed[1][1][f]), f
    for part in (0, 1):
        assert _same(adaptive[0][part][0], adaptive[1][part][0])
        for f in adaptive[0][part][1]:
            assert _same(adaptive[0][part][1][f], adaptive[1][part][1][f]), f
    assert _same(adaptive[0][2], adaptive[1][2])
    assert not np.array_equal(fixed[0][0][:, 0], fixed[0][0][:, -1])   # (the chains moved)


def test_launch_cuts_change_no_bit_of_the_adaptive_state_at_d100(ctx):
    """One launch against launches cut inside the warm-up -- one of them right after the first roll (sample 5) --, at its end and
    after it: samples, statistics and all six matrices of every chain."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import correlated_gaussian_spec
    d = 100
    spec, _ = correlated_gaussian_spec(d)
    dens = DeviceDensity(spec, ctx)
    x0 = _x0(d)
    out = {}
    for name, cuts in (('whole', None), ('cut', [6, 5, 7, 2]), ('cut2', [3, 13, 2, 2])):
        dc = DeviceChains(dens, x0, seed=SEED, metric='full', adapt_window=ADAPT_WINDOW)
        s, st = _run_dict(dc, N_ITER, 'NUTS', n_warmup=N_WARMUP, max_treedepth=4, launch_iters=cuts)
        out[name] = (s, st, dc.mat.cpu().numpy(), dc.sc.cpu().numpy(), dc.vec.cpu().numpy())
    assert tuple(out['whole'][3][0, [8, 9]]) == ROLLED_TWICE   # (SC_FIELDS: prev_update, adapt_window)
    for name in ('cut', 'cut2'):
        assert _same(out['whole'][0], out[name][0])
        for f in out['whole'][1]:
            assert _same(out['whole'][1][f], out[name][1][f]), (name, f)
        for k in (2, 3, 4):
            assert _same(out['whole'][k], out[name][k]), (name, k)
