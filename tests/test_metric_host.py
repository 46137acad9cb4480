"""tests/helpers/metric_reference.py pinned on the CPU, before tests/test_gpu_metric_full.py holds the kernels to it: the replay of
``QuadMetricFullAdapt.update`` against the oracle's chains bit for bit, the Cholesky restatement against an independent
high-precision backward bound, the failing pivots where they are meant to be, and the sensitivity of the two comparisons the GPU
tests rely on (the bound rejects one element moved by 1e-10 relative, the one-step comparison one moved by 1e-6)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))

import metric_reference as mr  # noqa: E402


@pytest.mark.parametrize('update_window', [1, 3])
@pytest.mark.parametrize('d', [7, 20, 70])
def test_replay_equals_the_oracles_matrices_bit_for_bit(d, update_window):
    """The oracle's NUTS chain with the adaptive full-rank metric (adapt_window = 5: rolls after samples 5 and 16, the window
    doubled each time), its warm-up samples replayed."""
    from bayesfast_amd.workloads import correlated_gaussian_spec
    from oracle import oracle as orc
    spec, _ = correlated_gaussian_spec(d)
    n_iter, n_warmup = 23, 20
    for stream, cov0 in ((0, None), (1, mr.dense_cov0(d, lo=-0.5, hi=0.5))):
        x0 = np.random.default_rng(70 + d + stream).normal(size=d) * 0.5
        metric = 'full' if cov0 is None else cov0
        ch = orc.Chain(x0, metric=metric, adapt_window=5, update_window=update_window, initial_weight=7.)
        s, st = orc.nuts_run(spec, ch, orc.make_rng('xoshiro', seed=11, stream=stream), n_iter, n_warmup, max_treedepth=4)
        assert st['warmup'][:n_warmup].all() and not st['warmup'][n_warmup:].any()
        rp = mr.FullMetricReplay(d, cov0, initial_weight=7., adapt_window=5, update_window=update_window, initial_mean=x0)
        rp.feed(s[:n_warmup])
        assert rp.n_roll == 2 and rp.state()[4] == 20 and rp.n_failed == 0   # two rolls, the window doubled twice
        assert rp.n_refresh == {1: 20, 3: 6}[update_window]
        for name, mine in (('cov', rp.cov), ('chol', rp.chol), ('fg_cov', rp.fg), ('bg_cov', rp.bg)):
            assert np.array_equal(mr.bits(mine), mr.bits(ch.mat(name))), (d, update_window, name)
        for name, mine in (('fg_mean', rp.fg_mean), ('bg_mean', rp.bg_mean)):
            assert np.array_equal(mr.bits(mine), mr.bits(ch.vec(name))), (d, update_window, name)
        assert rp.state() == (ch.scalar('fg_n'), ch.scalar('bg_n'), ch.scalar('n_samples'), ch.scalar('previous_update'),
                              ch.scalar('adapt_window'))


@pytest.mark.parametrize('d', mr.CHOL_DIMS)
def test_chol_columns_meets_the_backward_bound(d):
    for name, a in mr.chol_matrices(d):
        L, j_fail = mr.chol_columns(a)
        assert j_fail is None, (d, name)
        assert np.all(np.triu(L, 1) == 0.) and np.all(np.diag(L) > 0.)
        assert mr.meets_backward_bound(a, L), (d, name)
    # only the lower triangle is read
    (_, dense), (_, junk) = mr.chol_matrices(d)[1:]
    assert np.array_equal(mr.bits(mr.chol_columns(dense)[0]), mr.bits(mr.chol_columns(junk)[0]))
    if d > 1:
        assert not np.array_equal(np.triu(dense, 1), np.triu(junk, 1))


@pytest.mark.parametrize('d', [2, 17, 64, 65, 100, 128])
def test_backward_bound_rejects_one_element_moved_by_1e_10(d):
    """A correct factor passes; the same factor with ONE element moved by 1e-10 relative does not -- any diagonal element and
    any element of the first column, of both kinds of matrix (the bound is a few 1e-14 of |L||L|^T, element by element)."""
    rng = np.random.default_rng(d)
    for name, a in mr.chol_matrices(d)[:2]:
        L, _ = mr.chol_columns(a)
        assert mr.meets_backward_bound(a, L)
        picks = [(0, 0), (d - 1, d - 1), (d // 2, d // 2), (d - 1, 0), (d // 2, 0)]
        picks += [(int(i), int(i)) for i in rng.integers(0, d, size=3)]
        for i, j in picks:
            bad = L.copy()
            bad[i, j] *= 1. + 1e-10
            assert bad[i, j] != L[i, j]
            assert not mr.meets_backward_bound(a, bad), (d, name, i, j)


@pytest.mark.parametrize('d', mr.FAIL_DIMS)
def test_chol_columns_fails_at_the_intended_column(d):
    cases = mr.fail_cases(d)
    names = {c[0] for c in cases}
    assert {'first', 'inside_block', 'last', 'nan_diagonal'} <= names
    assert ('second_block' in names) == (d > 16) and ('odd_past_64' in names) == (d > 66)
    for name, a, j_star in cases:
        L, j_fail = mr.chol_columns(a)
        assert j_fail == j_star, (d, name, j_fail, j_star)
        assert np.all(L[:, j_star:] == 0.) and np.all(np.diag(L)[:j_star] > 0.)
        if name != 'nan_diagonal':   # the pivot is <= 0, not merely NaN
            good = a.copy()
            good[j_star, j_star] = 1e6
            Lg, _ = mr.chol_columns(good)
            piv = a[j_star, j_star] - float(np.sum(Lg[j_star, :j_star].astype(np.longdouble)**2))
            assert piv <= 0. and (j_star > 0 or piv == 0.), (d, name, piv)


@pytest.mark.parametrize('d', mr.ONE_STEP_DIMS)
def test_one_step_cases_move_every_chain_and_see_a_1e_6_change_of_the_factor(d):
    """Part C's runs on the oracle alone: every chain accepts at least one proposal, and the comparison the GPU test makes
    (positions, energy and energy_change to 1e-9) fails when ONE element of the covariance's factor is moved by 1e-6 relative
    -- what a wrong row of CHOL_ROWS or a wrong column of a tail loop would do, and far more."""
    case = mr.one_step_case(d)
    L, j_fail = mr.chol_columns(case['cov0'])
    assert j_fail is None
    i = int(np.argmax(np.diag(L)))
    Lp = L.copy()
    Lp[i, i] *= 1. + 1e-6
    cov_p = mr.lower_symmetric(Lp @ Lp.T)
    for sampler, kw in mr.ONE_STEP_RUNS:
        want = mr.oracle_one_step(case, sampler, kw)
        assert mr.every_chain_moves(case, want[0], want[1], sampler), (d, sampler, kw)
        mr.one_step_compare(mr.oracle_one_step(case, sampler, kw), want, sampler)   # (the oracle repeats itself exactly)
        with pytest.raises(AssertionError):
            mr.one_step_compare(mr.oracle_one_step(case, sampler, kw, cov0=cov_p), want, sampler)
