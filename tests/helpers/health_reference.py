"""The brute-force reference of the sampler health figures (tests/test_health_host.py, tests/test_gpu_health.py): ``np.longdouble``, a
plain Python loop over the rows (every chain's accumulators side by side), variances by a second pass about the mean; and the random
statistics tables the tests feed to it."""
import numpy as np

MAX_TREEDEPTH = 12
NSTATS = ('logp', 'energy', 'tree_depth', 'tree_size', 'mean_tree_accept', 'step_size', 'step_size_bar', 'warmup', 'energy_change',
          'max_energy_change', 'diverging')
HSTATS = ('logp', 'energy', 'n_int_step', 'accept_stat', 'accepted', 'step_size', 'step_size_bar', 'warmup', 'energy_change',
          'diverging')
INTS = ('n_divergent', 'n_max_treedepth', 'n_leapfrog', 'max_tree_size', 'n_accepted', 'n_nonfinite', 'n_moved')
FLOATS = ('mean_accept', 'logp_mean', 'logp_var', 'energy_mean', 'energy_var', 'bfmi', 'step_size')


def random_table(rng, n_chain, n, sampler):
    """(n_chain, n, 11) float64 in the layout of ``sampler``: logp and energy with |mean| / sd of 700 and 400, depths over the whole
    range 0 .. 12 with trees of up to 4095 leaves, one row in ten divergent."""
    st = np.zeros((n_chain, n, 11))
    it = HSTATS if sampler == 'HMC' else NSTATS
    st[:, :, it.index('logp')] = -490. + 0.7 * rng.standard_normal((n_chain, n))
    st[:, :, it.index('energy')] = 520. + 1.3 * rng.standard_normal((n_chain, n))
    st[:, :, it.index('step_size')] = rng.uniform(0.01, 1., (n_chain, n))
    st[:, :, it.index('step_size_bar')] = rng.uniform(0.01, 1., (n_chain, n))
    st[:, :, it.index('energy_change')] = rng.standard_normal((n_chain, n))
    st[:, :, it.index('diverging')] = rng.uniform(size=(n_chain, n)) < 0.1
    if sampler == 'HMC':
        st[:, :, it.index('n_int_step')] = rng.integers(1, 65, (n_chain, n))
        st[:, :, it.index('accept_stat')] = rng.uniform(size=(n_chain, n))
        st[:, :, it.index('accepted')] = rng.uniform(size=(n_chain, n)) < 0.7
    else:
        depth = rng.integers(0, MAX_TREEDEPTH + 1, (n_chain, n))
        st[:, :, it.index('tree_depth')] = depth
        st[:, :, it.index('tree_size')] = 2**depth - 1 + (depth == 0)      # (depth 12: 4095 leaves)
        st[:, :, it.index('mean_tree_accept')] = rng.uniform(size=(n_chain, n))
        st[:, :, it.index('max_energy_change')] = rng.standard_normal((n_chain, n))
    return st


def reference(st, sampler, max_treedepth):
    """dict: the INTS as int64 (n_chain,), 'depth_hist' (n_chain, 13), the FLOATS as longdouble (n_chain,)."""
    L = np.longdouble
    st = np.asarray(st, dtype=np.float64)
    n_c, n = st.shape[:2]
    hmc = sampler == 'HMC'
    it = HSTATS if hmc else NSTATS
    k = {name: it.index(name) for name in it}
    ints = {name: np.zeros(n_c, dtype=np.int64) for name in INTS}
    hist = np.zeros((n_c, MAX_TREEDEPTH + 1), dtype=np.int64)
    s_acc, s_lp, s_en, s_de = (np.zeros(n_c, dtype=L) for _ in range(4))
    every = np.arange(n_c)
    with np.errstate(all='ignore'):
        for i in range(n):
            row = st[:, i, :].astype(L)
            ints['n_divergent'] += row[:, k['diverging']] != 0
            size = row[:, k['n_int_step' if hmc else 'tree_size']].astype(np.int64)
            ints['n_leapfrog'] += size
            ints['max_tree_size'] = np.maximum(ints['max_tree_size'], size)
            ints['n_nonfinite'] += ~(np.isfinite(row[:, k['logp']]) & np.isfinite(row[:, k['energy']]))
            if hmc:
                ints['n_accepted'] += row[:, k['accepted']] != 0
            else:
                dp = row[:, k['tree_depth']]
                ints['n_max_treedepth'] += dp >= max_treedepth
                inside = (dp >= 0) & (dp <= MAX_TREEDEPTH)
                hist[every, np.where(inside, np.floor(np.where(inside, dp, 0)), MAX_TREEDEPTH).astype(np.int64)] += 1
            s_acc += row[:, k['accept_stat' if hmc else 'mean_tree_accept']]
            s_lp += row[:, k['logp']]
            s_en += row[:, k['energy']]
            if i > 0:
                ints['n_moved'] += st[:, i, k['logp']] != st[:, i - 1, k['logp']]
                s_de += (row[:, k['energy']] - st[:, i - 1, k['energy']].astype(L))**2
        m_lp, m_en = s_lp / n, s_en / n
        q_lp, q_en = np.zeros(n_c, dtype=L), np.zeros(n_c, dtype=L)
        for i in range(n):
            q_lp += (st[:, i, k['logp']].astype(L) - m_lp)**2
            q_en += (st[:, i, k['energy']].astype(L) - m_en)**2
        out = dict(ints, depth_hist=hist, mean_accept=s_acc / n, logp_mean=m_lp, logp_var=q_lp / (n - 1), energy_mean=m_en,
                   energy_var=q_en / (n - 1), bfmi=np.where(s_de == 0, L('nan'), s_de / q_en), step_size=st[:, -1, k['step_size']].astype(L))
        bad = ints['n_nonfinite'] > 0
        for name in ('logp_mean', 'logp_var', 'energy_mean', 'energy_var', 'bfmi'):
            out[name] = np.where(bad, L('nan'), out[name])
    return out


def assert_matches(got_i, got_hist, got_f, ref, rtol=1e-12, where=''):
    """got_i: dict name -> (n_chain,) ints; got_hist (n_chain, 13); got_f: dict name -> (n_chain,) float64.  Integers ==; doubles
    within ``rtol`` relative, a NaN where the reference has one."""
    for name in INTS:
        assert np.array_equal(np.asarray(got_i[name], dtype=np.int64), ref[name]), (where, name)
    assert np.array_equal(np.asarray(got_hist, dtype=np.int64), ref['depth_hist']), (where, 'depth_hist')
    for name in FLOATS:
        g, r = np.asarray(got_f[name], dtype=np.longdouble), ref[name]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (where, name)
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok]) / np.abs(r[ok])
        assert (err <= rtol).all(), (where, name, float(err.max()))
