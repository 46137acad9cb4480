"""The full-rank metric's matrices restated in plain NumPy (TEST INFRASTRUCTURE ONLY): the left-looking Cholesky factorisation of
``csrc/bfhip_metric.h`` (``bf_chol_rows``), an independent high-precision bound on its backward error, and
``QuadMetricFullAdapt.update`` (``samplers/hmc_utils/metrics.py:294-324``) as the sampler kernels evaluate it.

The header writes its arithmetic "with explicit non-fused multiplies and adds in the order of the CPU restatement".  NumPy's float64
ufuncs round once per operation, so every statement below rounds exactly as the header promises to: given the positions a chain
visited, the matrices are a deterministic element-wise function of them, and the tests want every bit.
``tests/test_metric_host.py`` pins this module to the oracle (``oracle/bf_oracle.c``) before anything on the GPU is held to it.

Matrices here are in their natural orientation, ``M[i][j]``; the device stores every one of them transposed (``MT[k * d + i] =
M[i][k]``) but for the row-major copy of the factor."""
import numpy as np

from adapt_reference import MetricWindow

U = 2.**-53   # unit roundoff of float64


def chol_columns(a):
    """Left-looking Cholesky, ``a = L L^T``, in float64 with one rounding per operation.  Only the lower triangle of ``a`` is read.
    For column j the terms ``L[i][k] * L[j][k]`` are subtracted for k = 0 .. j - 1 in this order (all rows i >= j at once), then the
    pivot's square root is taken and the rest of the column divided by it.  Returns ``(L, j_fail)``: ``j_fail`` is the first column
    whose pivot is not ``> 0`` (a NaN included; the columns before it are finished, the rest of ``L`` is zero), or None."""
    a = np.asarray(a, dtype=np.float64)
    d = a.shape[0]
    if a.shape != (d, d):
        raise ValueError('a should be square.')
    L = np.zeros((d, d))
    for j in range(d):
        col = a[j:, j].copy()
        for k in range(j):
            col = col - L[j:, k] * L[j, k]
        s = col[0]
        if not (s > 0.):
            return L, j
        ljj = np.sqrt(s)
        L[j, j] = ljj
        L[j + 1:, j] = col[1:] / ljj
    return L, None


def lower_symmetric(a):
    """the symmetric matrix that a routine reading only the lower triangle of ``a`` sees"""
    a = np.asarray(a)
    return np.tril(a) + np.tril(a, -1).T


def chol_backward_bound(a, L):
    """``(residual, bound)``, both (d, d) ``np.longdouble``: the element-wise residual ``|A - L L^T|`` (A: the lower triangle of
    ``a``, mirrored) and Higham's bound on it for a factor computed in float64, ``gamma_{d+1} |L| |L|^T`` with ``gamma_n = n u /
    (1 - n u)``, ``u = 2^-53`` (Accuracy and Stability of Numerical Algorithms, theorem 10.3).  The products are summed in extended
    precision by a matrix product: nothing of the summation order of the code under test is shared."""
    A = lower_symmetric(np.asarray(a, dtype=np.float64)).astype(np.longdouble)
    Ll = np.asarray(L, dtype=np.float64).astype(np.longdouble)
    d = A.shape[0]
    n = np.longdouble(d + 1)
    u = np.longdouble(U)
    gamma = n * u / (np.longdouble(1) - n * u)
    resid = np.abs(A - Ll @ Ll.T)
    bound = gamma * (np.abs(Ll) @ np.abs(Ll).T)
    return resid, bound


def meets_backward_bound(a, L):
    resid, bound = chol_backward_bound(a, L)
    return bool(np.all(np.isfinite(resid)) and np.all(resid <= bound))


class FullMetricReplay:
    """``QuadMetricFullAdapt.update`` fed one warm-up sample at a time, as the kernels do it.  ``initial_mean``: the foreground
    window's starting mean (the chain's starting point, ``sample_trace.py:424-455``; default zero)."""

    def __init__(self, d, cov0=None, initial_weight=10., adapt_window=60, update_window=1, doubling=True, initial_mean=None):
        self.d = d
        self.cov = np.eye(d) if cov0 is None else np.array(cov0, dtype=np.float64)
        if self.cov.shape != (d, d):
            raise ValueError('cov0 should be (d, d).')
        self.chol, j_fail = chol_columns(self.cov)
        if j_fail is not None:
            raise ValueError('the input covariance is not positive definite.')
        self.fg = self.cov * float(initial_weight)
        self.bg = np.eye(d) * 10.
        self.fg_mean = np.zeros(d) if initial_mean is None else np.array(initial_mean, dtype=np.float64)
        self.bg_mean = np.zeros(d)
        self.window = MetricWindow(float(initial_weight), 10., 0, 0, adapt_window, update_window, doubling)
        self.n_refresh = self.n_roll = self.n_failed = 0

    @staticmethod
    def _add(mean, raw, n, q):
        """_WeightedCovariance.add_sample with weight 1 (metrics.py:401-407); n is the window's weight AFTER its increment"""
        od = q - mean
        mean += od / n
        nd = q - mean
        raw += (1. * nd)[:, None] * od[None, :]

    def update(self, q):
        q = np.asarray(q, dtype=np.float64)
        w = self.window
        fg_n, bg_n = w.fg_n + 1., w.bg_n + 1.   # the windows' weights for this sample: after the increment, before a roll
        refresh, roll = w.update()
        self._add(self.fg_mean, self.fg, fg_n, q)
        self._add(self.bg_mean, self.bg, bg_n, q)
        if refresh:   # _update_from_weightvar: metrics.py:287-292
            self.n_refresh += 1
            self.cov = self.fg / fg_n
            L, j_fail = chol_columns(self.cov)
            if j_fail is None:
                self.chol = L
            else:
                self.n_failed += 1
        if roll:
            self.n_roll += 1
            self.fg, self.bg = self.bg, np.eye(self.d) * 10.
            self.fg_mean, self.bg_mean = self.bg_mean, np.zeros(self.d)
        return refresh, roll

    def feed(self, samples):
        for q in np.asarray(samples, dtype=np.float64):
            self.update(q)
        return self

    def state(self):
        """(fg_n, bg_n, n_samples, prev_update, adapt_window)"""
        return self.window.state()


# ---- the matrices the factorisation is tried on (shared by the host test and the GPU test) ---------------------------------------

CHOL_DIMS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 66, 71, 72, 73, 96, 97, 127, 128)
FAIL_DIMS = (16, 40, 64, 65, 100, 128)


def spd_well(d, seed=0):
    """a well-conditioned random symmetric positive definite matrix"""
    g = np.random.default_rng(1000 + 7 * d + seed).normal(size=(d, 2 * d + 3))
    a = g @ g.T / (2 * d + 3) + 0.5 * np.eye(d)
    return lower_symmetric(a)


def spd_dense_scaled(d, seed=0):
    """dense, correlations near 0.9, standard deviations spread over 1e-4 .. 1e4 (in a shuffled order)"""
    rng = np.random.default_rng(2000 + 7 * d + seed)
    v = 1. + 0.03 * rng.normal(size=d)
    c = 0.1 * np.eye(d) + 0.9 * np.outer(v, v)
    s = 10.**(np.linspace(-4., 4., d) if d > 1 else np.zeros(1))
    s = s[rng.permutation(d)]
    return lower_symmetric(c * np.outer(s, s))


def with_unrelated_upper(a, seed=0):
    """``a`` with its strict upper triangle replaced by unrelated finite numbers"""
    d = a.shape[0]
    junk = np.random.default_rng(3000 + d + seed).normal(size=(d, d)) * 1e3
    return np.tril(a) + np.triu(junk, 1)


def chol_matrices(d):
    """[(name, matrix)] of part A at dimension d"""
    dense = spd_dense_scaled(d)
    return [('well', spd_well(d)), ('dense', dense), ('dense_upper_junk', with_unrelated_upper(dense))]


def fail_columns(d):
    """{name: j*}: column 0, column 5, the first column of the second block of bf_chol_rows (16 columns a block at d <= 64, 8
    beyond), an odd column past 64, the last column -- where d has them"""
    jb = 16 if d <= 64 else 8
    out = {'first': 0, 'inside_block': 5, 'last': d - 1}
    if jb < d:
        out['second_block'] = jb
    if d > 66:
        out['odd_past_64'] = 65 + 2 * ((d - 66) // 3)
    assert all(0 <= j < d for j in out.values()) and out.get('odd_past_64', 65) % 2 == 1
    return out


def failing_matrix(d, j_star, seed=0):
    """``A = L0 L0^T`` with ``A[j*][j*]`` lowered so that the pivot of column j* is <= 0 (exactly 0 at j* = 0): the columns before
    j* do not read that element, so they factorise as before"""
    rng = np.random.default_rng(4000 + 131 * d + j_star + seed)
    l0 = np.tril(rng.normal(size=(d, d))) * 0.3 / np.sqrt(d)
    l0[np.diag_indices(d)] = 1. + rng.uniform(size=d)
    a = lower_symmetric(l0 @ l0.T)
    if j_star == 0:
        a[0, 0] = 0.
    else:
        L, j_fail = chol_columns(a)
        assert j_fail is None
        a[j_star, j_star] -= 1.5 * L[j_star, j_star]**2   # the pivot: about -0.5 of what it was
    return a


def nan_diagonal_matrix(d, seed=0):
    """(matrix, j*): a NaN on the diagonal at j* = d // 2 (read by column j* only)"""
    a = spd_well(d, seed=seed + 1)
    a[d // 2, d // 2] = np.nan
    return a, d // 2


def fail_cases(d):
    """[(name, matrix, j*)] of part A's failing pivots at dimension d"""
    out = [(name, failing_matrix(d, j), j) for name, j in sorted(fail_columns(d).items())]
    a, j = nan_diagonal_matrix(d)
    return out + [('nan_diagonal', a, j)]


def dense_cov0(d, seed=0, lo=-1.5, hi=1.5):
    """a dense, badly scaled starting covariance for the sampler runs: correlations near 0.6, standard deviations spread over
    10^lo .. 10^hi times the target's"""
    rng = np.random.default_rng(5000 + d + seed)
    v = 1. + 0.1 * rng.normal(size=d)
    c = 0.4 * np.eye(d) + 0.6 * np.outer(v, v)
    s = 10.**np.linspace(lo, hi, d)[rng.permutation(d)]
    return lower_symmetric(c * np.outer(s, s))


def bits(x):
    """the bit patterns of a float64 array (so that -0. differs from 0. and NaNs compare)"""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- part C: one or two leapfrog steps with a fixed dense metric, device against oracle ---------------------------------------------

ONE_STEP_DIMS = (17, 64, 65, 100, 127)
ONE_STEP_RUNS = (('HMC', dict(n_int_step=1)), ('HMC', dict(n_int_step=2)), ('NUTS', dict(max_treedepth=2)))
ONE_STEP_ITERS, ONE_STEP_CHAINS, ONE_STEP_SEED, ONE_STEP_SIZE = 3, 3, 20240917, 0.02


def one_step_case(d):
    """the density, the fixed covariance, the starting points and the step size of part C at dimension d"""
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, _ = correlated_gaussian_spec(d)
    x0 = np.random.default_rng(6000 + d).normal(size=(ONE_STEP_CHAINS, d)) * 0.5
    return dict(d=d, spec=spec, cov0=dense_cov0(d, lo=-1., hi=1.), x0=x0, step_size=ONE_STEP_SIZE)


def oracle_one_step(case, sampler, kw, cov0=None):
    """the oracle's chains of part C: (samples (n_chain, n_iter, d), {stat: (n_chain, n_iter)})"""
    from oracle import oracle as orc
    cov0 = case['cov0'] if cov0 is None else cov0
    s, st = [], []
    for i in range(case['x0'].shape[0]):
        ch = orc.Chain(case['x0'][i], step_size=case['step_size'], adapt_step_size=False, metric=cov0, adapt_metric=False)
        rng = orc.make_rng('xoshiro', seed=ONE_STEP_SEED, stream=i)
        if sampler == 'NUTS':
            so, sto = orc.nuts_run(case['spec'], ch, rng, ONE_STEP_ITERS, 0, **kw)
        else:
            so, sto = orc.hmc_run(case['spec'], ch, rng, ONE_STEP_ITERS, 0, **kw)
        s.append(so)
        st.append(sto)
    return np.stack(s), {k: np.stack([x[k] for x in st]) for k in st[0]}


def one_step_compare(got, want, sampler):
    """``got``, ``want``: (samples, stats dict).  Accept flags, tree sizes and depths exactly; positions, energy and energy_change to
    rtol = atol = 1e-9 (the head tolerance of test_gpu_sampler._full_metric_compare)."""
    (s, st), (so, sto) = got, want
    for f in (('tree_depth', 'tree_size', 'diverging') if sampler == 'NUTS' else ('accepted', 'diverging')):
        assert np.array_equal(st[f], sto[f]), (f, st[f], sto[f])
    np.testing.assert_allclose(s, so, rtol=1e-9, atol=1e-9)
    for f in ('energy', 'energy_change'):
        np.testing.assert_allclose(st[f], sto[f], rtol=1e-9, atol=1e-9, err_msg=f)


def every_chain_moves(case, samples, stats, sampler):
    """at least one accepted proposal per chain: the position changed between the start and the last iteration, and (HMC) the
    accept flags say so"""
    moved = np.any(samples[:, -1] != case['x0'], axis=1)
    if sampler == 'HMC':
        moved &= stats['accepted'].sum(1) >= 1
    return bool(np.all(moved))
