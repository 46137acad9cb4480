"""A plain extended-precision restatement of the two reductions behind the integrated autocorrelation time (include/bfhip.h:
bfhip_acor_moments, bfhip_acor_lag_sums), written from the definitions there and not from the kernels' tiling:

    y_wk(s) = x_wk(s) - mean_wk,   a_wk(t) = sum_{s < n_t - t} y_wk(s) y_wk(s + t),   S(t, k) = sum_w a_wk(t) inv_wk

NumPy only; numpy.longdouble (the x87 80-bit format: 64 significand bits) carries every sum.  ``groups`` and ``log_td`` restate
the two shape functions of csrc/bfhip_acor.hip (ac_groups, ac_log_td), so that a case list can say which path of the lag kernel
a shape takes."""
import numpy as np

LD = np.longdouble
# the tolerances of tests/test_gpu_acor_kernels.py take the reference's own rounding (n 2^-64 relative) as nothing next to the
# kernels' (n 2^-53): that needs the 80-bit format, which x86-64 Linux has
assert np.finfo(LD).eps <= 2.**-63, 'numpy.longdouble has to carry at least 64 significand bits'

SLOTS, LAGS, CHUNK, MAX_GROUPS = 16, 64, 256, 256   # AC_SLOTS, AC_LAGS, AC_CT, AC_MAXG


def groups(n_w):
    """(walkers per group, number of groups) of the lag pass: ac_groups."""
    wpg = (n_w + MAX_GROUPS - 1) // MAX_GROUPS
    return wpg, (n_w + wpg - 1) // wpg


def log_td(n_d):
    """log2 of the dimensions per workgroup of the lag pass, the smallest power of two >= n_d and at most 16: ac_log_td."""
    ltd = 0
    while (1 << ltd) < n_d and (1 << ltd) < SLOTS:
        ltd += 1
    return ltd


def _walkers(x, ldw):
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError('x is (n_w, n_t, n_d)')
    if ldw is not None and ldw < x.shape[1] * x.shape[2]:
        raise ValueError('ldw < n_t n_d')
    return x.astype(LD)


def moments(x, ldw=None):
    """x (n_w, n_t, n_d) -> mean (n_w, n_d) and inv = 1 / a_wk(0) (n_w, n_d), by two passes in longdouble, rounded to float64 at the
    end.  A series without spread has inv = +inf.  ``ldw`` is the walker stride the kernel would be given: the reference reads
    element (w, s, k) and nothing else, so it only checks ldw >= n_t n_d."""
    xl = _walkers(x, ldw)
    n_t = xl.shape[1]
    m = xl.sum(axis=1) / LD(n_t)
    d = xl - m[:, None, :]
    a0 = (d * d).sum(axis=1)
    with np.errstate(divide='ignore'):
        inv = LD(1) / a0
    return m.astype(np.float64), inv.astype(np.float64)


def a0_about(x, mean):
    """sum_s (x_wk(s) - mean_wk)^2 in longdouble about the float64 ``mean`` given (a kernel's own, say) -> (n_w, n_d) longdouble."""
    d = np.asarray(x).astype(LD) - np.asarray(mean, dtype=np.float64).astype(LD)[:, None, :]
    return (d * d).sum(axis=1)


def lag_sums(x, mean, inv, t0, n_lag):
    """(S, A), each (n_lag, n_d) longdouble: S[i, k] = sum_w inv[w, k] sum_{s < n_t - t} y(s) y(s + t) at t = t0 + i, with
    y = longdouble(x) - longdouble(mean) for the float64 ``mean`` passed in (what the kernel subtracts), and A the same sum with
    every factor replaced by its absolute value (the scale of the rounding error of S in any order of summation).  Rows with
    t >= n_t are exactly 0."""
    xl = _walkers(x, None)
    n_w, n_t, n_d = xl.shape
    mean = np.asarray(mean, dtype=np.float64).reshape(n_w, n_d).astype(LD)
    inv = np.asarray(inv, dtype=np.float64).reshape(n_w, n_d).astype(LD)
    y = xl - mean[:, None, :]
    ya, ia = np.abs(y), np.abs(inv)
    S, A = np.zeros((n_lag, n_d), dtype=LD), np.zeros((n_lag, n_d), dtype=LD)
    with np.errstate(invalid='ignore'):
        for i in range(n_lag):
            t = t0 + i
            if t >= n_t:
                break
            S[i] = (inv * (y[:, :n_t - t] * y[:, t:]).sum(axis=1)).sum(axis=0)
            A[i] = (ia * (ya[:, :n_t - t] * ya[:, t:]).sum(axis=1)).sum(axis=0)
    return S, A
