"""Reference values for pointwise PSIS-LOO and WAIC (bayesfast_amd/utils/data_loo.py), written from the definitions by direct loops
on top of ``psis_reference(lw, dtype)``; float64, or ``numpy.longdouble`` where a test wants to know what rounding alone does.  It
shares no code with the package.

``column_reference(ell, log_weights, z)``: b = log_weights - logsumexp(log_weights) (without them -log n), w = exp(b); rows with
b = -inf are left out of every sum and have the ratio -inf; lpd = logsumexp(b + ell); p_waic = sum w (ell - sum w ell)^2 / (1 - sum w^2);
r = b - ell (without weights -ell); v, khat, sigma, n_tail = psis_reference(r); elpd_loo = logsumexp(v + ell); p_loo = lpd - elpd_loo;
ess_loo = 1 / sum exp(2 v) (psis_reference's ess); pit = sum exp(v) Phi(z).  A non-finite ell in a row of non-zero weight, or no such
row, makes everything NaN.

``order_keys`` / ``tail_reference``: the order-preserving uint64 keys of float64 values (every NaN last, -0 == +0) and the M + 1
largest (key, row) pairs of a column by NumPy's stable argsort."""
import math

import numpy as np

from psis_reference import psis_reference, tail_size


def _lse(vals, dtype):
    top = max(vals)
    acc = dtype(0)
    for v in vals:
        acc += np.exp(v - top)
    return top + np.log(acc)


def normalise(log_weights, dtype=np.float64):
    g = np.asarray(log_weights, dtype=np.float64).reshape(-1).astype(dtype)
    return g - _lse(list(g), dtype)


def phi(z, dtype):
    return dtype(0.5 * math.erfc(-float(z) / math.sqrt(2.)))   # (float64 whatever dtype is: the sums around it are what dtype widens)


def column_reference(ell, log_weights=None, z=None, dtype=np.float64):
    """dict(lpd, p_waic, elpd_waic, elpd_loo, p_loo, khat, sigma, n_tail, ess_loo, pit) of one column ell (n,)."""
    ell = np.asarray(ell, dtype=np.float64).reshape(-1).astype(dtype)
    n = len(ell)
    nan = dtype(np.nan)
    out = dict(lpd=nan, p_waic=nan, elpd_waic=nan, elpd_loo=nan, p_loo=nan, khat=nan, sigma=nan, n_tail=tail_size(n), ess_loo=nan, pit=nan)
    b = np.full(n, -np.log(dtype(n))) if log_weights is None else normalise(log_weights, dtype)
    rows = [s for s in range(n) if b[s] != -np.inf]
    if not rows or not all(np.isfinite(ell[s]) for s in rows):
        return out
    with np.errstate(all='ignore'):
        lpd = _lse([b[s] + ell[s] for s in rows], dtype)
        mean = sw2 = dtype(0)
        for s in rows:
            w = np.exp(b[s]) if log_weights is not None else dtype(1) / dtype(n)
            mean += w * ell[s]
            sw2 += w * w
        var = dtype(0)
        for s in rows:
            w = np.exp(b[s]) if log_weights is not None else dtype(1) / dtype(n)
            var += w * (ell[s] - mean)**2
        p_waic = var / (dtype(1) - sw2)
        r = np.full(n, dtype(-np.inf))
        for s in rows:
            r[s] = (b[s] - ell[s]) if log_weights is not None else -ell[s]
        ps = psis_reference(r, dtype)   # (it takes float64 ratios, as the device forms them, and works in dtype)
        v = ps['log_weights']
        elpd = _lse([v[s] + ell[s] for s in rows], dtype)
        out.update(lpd=lpd, p_waic=p_waic, elpd_waic=lpd - p_waic, elpd_loo=elpd, p_loo=lpd - elpd, khat=ps['khat'], sigma=ps['sigma'],
                   ess_loo=ps['ess'])
        if z is not None:
            acc = dtype(0)
            for s in rows:
                acc += np.exp(v[s]) * phi(z[s], dtype)
            out['pit'] = acc
    return out


def order_keys(v):
    """uint64 keys whose unsigned order is the numeric order of the float64 values v; every NaN last, -0 == +0."""
    v = np.array(v, dtype=np.float64)
    v[v == 0] = 0.
    bits = v.view(np.uint64)
    keys = np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))
    keys[np.isnan(v)] = np.uint64(0xffffffffffffffff)
    return keys


def tail_reference(shifted):
    """(keys (M + 1,), rows (M + 1,)) of the M + 1 largest of the shifted ratios in the order of a stable ascending sort."""
    keys = order_keys(shifted)
    order = np.argsort(keys, kind='stable')
    m1 = tail_size(len(keys)) + 1
    last = order[len(keys) - m1:]
    return keys[last], last.astype(np.uint32)
