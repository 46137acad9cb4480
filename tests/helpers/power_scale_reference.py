"""Reference values for power-scaling sensitivity (bayesfast_amd/utils/power_scale.py), written from the definitions by direct loops
over the sorted draws on top of ``psis_reference`` and ``reweight_reference``; float64, or ``numpy.longdouble`` where a test wants to
know what rounding alone does.  It shares no code with the package.

``ecdf_reference(x, w, u)``: the rows with w != 0 are the sample; sorted by value, stable; P and Q the running sums of w and u,
h_p = x_(p+1) - x_(p); bound = sum h (P + Q); J = sum h M [(1 - t) log1p(-t) + (1 + t) log1p(t)] / ln 2 with M = (P + Q) / 2 and
t = (Q - P) / (P + Q), the numerator the running sum of u - w, 0 log 0 = 0 (no series: the logarithms themselves); cjs = sqrt(J / bound);
ks = max over h_p > 0 of |Q - P|.  A non-finite value in the sample makes all NaN; bound == 0 makes cjs and ks NaN.

``weights_reference(l, log_weights)``: u = exp(v) / sum over the rows of the sample of the smoothed log weights v of psis_reference on
r = b + l (without weights r = l), 0 in a row with b = -inf, NaN in the rows of the sample where reweight_reference flags 1 or 4.

``power_scale_reference(x, g, log_weights, alphas)``: scenario (c, a) -> column c A + a, l = (alpha_a - 1) g_c; reweight_reference's
figures, cjs and ks (K, d), and sensitivity, mean_gradient, sd_gradient (C, d) as the module's docstring defines them."""
import numpy as np

from psis_reference import psis_reference
from reweight_reference import normalise, reweight_reference


def ecdf_reference(x, w, u, dtype=np.float64):
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w).astype(dtype)
    u = np.asarray(u).astype(dtype)
    nan = dtype(np.nan)
    rows = [i for i in range(len(x)) if w[i] != 0]
    out = dict(J=nan, bound=nan, cjs=nan, ks=nan)
    if not all(np.isfinite(x[i]) for i in rows):
        return out
    rows = sorted(rows, key=lambda i: x[i])   # (sorted is stable)
    ln2 = np.log(dtype(2))
    big_p = big_d = dtype(0)
    big_j = bound = ks = dtype(0)
    with np.errstate(all='ignore'):
        for p in range(len(rows) - 1):
            i = rows[p]
            big_p += w[i]
            big_d += u[i] - w[i]
            h = dtype(x[rows[p + 1]]) - dtype(x[i])
            tot = big_p + (big_p + big_d)
            t = big_d / tot
            t = dtype(1) if t > 1 else dtype(-1) if t < -1 else t
            one = dtype(1)
            a, b = one - t, one + t
            f = (dtype(0) if a == 0 else a * np.log1p(-t)) + (dtype(0) if b == 0 else b * np.log1p(t))
            bound += h * tot
            big_j += h * (tot / dtype(2)) * f / ln2
            if h > 0 and not abs(big_d) <= ks:
                ks = abs(big_d)
        out.update(J=big_j, bound=bound)
        if bound != 0:
            out.update(cjs=np.sqrt(big_j / bound), ks=nan if np.isnan(big_j) else ks)
    return out


def weights_reference(l, log_weights=None, dtype=np.float64):
    """(w (n,), u (n, K)) in ``dtype``"""
    l = np.asarray(l, dtype=np.float64)
    n, big_k = l.shape
    b = np.full(n, -np.log(dtype(n))) if log_weights is None else normalise(log_weights, dtype)
    rows = [s for s in range(n) if b[s] != -np.inf]
    w = np.zeros(n, dtype=dtype)
    u = np.zeros((n, big_k), dtype=dtype)
    with np.errstate(all='ignore'):
        for s in rows:
            w[s] = np.exp(b[s]) if log_weights is not None else dtype(1) / dtype(n)
        for k in range(big_k):
            if not rows:
                continue
            if not all(np.isfinite(l[s, k]) for s in rows):
                for s in rows:
                    u[s, k] = np.nan
                continue
            r = np.full(n, dtype(-np.inf))
            for s in rows:
                r[s] = (b[s] + dtype(l[s, k])) if log_weights is not None else dtype(l[s, k])
            e = np.exp(psis_reference(np.asarray(r, dtype=np.float64), dtype)['log_weights'])
            total = dtype(0)
            for s in rows:
                total += e[s]
            for s in rows:
                u[s, k] = e[s] / total
    return w, u


def ratios(g, alphas):
    g = np.asarray(g, dtype=np.float64)
    a = np.asarray(alphas, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.stack([(a[j] - 1.) * g[:, c] for c in range(g.shape[1]) for j in range(len(a))], axis=1)


def power_scale_reference(x, g, log_weights=None, alphas=(0.99, 1.01), dtype=np.float64):
    x = np.asarray(x, dtype=np.float64)
    a = np.asarray(alphas, dtype=np.float64)
    n, d = x.shape
    n_comp, n_alpha = np.shape(g)[1], len(a)
    l = ratios(g, a)
    out = reweight_reference(x, l, log_weights, dtype=dtype)
    w, u = weights_reference(l, log_weights, dtype)
    big_k = l.shape[1]
    cjs, ks = np.full((big_k, d), dtype(np.nan)), np.full((big_k, d), dtype(np.nan))
    for k in range(big_k):
        if out['flags'][k] & 5:
            continue
        for j in range(d):
            r = ecdf_reference(x[:, j], w, u[:, k], dtype)
            cjs[k, j], ks[k, j] = r['cjs'], r['ks']
    lo = max((j for j in range(n_alpha) if a[j] < 1), key=lambda j: a[j])
    hi = min((j for j in range(n_alpha) if a[j] > 1), key=lambda j: a[j])
    l2lo, l2hi = np.log2(dtype(a[lo])), np.log2(dtype(a[hi]))
    c3 = cjs.reshape(n_comp, n_alpha, d)
    mean, sd = out['mean'].reshape(n_comp, n_alpha, d), out['sd'].reshape(n_comp, n_alpha, d)
    with np.errstate(all='ignore'):
        out.update(cjs=cjs, ks=ks, sensitivity=(c3[:, lo] / abs(l2lo) + c3[:, hi] / l2hi) / 2,
                   mean_gradient=(mean[:, hi] - mean[:, lo]) / (l2hi - l2lo) / out['sd_base'][None, :],
                   sd_gradient=(sd[:, hi] - sd[:, lo]) / (l2hi - l2lo) / out['sd_base'][None, :])
    return out
