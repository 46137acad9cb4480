"""Reference values for Pareto-smoothed importance sampling and the weighted posterior table, written from their specification by
direct loops in plain NumPy (float64, or ``numpy.longdouble`` where a test wants to know what rounding alone does).  It shares no
code with ``bayesfast_amd.utils.psis``.

``psis_reference(lw)``: for S log ratios -- shift by the maximum; M = min(floor(0.2 S), ceil(3 sqrt(S))); M < 5 or a tail without
spread: no smoothing, khat = inf; otherwise the generalised-Pareto fit of Zhang & Stephens (2009) to the M largest exceedances
exp(lw) - exp(cut), cut the value at sorted position S - M - 1, with m = 30 + floor(sqrt(M)) candidate thetas, khat = (k M + 5) / (M + 10);
sorted tail position i gets log(exp(cut) + sigma expm1(-khat log1p(-p_i)) / khat), p_i = (i - 1/2) / M (the fit's quantile function),
capped at 0; then log_mean_weight = max + logsumexp - log S, the normalisation, and Kish's 1 / sum w^2.  A NaN or +inf, or no value
above -inf, makes everything NaN.

``table_reference(x, w, probs)``: rows of zero weight are left out; mean = sum w x, sd^2 = sum w (x - mean)^2 / (1 - sum w^2),
mcse_mean^2 = sum w^2 (x - mean)^2, ess = sd^2 (1 - sum w^2) / mcse_mean^2, ess_kish = 1 / sum w^2, quantiles by the mid-point rule
on the running sum of the sorted weights; 'margin' is per parameter the smallest |pos_k - q| over all k and q, in units of 1 / n:
where it is tiny, the summation order decides the bracket and no comparison is meaningful."""
import numpy as np


def tail_size(s):
    return min(int(np.floor(0.2 * s)), int(np.ceil(3 * np.sqrt(s))))


def gaussian_pair(s, scale, seed):
    """(logp, logq, draws) for S draws of q = N(0, scale^2) and the target p = N(0, 1): khat is near 1 - scale^2."""
    x = np.random.default_rng(seed).standard_normal(s) * scale
    return -0.5 * x**2 - 0.5 * np.log(2 * np.pi), -0.5 * (x / scale)**2 - np.log(scale) - 0.5 * np.log(2 * np.pi), x


def psis_reference(lw, dtype=np.float64):
    """dict(log_weights (S,), khat, sigma, n_tail, log_mean_weight, ess) of the log ratios lw, any shape, flattened."""
    lw = np.asarray(lw, dtype=np.float64).reshape(-1).astype(dtype)
    s = len(lw)
    big_m = tail_size(s)
    nan = dtype(np.nan)
    out = dict(log_weights=np.full(s, nan), khat=nan, sigma=nan, n_tail=big_m, log_mean_weight=nan, ess=nan)
    top = dtype(-np.inf)
    for v in lw:
        if np.isnan(v) or v == np.inf:
            return out
        if v > top:
            top = v
    if top == -np.inf:
        return out
    with np.errstate(all='ignore'):
        lw = lw - top
        khat, sigma = dtype(np.inf), nan
        if big_m >= 5:
            order = np.argsort(lw, kind='stable')
            cut = lw[order[s - big_m - 1]]
            x = [np.exp(lw[order[s - big_m + i]]) - np.exp(cut) for i in range(big_m)]
            if x[-1] > 0:
                n = big_m
                m = 30 + int(np.floor(np.sqrt(n)))
                half, one, three = dtype(0.5), dtype(1), dtype(3)
                xq = x[int(np.floor(n / 4 + 0.5)) - 1]
                theta, ks, ls = [], [], []
                for j in range(1, m + 1):
                    th = one / x[-1] + (one - np.sqrt(dtype(m) / (dtype(j) - half))) / (three * xq)
                    acc = dtype(0)
                    for xi in x:
                        acc += np.log1p(-th * xi)
                    kj = acc / dtype(n)
                    theta.append(th)
                    ks.append(kj)
                    ls.append(dtype(n) * (np.log(-th / kj) - kj - one))
                th = dtype(0)
                for j in range(m):
                    acc = dtype(0)
                    for l in range(m):
                        acc += np.exp(ls[l] - ls[j])
                    th += theta[j] / acc
                acc = dtype(0)
                for xi in x:
                    acc += np.log1p(-th * xi)
                k = acc / dtype(n)
                sigma = -k / th
                khat = (k * dtype(n) + dtype(5)) / (dtype(n) + dtype(10))
                for i in range(big_m):
                    l1p = np.log1p(-(dtype(i) + half) / dtype(big_m))
                    q = -sigma * l1p if khat == 0 else sigma * np.expm1(-khat * l1p) / khat
                    v = np.log(np.exp(cut) + q)
                    lw[order[s - big_m + i]] = dtype(0) if v > 0 else v
        peak = lw.max()
        acc = dtype(0)
        for v in lw:
            acc += np.exp(v - peak)
        lse = peak + np.log(acc)
        lw = lw - lse
        acc = dtype(0)
        for v in lw:
            acc += np.exp(v)**2
        out.update(log_weights=lw, khat=khat, sigma=sigma, log_mean_weight=top + lse - np.log(dtype(s)), ess=one_over(acc, dtype))
    return out


def one_over(v, dtype):
    return dtype(1) / v


def table_one(x, w, probs):
    """Every figure of one parameter: x (n,), w (n,) normalised."""
    names = ['mean', 'sd'] + ['q%g' % (100 * p) for p in probs] + ['mcse_mean', 'ess', 'ess_kish', 'margin']
    out = {k: np.nan for k in names}
    out['margin'] = np.inf   # (no bracket is taken in a column that is NaN or constant)
    sw2 = 0.
    for wi in w:
        sw2 += wi * wi
    rows = [i for i in range(len(x)) if w[i] != 0]
    xs, ws = [x[i] for i in rows], [w[i] for i in rows]
    n = len(xs)
    if not np.all(np.isfinite(xs)):
        return out
    order = sorted(range(n), key=lambda i: xs[i])   # (sorted is stable)
    v, wp = [xs[i] for i in order], [ws[i] for i in order]
    if v[0] == v[-1]:
        out.update({'mean': v[0], 'sd': 0.}, **{'q%g' % (100 * p): v[0] for p in probs})
        if n == 1 or not 1. - sw2 > 0:
            out['sd'] = np.nan
        return out
    mean = 0.
    for i in range(n):
        mean += ws[i] * xs[i]
    s2 = s4 = 0.
    for i in range(n):
        s2 += ws[i] * (xs[i] - mean)**2
        s4 += ws[i]**2 * (xs[i] - mean)**2
    c, mid = 0., []
    for i in range(n):
        c += wp[i]
        mid.append(c - wp[i] / 2)
    pos = [(mk - mid[0]) / (mid[-1] - mid[0]) for mk in mid]
    margin = np.inf
    for p in probs:
        k = 0
        for i in range(n):
            if pos[i] <= p:
                k = i
            margin = min(margin, abs(pos[i] - p) * n)
        if k == n - 1:
            qv = v[k]
        else:
            t = (p - pos[k]) / (pos[k + 1] - pos[k])
            d = v[k + 1] - v[k]
            qv = v[k + 1] - d * (1 - t) if t >= 0.5 else v[k] + d * t
        out['q%g' % (100 * p)] = qv
    out.update(mean=mean, margin=margin)
    if 1. - sw2 > 0:
        with np.errstate(all='ignore'):
            out.update(sd=np.sqrt(s2 / (1. - sw2)), mcse_mean=np.sqrt(s4), ess=s2 / s4, ess_kish=1. / sw2)
    return out


def table_reference(x, weights=None, log_weights=None, probs=(0.05, 0.5, 0.95)):
    """x (n, d) or (n_chain, n_draw, d) -> dict of (d,) arrays."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    if weights is None:
        g = np.asarray(log_weights, dtype=np.float64).reshape(-1)
        weights = np.exp(g - g.max())
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    total = 0.
    for wi in w:
        total += wi
    w = w / total
    rows = [table_one(x[:, k], w, probs) for k in range(x.shape[1])]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}
