"""Reference values for the convergence diagnostics, written from the estimators' specification by direct loops over the
parameters, the series and the lags: the O(n lags) autocovariance, ``scipy.stats.rankdata(method='average')`` and
``scipy.special.ndtri``.  It shares no code with ``bayesfast_amd.utils.diagnostics``.

For one parameter, x (M chains, N draws): h = N // 2, an odd N drops every chain's first draw, each chain gives two split chains
of n = h draws, m = 2 M, S = m n.  ``reference(x)`` returns the table's columns as (n_d,) arrays, 'rhat_split' and 'ess_mean',
and 'margin': per parameter the smallest |P_k| among the pairs of Geyer's sequence up to and including the deciding one, over
every series whose ESS enters the table (plain, rank-normalised, the tail indicators)."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata


def split(x):
    """(M, N) -> (2 M, N // 2)"""
    big_m, n_t = x.shape
    h = n_t // 2
    x = x[:, n_t - 2 * h:]
    return np.stack([x[c, half * h:(half + 1) * h] for c in range(big_m) for half in (0, 1)])


def z_scores(y):
    s = y.size
    r = rankdata(y.reshape(-1), method='average')
    return ndtri((r - 3. / 8.) / (s + 1. / 4.)).reshape(y.shape)


def w_varp(y):
    m, n = y.shape
    means = np.array([y[j].mean() for j in range(m)])
    s2 = np.array([((y[j] - means[j])**2).sum() / (n - 1) for j in range(m)])
    w = s2.mean()
    v = ((means - means.mean())**2).sum() / (m - 1)
    return w, (n - 1) / n * w + v


def r_hat(y):
    with np.errstate(all='ignore'):
        w, varp = w_varp(y)
        return np.sqrt(varp / w)


def ess_margin(y):
    """(ESS, the smallest |P_k| for k up to and including the deciding pair) of an (m, n) series."""
    m, n = y.shape
    s = m * n
    with np.errstate(all='ignore'):
        w, varp = w_varp(y)
        c = y - y.mean(axis=1, keepdims=True)

        def rho(t):
            a = np.array([np.dot(c[j, :n - t], c[j, t:]) for j in range(m)])
            return 1. - (w - (a / (n - 1)).mean()) / varp

        n_pairs = n // 2   # 2 k + 1 <= n - 1
        p = []
        for k in range(n_pairs):
            p.append(rho(2 * k) + rho(2 * k + 1))
            if k >= 1 and p[k] < 0:
                break
        k_stop = len(p) - 1 if (len(p) > 1 and p[-1] < 0) else len(p)
        total, low = 0., np.inf
        for k in range(k_stop):
            low = np.minimum(low, p[k])
            total += low
        tau = np.maximum(-1. + 2. * total, 1. / np.log10(s))
        return s / tau, float(np.min(np.abs(p)))


def reference_one(x, probs=(0.05, 0.5, 0.95), prob=(0.05, 0.95)):
    """Every figure of one parameter, x (M, N)."""
    x = np.asarray(x, dtype=np.float64)
    y = split(x)
    names = ['mean', 'sd'] + ['q%g' % (100 * p) for p in probs] + ['mcse_mean', 'ess_bulk', 'ess_tail', 'rhat', 'rhat_split',
                                                                   'ess_mean', 'margin']
    if not np.isfinite(y).all():
        return {k: np.nan for k in names}
    if y.min() == y.max():
        # a constant parameter: the 0 / 0 of the formulas, whatever the rounded sum of n copies makes of the variance
        out = {k: np.nan for k in names}
        out.update({'mean': y[0, 0], 'sd': 0.}, **{'q%g' % (100 * p): y[0, 0] for p in probs})
        return out
    with np.errstate(all='ignore'):
        out = {'mean': y.mean(), 'sd': y.std(ddof=1)}
        for p in probs:
            out['q%g' % (100 * p)] = np.quantile(y, p)
        z = z_scores(y)
        ess_mean, mg_mean = ess_margin(y)
        ess_bulk, mg_bulk = ess_margin(z)
        tails = [ess_margin((y <= np.quantile(y, q)).astype(np.float64)) for q in prob]
        out['mcse_mean'] = out['sd'] / np.sqrt(ess_mean)
        out['ess_bulk'] = ess_bulk
        out['ess_tail'] = np.minimum.reduce([t[0] for t in tails])
        out['rhat'] = np.maximum(r_hat(z), r_hat(z_scores(np.abs(y - np.median(y)))))
        out['rhat_split'] = r_hat(y)
        out['ess_mean'] = ess_mean
        out['margin'] = min([mg_mean, mg_bulk] + [t[1] for t in tails])
    return out


def reference(x, probs=(0.05, 0.5, 0.95), prob=(0.05, 0.95)):
    """x (M, N) or (M, N, n_d) -> dict of (n_d,) arrays."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    rows = [reference_one(x[:, :, k], probs, prob) for k in range(x.shape[2])]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def ar1(shape, phis=(0., 0.5, 0.9, 0.98), seed=0):
    """(M, N, d) stationary AR(1) columns of unit variance, phi cycling through ``phis`` along the last axis."""
    big_m, n_t, d = shape
    rng = np.random.default_rng(seed)
    phi = np.array([phis[k % len(phis)] for k in range(d)])
    e = rng.standard_normal(shape)
    x = np.empty(shape)
    x[:, 0] = e[:, 0]
    for t in range(1, n_t):
        x[:, t] = phi * x[:, t - 1] + np.sqrt(1. - phi**2) * e[:, t]
    return x
