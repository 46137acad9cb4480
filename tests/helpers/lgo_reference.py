"""Reference values for leave-group-out cross-validation (bayesfast_amd/utils/data_lgo.py), written from the definitions by direct
loops on top of ``psis_reference(lw, dtype)``, as helpers/data_loo_reference.py is; float64, or ``numpy.longdouble`` where a
test wants to know what rounding alone does.  It shares no code with the package.

``group_reference(q, dof, c, log_weights)``: ell = c - q / 2; lpd, p_waic, elpd_waic, khat, sigma, n_tail as
``data_loo_reference.column_reference(ell)`` defines them, elpd_lgo, p_lgo and ess_lgo as its elpd_loo, p_loo and ess_loo; with
b = log_weights - logsumexp(log_weights) (without them -log n), w = exp(b), v = psis_reference(b - ell)'s log weights and Q = Q(dof / 2, q / 2) over the rows with b > -inf:
chi2_base = sum w q, chi2_lgo = sum exp(v) q, ppp_base = sum w Q, ppp_lgo = sum exp(v) Q.  A non-finite ell in a row of non-zero weight,
or no such row, makes everything NaN.

``accum_reference(z, slots, c)``: the NumPy loop of ``bfhip_lgo_accum``: acc = c, then acc = acc - 0.5 * (z_j * z_j) column by column.

``whiten_reference(prec, y, f, group)``: log p(y_B | y_-B, f) by the textbook route, without the precision's blocks: the covariance
Sigma = P^-1, the conditional mean f_B + Sigma_B,-B Sigma_-B,-B^-1 (y - f)_-B and the Schur-complement covariance."""
import numpy as np

from data_loo_reference import normalise
from psis_reference import psis_reference, tail_size


def survival(dof, q):
    """Q(dof / 2, q / 2) of float64 values (float64 whatever the sums around it are widened to)."""
    from scipy.special import gammaincc
    return gammaincc(0.5 * float(dof), 0.5 * np.asarray(q, dtype=np.float64))


def _lse(vals, dtype):
    top = max(vals)
    acc = dtype(0)
    for v in vals:
        acc += np.exp(v - top)
    return top + np.log(acc)


def group_reference(q, dof, c=0., log_weights=None, dtype=np.float64):
    """dict(lpd, p_waic, elpd_waic, elpd_lgo, p_lgo, khat, sigma, n_tail, ess_lgo, chi2_base, chi2_lgo, ppp_base, ppp_lgo) of one
    column q (n,) of conditional chi-squares."""
    q64 = np.asarray(q, dtype=np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        ell = (np.float64(c) - 0.5 * q64).astype(dtype)   # (formed in float64 as the package forms it; the sums are what dtype widens)
    n = len(q64)
    nan = dtype(np.nan)
    out = dict(lpd=nan, p_waic=nan, elpd_waic=nan, elpd_lgo=nan, p_lgo=nan, khat=nan, sigma=nan, n_tail=tail_size(n), ess_lgo=nan,
               chi2_base=nan, chi2_lgo=nan, ppp_base=nan, ppp_lgo=nan)
    b = np.full(n, -np.log(dtype(n))) if log_weights is None else normalise(log_weights, dtype)
    rows = [s for s in range(n) if b[s] != -np.inf]
    if not rows or not all(np.isfinite(ell[s]) for s in rows):
        return out
    with np.errstate(all='ignore'):
        big_q = survival(dof, q64).astype(dtype)
        qd = q64.astype(dtype)
        lpd = _lse([b[s] + ell[s] for s in rows], dtype)
        mean = sw2 = cb = pb = dtype(0)
        for s in rows:
            w = np.exp(b[s]) if log_weights is not None else dtype(1) / dtype(n)
            mean += w * ell[s]
            sw2 += w * w
            cb += w * qd[s]
            pb += w * big_q[s]
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
        cl = pl = dtype(0)
        for s in rows:
            e = np.exp(v[s])
            cl += e * qd[s]
            pl += e * big_q[s]
        out.update(lpd=lpd, p_waic=p_waic, elpd_waic=lpd - p_waic, elpd_lgo=elpd, p_lgo=lpd - elpd, khat=ps['khat'], sigma=ps['sigma'],
                   ess_lgo=ps['ess'], chi2_base=cb, chi2_lgo=cl, ppp_base=pb, ppp_lgo=pl)
    return out


def accum_reference(z, slots, c, acc=None, start=None):
    """z (n, nb), slots (nb,) in -1 .. 15, c (16,) -> acc (n, 16): the slots in ``start`` begin at c, the others go on from ``acc``."""
    n, nb = z.shape
    out = np.zeros((n, 16)) if acc is None else np.array(acc, dtype=np.float64)
    for s in (range(16) if start is None else start):
        out[:, s] = c[s]
    for j in range(nb):
        if slots[j] >= 0:
            out[:, slots[j]] = out[:, slots[j]] - 0.5 * (z[:, j] * z[:, j])
    return out


def whiten_reference(prec, y, f, group):
    """log p(y_B | y_-B) under y ~ N(f, prec^-1), from the covariance."""
    from scipy.stats import multivariate_normal
    m = len(y)
    sigma = np.linalg.inv(np.asarray(prec, dtype=np.float64))
    inside = np.asarray(group)
    rest = np.setdiff1d(np.arange(m), inside)
    if rest.size:
        gain = sigma[np.ix_(inside, rest)] @ np.linalg.inv(sigma[np.ix_(rest, rest)])
        mean = f[inside] + gain @ (y - f)[rest]
        cov = sigma[np.ix_(inside, inside)] - gain @ sigma[np.ix_(rest, inside)]
    else:
        mean, cov = f[inside], sigma
    cov = 0.5 * (cov + cov.T)
    return float(multivariate_normal.logpdf(y[inside], mean=mean, cov=cov))
