"""Loop-written NumPy reference of the leave-one-out validation of the polynomial fit (PolyModel.fit_loo), independent of the package.

The design matrix of a linear ([1 | x]) or quadratic ([1 | x | x_j x_k, j <= k]) model, leverages from a QR factorisation of the
weighted design, the identity e_loo = e / (1 - h), and -- to check that identity itself -- ``loo_explicit``: n refits, each without
one point."""
import numpy as np


def design(x, order):
    """(n, P) design of ``PolyModel('linear')`` or ``PolyModel('quadratic')``; only its column space matters here."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    cols = [np.ones(n)]
    for j in range(d):
        cols.append(x[:, j].copy())
    if order == 'quadratic':
        for j in range(d):
            for k in range(j, d):
                cols.append(x[:, j] * x[:, k])
    elif order != 'linear':
        raise ValueError(order)
    return np.stack(cols, axis=1)


def make_case(n_in, n, m, weighted, seed):
    """Standard-normal x, y_q = sin(q x_0) + x_1^2 + 0.1 noise, weights exp(0.3 N(0, 1)) or None."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, n_in))
    y = np.empty((n, m))
    for q in range(m):
        y[:, q] = np.sin(q * x[:, 0]) + x[:, 1]**2 + 0.1 * rng.standard_normal(n)
    w = np.exp(0.3 * rng.standard_normal(n)) if weighted else None
    return x, y, w


def leverage_qr(Aw):
    """Diagonal of the hat matrix of a full-rank design: the squared row norms of the thin Q."""
    Q, _ = np.linalg.qr(Aw)
    h = np.zeros(Aw.shape[0])
    for i in range(Aw.shape[0]):
        h[i] = np.dot(Q[i], Q[i])
    return h


def leverage_svd(Aw, rcond=3e-6):
    """Hat diagonal of a rank-deficient design from its truncated SVD (singular values below rcond of the largest dropped);
    returns (h, rank)."""
    U, s, _ = np.linalg.svd(Aw, full_matrices=False)
    keep = s > rcond * s[0]
    Uk = U[:, keep]
    return np.sum(Uk * Uk, axis=1), int(keep.sum())


def stats_from(S, h, B, w):
    """Everything the report holds for one design, from the weighted residual S (n, m), the leverages and the weighted targets B:
    the per-output sums in the device's order, the derived numbers, and the residuals in the units of y."""
    n, m = S.shape
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    resid = S / wv[:, None]
    loo = S / ((1. - h) * wv)[:, None]
    sums = np.zeros((m, 8))
    out = dict(residual=resid, loo_residual=loo, sums=sums)
    for k in ('rmse', 'loo_rmse', 'r2', 'q2', 'max_abs_loo'):
        out[k] = np.zeros(m)
    out['argmax_abs_loo'] = np.zeros(m, dtype=int)
    for q in range(m):
        sse = press = sy = syy = 0.
        for i in range(n):
            sse += S[i, q]**2
            press += (S[i, q] / (1. - h[i]))**2
            sy += B[i, q]
            syy += B[i, q]**2
        ss_tot = 0.
        for i in range(n):  # (two-pass: the reference does not share the one-pass formula's cancellation)
            ss_tot += (B[i, q] - sy / n)**2
        am = int(np.argmax(np.abs(loo[:, q])))
        sums[q] = [sse, press, abs(loo[am, q]), am, sy, syy, float(np.sum(1. - h <= 0.)), 0.]
        out['rmse'][q] = np.sqrt(sse / n)
        out['loo_rmse'][q] = np.sqrt(press / n)
        out['r2'][q] = 1. - sse / ss_tot
        out['q2'][q] = 1. - press / ss_tot
        out['max_abs_loo'][q] = abs(loo[am, q])
        out['argmax_abs_loo'][q] = am
    return out


def reference(x, y, order, w=None):
    """The report's numbers for a full-rank design: the weighted least-squares fit by an orthogonal method (numpy.linalg.lstsq),
    leverages by QR, the rest by ``stats_from``."""
    A = design(x, order)
    wv = np.ones(A.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    Aw = A * wv[:, None]
    B = np.asarray(y, dtype=np.float64) * wv[:, None]
    c = np.linalg.lstsq(Aw, B, rcond=None)[0]
    h = leverage_qr(Aw)
    out = stats_from(B - Aw @ c, h, B, w)
    out.update(leverage=h, P=A.shape[1], coef=c)
    return out


def loo_explicit(x, y, order, w=None):
    """Held-out residuals (n, m) in the units of y: for every point i a fit without it, evaluated at it."""
    A = design(x, order)
    y = np.asarray(y, dtype=np.float64)
    n = A.shape[0]
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty_like(y)
    for i in range(n):
        keep = np.arange(n) != i
        c = np.linalg.lstsq(A[keep] * wv[keep, None], y[keep] * wv[keep, None], rcond=None)[0]
        out[i] = y[i] - A[i] @ c
    return out
