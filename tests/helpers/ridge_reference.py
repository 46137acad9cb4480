"""Loop-written NumPy reference of the ridge path of the polynomial fit (PolyModel.fit_ridge), independent of the package.

The fit minimises |w (y - A c)|^2 + n rho sum_{j >= 1} D_j c_j^2 over the helper's plain monomial design (loo_reference.design:
column 0 is the constant and is not penalised), D_j = sum_i (w_i A_ij)^2 / n.  It is solved as ordinary least squares on augmented
data -- P - 1 extra rows sqrt(n rho D_j) e_j with target zero -- by numpy.linalg.lstsq; the hat diagonal is the squared row norms of
the thin Q of the augmented design (its first n rows); the held-out residuals follow from e / (1 - h) and, to check that identity
itself, from ``ridge_loo_explicit``: n refits, each without one point, at the SAME D and the SAME n rho."""
import numpy as np

import loo_reference as lr


def _weighted(x, y, order, w):
    A = lr.design(x, order)
    n = A.shape[0]
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    return A, A * wv[:, None], np.asarray(y, dtype=np.float64) * wv[:, None], wv


def column_scale(Aw):
    """D (P,): the mean square of every weighted column, zero for the constant (not penalised)."""
    n, P = Aw.shape
    D = np.zeros(P)
    for j in range(1, P):
        s = 0.
        for i in range(n):
            s += Aw[i, j]**2
        D[j] = s / n
    return D


def augment(Aw, B, D, lam):
    """The augmented design and targets of the ridge fit with penalty lam D_j on column j >= 1."""
    P = Aw.shape[1]
    extra = np.zeros((P - 1, P))
    for j in range(1, P):
        extra[j - 1, j] = np.sqrt(lam * D[j])
    return np.vstack([Aw, extra]), np.vstack([B, np.zeros((P - 1, B.shape[1]))])


def ridge_reference(x, y, order, rho, w=None):
    """Everything the report holds at one penalty: coef (P, m) on the helper's design, leverage, dof, and what
    loo_reference.stats_from derives (residual, loo_residual, sums, rmse, loo_rmse, r2, q2, ...), plus press (m,)."""
    A, Aw, B, wv = _weighted(x, y, order, w)
    n = A.shape[0]
    D = column_scale(Aw)
    Aaug, Baug = augment(Aw, B, D, n * rho)
    c = np.linalg.lstsq(Aaug, Baug, rcond=None)[0]
    Q, _ = np.linalg.qr(Aaug)
    h = np.zeros(n)
    for i in range(n):
        h[i] = np.dot(Q[i], Q[i])
    out = lr.stats_from(B - Aw @ c, h, B, w)
    out.update(leverage=h, dof=float(np.sum(h)), coef=c, P=A.shape[1], press=out['sums'][:, 1].copy())
    return out


def ridge_loo_explicit(x, y, order, rho, w=None):
    """Held-out residuals (n, m) in the units of y: for every point a refit without it (D and n rho of the full fit), evaluated at it."""
    A, Aw, B, wv = _weighted(x, y, order, w)
    y = np.asarray(y, dtype=np.float64)
    n = A.shape[0]
    D = column_scale(Aw)
    out = np.empty_like(y)
    for i in range(n):
        keep = np.arange(n) != i
        Aaug, Baug = augment(Aw[keep], B[keep], D, n * rho)
        c = np.linalg.lstsq(Aaug, Baug, rcond=None)[0]
        out[i] = y[i] - A[i] @ c
    return out


def ridge_path_reference(x, y, order, rhos, w=None):
    """The references of a whole path, the selection criterion (the mean over the outputs of PRESS / SS_tot = 1 - q2) and the index
    it picks (the smallest score, ties to the larger penalty)."""
    refs = [ridge_reference(x, y, order, rho, w) for rho in rhos]
    score = np.zeros(len(refs))
    for l, ref in enumerate(refs):
        s = 0.
        for q in range(ref['q2'].size):
            s += 1. - ref['q2'][q]
        score[l] = s / ref['q2'].size
    best = 0
    for l in range(1, len(refs)):
        if score[l] < score[best] or (score[l] == score[best] and rhos[l] > rhos[best]):
            best = l
    return dict(refs=refs, score=score, index=best)


# ---- the cases of tests/test_fit_ridge_host.py and tests/test_gpu_fit_ridge.py: (inputs, order, n, outputs, weighted) ----
# primal side (n >= P - 1): P = 15; 78; r = 63 with n one past 256; P = 136 with one output past a batch of 16
PRIMAL = [(4, 'quadratic', 40, 3, True), (11, 'quadratic', 200, 2, True), (63, 'linear', 257, 2, False), (15, 'quadratic', 333, 17, True)]
# dual side (n < P - 1): P = 28 without and with weights; 78; 136 with n one past 64; 595
DUAL = [(6, 'quadratic', 20, 2, False), (6, 'quadratic', 20, 2, True), (11, 'quadratic', 60, 2, False), (15, 'quadratic', 65, 3, True),
        (33, 'quadratic', 129, 1, False)]
RHO_PRIMAL = (1e-6, 1e-3, 1e-1, 1., 10.)
RHO_DUAL = (1e-2, 1e-1, 1., 10.)
_CASES = {}


def rhos_of(shape):
    return RHO_PRIMAL if shape in PRIMAL else RHO_DUAL


def case(shape):
    """x, y, w and the path reference of a shape, computed once and shared (nobody changes it)."""
    if shape not in _CASES:
        n_in, order, n, m, weighted = shape
        x, y, w = lr.make_case(n_in, n, m, weighted, seed=n)
        _CASES[shape] = (x, y, w, ridge_path_reference(x, y, order, rhos_of(shape), w))
    return _CASES[shape]
