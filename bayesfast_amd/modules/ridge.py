"""The ridge path of the polynomial fit, scored by exact leave-one-out (``PolyModel.fit_ridge``).

Per design group, with A (n, P) the weighted design, B (n, m) the weighted targets and u the constant column (never penalised):

    minimise |B - A c|^2 + n rho sum_j D_j c_j^2,     D_j = sum_i A_ij^2 / n  (the mean square of column j: a convention that makes the
                                                       fit invariant to the scale of a column),

over the penalised columns.  u is projected out of the other columns and of B (A', B'), the columns are scaled (A_s = A' D^-1/2),
and ONE symmetric eigen-decomposition of the smaller side -- A_s^T A_s when n >= P_pen, A_s A_s^T otherwise -- gives eigenvalues Lam
and rows z_i with, for every lam = n rho,

    h_i = u_i^2 / |u|^2 + sum_j z_ij^2 / (Lam_j + lam),   fitted_i = sum_j z_ij T_j / (Lam_j + lam),   T = Z^T B',

and the held-out residual S_i / ((1 - h_i) w_i) exactly (ridge is least squares on augmented data; D is held fixed).  On the dual
side Z = U spans the complement of u and ``1 - h_i = sum_j U_ij^2 lam / (Lam_j + lam)``, ``S_i = sum_j U_ij lam / (Lam_j + lam) T_j``
are summed directly: ``1 - h`` is of the order lam / Lam there and ``1 - (...)`` would cancel.  u is kept out of U exactly by a shift:
u / |u| is a null vector of A_s A_s^T, and adding 2 trace(.) u u^T / |u|^2 makes it the eigenvector of the LARGEST eigenvalue, which
is dropped.

``ridge_path_host`` is this arithmetic in NumPy (tests of the selection and of ``RidgeReport`` need no GPU); ``ridge_group_device``
is the route of ``fit_ridge``: torch for the projection and ``eigh``, ``bfhip_gram``, ``bfhip_ridge_rotate`` and
``bfhip_ridge_path`` (csrc/bfhip_ridge.hip) for the passes over the rows.
"""
import numpy as np

from .. import _lib
from .fit_report import SUM_NAMES, ridge_score, ridge_choose

__all__ = ['DEFAULT_RIDGE', 'check_ridge', 'ridge_path_host', 'ridge_group_device']

# the default grid of rho: 15 half-decades from 1e-6 (on the dual side 1 - h is of the order rho: it is summed directly, and stays within
# 1.2e-12 of explicit refits at 1e-6 on the host, P = 78, n = 60; much below that the identity is noise whatever the route)
DEFAULT_RIDGE = tuple(10.**(-6 + k / 2) for k in range(15))


def check_ridge(ridge):
    """The grid of rho as a (L,) array: None is the default grid, else 1 to 32 positive numbers."""
    if ridge is None or ridge is True:
        ridge = DEFAULT_RIDGE
    try:
        ridge = np.array(ridge, dtype=np.float64).reshape(-1) if np.ndim(ridge) <= 1 else None
    except (TypeError, ValueError):
        ridge = None
    if ridge is None:
        raise ValueError('ridge should be None or a sequence of positive numbers.')
    if not 1 <= ridge.size <= _lib.RIDGE_MAX_L:
        raise ValueError('ridge should hold 1 to {} values, instead of {}.'.format(_lib.RIDGE_MAX_L, ridge.size))
    if not np.all(ridge > 0.) or not np.all(np.isfinite(ridge)):
        raise ValueError('every value of ridge should be positive and finite (rho <= 0 is not a ridge fit).')
    return ridge


def _sums_host(S, d, Bw, w):
    """The (m, 8) sums of fit_report.SUM_NAMES, resid and e_loo from S (n, m), d = 1 - h (n,), the weighted targets and the weights."""
    n, m = S.shape
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    ok = d > 0.
    inf = np.where(S < 0., -np.inf, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        sl = np.where(ok[:, None], S / d[:, None], inf)
        el = np.where(ok[:, None], S / (d * wv)[:, None], inf)
    al = np.abs(el)
    sums = np.zeros((m, len(SUM_NAMES)))
    sums[:, 0] = np.sum(S * S, axis=0)
    sums[:, 1] = np.sum(sl * sl, axis=0)
    sums[:, 2] = np.max(al, axis=0)
    sums[:, 3] = np.argmax(al, axis=0)
    sums[:, 4] = np.sum(Bw, axis=0)
    sums[:, 5] = np.sum(Bw * Bw, axis=0)
    sums[:, 6] = float(np.sum(~ok))
    return sums, S / wv[:, None], el


def ridge_path_host(A, B, ridge, u_col=0, w=None):
    """The tables of the ridge path of one design group, on the host.

    A (n, P) weighted design, B (n, m) weighted targets, ridge as for ``check_ridge``, u_col the index of the constant column or
    None (every column penalised then), w (n,) the row weights A and B were built with (only the units of ``e_loo`` and ``resid``
    need them).  Returns a dict: ridge (L,), h (n, L), sums (L, m, 8), dof (L,), resid and e_loo (L, n, m), coef (L, P, m), score
    (L,), index, at_edge, and dual (which side was decomposed)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    ridge = check_ridge(ridge)
    if not (A.ndim == 2 and B.ndim == 2 and A.shape[0] == B.shape[0]):
        raise ValueError('A (n, P) and B (n, m) should be 2-d arrays of one height.')
    n, P = A.shape
    if n < 3:
        raise ValueError('I need at least 3 points, but you only gave me {}.'.format(n))
    D = np.sum(A * A, axis=0) / n
    if u_col is None:
        pen, Ap, Bp, h0 = np.arange(P), A, B, np.zeros(n)
    else:
        u = A[:, u_col]
        uu = u @ u
        pen = np.delete(np.arange(P), u_col)
        uA, uB = u @ A[:, pen], u @ B
        Ap, Bp, h0 = A[:, pen] - np.outer(u, uA) / uu, B - np.outer(u, uB) / uu, u * u / uu
    with np.errstate(divide='ignore'):
        sc = np.where(D[pen] > 0., 1. / np.sqrt(D[pen]), 0.)   # (a column of zeros keeps a zero coefficient)
    As = Ap * sc
    dual = n < pen.size
    if not dual:
        Lam, V = np.linalg.eigh(As.T @ As)
        Z = As @ V
    else:
        M = As @ As.T
        if u_col is not None:
            c = 2. * np.trace(M)
            M = M + np.outer(u, u) * ((c if c > 0. else 1.) / uu)
        Lam, Z = np.linalg.eigh(M)
        if u_col is not None:
            Lam, Z = Lam[:-1], Z[:, :-1]
    Lam = np.maximum(Lam, 0.)
    T = Z.T @ Bp
    L, m = ridge.size, B.shape[1]
    out = dict(ridge=ridge, dual=bool(dual), h=np.zeros((n, L)), sums=np.zeros((L, m, len(SUM_NAMES))), resid=np.zeros((L, n, m)),
               e_loo=np.zeros((L, n, m)), coef=np.zeros((L, P, m)))
    for l in range(L):
        lam = n * ridge[l]
        g = (lam if dual else 1.) / (Lam + lam)
        acc_h, acc_f = (Z * Z) @ g, Z @ (T * g[:, None])
        if dual:
            d, S = acc_h, acc_f
            out['h'][:, l] = 1. - d
        else:
            out['h'][:, l] = h0 + acc_h
            d, S = 1. - out['h'][:, l], Bp - acc_f
        out['sums'][l], out['resid'][l], out['e_loo'][l] = _sums_host(S, d, B, w)
        q = T / (Lam + lam)[:, None]
        c_pen = sc[:, None] * ((As.T @ (Z @ q)) if dual else (V @ q))
        out['coef'][l][pen] = c_pen
        if u_col is not None:
            out['coef'][l][u_col] = (uB - uA @ c_pen) / uu
    out['dof'] = np.sum(out['h'], axis=0)
    out['score'] = ridge_score(out['sums'], n)
    out['index'], out['at_edge'] = ridge_choose(out['score'], ridge)
    return out


def ridge_group_device(ctx, A, B, wt, u_col, ridge, ws_doubles):
    """The ridge path of one design group on the device.  A (n, P) and B (n, m) are the weighted design and targets (device tensors of
    the context), wt the weights or None, ridge a checked (L,) array, ws_doubles the cap on the workspace the rotated rows take (the
    rows go through in passes beyond it; at least one tile of BFHIP_RIDGE_TILE rows is always given).  Returns the group's entry of a
    ``RidgeReport`` -- h (n,), resid and e_loo (n, m) at the chosen penalty as device tensors, path_sums (L, m, 8) and dof (L,) on
    the host -- and the coefficients (P, m) on the host."""
    import torch
    from ..device import _ptr
    lib, hd = ctx._lib, ctx.handle
    n, P = A.shape
    m = B.shape[1]
    cur = torch.cuda.current_stream(ctx.device)

    def to_torch():
        cur.wait_stream(ctx.stream)

    def to_lib():
        ctx.stream.wait_stream(cur)

    to_torch()
    D = (A * A).sum(0) / n
    if u_col is None:
        pen, As, Bp, h0 = None, A.clone(), B, None
        Dp = D
    else:
        u = A[:, u_col].clone()
        uu = u @ u
        pen = torch.cat([torch.arange(0, u_col, device=ctx.device), torch.arange(u_col + 1, P, device=ctx.device)])
        As = A[:, pen]
        uA, uB = u @ As, u @ B
        As -= u[:, None] * (uA / uu)[None, :]
        Bp = (B - u[:, None] * (uB / uu)[None, :]).contiguous()
        h0 = (u * u / uu).contiguous()
        Dp = D[pen]
    sc = torch.where(Dp > 0., 1. / torch.sqrt(Dp), torch.zeros_like(Dp))
    As *= sc[None, :]
    Pp = As.shape[1]
    dual = n < Pp
    if not dual:
        G, rhs = ctx.empty((Pp, Pp)), ctx.empty((Pp, m))
        to_lib()
        _lib.check(lib.bfhip_gram(hd, n, Pp, m, _ptr(As), Pp, _ptr(Bp), _ptr(G), _ptr(rhs)))
        to_torch()
        Lam, V = torch.linalg.eigh(G, UPLO='U')
        V = V.contiguous()
        T = (V.T @ rhs).contiguous()
        r, ldz = Pp, Pp
    else:
        M = As @ As.T
        if u_col is not None:
            c = 2. * torch.trace(M)
            M += (u[:, None] * u[None, :]) * (torch.where(c > 0., c, torch.ones_like(c)) / uu)
        Lam, V = torch.linalg.eigh(M)
        V = V.contiguous()
        r, ldz = (n - 1 if u_col is not None else n), n
        Lam = Lam[:r]
        T = (V[:, :r].T @ Bp).contiguous()
    if not bool(torch.isfinite(Lam).all()):
        raise np.linalg.LinAlgError('the eigen-decomposition of the ridge fit did not converge.')
    Lam = Lam.clamp(min=0.).contiguous()
    # rows per pass of the primal side's rotation Z = A_s V (the dual side's Z is U itself)
    tile = _lib.RIDGE_TILE
    n_up = -(-n // tile) * tile
    rows = n if dual else max(tile, min(n_up, int(ws_doubles) // r // tile * tile))
    Zws = V if dual else ctx.empty((min(rows, n), r))
    one_pass = rows >= n   # (the rotated rows then stay for the second sweep)

    def sweep(lams, with_resid, rotate):
        """h (n, L), sums (L, m, 8) and, for one penalty, resid and e_loo (n, m), with the buffers the launches use."""
        L = lams.size
        lam_t = ctx.tensor(lams, torch.float64)
        h, sums = ctx.empty((n, L)), ctx.empty((L, m, _lib.LOO_NSUM))
        resid = ctx.empty((n, m)) if with_resid else None
        e_loo = ctx.empty((n, m)) if with_resid else None
        n_work = _lib.ridge_work(min(rows, n), r, m, L)
        work = ctx.empty((n_work,))
        to_lib()
        for row0 in range(0, n, rows):
            nr = min(rows, n - row0)
            if rotate:
                _lib.check(lib.bfhip_ridge_rotate(hd, nr, Pp, r, _ptr(As[row0:]), Pp, _ptr(V), Pp, _ptr(Zws), r))
            _lib.check(lib.bfhip_ridge_path(
                hd, nr, r, m, L, _ptr(Zws), ldz, _ptr(Lam), _ptr(T), _ptr(lam_t), _ptr(Bp[row0:]), _ptr(B[row0:]),
                None if (dual or h0 is None) else _ptr(h0[row0:]), None if wt is None else _ptr(wt[row0:]), int(dual), row0,
                _ptr(h[row0:]), _ptr(sums), None if resid is None else _ptr(resid[row0:]),
                None if e_loo is None else _ptr(e_loo[row0:]), _ptr(work), n_work))
        to_torch()
        return h, sums, resid, e_loo, (lam_t, work)

    h, path_sums, _, _, buffers0 = sweep(n * ridge, False, not dual)
    dof = h.sum(0).cpu().numpy()
    path_sums = path_sums.cpu().numpy()
    index, _ = ridge_choose(ridge_score(path_sums, n), ridge)
    lam = float(n * ridge[index])
    h1, _, resid, e_loo, buffers1 = sweep(np.array([lam]), True, not dual and not one_pass)
    q = T / (Lam + lam)[:, None]
    c_pen = sc[:, None] * ((As.T @ (V[:, :r] @ q)) if dual else (V @ q))
    coef = torch.zeros((P, m), dtype=torch.float64, device=ctx.device)
    if u_col is None:
        coef.copy_(c_pen)
    else:
        coef[pen] = c_pen
        coef[u_col] = (uB - uA @ c_pen) / uu
    to_lib()
    ctx.synchronize()   # every launch above has run: the sweeps' buffers may go
    del buffers0, buffers1
    return dict(h=h1[:, 0].contiguous(), resid=resid, e_loo=e_loo, path_sums=path_sums, dof=dof), coef.cpu().numpy()
