"""Reference values for the kernels of the device-resident FastICA iteration (``bfhip_ica_tanh``, ``bfhip_ica_assemble``,
``bfhip_ica_post``, ``bfhip_polar_ns``) and for the chunk logic around them, written from the operations' definitions in NumPy
``longdouble`` (x87 extended precision: 11 more bits than float64) and ``mpmath``.  It shares no code with
``bayesfast_amd.transforms.ica``.

One iteration of the parallel FastICA fixed point with the logcosh contrast, for white data X1 (n, d) and W (d, d):
    G = tanh(X1 W^T),  gmean_i = mean_r (1 - G[r, i]^2),  A = G^T X1 / n - gmean[:, None] W,
    W1 = (A A^T)^{-1/2} A,  lim = max_i | |sum_j W1[i, j] W[i, j]| - 1 |.
The device splits the rows into blocks of ``ROW_BLOCK`` for the sums of 1 - G^2 and into batches for G^T X1."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
ROW_BLOCK = 32
HAS_EXTENDED = np.finfo(LD).eps < 2.**-60


# ---- tanh ---------------------------------------------------------------------------------------------------------------

def tanh_mp(values):
    """tanh of float64 values by mpmath at 120 bits, as a longdouble array (non-finite inputs by the limits)."""
    import mpmath
    out = np.empty(len(values), dtype=LD)
    with mpmath.workprec(120):
        for i, v in enumerate(values):
            v = float(v)
            if np.isnan(v):
                out[i] = np.nan
            elif np.isinf(v):
                out[i] = np.sign(v)
            else:
                t = mpmath.tanh(mpmath.mpf(v))
                hi = float(t)                       # (two float64 pieces carry 106 bits into the longdouble)
                out[i] = LD(hi) + LD(float(t - mpmath.mpf(hi)))
    return out


def tanh_ld(y):
    """tanh of a float64 array in extended precision (the C library's tanhl; mpmath where longdouble is only a double)."""
    y = np.asarray(y, dtype=np.float64)
    if not HAS_EXTENDED:
        return tanh_mp(y.ravel()).reshape(y.shape)
    with np.errstate(all='ignore'):
        return np.tanh(y.astype(LD))


def ulp_distance(g, t):
    """|g - t| in units of the float64 spacing at |t|, for float64 g and extended-precision t (finite entries only: the others
    give 0 where both agree in kind and inf where they do not)."""
    g = np.asarray(g, dtype=np.float64)
    t64 = np.abs(t).astype(np.float64)
    fin = np.isfinite(t64)
    out = np.zeros(g.shape)
    with np.errstate(all='ignore'):
        out[fin] = (np.abs(g[fin].astype(LD) - t[fin]) / np.spacing(t64[fin]).astype(LD)).astype(np.float64)
    bad = ~fin & ~(np.isnan(g) & np.isnan(t64))
    out[bad] = np.inf
    out[fin & ~np.isfinite(g)] = np.inf
    return out


def tanh_partials(y, n):
    """For Y (n_pad, d): (tanh(Y) in extended precision, the (ceil(n_pad / ROW_BLOCK), d) sums of 1 - tanh^2 over each block's
    rows < n, the number of such rows per block)."""
    n_pad, d = y.shape
    t = tanh_ld(y)
    n_blk = -(-n_pad // ROW_BLOCK)
    part = np.zeros((n_blk, d), dtype=LD)
    rows = np.zeros(n_blk, dtype=int)
    with np.errstate(all='ignore'):
        for b in range(n_blk):
            lo, hi = b * ROW_BLOCK, min((b + 1) * ROW_BLOCK, n)
            if hi > lo:
                part[b] = (LD(1) - t[lo:hi] * t[lo:hi]).sum(0)
                rows[b] = hi - lo
    return t, part, rows


# ---- assemble and the convergence measure -------------------------------------------------------------------------------

def assemble(p, partial, w, n):
    """A = (sum_b P[b]) / n - gmean[:, None] W with gmean = colsum(partial) / n, and the worst-case bound of a float64
    evaluation in any summation order:  EPS ((nb + 1) sum_b |P[b, i, j]| / n + (n_blk + 3) sum_blk |partial[blk, i]| / n |W[i, j]|)."""
    nb, n_blk = p.shape[0], partial.shape[0]
    pl, gl, wl = p.astype(LD), partial.astype(LD), w.astype(LD)
    a = pl.sum(0) / LD(n) - (gl.sum(0) / LD(n))[:, None] * wl
    tol = EPS * ((nb + 1) * np.abs(pl).sum(0) / LD(n) + (n_blk + 3) * (np.abs(gl).sum(0) / LD(n))[:, None] * np.abs(wl))
    return a, tol.astype(np.float64)


def lim_measure(w1, w_old):
    """max_i | |sum_j W1[i, j] W_old[i, j]| - 1 | and the bound (d + 2) EPS max_i sum_j |W1 W_old| of a float64 evaluation."""
    prod = w1.astype(LD) * w_old.astype(LD)
    d = w1.shape[0]
    lim = np.max(np.abs(np.abs(prod.sum(1)) - LD(1)))
    return lim, float((d + 2) * EPS * np.abs(prod).sum(1).max())


def random_orthogonal(rng, d):
    q, r = np.linalg.qr(rng.normal(size=(d, d)))
    return np.ascontiguousarray(q * np.sign(np.diag(r)))


# ---- Newton-Schulz steps in extended precision --------------------------------------------------------------------------

def _matmul_ld(a, b, n_threads=8):
    """a @ b for longdouble matrices (NumPy's plain loops, row blocks side by side)."""
    idx = [i for i in np.array_split(np.arange(a.shape[0]), n_threads) if i.size]
    with ThreadPoolExecutor(len(idx)) as ex:
        return np.concatenate(list(ex.map(lambda i: a[i] @ b, idx)))


def newton_schulz(a, n_steps):
    """The iterates X_1 .. X_n_steps of X <- 1.5 X - 0.5 (X X^T) X from X_0 = A / sqrt(|A|_1 |A|_inf), in extended precision
    (X_0 itself is the float64 quotient the device starts from, to its rounding)."""
    al = a.astype(LD)
    x = al / np.sqrt(np.abs(al).sum(0).max() * np.abs(al).sum(1).max())
    out = []
    for _ in range(n_steps):
        t = _matmul_ld(x, np.ascontiguousarray(x.T))
        x = LD(1.5) * x - LD(0.5) * _matmul_ld(t, x)
        out.append(x)
    return out


# ---- the sequential fixed-point iteration on the host -------------------------------------------------------------------

def sources(rng, n, d):
    """Alternating Laplace and uniform sources mixed by I + 0.3 N(0, 1)."""
    s = np.empty((n, d))
    for j in range(d):
        s[:, j] = rng.laplace(size=n) if j % 2 == 0 else rng.uniform(-np.sqrt(3.), np.sqrt(3.), size=n)
    return s @ (np.eye(d) + 0.3 * rng.normal(size=(d, d)))


def whiten(x):
    """White data (n, d) with unit covariance from x (n, d), by the SVD of the centred data."""
    xc = x - x.mean(0)
    u, s, _ = np.linalg.svd(xc.T, full_matrices=False)
    u = u * np.sign(u[0])
    return np.ascontiguousarray((xc @ (u / s)) * np.sqrt(x.shape[0]))


def decorrelate(w):
    """(W W^T)^{-1/2} W by the symmetric eigen-decomposition."""
    s, u = np.linalg.eigh(w @ w.T)
    return (u / np.sqrt(s)) @ u.T @ w


def start_matrix(d, seed):
    """The decorrelated normal draw FastICA starts from for ``random_state=seed``."""
    return decorrelate(np.random.RandomState(seed).normal(size=(d, d)))


def fixed_point_sequence(x1, w0, n_iter):
    """n_iter iterations from w0 on white data x1 (n, d), float64: (iterates [W_1 ..], lims [lim_1 ..], assembled matrices [A_1 ..])."""
    n = x1.shape[0]
    w = np.array(w0, dtype=np.float64)
    iterates, lims, mats = [], [], []
    for _ in range(n_iter):
        g = np.tanh(x1 @ w.T)
        a = g.T @ x1 / n - (1. - g**2).mean(0)[:, None] * w
        w1 = decorrelate(a)
        lims.append(float(np.max(np.abs(np.abs((w1 * w).sum(1)) - 1.))))
        iterates.append(w1)
        mats.append(a)
        w = w1
    return iterates, np.array(lims), mats


def growth_ratios(x1, w0, n_iter, iterates, rng, size=1e-12):
    """How far a start perturbed by ``size`` (largest entry) has moved each iterate of the sequence, in units of ``size``: one
    ratio per iteration."""
    dw = rng.normal(size=w0.shape)
    dw *= size / np.abs(dw).max()
    moved, _, _ = fixed_point_sequence(x1, w0 + dw, n_iter)
    return np.array([np.abs(m - w).max() / size for m, w in zip(moved, iterates)])
