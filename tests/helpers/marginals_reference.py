"""A reference for ``bayesfast_amd.utils.marginals`` written from the definitions in its docstring and independently of its host
port: Python integers throughout (no uint64 array arithmetic), the histograms by ``np.bincount`` on 21-bit limbs of the
fixed-point weights (every limb sum stays below 2^21 2^31 = 2^52, so the float64 sums of ``bincount`` are exact) or, for small inputs, by a
loop over the rows with ``math.floor``; the level by trying every distinct bin value."""
import math

import numpy as np


def shift(n_all):
    """62 - ceil(log2 n), the ceiling found by search: the largest k with n 2^k <= 2^62."""
    c = 0
    while (1 << c) < n_all:
        c += 1
    return 62 - c


def quantise(n, weights=None, log_weights=None, n_all=None, top=None):
    """-> (list of n Python ints, bad).  ``top`` / ``n_all``: the maximum and the draw count of all shards, when this is one shard."""
    n_all = n if n_all is None else n_all
    k = shift(n_all)
    if weights is None and log_weights is None:
        return [1] * n, False
    g = np.asarray(weights if log_weights is None else log_weights, dtype=np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        bad = bool(np.isnan(g).any() or (g == np.inf).any() or (weights is not None and (g < 0).any()))
        if top is None:
            top = g.max()
        wp = g / top if log_weights is None else np.exp(g - top)
    if bad or not np.isfinite(top) or (log_weights is None and not top > 0):
        return [0] * n, True
    return [int(math.floor(math.ldexp(float(v), k))) for v in wp], False


def slot(v, lo, hi, inv, b):
    """One value: its bin, or b below, b + 1 above, b + 2 not finite."""
    if not math.isfinite(v):
        return b + 2
    if v < lo:
        return b
    if v > hi:
        return b + 1
    if not (lo <= v <= hi):
        return b + 2
    return min(int(math.floor((v - lo) * inv)), b - 1)


def slots(x, lo, hi, inv, b):
    """A column, vectorised; the same rule (tests hold it to ``slot`` on small inputs)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape, dtype=np.int64)
    with np.errstate(all='ignore'):
        fin = np.isfinite(x)
        below, above = fin & (x < lo), fin & (x > hi)
        inside = fin & ~below & ~above & (x >= lo) & (x <= hi)
        out[:] = b + 2
        out[below] = b
        out[above] = b + 1
        out[inside] = np.minimum(np.floor((x[inside] - lo) * inv), b - 1).astype(np.int64)
    return out


def exact_bincount(where, q, size):
    """sum of the Python ints q over equal ``where``: three limbs of 21 bits."""
    ql = np.array([[(v >> s) & 0x1fffff for s in (0, 21, 42)] for v in q], dtype=np.float64).reshape(-1, 3)
    out = [0] * size
    for li, s in enumerate((0, 21, 42)):
        c = np.bincount(where, weights=ql[:, li], minlength=size)
        for j in np.flatnonzero(c):
            out[j] += int(c[j]) << s
    return out


def default_ranges(x, q):
    d = x.shape[1]
    lo, hi = np.full(d, np.nan), np.full(d, np.nan)
    keep = np.array([v > 0 for v in q], dtype=bool)
    for c in range(d):
        col = x[keep, c]
        col = col[np.isfinite(col)]
        if col.size:
            a, e = float(col.min()) + 0., float(col.max()) + 0.
            if a == e:
                a, e = a - 0.5, e + 0.5
            lo[c], hi[c] = a, e
    return lo, hi


def level(h, p):
    """The largest bin value v with float(sum of bins >= v) >= p float(S); h a list of Python ints."""
    total = sum(h)
    if total == 0:
        return 0
    vals, counts = _unique(h)
    best, run = None, 0
    for v, c in zip(vals[::-1], counts[::-1]):    # descending: run = sum of the bins >= v
        run += v * c
        if float(run) >= p * float(total) and best is None:
            best = v
    return best


def _unique(h):
    cnt = {}
    for v in h:
        cnt[v] = cnt.get(v, 0) + 1
    vals = sorted(cnt)
    return vals, [cnt[v] for v in vals]


def histograms(x, q, lo, hi, bins, bins2d, pairs, loops=False):
    """-> mass1d (d x bins), outside (d x 3), mass2d (n_pair x bins2d^2) as lists of Python ints."""
    n, d = x.shape
    keep = [i for i in range(n) if q[i] > 0]
    qk = [q[i] for i in keep]
    m1, out, idx2 = [], [], {}
    with np.errstate(all='ignore'):
        inv, inv2 = bins / (hi - lo), bins2d / (hi - lo)
    for c in range(d):
        col = x[keep, c]
        if loops:
            s = np.array([slot(float(v), lo[c], hi[c], inv[c], bins) for v in col], dtype=np.int64).reshape(-1)
            s2 = np.array([slot(float(v), lo[c], hi[c], inv2[c], bins2d) for v in col], dtype=np.int64).reshape(-1)
        else:
            s, s2 = slots(col, lo[c], hi[c], inv[c], bins), slots(col, lo[c], hi[c], inv2[c], bins2d)
        if loops:
            row = [0] * (bins + 3)
            for j, v in zip(s, qk):
                row[j] += v
        else:
            row = exact_bincount(s, qk, bins + 3)
        m1.append(row[:bins])
        out.append(row[bins:])
        idx2[c] = s2
    m2 = []
    for i, j in pairs:
        ok = (idx2[i] < bins2d) & (idx2[j] < bins2d)
        where = idx2[i][ok] * bins2d + idx2[j][ok]
        qq = [v for v, o in zip(qk, ok) if o]
        if loops:
            row = [0] * (bins2d * bins2d)
            for w_, v in zip(where, qq):
                row[w_] += v
        else:
            row = exact_bincount(where, qq, bins2d * bins2d)
        m2.append(row)
    return m1, out, m2


def reference(x, weights=None, log_weights=None, bins=64, bins2d=64, ranges=None, pairs='all', probs=(0.68, 0.95), loops=False,
              levels=True):
    """The whole result as a dict of uint64 arrays (and ``total`` a Python int, ``lo`` / ``hi``, ``bad``)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    n, d = x.shape
    q, bad = quantise(n, weights, log_weights)
    if pairs == 'all':
        pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    elif pairs is None:
        pairs = []
    if ranges is None:
        lo, hi = default_ranges(x, q)
    else:
        lo, hi = np.asarray(ranges, dtype=np.float64)[:, 0], np.asarray(ranges, dtype=np.float64)[:, 1]
    m1, out, m2 = histograms(x, q, lo, hi, bins, bins2d, pairs, loops)
    total = sum(q)
    u = lambda rows, m: np.array([[int(v) for v in r] for r in rows], dtype=np.uint64).reshape(len(rows), m)
    res = dict(mass1d=u(m1, bins), outside=u(out, 3), mass2d=u(m2, bins2d * bins2d).reshape(len(pairs), bins2d, bins2d), total=total,
               lo=lo, hi=hi, bad=bad or total == 0, q=q, pairs=pairs)
    if levels:
        res['levels1d'] = np.array([[level(h, p) for h in m1] for p in probs], dtype=np.uint64).reshape(len(probs), d)
        res['levels2d'] = np.array([[level(h, p) for h in m2] for p in probs], dtype=np.uint64).reshape(len(probs), len(pairs))
    return res


def assert_equal(got, ref, label=''):
    """Every integer of a ``Marginals`` against the reference, with ==."""
    if ref['bad']:
        assert got.total == 0 and not got.mass1d.any() and not got.mass2d.any() and not got.outside.any(), label
        assert np.isnan(got.edges).all() and np.isnan(got.edges2d).all(), label
        assert not got.levels1d.any() and not got.levels2d.any(), label
        return
    assert got.total == ref['total'], (label, got.total, ref['total'])
    for k in ('mass1d', 'outside', 'mass2d') + (('levels1d', 'levels2d') if 'levels1d' in ref else ()):
        a, b = getattr(got, k), ref[k]
        assert a.dtype == np.uint64 and a.shape == b.shape, (label, k, a.shape, b.shape)
        assert np.array_equal(a, b), (label, k, int((a != b).sum()))
    assert np.array_equal(got.ranges[:, 0], ref['lo'], equal_nan=True) and np.array_equal(got.ranges[:, 1], ref['hi'], equal_nan=True), label
    assert np.array_equal(got.edges[:, 0], ref['lo'], equal_nan=True), label
