"""What every user does next with the draws: look at the posterior.  ``marginals`` gives the one-dimensional histograms of the
parameters, the two-dimensional ones of their pairs and the bin values that enclose given fractions of the mass (the contour
levels of a triangle plot), computed where ``sample()`` left the draws: a few tens of MB of bins instead of the sample tensor over
PCIe and a host pass per pair.  The reference hands ``get()`` to getdist, and its SIT has a ``triangle_plot`` of its own.

Everything that is accumulated is a 64-bit integer.  Float atomics depend on the order of arrival; integer sums do not, so the
histograms are bitwise repeatable, whichever kernel shape, batch, column or rank a draw lands in -- and bins add, so under
``torch.distributed`` only bins cross between the ranks.

For n draws (all ranks) x (n, d):

  weights  w'_i = w_i / max(w), or exp(lw_i - max(lw)) for log weights; q_i = floor(w'_i 2^k) as uint64, k = 62 - ceil(log2 n)
           (62 for n = 1), so that sum q <= 2^62 fits a signed 64-bit sum over the ranks; q_i = 1 without weights.  The largest
           weight has q = 2^k exactly, so total = sum q >= 2^k; the truncation loses less than 2^-k of the largest weight per draw,
           n 2^-k <= 2^-30 of it in all (n <= 2^31 - 1, k >= 31).  Rows with q_i = 0 are not part of the sample, whatever they hold.
           A negative, NaN or +inf weight -- or no weight above zero -- makes every floating-point output NaN (as
           ``weighted_summary`` does) and every integer output 0.  No floating-point sum of weights is ever formed.
  ranges   given (lo < hi, finite, hi - lo finite), or per parameter the smallest and largest finite value among the rows with q > 0;
           lo == hi becomes [lo - 0.5, hi + 0.5]; a column with no finite value gets NaN edges and empty histograms.
  bins     inv = B / (hi - lo), once, on the host, in float64.  A finite value with lo <= x <= hi goes to bin
           min(floor((x - lo) inv), B - 1): a subtraction, then a multiplication.  Everything else is tallied per parameter in
           outside[:, 0 .. 2] -- below, above, not finite -- in units of q.  Edges are lo + j (hi - lo) / B.
           1 <= bins <= 1024, 1 <= bins2d <= 128.
  2-D      the pair (i, j) takes the rows where both coordinates are in range, at bins2d per axis: mass2d[p, a, b], a the bin of
           the pair's first parameter.  pairs='all': every i < j of ``params``; None: 1-D only; or a list of index pairs
           (positions in ``params``).  More than 2^31 - 1 bins in all raises.
  levels   for a histogram h with S = sum h and a probability p in (0, 1]: the largest bin value v with
           double(sum of the bins >= v) >= p double(S): the value at the first position of the descending order whose running sum
           reaches p S; invariant under ties and permutations, exact in integers.  An empty histogram has level 0.

Two routes compute the same integers.  NumPy arrays and CPU tensors take the host port; a GPU tensor takes the device route
(csrc/bfhip_marg.hip), batch by batch of 16 parameters as ``weighted_summary`` does: one batch buffer (8 bytes per draw and column
of the batch), q (8 bytes per draw, with weights only) and, when pairs are asked for, one byte per value of the bin indices -- an
eighth of a float32 sample tensor.  float32 and ``[:, since:]`` views go in without a copy.  The integers come to the host in one
copy at the end (with ``ranges=None`` the 2 d extremes come first: ``inv`` is formed on the host), and what follows from them --
edges, densities, intervals -- is host arithmetic in both routes, so the two agree bit for bit.  With ``weights=`` that holds for
everything; with ``log_weights=`` the device's exp and NumPy's may differ in the last place, which moves a q by a few units.  At most
2^31 - 1 draws; on the device route with pairs at most 256 parameters.

``marginals_sharded`` is the driver of both routes and of ``TraceTuple.marginals`` under ``torch.distributed``: the data passes sit
behind one object (``_HostPasses``, ``_DevicePasses``), the driver between them reduces over the ranks -- the maximum of the
weights, the number of draws, the extremes (``ranges=None``), and ONE sum of the int64 masses -- and the levels are computed after the
sum, on every rank.  The result is identical, bin for bin, to one process over all draws."""
import inspect

import numpy as np

from ._pipeline_data import host_f64

__all__ = ['marginals', 'marginals_of_shard', 'marginals_sharded', 'Marginals']

MAX_BINS, MAX_BINS2D = 1024, 128
_U64 = np.uint64


class Marginals:
    """``params`` (d,) the columns of x; ``ranges`` (d, 2) the lo, hi that were used; ``edges`` (d, bins + 1), ``edges2d`` (d, bins2d + 1); ``mass1d`` (d, bins) uint64;
    ``pairs`` (n_pair, 2) positions in ``params``, ``mass2d`` (n_pair, bins2d, bins2d) uint64, first axis the pair's first
    parameter; ``outside`` (d, 3) uint64: below, above, not finite; ``total`` = sum q over all rows (a Python int); ``probs``
    (n_p,), ``levels1d`` (n_p, d) and ``levels2d`` (n_p, n_pair) uint64.  Positions i, j below are positions in ``params``."""

    def __init__(self, params, ranges, edges, edges2d, mass1d, pairs, mass2d, outside, total, probs, levels1d, levels2d):
        self.params, self.edges, self.edges2d, self.mass1d, self.pairs, self.mass2d = params, edges, edges2d, mass1d, pairs, mass2d
        self.outside, self.total, self.probs, self.levels1d, self.levels2d = outside, int(total), probs, levels1d, levels2d
        self.ranges = ranges
        self._pair = {(int(a), int(b)): k for k, (a, b) in reversed(list(enumerate(pairs)))}

    def _width(self, edges, i):
        return (edges[i, -1] - edges[i, 0]) / (edges.shape[1] - 1)

    def _den(self):
        return float(self.total) if self.total > 0 else np.nan

    def density1d(self, i):
        """(bins,) mass / total / bin width: integrates to the fraction of the mass inside the range."""
        with np.errstate(all='ignore'):
            return self.mass1d[i].astype(np.float64) / self._den() / self._width(self.edges, i)

    def _pair_index(self, i, j):
        if (i, j) not in self._pair:
            raise KeyError('the pair (%d, %d) was not asked for.' % (i, j))
        return self._pair[(i, j)]

    def density2d(self, i, j):
        """(bins2d, bins2d) mass / total / bin area of the pair (i, j), first axis parameter i."""
        with np.errstate(all='ignore'):
            area = self._width(self.edges2d, i) * self._width(self.edges2d, j)
            return self.mass2d[self._pair_index(i, j)].astype(np.float64) / self._den() / area

    def level_density1d(self, i):
        """(n_p,) the levels of parameter i in the units of ``density1d``."""
        with np.errstate(all='ignore'):
            return self.levels1d[:, i].astype(np.float64) / self._den() / self._width(self.edges, i)

    def level_density2d(self, i, j):
        """(n_p,) the levels of the pair in the units of ``density2d``: what ``contour(levels=...)`` wants (ascending: reversed)."""
        with np.errstate(all='ignore'):
            area = self._width(self.edges2d, i) * self._width(self.edges2d, j)
            return self.levels2d[:, self._pair_index(i, j)].astype(np.float64) / self._den() / area

    def interval(self, i, prob):
        """The credible region of parameter i at ``prob`` (one of ``probs``): the list of [a, b] runs of bins at or above the level."""
        k = np.flatnonzero(self.probs == prob)
        if k.size == 0:
            raise ValueError('prob should be one of probs.')
        level = self.levels1d[k[0], i]
        on = (self.mass1d[i] >= level) & (self.mass1d[i] > 0)
        step = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
        return [[float(self.edges[i, a]), float(self.edges[i, b])] for a, b in zip(np.flatnonzero(step == 1), np.flatnonzero(step == -1))]

    def __repr__(self):
        return 'Marginals(n_param=%d, bins=%d, n_pair=%d, bins2d=%d, total=%d, probs=%s)' % (
            len(self.params), self.mass1d.shape[1], len(self.pairs), self.edges2d.shape[1] - 1, self.total,
            tuple(float(p) for p in self.probs))


def weight_shift(n):
    """k of the fixed-point weights of n draws: n 2^k <= 2^62."""
    return 62 - (int(n) - 1).bit_length()


# ---- arithmetic shared by the routes (host, float64) -------------------------------------------------------------------------------
def _bin_constants(lo, hi, bins):
    """inv (d,) and edges (d, bins + 1) of the ranges lo, hi (d,); NaN where the range is NaN."""
    with np.errstate(all='ignore'):
        span = hi - lo
        return bins / span, lo[:, None] + np.arange(bins + 1, dtype=np.float64)[None, :] * span[:, None] / bins


def _default_ranges(lo, hi):
    """The ranges from the extremes: +inf / -inf (no finite value) -> NaN; lo == hi -> half a unit to either side."""
    lo, hi = np.array(lo, dtype=np.float64) + 0., np.array(hi, dtype=np.float64) + 0.    # (-0. -> 0.: one sign for both routes)
    none = ~(lo <= hi)
    lo[none], hi[none] = np.nan, np.nan
    flat = lo == hi
    lo[flat], hi[flat] = lo[flat] - 0.5, hi[flat] + 0.5
    with np.errstate(all='ignore'):
        if np.isinf(hi - lo).any():
            raise ValueError('the range of a parameter overflows float64: give ranges.')
    return lo, hi


def _levels_host(h, probs):
    """h (n_hist, m) uint64 -> (levels (n_p, n_hist) uint64, S (n_hist,) uint64): the descending order's running sum."""
    out = np.zeros((len(probs), h.shape[0]), dtype=_U64)
    tot = h.sum(axis=1, dtype=_U64)
    for a in range(h.shape[0]):
        if tot[a] == 0:
            continue
        v = np.sort(h[a])[::-1]
        # the running sum at the LAST position of every run of equal values, as a double: the sum of the bins >= that value
        run = np.cumsum(v, dtype=_U64)
        last = np.concatenate([v[1:] != v[:-1], [True]])
        vals, sums = v[last], run[last].astype(np.float64)
        for i, p in enumerate(probs):
            out[i, a] = vals[np.argmax(sums >= p * np.float64(tot[a]))]
    return out, tot


def _slots(x, lo, hi, inv, bins):
    """The bin 0 .. bins - 1 of every value of x (n,), or bins below, bins + 1 above, bins + 2 not finite."""
    with np.errstate(all='ignore'):
        s = np.full(x.shape, bins + 2, dtype=np.int64)
        fin = np.isfinite(x)
        s[fin & (x < lo)] = bins
        s[fin & (x > hi)] = bins + 1
        inside = fin & (lo <= x) & (x <= hi)
        t = np.floor((x[inside] - lo) * inv)
        s[inside] = np.where(t < bins - 1, t, bins - 1).astype(np.int64)
    return s


class _HostPasses:
    """The data passes on a host shard: x (n, d) float64, the weights as given (``kind`` 'log', 'lin' or None)."""
    device = 'cpu'

    def __init__(self, x, given, kind):
        self.x, self.given, self.kind = x, given, kind
        self.n, self.d = x.shape
        self.q = None

    def weight_top(self):
        import torch
        g = self.given
        with np.errstate(all='ignore'):
            bad = np.isnan(g) | (g == np.inf) | ((g < 0) if self.kind == 'lin' else False)
            top = np.where(np.isnan(g), -np.inf, g).max() if g.size else -np.inf
        return torch.tensor([top, float(bad.any())], dtype=torch.float64)

    def quantise(self, top, k):
        if self.kind is None:
            self.q = np.ones(self.n, dtype=_U64)
            return
        top, g = float(top), self.given
        with np.errstate(all='ignore'):
            wp = np.exp(g - top) if self.kind == 'log' else g / top
            ok = (wp >= 0) & (wp <= 1)
            self.q = np.floor(np.ldexp(np.where(ok, wp, 0.), k)).astype(_U64)
        self.n_bad = int((~ok).sum())

    def extent(self):
        import torch
        keep = self.q > 0
        x = np.where(np.isfinite(self.x[keep]), self.x[keep], np.nan)
        out = np.full((2, self.d), -np.inf)
        if x.shape[0]:
            with np.errstate(all='ignore'):
                out[0], out[1] = np.fmax.reduce(-x, axis=0), np.fmax.reduce(x, axis=0)
            out[np.isnan(out)] = -np.inf
        return torch.as_tensor(out)

    def hist(self, lo, hi, bins, bins2d, pairs):
        import torch
        d, q = self.d, self.q
        inv, inv2 = _bin_constants(lo, hi, bins)[0], _bin_constants(lo, hi, bins2d)[0]
        m1, out = np.zeros((d, bins), dtype=_U64), np.zeros((d, 3), dtype=_U64)
        idx = np.empty((self.n, d), dtype=np.int64)
        keep = q > 0
        for c in range(d):    # a column at a time
            xc = np.ascontiguousarray(self.x[:, c])
            s = _slots(xc, lo[c], hi[c], inv[c], bins)
            np.add.at(m1[c], s[keep & (s < bins)], q[keep & (s < bins)])
            np.add.at(out[c], s[keep & (s >= bins)] - bins, q[keep & (s >= bins)])
            if len(pairs):
                idx[:, c] = _slots(xc, lo[c], hi[c], inv2[c], bins2d)
        m2 = np.zeros((len(pairs), bins2d * bins2d), dtype=_U64)
        for p, (i, j) in enumerate(pairs):
            ok = keep & (idx[:, i] < bins2d) & (idx[:, j] < bins2d)
            np.add.at(m2[p], idx[ok, i] * bins2d + idx[ok, j], q[ok])
        flag = np.array([getattr(self, 'n_bad', 0)], dtype=_U64)
        return torch.as_tensor(np.concatenate([m1.reshape(-1), out.reshape(-1), m2.reshape(-1), flag]).view(np.int64))

    def levels(self, flat, d, bins, n_pair, bins2d, probs):
        f = flat.numpy().view(_U64)
        m1, m2 = f[:d * bins].reshape(d, bins), f[d * (bins + 3):d * (bins + 3) + n_pair * bins2d**2].reshape(n_pair, bins2d**2)
        l1 = _levels_host(m1, probs)[0]
        l2 = _levels_host(m2, probs)[0] if n_pair else np.zeros((len(probs), 0), dtype=_U64)
        return f, l1, l2


class _DevicePasses:
    """The data passes on a device shard: x (n_chain, n_draw, d) device tensor, the weights (n,) float64 on the same device."""

    def __init__(self, x, given, kind):
        import torch
        from .. import _lib
        from ..device import get_context
        from .diagnostics import _device_batches
        self.x, self.given, self.kind = x, given, kind
        self.n, self.d = int(x.shape[0]) * int(x.shape[1]), int(x.shape[2])
        self.device = x.device
        _device_batches(x, self.n)    # (the size limit, before anything is allocated)
        self.ctx = get_context(x.device.index)
        self.q = None
        self.flag = torch.zeros((1,), dtype=torch.int64, device=x.device)
        self.buf = self.ctx.empty((max(self.n, 1), _lib.DIAG_BATCH))

    def _batches(self):
        from .diagnostics import _device_batches
        return _device_batches(self.x, self.n)

    def _columns(self, xb, kb, nb):
        import torch
        from .. import _lib
        from ..device import _ptr
        _lib.check(self.ctx._lib.bfhip_wstat_columns(self.ctx.handle, int(xb.shape[0]), int(xb.shape[1]), int(xb.stride(0)),
                                                     int(xb.stride(1)), _ptr(xb), int(xb.dtype == torch.float32), 0, kb, nb, None,
                                                     _ptr(self.buf)))

    def weight_top(self):
        import torch
        g = self.given
        bad = torch.isnan(g) | (g == np.inf)
        if self.kind == 'lin':
            bad |= g < 0
        if g.numel() == 0:
            return torch.tensor([-np.inf, 0.], dtype=torch.float64, device=self.device)
        top = torch.where(torch.isnan(g), torch.full_like(g, -np.inf), g).max()
        return torch.stack([top, bad.any().to(torch.float64)])

    def quantise(self, top, k):
        import torch
        from .. import _lib
        from ..device import _ptr
        if self.kind is None or self.n == 0:
            return    # q = None: every row counts once
        with torch.cuda.device(self.device):
            wp = (torch.exp(self.given - top) if self.kind == 'log' else self.given / top).contiguous()
            self.q = torch.empty((self.n,), dtype=torch.int64, device=self.device)
            _lib.check(self.ctx._lib.bfhip_marg_quantise(self.ctx.handle, self.n, _ptr(wp), int(k), _ptr(self.q), _ptr(self.flag)))

    def extent(self):
        import torch
        from .. import _lib
        from ..device import _ptr
        out = torch.full((2, self.d), -np.inf, dtype=torch.float64, device=self.device)
        if self.n == 0:
            return out
        with torch.cuda.device(self.device):
            work = self.ctx.empty((_lib.MARG_EXTENT_WORK,))
            lo, hi = self.ctx.empty((_lib.DIAG_BATCH,)), self.ctx.empty((_lib.DIAG_BATCH,))
            k0 = 0
            for xb, kb, nb in self._batches():
                self._columns(xb, kb, nb)
                _lib.check(self.ctx._lib.bfhip_marg_extent(self.ctx.handle, self.n, _ptr(self.buf), _ptr(self.q), _ptr(lo), _ptr(hi),
                                                           _ptr(work)))
                out[0, k0:k0 + nb], out[1, k0:k0 + nb] = -lo[:nb], hi[:nb]
                k0 += nb
        return out

    def hist(self, lo, hi, bins, bins2d, pairs):
        import torch
        from .. import _lib
        from ..device import _ptr
        d, n, w = self.d, self.n, _lib.DIAG_BATCH
        n_pair = len(pairs)
        n1, n2 = d * bins, n_pair * bins2d * bins2d
        flat = torch.zeros((d * (bins + 3) + n2 + 1,), dtype=torch.int64, device=self.device)
        if n == 0:
            return flat
        lib, h = self.ctx._lib, self.ctx.handle
        with torch.cuda.device(self.device):
            pad = lambda v: np.concatenate([v, np.full((-len(v)) % w, np.nan)]).reshape(-1, w)
            inv, inv2 = _bin_constants(lo, hi, bins)[0], _bin_constants(lo, hi, bins2d)[0]
            consts = torch.as_tensor(np.stack([pad(lo), pad(hi), pad(inv), pad(inv2)]), device=self.device)   # (4, n_batch, 16)
            if n_pair:
                ld = 16
                while ld < d:
                    ld *= 2
                idx = torch.empty((n, ld), dtype=torch.uint8, device=self.device)
            for b, (xb, kb, nb) in enumerate(self._batches()):
                self._columns(xb, kb, nb)
                # a batch's histograms are rows b 16 .. of (d, bins): whole batches are contiguous, the last one gets a buffer of its own
                h1 = torch.zeros((w, bins), dtype=torch.int64, device=self.device)
                o1 = torch.zeros((w, 3), dtype=torch.int64, device=self.device)
                _lib.check(lib.bfhip_marg_hist1d(h, n, _ptr(self.buf), _ptr(self.q), _ptr(consts[0, b]), _ptr(consts[1, b]),
                                                 _ptr(consts[2, b]), nb, bins, _ptr(h1), _ptr(o1)))
                flat[b * w * bins:(b * w + nb) * bins] = h1[:nb].reshape(-1)
                flat[n1 + b * w * 3:n1 + (b * w + nb) * 3] = o1[:nb].reshape(-1)
                if n_pair:
                    _lib.check(lib.bfhip_marg_index(h, n, _ptr(self.buf), _ptr(consts[0, b]), _ptr(consts[1, b]), _ptr(consts[3, b]), nb,
                                                    bins2d, _ptr(idx), ld, b * w))
            if n_pair:
                pairs_d = torch.as_tensor(np.ascontiguousarray(pairs, dtype=np.int32), device=self.device)
                h2 = flat[d * (bins + 3):d * (bins + 3) + n2]
                if h2.data_ptr() % 8:
                    raise RuntimeError('misaligned histogram buffer.')
                _lib.check(lib.bfhip_marg_hist2d(h, n, _ptr(idx), ld, _ptr(pairs_d), n_pair, _ptr(self.q), bins2d, _ptr(h2)))
            flat[-1:] = self.flag
        return flat

    def levels(self, flat, d, bins, n_pair, bins2d, probs):
        import torch
        from .. import _lib
        from ..device import _ptr
        lib, h = self.ctx._lib, self.ctx.handle
        n_p = len(probs)
        with torch.cuda.device(self.device):
            flat = flat.contiguous()
            probs_d = torch.as_tensor(probs, device=self.device)
            lv = torch.zeros(((d + n_pair) * n_p + d + n_pair,), dtype=torch.int64, device=self.device)
            l1, l2 = lv[:d * n_p], lv[d * n_p:(d + n_pair) * n_p]
            tot = lv[(d + n_pair) * n_p:]
            _lib.check(lib.bfhip_marg_levels(h, d, bins, _ptr(flat), n_p, _ptr(probs_d), _ptr(l1), _ptr(tot[:d])))
            if n_pair:
                h2 = flat[d * (bins + 3):]
                _lib.check(lib.bfhip_marg_levels(h, n_pair, bins2d * bins2d, _ptr(h2), n_p, _ptr(probs_d), _ptr(l2), _ptr(tot[d:])))
            both = torch.cat([flat, lv]).cpu().numpy().view(_U64)    # the one copy to the host, after the last launch
        f, lv = both[:flat.numel()], both[flat.numel():]
        return (f, np.ascontiguousarray(lv[:d * n_p].reshape(d, n_p).T),
                np.ascontiguousarray(lv[d * n_p:(d + n_pair) * n_p].reshape(n_pair, n_p).T))


# ---- options -------------------------------------------------------------------------------------------------------------------------
def _check_options(d_all, bins, bins2d, ranges, params, pairs, probs):
    bins, bins2d = int(bins), int(bins2d)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError('bins should be in 1 .. %d.' % MAX_BINS)
    if not 1 <= bins2d <= MAX_BINS2D:
        raise ValueError('bins2d should be in 1 .. %d.' % MAX_BINS2D)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if probs.ndim != 1 or probs.size == 0 or not ((probs > 0) & (probs <= 1)).all():
        raise ValueError('probs should be probabilities in (0, 1].')
    params = np.arange(d_all) if params is None else np.atleast_1d(np.asarray(params)).astype(np.int64)
    if params.ndim != 1 or params.size == 0 or (params < 0).any() or (params >= d_all).any():
        raise ValueError('params should be column indices of x.')
    d = len(params)
    if pairs is None:
        pairs = np.zeros((0, 2), dtype=np.int64)
    elif isinstance(pairs, str):
        if pairs != 'all':
            raise ValueError('pairs should be \'all\', None or a list of index pairs.')
        if d * (d - 1) // 2 * bins2d * bins2d > 2**31 - 1:
            raise ValueError('more than 2^31 - 1 two-dimensional bins.')
        pairs = np.stack(np.triu_indices(d, 1), axis=1).astype(np.int64)
    else:
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if (pairs < 0).any() or (pairs >= d).any():
            raise ValueError('pairs should hold positions in params.')
    if len(pairs) * bins2d * bins2d > 2**31 - 1:
        raise ValueError('more than 2^31 - 1 two-dimensional bins.')
    if ranges is not None:
        ranges = np.asarray(ranges, dtype=np.float64)
        if ranges.shape != (d, 2):
            raise ValueError('ranges should be (n_param, 2).')
        with np.errstate(all='ignore'):
            if not (np.isfinite(ranges).all() and (ranges[:, 0] < ranges[:, 1]).all() and np.isfinite(ranges[:, 1] - ranges[:, 0]).all()):
                raise ValueError('ranges should be finite with lo < hi.')
    return bins, bins2d, ranges, params, pairs, probs


def marginals_sharded(passes, bins, bins2d, ranges, params, pairs, probs, stats=None, collective=True):
    """The driver: ``passes`` holds this rank's draws (columns ``params`` already selected) and weights; the options are checked
    ones.  With more than one rank a collective that every rank calls; every rank returns the same ``Marginals``.  ``stats``, if a
    dict, receives 'collectives'.  ``collective=False``: this process alone, whatever the process group (``utils.marginals``)."""
    import torch
    from .. import parallel
    ws = parallel.world()[1] if collective else 1
    n_coll = 0
    d, n_pair = passes.d, len(pairs)
    top = None
    if passes.kind is not None:
        t = passes.weight_top()
        if ws > 1:
            t = parallel.all_reduce_max(t)
            n_coll += 1
        top = torch.where(t[1] > 0, torch.full_like(t[0], np.nan), t[0])
    n_all = passes.n
    if ws > 1:
        n_all = int(parallel.all_reduce_sum(torch.tensor([passes.n], dtype=torch.int64, device=passes.device)).item())
        n_coll += 1
    if n_all < 1:
        raise ValueError('x is empty.')
    if n_all > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 draws.')
    k = weight_shift(n_all)
    passes.quantise(top, k)
    if ranges is None:
        e = passes.extent()
        if ws > 1:
            e = parallel.all_reduce_max(e)
            n_coll += 1
        e = e.cpu().numpy()
        lo, hi = _default_ranges(-e[0], e[1])
    else:
        lo, hi = np.array(ranges[:, 0]), np.array(ranges[:, 1])
    flat = passes.hist(lo, hi, bins, bins2d, pairs)
    if ws > 1:
        flat = parallel.all_reduce_sum(flat)      # the one sum of the masses: bins add
        n_coll += 1
    f, l1, l2 = passes.levels(flat, d, bins, n_pair, bins2d, probs)
    if stats is not None:
        stats['collectives'] = n_coll
    n1, n2 = d * bins, n_pair * bins2d * bins2d
    mass1d, outside = np.array(f[:n1]).reshape(d, bins), np.array(f[n1:n1 + 3 * d]).reshape(d, 3)
    mass2d = np.array(f[n1 + 3 * d:n1 + 3 * d + n2]).reshape(n_pair, bins2d, bins2d)
    total = int(mass1d[0].sum(dtype=_U64)) + int(outside[0].sum(dtype=_U64))
    edges, edges2d = _bin_constants(lo, hi, bins)[1], _bin_constants(lo, hi, bins2d)[1]
    if int(f[-1]) != 0 or total == 0:    # a weight that is negative or not finite, or none above zero
        mass1d[:], outside[:], mass2d[:], l1[:], l2[:], total = 0, 0, 0, 0, 0, 0
        edges[:], edges2d[:], lo[:], hi[:] = np.nan, np.nan, np.nan, np.nan
    return Marginals(params, np.stack([lo, hi], axis=1), edges, edges2d, mass1d, pairs, mass2d, outside, total, probs, l1, l2)


def _weights_of(x_shape, log_weights, weights):
    if log_weights is not None and weights is not None:
        raise ValueError('at most one of log_weights and weights should be given.')
    given = weights if log_weights is None else log_weights
    kind = None if given is None else ('lin' if log_weights is None else 'log')
    n = int(np.prod(x_shape[:-1]))
    if given is not None and tuple(given.shape) != tuple(x_shape[:-1]) and tuple(given.shape) != (n,):
        raise ValueError('the weights should have the shape x.shape[:-1], or be flat of that size.')
    return given, kind


def _make_passes(x, given, kind, params, d_all):
    """x (n, d) or (n_chain, n_draw, d), host or device, with its weights -> the passes over the columns ``params``."""
    whole = len(params) == d_all and (params == np.arange(d_all)).all()
    if getattr(x, 'is_cuda', False):
        import torch
        if not whole:
            x = x[..., torch.as_tensor(params, device=x.device)]
        g = None if given is None else torch.as_tensor(given, device=x.device).detach().reshape(-1).to(torch.float64)
        return _DevicePasses(x.detach() if x.ndim == 3 else x.detach()[None], g, kind)
    xh = host_f64(x).reshape(-1, x.shape[-1])
    return _HostPasses(xh if whole else xh[:, params], None if given is None else host_f64(given).reshape(-1), kind)


def marginals_of_shard(x, log_weights=None, weights=None, collective=True, **options):
    """``marginals`` of ALL ranks' draws, of which ``x`` (n, d) or (n_chain_local, n_draw, d), host or device, with its weights is
    this rank's shard; ``options`` are those of ``marginals`` (``OPTIONS`` has the defaults).  With more than one rank a collective
    that every rank calls (``marginals_sharded``); every rank returns the same ``Marginals``.  ``collective=False``: this process
    alone, which a device shard allows only without a process group."""
    unknown = set(options) - set(OPTIONS)
    if unknown:
        raise TypeError('unexpected options: %s.' % ', '.join(sorted(unknown)))
    d_all = int(x.shape[-1])
    given, kind = _weights_of(tuple(x.shape), log_weights, weights)
    checked = _check_options(d_all, **dict(OPTIONS, **options))
    if getattr(x, 'is_cuda', False):
        from .. import _lib, parallel
        if not collective and parallel.world()[1] > 1:
            raise NotImplementedError('utils.marginals on a device tensor is single-process: TraceTuple.marginals is the collective.')
        if len(checked[4]) and len(checked[3]) > _lib.MARG_MAX_LD:
            raise NotImplementedError('pairs of more than %d parameters on the device route.' % _lib.MARG_MAX_LD)
    return marginals_sharded(_make_passes(x, given, kind, checked[3], d_all), *checked, collective=collective)


def marginals(x, log_weights=None, weights=None, bins=64, bins2d=64, ranges=None, params=None, pairs='all', probs=(0.68, 0.95)):
    """The marginal histograms of the draws x (n, d) or (n_chain, n_draw, d): a ``Marginals`` with the 1-D histograms of the columns
    ``params`` (default: all) at ``bins`` bins, the 2-D ones of ``pairs`` ('all': every i < j; None; or a list of pairs of positions
    in ``params``) at ``bins2d`` bins per axis, and the levels that enclose the fractions ``probs`` of each histogram's mass.
    At most one of ``log_weights`` / ``weights``, of shape ``x.shape[:-1]`` or flat of that size, not necessarily normalised;
    ``ranges`` (n_param, 2), default the extremes of the draws.  A GPU ``x`` is reduced on its device (float32 is read as float64, a
    ``[:, since:]`` view goes in without a copy; single process); arrays and CPU tensors take the host port."""
    if x.ndim not in (2, 3):
        raise ValueError('x should be (n, d) or (n_chain, n_draw, d).')
    if int(np.prod(x.shape[:-1])) < 1 or x.shape[-1] < 1:
        raise ValueError('x is empty.')
    return marginals_of_shard(x, log_weights, weights, collective=False, bins=bins, bins2d=bins2d, ranges=ranges, params=params,
                              pairs=pairs, probs=probs)


# the options and their defaults, as ``marginals`` declares them: bins, bins2d, ranges, params, pairs, probs
OPTIONS = {name: p.default for name, p in list(inspect.signature(marginals).parameters.items())[3:]}
