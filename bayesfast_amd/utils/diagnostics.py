"""Convergence diagnostics of many chains: rank-normalised split-R-hat, bulk / tail / mean effective sample size and the
per-parameter table of mean, sd and quantiles (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021, "Rank-normalization, folding,
and localization: an improved R-hat for assessing convergence of MCMC").  The reference has no such diagnostic (its DynamicSample
recipe raises NotImplementedError, core/recipe.py:571-574); ``integrated_time`` normalises every walker by its own variance, so it
cannot see chains that disagree with each other -- these can.

For one parameter, x (M chains, N draws), N >= 4:

  split   h = N // 2; with N odd the first draw of every chain is left out of everything.  Every chain gives two chains of n = h
          consecutive draws: m = 2 M split chains, S = m n values.
  z(y)    rank normalisation: r the 1-based rank among the S values, ties sharing their mean rank; z = ndtri((r - 3/8) / (S + 1/4))
  R(y)    W = mean_j s_j^2 (ddof 1), V = sum_j (ybar_j - ybar)^2 / (m - 1), var+ = (n - 1) / n W + V, R = sqrt(var+ / W)
  rhat    'rank': max(R(z(x)), R(z(|x - median|)));  'split': R(x)
  ESS(y)  a_j(t) = sum_{s < n - t} (y_js - ybar_j)(y_j,s+t - ybar_j), rho_t = 1 - (W - mean_j a_j(t) / (n - 1)) / var+,
          P_k = rho_2k + rho_2k+1 (2 k + 1 <= n - 1), K the first k >= 1 with P_k < 0 (or the number of pairs), P'_k the running
          minimum, tau = max(-1 + 2 sum_{k < K} P'_k, 1 / log10 S), ESS = S / tau   (Geyer's initial monotone sequence)
  ess     'bulk': ESS(z(x));  'tail': min over q in prob of ESS(1[x <= Q_q]);  'mean': ESS(x);  mcse_mean = sd / sqrt(ess_mean)

A parameter with a non-finite draw has NaN in every column.  A constant parameter has its value as mean and quantiles, sd 0 and
NaN (the 0 / 0 of the formulas) elsewhere -- in every function and method, decided by comparing the smallest draw with the largest,
not by a variance of 0 (the sum of n copies of 0.1 is not n times 0.1, and the rounding would pass for a converged chain).

Two routes compute the same numbers.  NumPy arrays and CPU tensors take the host port (FFT autocovariances,
``scipy.stats.rankdata``).  A GPU tensor takes the device route, batch by batch of 16 parameters (csrc/bfhip_diag.hip): the column
kernel writes the batch's split layout (m, n, 16) -- plain, folded or as an indicator -- straight out of the time-major sample
tensor (a ``[:, since:]`` view goes in without a copy), every column is sorted once (the sorted keys give the median, the table's
quantiles and the tail thresholds; the rank kernel turns them into normal scores in place), and the chain moments and
autocovariance sums are ``bfhip_acor_moments`` / ``bfhip_acor_lag_sums``.  Geyer's sequence is walked over lag blocks as
``integrated_time_sharded`` does: 64 lags first, every further block twice as long, until every series of the batch has met its
first negative pair; only the (n_lag, 16) sums of a block reach the host.  Working memory is one batch whatever n_d is: the series
buffer (8 bytes per value) and one column's sort buffers (about 36 bytes per value of ONE column): 0.3 of the sample tensor at
n_d = 64.  Input that the column kernel cannot read in place (a dtype other than float64 / float32, or a last axis that is not
contiguous) is converted one batch at a time: one more batch-sized buffer, 0.55 in all.
Every reduction has a fixed order and a batch always has 16 columns (unused ones are zero), so the same input gives the same
bits, whichever batch or column a parameter lands in.

Single process: the ranks are global over all chains, so under ``torch.distributed`` the chains have to be gathered first.
At most 2^31 - 1 values per column."""
import time

import numpy as np

__all__ = ['rhat', 'ess', 'summary', 'Summary']

FIRST_BLOCK = 64   # lags of the first block of the Geyer walk; every further block doubles
_PLAIN, _FOLD, _BELOW = 0, 1, 2


# ---- the estimators on (m, B)-sized arrays: shared by the two routes -------------------------------------------------------------
def _chain_stats(cm, a0, n):
    """cm, a0 (m, B): the chains' means and centred sums of squares -> dict of (B,) arrays.  Every column is reduced on its own
    contiguous row, so its bits do not depend on its neighbours."""
    cm, a0 = np.ascontiguousarray(cm.T), np.ascontiguousarray(a0.T)
    m = cm.shape[1]
    with np.errstate(all='ignore'):
        w = (a0 / (n - 1)).sum(axis=1) / m
        mean = cm.sum(axis=1) / m
        dev2 = ((cm - mean[:, None])**2).sum(axis=1)
        varp = (n - 1) / n * w + dev2 / (m - 1)
        return dict(w=w, varp=varp, mean=mean, rhat=np.sqrt(varp / w), sd=np.sqrt((a0.sum(axis=1) + n * dev2) / (m * n - 1)))


def _geyer_tau(st, m, n, lag_sums, skip):
    """tau (B,) by Geyer's initial monotone sequence.  ``lag_sums(t0, n_lag)`` -> (n_lag, B) host array of sum_j a_j(t) for
    t0 <= t < t0 + n_lag, asked for in blocks of 64, 128, 256 ... lags until every column not in ``skip`` has a negative pair
    (or a NaN sequence, which never gets one)."""
    w, varp = st['w'], st['varp']
    n_lags = 2 * (n // 2)   # the pairs k with 2 k + 1 <= n - 1
    pairs, t0, n_lag = [], 0, FIRST_BLOCK
    decided = np.array(skip, dtype=bool)
    with np.errstate(all='ignore'):
        while True:
            nl = min(n_lag, n_lags - t0)
            rho = 1. - (w - np.asarray(lag_sums(t0, nl), dtype=np.float64) / m / (n - 1)) / varp
            pairs.append(rho[0::2] + rho[1::2])
            t0 += nl
            p = np.concatenate(pairs, axis=0)
            neg = p[1:] < 0
            decided |= neg.any(axis=0) | np.isnan(p[0])
            if t0 >= n_lags or decided.all():
                break
            n_lag *= 2
        k_stop = np.where(neg.any(axis=0), neg.argmax(axis=0) + 1, p.shape[0]) if neg.shape[0] else 1
        kept = np.where(np.arange(p.shape[0])[:, None] < k_stop, np.minimum.accumulate(p, axis=0), 0.)
        tau = -1. + 2. * kept.sum(axis=0)    # (rows are added in order; the zeros beyond a column's K change nothing)
        return np.maximum(tau, 1. / np.log10(m * n))


def _positions(s, q):
    """np.quantile's linear rule on s sorted values: (lower index, upper index, weight) per probability."""
    q = np.asarray(q, dtype=np.float64)
    pos = s * q + (1. + q * -1.) - 1.
    lo = np.clip(np.floor(pos), 0, s - 1).astype(np.int64)
    return lo, np.minimum(lo + 1, s - 1), pos - lo


def _lerp(a, b, t):
    with np.errstate(all='ignore'):
        d = b - a
        return np.where(t >= 0.5, b - d * (1. - t), a + d * t)


def _check_probs(p, name):
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if p.ndim != 1 or p.size == 0 or not ((p >= 0) & (p <= 1)).all():
        raise ValueError(name + ' should be probabilities in [0, 1].')
    return p


def _batch(be, want, probs, prob):
    """Every requested statistic of one batch.  ``be``: the route's backend, with ``m``, ``n``, ``columns(mode, c)`` -> a series
    (``moments()`` -> (cm, a0) host (m, B); ``extent()`` -> (smallest, largest) host (B,); ``lag_sums(t0, n_lag)``) and ``sort_rank(series, idx)`` -> (sorted values at idx,
    (len(idx), B) host; the series of normal scores, which may take the place of the sorted one)."""
    m, n = be.m, be.n
    s = m * n
    out = {}
    x = be.columns(_PLAIN, None)
    st = _chain_stats(*x.moments(), n)
    bad = ~np.isfinite(st['mean']) | ~np.isfinite(st['sd'])
    # a constant column by exact comparison: the centred sums of n copies of 0.1 are not 0, and would pass for a converged chain
    first, last = x.extent()
    const = (first == last) & ~bad
    out.update(mean=st['mean'], sd=st['sd'], rhat_split=st['rhat'])
    if 'ess_mean' in want:
        out['ess_mean'] = s / _geyer_tau(st, m, n, x.lag_sums, bad | const)
        with np.errstate(all='ignore'):
            out['mcse_mean'] = st['sd'] / np.sqrt(out['ess_mean'])
    if want & {'quantiles', 'rhat', 'ess_bulk', 'ess_tail'}:
        # one sort of the plain column: ends (non-finite columns), median, table quantiles, tail thresholds
        lo_q, hi_q, t_q = _positions(s, np.concatenate([probs, prob]))
        idx = np.concatenate([[0, s - 1, s // 2 - 1, s // 2], lo_q, hi_q])
        v, z = be.sort_rank(x, idx)
        bad |= ~np.isfinite(v[0]) | ~np.isfinite(v[1])
        const &= ~bad
        with np.errstate(all='ignore'):
            median = (v[2] + v[3]) / 2.
        nq = len(lo_q)
        qv = _lerp(v[4:4 + nq], v[4 + nq:], t_q[:, None])
        out['quantiles'] = qv[:len(probs)]
        zst = _chain_stats(*z.moments(), n)
        if 'ess_bulk' in want:
            out['ess_bulk'] = s / _geyer_tau(zst, m, n, z.lag_sums, bad | const)
        if 'rhat' in want:
            _, zf = be.sort_rank(be.columns(_FOLD, median), idx[:1])
            out['rhat'] = np.maximum(zst['rhat'], _chain_stats(*zf.moments(), n)['rhat'])
        if 'ess_tail' in want:
            tails = []
            for c in qv[len(probs):]:
                ind = be.columns(_BELOW, c)
                tails.append(s / _geyer_tau(_chain_stats(*ind.moments(), n), m, n, ind.lag_sums, bad | const))
            out['ess_tail'] = np.minimum.reduce(tails)
    # a constant column: mean and quantiles are the constant (not what a rounded sum of n copies gives), sd 0, the rest 0 / 0
    for k, v in out.items():
        if k == 'mean' and const.any():
            v[const] = first[const]
        elif k == 'sd':
            v[const] = 0.
        elif k != 'quantiles' and k != 'mean':
            v[const] = np.nan
        v[..., bad] = np.nan
    return out


# ---- the host port ----------------------------------------------------------------------------------------------------------------
class _HostSeries:
    def __init__(self, y):
        self.y = y       # (m, n, B)
        self._acov = None

    def moments(self):
        with np.errstate(all='ignore'):
            cm = self.y.mean(axis=1)
            return cm, ((self.y - cm[:, None])**2).sum(axis=1)

    def extent(self):
        with np.errstate(all='ignore'):
            return self.y.min(axis=(0, 1)), self.y.max(axis=(0, 1))

    def lag_sums(self, t0, n_lag):
        if self._acov is None:   # every lag at once: the zero-padded FFT gives the linear autocovariance sums
            n = self.y.shape[1]
            n_fft = 2 << max(n - 1, 0).bit_length()
            with np.errstate(all='ignore'):
                spec = np.fft.rfft(self.y - self.y.mean(axis=1, keepdims=True), n=n_fft, axis=1)
                self._acov = np.fft.irfft(spec * np.conjugate(spec), n=n_fft, axis=1)[:, :n].sum(axis=0)
        return self._acov[t0:t0 + n_lag]


class _HostBackend:
    def __init__(self, x):
        """x (M, 2 h, B) float64"""
        big_m, n2, b = x.shape
        self.m, self.n = 2 * big_m, n2 // 2
        self.x = x.reshape(self.m, self.n, b)

    def columns(self, mode, c):
        with np.errstate(all='ignore'):
            if mode == _FOLD:
                return _HostSeries(np.abs(self.x - c))
            if mode == _BELOW:
                return _HostSeries((self.x <= c).astype(np.float64))
        return _HostSeries(self.x)

    def sort_rank(self, series, idx):
        from scipy.special import ndtri
        from scipy.stats import rankdata
        flat = series.y.reshape(-1, series.y.shape[2])
        s = flat.shape[0]
        v = np.sort(flat, axis=0)[idx]
        z = ndtri((rankdata(flat, method='average', axis=0) - 0.375) / (s + 0.25))
        return v, _HostSeries(z.reshape(series.y.shape))


# ---- the device route -------------------------------------------------------------------------------------------------------------
class _Clock:
    """Wall-clock seconds per phase around a synchronise, when the caller asked for them (``stats``); nothing otherwise."""

    def __init__(self, stats, torch):
        self.stats, self.torch = stats, torch

    def __call__(self, name):
        self.name = name
        return self

    def __enter__(self):
        if self.stats is not None:
            self.torch.cuda.synchronize()
            self.t = time.perf_counter()

    def __exit__(self, *exc):
        if self.stats is not None:
            self.torch.cuda.synchronize()
            self.stats[self.name] = self.stats.get(self.name, 0.) + time.perf_counter() - self.t


class _DeviceSeries:
    def __init__(self, be, buf):
        self.be, self.buf, self.mean = be, buf, None

    def moments(self):
        from .. import _lib
        from ..device import _ptr
        be = self.be
        with be.clock('moments'):
            self.mean = be.ctx.empty((be.m, _lib.DIAG_BATCH))
            inv = be.ctx.empty((be.m, _lib.DIAG_BATCH))
            _lib.check(be.lib.bfhip_acor_moments(be.ctx.handle, be.m, be.n, _lib.DIAG_BATCH, be.n * _lib.DIAG_BATCH, _ptr(self.buf),
                                                 _ptr(self.mean), _ptr(inv)))
            cm, inv = self.mean.cpu().numpy()[:, :be.nb], inv.cpu().numpy()[:, :be.nb]
        with np.errstate(all='ignore'):
            return cm, 1. / inv

    def extent(self):
        from .. import _lib
        from ..device import _ptr
        be = self.be
        with be.clock('moments'):
            lo, hi = be.ctx.empty((be.m, _lib.DIAG_BATCH)), be.ctx.empty((be.m, _lib.DIAG_BATCH))
            _lib.check(be.lib.bfhip_diag_extent(be.ctx.handle, be.m, be.n, _ptr(self.buf), _ptr(lo), _ptr(hi)))
            return lo.cpu().numpy()[:, :be.nb].min(axis=0), hi.cpu().numpy()[:, :be.nb].max(axis=0)

    def lag_sums(self, t0, n_lag):
        from .. import _lib
        from ..device import _ptr
        be = self.be
        with be.clock('lags'):
            work = be.ctx.empty((min(be.m, _lib.ACOR_MAX_GROUPS) * n_lag * _lib.DIAG_BATCH,))
            out = be.ctx.empty((n_lag, _lib.DIAG_BATCH))
            _lib.check(be.lib.bfhip_acor_lag_sums(be.ctx.handle, be.m, be.n, _lib.DIAG_BATCH, be.n * _lib.DIAG_BATCH, _ptr(self.buf),
                                                  _ptr(self.mean), _ptr(be.ones), int(t0), int(n_lag), _ptr(work), _ptr(out)))
            return out.cpu().numpy()[:, :be.nb]


class _DeviceBackend:
    """One batch of at most 16 parameters of x (M, N, n_d), a float64 or float32 device tensor with unit stride along n_d.  The
    buffers (``shared``) are allocated once per call and reused by every batch."""

    def __init__(self, x, row0, h, k0, nb, shared, clock):
        self.x, self.row0, self.k0, self.nb, self.clock = x, row0, k0, nb, clock
        self.m, self.n = 2 * int(x.shape[0]), h
        self.ctx, self.lib = shared['ctx'], shared['ctx']._lib
        self.buf, self.keys, self.order, self.ones = shared['buf'], shared['keys'], shared['order'], shared['ones']

    def columns(self, mode, c):
        import torch
        from .. import _lib
        from ..device import _ptr
        x = self.x
        with self.clock('columns'):
            cd = None if c is None else torch.as_tensor(np.ascontiguousarray(c, dtype=np.float64), device=x.device)
            _lib.check(self.lib.bfhip_diag_columns(self.ctx.handle, int(x.shape[0]), self.n, int(x.stride(0)), int(x.stride(1)), _ptr(x),
                                                   int(x.dtype == torch.float32), self.row0, self.k0, self.nb, mode, _ptr(cd),
                                                   _ptr(self.buf)))
        return _DeviceSeries(self, self.buf)

    def sort_rank(self, series, idx):
        import torch
        from .. import _lib
        from ..device import _ptr
        s = self.m * self.n
        idx_d = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=self.x.device)
        picked = torch.empty((self.nb, len(idx)), dtype=torch.int64, device=self.x.device)
        for b in range(self.nb):
            with self.clock('sort'):
                _lib.check(self.lib.bfhip_diag_sort(self.ctx.handle, s, _ptr(series.buf), b, _ptr(self.keys), _ptr(self.order)))
                picked[b] = self.keys[idx_d]
            with self.clock('rank'):
                _lib.check(self.lib.bfhip_diag_rank(self.ctx.handle, s, _ptr(self.keys), _ptr(self.order), b, _ptr(series.buf)))
        # the order-preserving keys back to float64 (bf_order_key: sign bit set for v >= 0, all bits flipped below)
        u = picked.cpu().numpy().T.view(np.uint64)
        bits = np.where(u >> np.uint64(63), u & np.uint64(0x7fffffffffffffff), ~u)
        return bits.view(np.float64), _DeviceSeries(self, series.buf)


def _device_batches(x, n_rows):
    """The batches of at most 16 parameters of x (n_chain, n_t, n_d), each as (tensor the column kernels read, first column in
    it, number of columns); ``n_rows`` values per parameter go through the kernels.  They read float64 or float32 with unit stride
    along n_d in place; anything else is converted batch by batch (one more batch-sized buffer, never a copy of the whole tensor).
    The size limit is checked at the call, before the caller allocates anything; the batches come from the generator returned."""
    import torch
    from .. import _lib
    if n_rows > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 values per parameter.')
    in_place = x.dtype in (torch.float64, torch.float32) and (x.shape[2] == 1 or x.stride(2) == 1)
    n_d, w = int(x.shape[2]), _lib.DIAG_BATCH

    def batches():
        for k0 in range(0, n_d, w):
            nb = min(w, n_d - k0)
            if in_place:
                yield x, k0, nb
            else:
                yield x[:, :, k0:k0 + nb].to(torch.float64).contiguous(), 0, nb
    return batches()


def _device_backends(x, clock):
    import torch
    from .. import _lib
    from ..device import get_context
    big_m, n_t = int(x.shape[0]), int(x.shape[1])
    h = n_t // 2
    s = 2 * big_m * h
    batches = _device_batches(x, s)
    ctx = get_context(x.device.index)
    shared = dict(ctx=ctx, buf=ctx.empty((2 * big_m, h, _lib.DIAG_BATCH)), keys=ctx.empty((s,), dtype=torch.int64),
                  order=ctx.empty((s,), dtype=torch.int32),
                  ones=torch.ones((2 * big_m, _lib.DIAG_BATCH), dtype=torch.float64, device=x.device))
    for xb, k0, nb in batches:
        yield _DeviceBackend(xb, n_t & 1, h, k0, nb, shared, clock)


def _host_batches(x):
    from .. import _lib
    x = np.asarray(x.detach().numpy() if hasattr(x, 'detach') else x, dtype=np.float64)
    n_t = x.shape[1]
    for k0 in range(0, x.shape[2], _lib.DIAG_BATCH):
        yield _HostBackend(np.ascontiguousarray(x[:, n_t & 1:, k0:k0 + _lib.DIAG_BATCH]))


def _compute(x, want, probs=(), prob=(0.05, 0.95), stats=None):
    probs, prob = _check_probs(probs, 'probs') if len(probs) else np.zeros(0), _check_probs(prob, 'prob')
    if x.ndim not in (2, 3):
        raise ValueError('x should be (n_chain, n_t) or (n_chain, n_t, n_d).')
    if x.ndim == 2:
        x = x[:, :, None]
    if x.shape[1] < 4:
        raise ValueError('at least 4 draws per chain are needed.')
    if x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError('x is empty.')
    if getattr(x, 'is_cuda', False):
        import torch
        with torch.cuda.device(x.device):
            parts = [_batch(be, want, probs, prob) for be in _device_backends(x, _Clock(stats, torch))]
    else:
        parts = [_batch(be, want, probs, prob) for be in _host_batches(x)]
    return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]}


def rhat(x, method='rank'):
    """R-hat (n_d,) of x (n_chain, n_t) or (n_chain, n_t, n_d): 'rank', the larger of the rank-normalised split-R-hat of the draws
    and of their absolute deviations from the median, or 'split', the plain split-R-hat.  Values above about 1.01 say that the
    chains have not mixed.  A GPU tensor is reduced on its device; arrays and CPU tensors take the host port."""
    if method not in ('rank', 'split'):
        raise ValueError('invalid value for method.')
    return _compute(x, {'rhat'} if method == 'rank' else set())['rhat' if method == 'rank' else 'rhat_split']


def ess(x, method='bulk', prob=(0.05, 0.95)):
    """Effective sample size (n_d,): 'bulk' (of the rank-normalised draws), 'tail' (the smaller of the ESS of the indicators
    x <= Q_q, q in ``prob``) or 'mean' (of the draws themselves)."""
    if method not in ('bulk', 'tail', 'mean'):
        raise ValueError('invalid value for method.')
    return _compute(x, {'ess_' + method}, prob=prob)['ess_' + method]


class Summary:
    """The table of ``summary``: ``names`` and one (n_d,) array per column, as attributes, by ``[name]`` and in ``as_dict()``."""

    def __init__(self, columns):
        self._columns = dict(columns)
        self.names = tuple(self._columns)
        self.__dict__.update(self._columns)

    def __getitem__(self, name):
        return self._columns[name]

    def as_dict(self):
        return dict(self._columns)

    def __str__(self):
        rows = [''.join(['%5s' % ''] + ['%12s' % k for k in self.names])]
        for i in range(len(self._columns[self.names[0]])):
            rows.append('%5d' % i + ''.join('%12.5g' % self._columns[k][i] for k in self.names))
        return '\n'.join(rows)

    __repr__ = __str__


def _table(x, probs, prob, stats=None):
    """``summary``; ``stats``, if a dict, makes the device route synchronise around its phases and receives their seconds
    ('columns', 'sort', 'rank', 'moments', 'lags'): for tools/diag_rate.py."""
    probs = _check_probs(probs, 'probs')
    r = _compute(x, {'quantiles', 'ess_mean', 'ess_bulk', 'ess_tail', 'rhat'}, probs, prob, stats)
    cols = [('mean', r['mean']), ('sd', r['sd'])]
    cols += [('q%g' % (100 * p), r['quantiles'][i]) for i, p in enumerate(probs)]
    cols += [(k, r[k]) for k in ('mcse_mean', 'ess_bulk', 'ess_tail', 'rhat')]
    return Summary(cols)


def summary(x, probs=(0.05, 0.5, 0.95), prob=(0.05, 0.95)):
    """The posterior table of x (n_chain, n_t) or (n_chain, n_t, n_d): mean, sd (ddof 1), the quantiles at ``probs``
    (``np.quantile``'s linear rule; columns 'q5', 'q50', 'q95'), mcse_mean, ess_bulk, ess_tail (thresholds at ``prob``) and rhat,
    each column sorted once."""
    return _table(x, probs, prob)
