"""What follows the importance weights of the PostStep: Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry
2024, "Pareto smoothed importance sampling"; the tail fit is Zhang & Stephens 2009) and the posterior table of WEIGHTED draws.  The
reference clips the weights at mean(w) n^k_trunc (core/recipe.py:1289-1296), which hides a heavy tail instead of reporting it;
``psis`` reports the tail's shape ``khat`` -- below 0.5 good, above 0.7 unreliable: refit the surrogate -- and ``weighted_summary``
gives mean, sd and quantiles once the weights are applied.

``psis``, for S log ratios lw:

  shift    lw -= max(lw)
  tail     M = min(floor(0.2 S), ceil(3 sqrt(S))).  M < 5: no smoothing, khat = inf.  Otherwise a stable ascending sort; cut is the
           value at sorted position S - M - 1 (0-based), the tail the last M sorted values, x_i = exp(tail_i) - exp(cut) ascending.
           x_M <= 0 (a tail without spread): no smoothing, khat = inf.
  fit      n = M, m = 30 + floor(sqrt(n)); theta_j = 1 / x_n + (1 - sqrt(m / (j - 1/2))) / (3 x_[floor(n / 4 + 1/2)]), j = 1 .. m;
           k_j = mean_i log1p(-theta_j x_i); L_j = n (log(-theta_j / k_j) - k_j - 1); omega_j = 1 / sum_l exp(L_l - L_j);
           theta = sum_j omega_j theta_j; k = mean_i log1p(-theta x_i); sigma = -k / theta; khat = (k n + 5) / (n + 10)
  smooth   sorted tail position i = 1 .. M gets log(exp(cut) + sigma expm1(-khat log1p(-p_i)) / khat), p_i = (i - 1/2) / M -- the
           fitted distribution's quantile function; -sigma log1p(-p_i) inside the logarithm when khat == 0 -- capped at 0, the
           shifted maximum, and goes back to its original position through the sort's permutation
  results  log_mean_weight = max + logsumexp(lw) - log S, the smoothed estimate of log(Z_p / Z_q); log_weights = lw - logsumexp(lw);
           ess = 1 / sum w^2 (Kish)

-inf entries are zero weights: they sort first and count in S.  A NaN or +inf anywhere -- or no entry above -inf -- makes every
output NaN.

``weighted_summary``, with the weights normalised to sum 1; rows of zero weight are not part of the sample, whatever they hold:

  mean       sum w x
  sd         sqrt(sum w (x - mean)^2 / (1 - sum w^2)): with equal weights the ddof = 1 of ``summary``
  mcse_mean  sqrt(sum w^2 (x - mean)^2): the standard error of self-normalised importance sampling with INDEPENDENT draws.  It
             ignores the autocorrelation between the draws of a chain; where that matters, ``summary``'s ess_bulk says by how much.
  ess        sd^2 (1 - sum w^2) / mcse_mean^2, per parameter;  ess_kish = 1 / sum w^2, the one global number, in every row
  quantiles  the column sorted (stable), C_k the running sum of the permuted weights, mid_k = C_k - w_(k) / 2, pos_k = (mid_k - mid_1) /
             (mid_n - mid_1); for probability q, k the last index with pos_k <= q; the value is x_(n) for k = n, otherwise
             lerp(x_(k), x_(k+1), (q - pos_k) / (pos_(k+1) - pos_k)).  With equal weights this is ``np.quantile``'s linear rule.

A column with a non-finite draw of non-zero weight is NaN everywhere.  A constant column (smallest == largest among the rows of
non-zero weight, compared exactly, as in ``diagnostics``) has its value as mean and quantiles, sd 0 and NaN elsewhere.  With one
draw, or one weight equal to 1, mean and quantiles are that draw and the rest is NaN.  A negative or non-finite weight makes
the whole table NaN.

Two routes compute the same numbers, as in ``diagnostics``: NumPy arrays and CPU tensors take a host port, a GPU tensor the device
route (csrc/bfhip_psis.hip).  The table walks the parameters in batches of 16: one batch buffer and one column's sort buffers,
whatever n_d is.  Every device reduction has a fixed order, so the same input gives the same bits, whichever batch or column
a parameter lands in.  At most 2^31 - 1 values."""
import numpy as np

from ._pipeline_data import host_f64
from .diagnostics import Summary, _check_probs, _device_batches, _lerp

__all__ = ['psis', 'PSISResult', 'weighted_summary']


class PSISResult:
    """``log_weights`` (smoothed, logsumexp 0, the input's shape and order: a device tensor on the device route, an array on the
    host port) and the floats ``khat``, ``sigma``, ``log_mean_weight``, ``ess`` and the int ``n_tail``."""

    def __init__(self, log_weights, khat, sigma, n_tail, log_mean_weight, ess):
        self.log_weights, self.khat, self.sigma, self.n_tail = log_weights, float(khat), float(sigma), int(n_tail)
        self.log_mean_weight, self.ess = float(log_mean_weight), float(ess)

    def __repr__(self):
        return 'PSISResult(khat=%.4g, sigma=%.4g, n_tail=%d, log_mean_weight=%.6g, ess=%.6g)' % (
            self.khat, self.sigma, self.n_tail, self.log_mean_weight, self.ess)


def tail_size(s):
    """M of ``psis`` for S values."""
    return min(int(np.floor(0.2 * s)), int(np.ceil(3. * np.sqrt(s))))


# ---- psis: the host port -------------------------------------------------------------------------------------------------------------
def _gpd_fit(x):
    """Zhang & Stephens' posterior-mean fit to ascending exceedances x (n,): (k, sigma) before the prior on k."""
    n = len(x)
    m = 30 + int(np.floor(np.sqrt(n)))
    j = np.arange(1, m + 1, dtype=np.float64)
    theta = 1. / x[-1] + (1. - np.sqrt(m / (j - 0.5))) / (3. * x[int(np.floor(n / 4. + 0.5)) - 1])
    k = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
    big_l = n * (np.log(-theta / k) - k - 1.)
    omega = 1. / np.exp(big_l[None, :] - big_l[:, None]).sum(axis=1)
    th = (omega * theta).sum()
    k = np.log1p(-th * x).mean()
    return k, -k / th


def _psis_host(lw):
    s = lw.size
    m_tail = tail_size(s)
    nan = np.nan
    with np.errstate(all='ignore'):
        top = lw.max() if not np.isnan(lw).any() else nan
        if not np.isfinite(top):
            return np.full(s, nan), nan, nan, m_tail, nan, nan
        lw = lw - top
        khat, sigma = np.inf, nan
        if m_tail >= 5:
            order = np.argsort(lw, kind='stable')
            cut = lw[order[s - m_tail - 1]]
            x = np.exp(lw[order[s - m_tail:]]) - np.exp(cut)
            if x[-1] > 0:
                k, sigma = _gpd_fit(x)
                khat = (k * m_tail + 5.) / (m_tail + 10.)
                l1p = np.log1p(-(np.arange(m_tail) + 0.5) / m_tail)
                q = -sigma * l1p if khat == 0 else sigma * np.expm1(-khat * l1p) / khat
                v = np.log(np.exp(cut) + q)
                lw[order[s - m_tail:]] = np.where(v > 0, 0., v)
        lse = np.log(np.exp(lw).sum())
        lw = lw - lse
        return lw, khat, sigma, m_tail, top + lse - np.log(s), 1. / np.exp(2. * lw).sum()


# ---- psis: the device route ----------------------------------------------------------------------------------------------------------
def _psis_device(logp, logq):
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    n = logp.numel()
    if n > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 values.')
    with torch.cuda.device(logp.device):
        ctx = get_context(logp.device.index)
        a = logp.detach().reshape(-1).to(torch.float64).contiguous()
        b = None if logq is None else torch.as_tensor(logq, device=logp.device).detach().reshape(-1).to(torch.float64).contiguous()
        lw, out8 = ctx.empty((n,)), ctx.empty((8,))
        work = ctx.empty((_lib.psis_work_bytes(n),), dtype=torch.uint8)
        _lib.check(ctx._lib.bfhip_psis(ctx.handle, n, _ptr(a), _ptr(b), _ptr(lw), _ptr(out8), _ptr(work), work.numel()))
        o = out8.cpu().numpy()   # the one copy to the host, after the last launch
    return PSISResult(lw.reshape(logp.shape), o[0], o[1], o[2], o[4], o[5])


def psis(logp, logq=None):
    """Pareto-smoothed importance weights of the log ratios ``logp - logq`` (``logq=None``: ``logp`` holds the ratios), any shape,
    flattened: a ``PSISResult``.  ``khat`` below 0.5 is good, above 0.7 the weights are unreliable and the surrogate wants another
    refit; it is inf where nothing was smoothed (fewer than 25 values, or a tail without spread).  A GPU tensor takes the device
    route and returns a device tensor, arrays and CPU tensors take the host port."""
    if getattr(logp, 'is_cuda', False):
        if logq is not None and logp.numel() != (logq.numel() if hasattr(logq, 'numel') else np.size(logq)):
            raise ValueError('logp and logq should have the same size.')
        if logp.numel() < 1:
            raise ValueError('logp is empty.')
        return _psis_device(logp, logq)
    lw = host_f64(logp)
    shape = lw.shape
    if logq is not None:
        lq = host_f64(logq)
        if lq.size != lw.size:
            raise ValueError('logp and logq should have the same size.')
        with np.errstate(all='ignore'):
            lw = lw.reshape(-1) - lq.reshape(-1)
    if lw.size < 1:
        raise ValueError('logp is empty.')
    out = _psis_host(np.array(lw.reshape(-1)))
    return PSISResult(out[0].reshape(shape), *out[1:])


# ---- the weighted table ----------------------------------------------------------------------------------------------------------------
def _finish(raw, sw2, n_pos, w_bad, probs):
    """The table from the routes' raw figures: ``raw`` a dict of (d,) arrays mean, s2 = sum w (x - mean)^2, s4 = sum w^2 (x - mean)^2,
    lo, hi and (n_q, d) q."""
    mean, qv = np.array(raw['mean']), np.array(raw['q'])
    with np.errstate(all='ignore'):
        rest = 1. - sw2
        one = not (n_pos > 1 and rest > 0)       # one draw, or one weight that is 1: nothing to spread
        sd = np.sqrt(raw['s2'] / rest)
        mcse = np.sqrt(raw['s4'])
        ess = raw['s2'] / raw['s4']              # sd^2 (1 - sum w^2) / mcse_mean^2
        kish = np.full(mean.shape, 1. / sw2)
    bad = ~np.isfinite(mean) | ~np.isfinite(raw['s2']) | ~np.isfinite(raw['lo']) | ~np.isfinite(raw['hi'])
    const = (raw['lo'] == raw['hi']) & ~bad
    mean[const] = raw['lo'][const]
    qv[:, const] = raw['lo'][const]
    sd[const] = 0.
    for v in (mcse, ess, kish):
        v[const] = np.nan
    if one:
        for v in (sd, mcse, ess, kish):
            v[:] = np.nan
    cols = [('mean', mean), ('sd', sd)] + [('q%g' % (100 * p), qv[i]) for i, p in enumerate(probs)]
    cols += [('mcse_mean', mcse), ('ess', ess), ('ess_kish', kish)]
    for _, v in cols:
        v[bad] = np.nan
        if w_bad:
            v[:] = np.nan
    return Summary(cols)


def _host_table(x, w, probs):
    """x (n, d) float64, w (n,) raw weights"""
    with np.errstate(all='ignore'):
        w_bad = bool((~(w >= 0) | np.isinf(w)).any())
        w = w / w.sum()
        keep = w != 0
        n_pos = int(keep.sum())
        sw2 = float((w * w).sum())
        if w_bad or n_pos < 1:
            nan = np.full(x.shape[1], np.nan)
            return _finish(dict(mean=nan, s2=nan, s4=nan, lo=nan, hi=nan, q=np.full((len(probs), x.shape[1]), np.nan)), sw2, n_pos,
                           True, probs)
        ws = w[keep]
        raw = {k: np.empty(x.shape[1]) for k in ('mean', 's2', 's4', 'lo', 'hi')}
        raw['q'] = np.empty((len(probs), x.shape[1]))
        for c in range(x.shape[1]):   # a column at a time: working memory of a few columns, whatever d is
            xc = np.ascontiguousarray(x[:, c])[keep]
            mean = (ws * xc).sum()
            d2 = (xc - mean)**2
            raw['mean'][c], raw['s2'][c], raw['s4'][c] = mean, (ws * d2).sum(), (ws * ws * d2).sum()
            raw['lo'][c], raw['hi'][c] = np.fmin.reduce(xc), np.fmax.reduce(xc)
            order = np.argsort(xc, kind='stable')
            v, wp = xc[order], ws[order]
            mid = np.cumsum(wp) - wp / 2.
            if n_pos == 1 or not mid[-1] - mid[0] > 0:
                raw['q'][:, c] = v[-1] if n_pos == 1 else np.nan
                continue
            pos = (mid - mid[0]) / (mid[-1] - mid[0])
            k = np.clip(np.searchsorted(pos, probs, side='right') - 1, 0, n_pos - 1)
            k1 = np.minimum(k + 1, n_pos - 1)
            t = np.where(k1 > k, (probs - pos[k]) / np.where(k1 > k, pos[k1] - pos[k], 1.), 0.)
            raw['q'][:, c] = np.where(k1 > k, _lerp(v[k], v[k1], t), v[k])
    return _finish(raw, sw2, n_pos, False, probs)


def _device_table(x, w, probs):
    """x (n_chain, n_draw, d) device tensor, w (n,) raw float64 device weights"""
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    n_chain, n_draw = int(x.shape[0]), int(x.shape[1])
    n = n_chain * n_draw
    batches = _device_batches(x, n)
    with torch.cuda.device(x.device):
        ctx = get_context(x.device.index)
        lib, h, width = ctx._lib, ctx.handle, _lib.DIAG_BATCH
        work = ctx.empty((max(_lib.WSTAT_WORK, (n + _lib.WSTAT_TILE - 1) // _lib.WSTAT_TILE),))
        wsum_raw, wsum = ctx.empty((4,)), ctx.empty((4,))
        _lib.check(lib.bfhip_wstat_moments(h, n, None, _ptr(w), _ptr(wsum_raw), None, _ptr(work)))
        w = w / wsum_raw[0]
        _lib.check(lib.bfhip_wstat_moments(h, n, None, _ptr(w), _ptr(wsum), None, _ptr(work)))
        buf, cum = ctx.empty((n, width)), ctx.empty((n,))
        keys, order = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int32)
        probs_d = torch.as_tensor(probs, device=x.device)
        parts = []
        for xb, kb, nb in batches:
            out, qout = ctx.empty((5, width)), ctx.empty((len(probs), width))
            _lib.check(lib.bfhip_wstat_columns(h, n_chain, n_draw, int(xb.stride(0)), int(xb.stride(1)), _ptr(xb),
                                               int(xb.dtype == torch.float32), 0, kb, nb, _ptr(w), _ptr(buf)))
            _lib.check(lib.bfhip_wstat_moments(h, n, _ptr(buf), _ptr(w), None, _ptr(out), _ptr(work)))
            for b in range(nb):
                _lib.check(lib.bfhip_diag_sort(h, n, _ptr(buf), b, _ptr(keys), _ptr(order)))
                _lib.check(lib.bfhip_wstat_cumweights(h, n, _ptr(order), _ptr(w), _ptr(cum), _ptr(work)))
                _lib.check(lib.bfhip_wstat_quantiles(h, n, _ptr(keys), _ptr(order), _ptr(w), _ptr(cum), _ptr(wsum), len(probs),
                                                     _ptr(probs_d), b, _ptr(qout)))
            o, q = out.cpu().numpy()[:, :nb], qout.cpu().numpy()[:, :nb]
            parts.append(dict(mean=o[0], s2=o[1], s4=o[2], lo=o[3], hi=o[4], q=q))
        ws_raw, ws = wsum_raw.cpu().numpy(), wsum.cpu().numpy()
    raw = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]}
    return _finish(raw, float(ws[1]), int(ws[2]) if np.isfinite(ws[2]) else 0, bool(ws_raw[3] != 0 or ws[3] != 0 or not ws_raw[0] > 0),
                   probs)


def weighted_summary(x, log_weights=None, weights=None, probs=(0.05, 0.5, 0.95)):
    """The posterior table of weighted draws: x (n, d) or (n_chain, n_draw, d), exactly one of ``log_weights`` / ``weights`` of shape
    ``x.shape[:-1]`` (or flat of that size), not necessarily normalised -> a ``Summary`` with mean, sd, the quantiles at ``probs``
    ('q5', 'q50', 'q95'), mcse_mean, ess and ess_kish.  mcse_mean is the standard error of self-normalised importance sampling and
    ignores the autocorrelation between the draws of a chain.  A GPU ``x`` is reduced on its device (float32 is read as float64, a
    ``[:, since:]`` view goes in without a copy); arrays and CPU tensors take the host port."""
    if (log_weights is None) == (weights is None):
        raise ValueError('exactly one of log_weights and weights should be given.')
    probs = _check_probs(probs, 'probs')
    if x.ndim not in (2, 3):
        raise ValueError('x should be (n, d) or (n_chain, n_draw, d).')
    n = int(np.prod(x.shape[:-1]))
    if n < 1 or x.shape[-1] < 1:
        raise ValueError('x is empty.')
    given = weights if log_weights is None else log_weights
    if tuple(given.shape) != tuple(x.shape[:-1]) and tuple(given.shape) != (n,):
        raise ValueError('the weights should have the shape x.shape[:-1], or be flat of that size.')
    if getattr(x, 'is_cuda', False):
        import torch
        g = torch.as_tensor(given, device=x.device).detach().reshape(-1).to(torch.float64)
        w = (torch.exp(g - g.max()) if weights is None else g).contiguous()
        return _device_table(x if x.ndim == 3 else x[None], w, probs)
    g = host_f64(given).reshape(-1)
    with np.errstate(all='ignore'):
        w = np.exp(g - g.max()) if weights is None else g
    return _host_table(host_f64(x).reshape(n, x.shape[-1]), w, probs)
