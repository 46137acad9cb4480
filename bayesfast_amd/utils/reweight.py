"""What would the posterior be had the data vector been different?  Importance reweighting of one set of draws to K alternative
posteriors at once: a contaminated data vector, a data vector with one probe's points moved, a few hundred mock realisations for a
coverage test -- without a new ``sample()`` per data vector and without a sort per scenario.

The ratio of a ``Chi2PipelineDensity``.  y is the data, f(x) the surrogate's m outputs, P the precision (``prec``, or
``diag(prec_diag)``), fixed.  For another data vector y_k the log-likelihood ratio is linear in the outputs:

  l_k(x) = log L(x | y_k) - log L(x | y) = a_k . f(x) - a_k . (y + y_k) / 2,      a_k = P (y_k - y)

so the K ratios are a K-output PolyModel on the same inputs, bound and alpha (``device.linear_dense``), whose ``fun_columns`` fills
one (n, 16) buffer per batch, 128 bytes per draw whatever m and K are.  ``reweight_moments`` takes any log ratios, a changed prior
included.

Per scenario k, with base log weights b_s normalised to logsumexp 0 (``log_weights``; without them b_s = -log n) and r_s = b_s + l_ks:

  v_s, khat, sigma, n_tail, ess   ``psis(r)`` exactly as utils/psis.py defines it; w_s = exp(v_s)
  log_evidence_ratio   max r + log sum exp(smoothed shifted r): log p(y_k) / p(y) under the surrogate, ``psis``'s log_mean_weight + log n
  mean        sum w x
  sd          sqrt(sum w (x - mean)^2 / (1 - sum w^2))
  mcse_mean   sqrt(sum w^2 (x - mean)^2): the standard error of self-normalised importance sampling with INDEPENDENT draws
  mean_base, sd_base   the same table with l = 0 and nothing smoothed
  shift       (mean - mean_base) / sd_base;  shift_mcse = mcse_mean / sd_base

The sums are taken about the centre c = mean_base and recentred in closed form: with D = sum w (x - c), mean = c + D,
sum w (x - mean)^2 = sum w (x - c)^2 - D^2 and sum w^2 (x - mean)^2 = sum w^2 (x - c)^2 - 2 D sum w^2 (x - c) + D^2 sum w^2.

Rows with b_s = -inf are not part of the sample, whatever they hold: they count in n for the tail size and are left out of every
sum over s.  Where fewer than n_tail + 1 rows have any weight, ``psis`` hands smoothed weight to some of them: it stays in ``psis``'s
own figures, ess and log_evidence_ratio, and the table's weights are exp(v_s) over the rows of the sample, normalised to sum 1 over
THEM -- a mean whose weights do not sum to 1 would depend on the origin.  A non-finite draw in a row with b_s > -inf makes that parameter NaN in every
scenario; a non-finite l in such a row makes that scenario NaN (flag 1), as does a sample without a row of non-zero weight (flag
4).  n < 25, or a tail without spread, gives khat = inf and unsmoothed weights (flag 2), as in ``psis``: y_k = y without weights is
that case and returns the base table and a ratio of 0.

Two routes compute the same numbers: NumPy arrays and CPU tensors take the host port below; GPU tensors take the device route in
batches of 16 scenarios -- ``bfhip_ploo_moments`` and ``bfhip_ploo_tail`` on -l (their ratio lb - ell is then r), and
``bfhip_rw_finish`` (csrc/bfhip_rw.h): the fit of ``bfhip_psis`` on each tail, then one pass over the draws in place on the FP64
matrix cores that turns the 16 columns of smoothed weights into 16 tables of moments.

Limits: a Gaussian likelihood with a fixed covariance; the likelihood only in ``data_reweight``'s ratio (prior and decay term cancel);
moments, not quantiles (``data_log_ratio`` with ``psis`` and ``weighted_summary`` gives one scenario's quantiles); importance sampling
breaks beyond roughly one posterior sd of shift in several directions, and ``khat`` says so; the surrogate must still hold where the new
posterior sits; mcse_mean ignores the autocorrelation of a chain; one process; ``data_reweight`` reads device tensors only;
n <= 2^31 - 1."""
import numpy as np

from ._pipeline_data import (PsisStages, base_log_weights, check_density, check_gpu_draws, check_one_process, host_f64, input_map,
                             logsumexp_host, shaped_draws)
from .psis import _psis_host, tail_size

__all__ = ['reweight_moments', 'data_reweight', 'data_log_ratio', 'Reweighted']

_PER_K = ('log_evidence_ratio', 'khat', 'sigma', 'ess')
_PER_KD = ('mean', 'sd', 'mcse_mean', 'shift', 'shift_mcse')


class Reweighted:
    """What ``reweight_moments`` and ``data_reweight`` return.  Per scenario, (K,) arrays: ``log_evidence_ratio``, ``khat``, ``sigma``,
    ``n_tail`` (int), ``ess`` and ``flags`` (int; 1 a non-finite ratio, 2 nothing smoothed, 4 no draw of non-zero weight).  (K, d)
    arrays: ``mean``, ``sd``, ``mcse_mean``, ``shift`` and ``shift_mcse``.  (d,) arrays: ``mean_base`` and ``sd_base``.  ``n`` draws;
    ``n_khat_bad``, the number of scenarios with khat > 0.7."""

    def __init__(self, n, cols, mean_base, sd_base):
        self.n = int(n)
        for name in _PER_K + _PER_KD:
            setattr(self, name, np.asarray(cols[name], dtype=np.float64))
        self.n_tail = np.asarray(cols['n_tail'], dtype=np.int64)
        self.flags = np.asarray(cols['flags'], dtype=np.int64)
        self.mean_base, self.sd_base = np.asarray(mean_base, dtype=np.float64), np.asarray(sd_base, dtype=np.float64)
        with np.errstate(all='ignore'):
            self.n_khat_bad = int((self.khat > 0.7).sum())

    def __str__(self):
        k = len(self.khat)
        rows = ['Reweighted: %d scenarios, %d parameters at %d draws' % (k, len(self.mean_base), self.n),
                '  khat > 0.7 at %d scenarios' % self.n_khat_bad]
        fin = np.isfinite(self.khat)
        if k and fin.any():
            i = int(np.argmax(np.where(fin, self.khat, -np.inf)))
            with np.errstate(all='ignore'):
                sh = np.abs(self.shift[i])
                j = int(np.nanargmax(sh)) if np.isfinite(sh).any() else 0
            rows.append('  worst: scenario %d, khat %.3g (ess %.4g, log evidence ratio %.6g), largest shift %.3g sd_base (mcse %.2g) in '
                        'parameter %d' % (i, self.khat[i], self.ess[i], self.log_evidence_ratio[i], self.shift[i, j], self.shift_mcse[i, j], j))
        return '\n'.join(rows)

    __repr__ = __str__


def _finish(n, head, s1, s2, sums, mean_base, s2_base, sw2_base):
    """The result from the routes' raw figures: ``head`` a dict of (K,) arrays log_evidence_ratio, khat, sigma, n_tail, ess, flags; s1 =
    sum e and s2 = sum e^2 over the rows of the sample, (K,); ``sums`` the (K, d) arrays e1 = sum e (x - c), e2 = sum e (x - c)^2, q1 = sum e^2 (x - c) and q2 =
    sum e^2 (x - c)^2 about c = mean_base; s2_base = sum w (x - c)^2 and sw2_base = sum w^2 of the base weights."""
    with np.errstate(all='ignore'):
        bad_base = ~(np.isfinite(mean_base) & np.isfinite(s2_base))   # a non-finite draw of non-zero weight: the parameter is NaN
        mean_base = np.where(bad_base, np.nan, mean_base)
        sd_base = np.where(bad_base, np.nan, np.sqrt(s2_base / (1. - sw2_base)))
        s1c = s1[:, None]
        delta = sums['e1'] / s1c
        mean = mean_base[None, :] + delta
        var = sums['e2'] / s1c - delta * delta
        sw2 = (s2 / (s1 * s1))[:, None]
        s4 = (sums['q2'] - 2. * delta * sums['q1'] + delta * delta * s2[:, None]) / (s1c * s1c)
        sd = np.sqrt(var / (1. - sw2))
        mcse = np.sqrt(s4)
        bad = ~(np.isfinite(sums['e1']) & np.isfinite(sums['e2'])) | ~np.isfinite(s1c)
        cols = dict(head, mean=mean, sd=sd, mcse_mean=mcse, shift=delta / sd_base[None, :], shift_mcse=mcse / sd_base[None, :])
        for name in _PER_KD:
            cols[name] = np.where(bad, np.nan, cols[name])
    return Reweighted(n, cols, mean_base, sd_base)


# ---- the host port ---------------------------------------------------------------------------------------------------------------------
def _host(x, l, log_weights):
    """x (n, d), l (n, K) float64, log_weights (n,) or None"""
    n, d = x.shape
    big_k = l.shape[1]
    nan = np.nan
    with np.errstate(all='ignore'):
        lb = None
        if log_weights is not None:
            lb = log_weights - logsumexp_host(log_weights)
        keep = np.ones(n, dtype=bool) if lb is None else lb > -np.inf
        xk = x[keep]
        wb = np.exp(lb[keep]) if lb is not None else np.full(xk.shape[0], 1. / n)
        mean_base = (wb[:, None] * xk).sum(axis=0) if xk.shape[0] else np.full(d, nan)
        dx = xk - mean_base[None, :]
        dx2 = dx * dx
        s2_base = (wb[:, None] * dx2).sum(axis=0) if xk.shape[0] else np.full(d, nan)
        sw2_base = (wb * wb).sum()
        head = {name: np.full(big_k, nan) for name in _PER_K}
        head['n_tail'] = np.full(big_k, tail_size(n))
        head['flags'] = np.zeros(big_k, dtype=np.int64)
        s1, s2 = np.full(big_k, nan), np.full(big_k, nan)
        sums = {name: np.full((big_k, d), nan) for name in ('e1', 'e2', 'q1', 'q2')}
        for k in range(big_k):
            lk = l[keep, k]
            if not keep.any():
                head['flags'][k] = 4
                continue
            if not np.isfinite(lk).all():
                head['flags'][k] = 1
                continue
            r = np.full(n, -np.inf)
            r[keep] = lk if lb is None else lb[keep] + lk
            v, khat, sigma, _, lmw, ess = _psis_host(r)
            e = np.exp(v)
            ek = e[keep]
            head['log_evidence_ratio'][k] = lmw + (np.log(n) if lb is not None else 0.)
            head['khat'][k], head['sigma'][k], head['ess'][k] = khat, sigma, ess
            head['flags'][k] = 2 if np.isinf(khat) else 0
            s1[k], s2[k] = ek.sum(), (ek * ek).sum()
            sums['e1'][k], sums['e2'][k] = (ek[:, None] * dx).sum(axis=0), (ek[:, None] * dx2).sum(axis=0)
            sums['q1'][k], sums['q2'][k] = ((ek * ek)[:, None] * dx).sum(axis=0), ((ek * ek)[:, None] * dx2).sum(axis=0)
    return _finish(n, head, s1, s2, sums, mean_base, s2_base, sw2_base)


# ---- the device route ------------------------------------------------------------------------------------------------------------------
class _Stages(PsisStages):
    """Base table and scenario batches on one set of draws x (n_chain, n_draw, d), a device tensor read in place: ``run(buf, nb)``
    queues the three stages on an (n, 16) series buffer that holds -l, ``result()`` makes the one copy to the host.  ``w`` (n,) are
    the base weights, ``wsum`` their ``bfhip_wstat_moments`` figures."""

    def __init__(self, ctx, x, log_weights):
        import torch
        from .. import _lib
        from ..device import _ptr
        from .diagnostics import _device_batches
        self.x = x
        self.n_chain, self.n_draw, self.d = (int(v) for v in x.shape)
        n = self.n_chain * self.n_draw
        lib, h, width = ctx._lib, ctx.handle, _lib.DIAG_BATCH
        lb = base_log_weights(log_weights, x, n)
        # the base table: bfhip_wstat_moments on batches of 16 parameters under the base weights
        w = torch.exp(lb) if lb is not None else torch.full((n,), 1. / n, dtype=torch.float64, device=x.device)
        work = ctx.empty((_lib.WSTAT_WORK,))
        self.w = w
        self.wsum = ctx.empty((4,))
        _lib.check(lib.bfhip_wstat_moments(h, n, None, _ptr(w), _ptr(self.wsum), None, _ptr(work)))
        buf = ctx.empty((n, width))
        parts = []
        for xb, kb, nb in _device_batches(x, n):
            out = ctx.empty((5, width))
            _lib.check(lib.bfhip_wstat_columns(h, self.n_chain, self.n_draw, int(xb.stride(0)), int(xb.stride(1)), _ptr(xb),
                                               int(xb.dtype == torch.float32), 0, kb, nb, _ptr(w), _ptr(buf)))
            _lib.check(lib.bfhip_wstat_moments(h, n, _ptr(buf), _ptr(w), None, _ptr(out), _ptr(work)))
            parts.append(out[:, :nb])
        self.base = torch.cat(parts, dim=1)            # rows mean, sum w (x - mean)^2, ...
        self.centre = self.base[0].contiguous()
        super().__init__(ctx, n, lb)
        self.rw_work = ctx.empty((int(lib.bfhip_rw_work_bytes(n, self.d)),), dtype=torch.uint8)
        self.outs = []

    def run(self, buf, nb):
        import torch
        from ..device import _ptr
        _lib, x = self._lib, self.x
        out, head, tail = self.front(buf, _lib.DIAG_BATCH, nb, _lib.PLOO_ELL)
        rw = self.ctx.empty((_lib.RW_SUMS + 2 * (1 + 2 * self.d), _lib.DIAG_BATCH))
        ldr = int(x.stride(1)) if self.n_draw > 1 else self.d
        _lib.check(self.ctx._lib.bfhip_rw_finish(*head, _ptr(self.keys), _ptr(self.idx), _ptr(out), *tail, self.n_chain, self.n_draw,
                                                 int(x.stride(0)), ldr, _ptr(x), int(x.dtype == torch.float32), 0, self.d, _ptr(self.centre),
                                                 _ptr(rw), _ptr(self.rw_work), self.rw_work.numel()))
        self.outs.append(rw)
        return out, head, tail   # what a further stage of the batch shares with the three (power_scale.py: bfhip_rw_weights)

    def result(self):
        d, r0 = self.d, self._lib.RW_SUMS
        base, ws = self.base.cpu().numpy(), self.wsum.cpu().numpy()
        o = self.collect(self.outs, r0 + 2 * (1 + 2 * d))   # the one copy of the scenarios to the host
        raw = {name: o[i] for i, name in enumerate(self._lib.RW_ROWS)}
        head = {name: raw[name] for name in ('khat', 'sigma', 'ess')}
        head['log_evidence_ratio'] = raw['log_evidence_ratio'] + (0. if self.lb is not None else -np.log(self.n))
        head['n_tail'], head['flags'] = raw['n_tail'].astype(np.int64), raw['flags'].astype(np.int64)
        nf = 1 + 2 * d
        sums = dict(e1=o[r0 + 1:r0 + 1 + d].T, e2=o[r0 + 1 + d:r0 + nf].T, q1=o[r0 + nf + 1:r0 + nf + 1 + d].T, q2=o[r0 + nf + 1 + d:r0 + 2 * nf].T)
        return _finish(self.n, head, o[r0], o[r0 + nf], sums, base[0], base[1], float(ws[1]))


def _device(x, l, log_weights):
    """x (n_chain, n_draw, d) and l (n_chain, n_draw, K) device tensors"""
    import torch
    from .. import _lib
    from ..device import get_context
    n_chain, n_draw, big_k = (int(v) for v in l.shape)
    n = n_chain * n_draw
    x = shaped_draws(x, x.shape[2])   # (refuses n > 2^31 - 1 before anything is allocated)
    if int(x.shape[2]) > _lib.MAX_DIM:
        raise NotImplementedError('more than %d parameters.' % _lib.MAX_DIM)
    with torch.cuda.device(x.device):
        ctx = get_context(x.device.index)
        st = _Stages(ctx, x, log_weights)
        buf = ctx.empty((n, _lib.DIAG_BATCH))
        lf = l.detach().reshape(n, big_k)
        for k0 in range(0, big_k, _lib.DIAG_BATCH):
            nb = min(_lib.DIAG_BATCH, big_k - k0)
            buf[:, :nb] = -lf[:, k0:k0 + nb]   # the stages' ratio lb - ell is then lb + l
            st.run(buf, nb)
        return st.result()


def reweight_moments(x, log_ratio, log_weights=None):
    """The moments of the draws ``x``, (n, d) or (n_chain, n_draw, d), under each of the K columns of log ratios ``log_ratio``, of shape
    ``x.shape[:-1] + (K,)`` -> a ``Reweighted``.  The ratios may be anything: a changed likelihood, a changed prior.  ``log_weights``:
    one base log weight per draw (``x.shape[:-1]``, or flat), not necessarily normalised, -inf for a draw that is not part of the
    sample.  GPU tensors take the device route (float32 draws are read as float64, a strided view of the draws goes in without a
    copy); NumPy arrays and CPU tensors take the host port."""
    if x.ndim not in (2, 3):
        raise ValueError('x should be (n, d) or (n_chain, n_draw, d).')
    n, d = int(np.prod(x.shape[:-1])), int(x.shape[-1])
    if n < 1 or d < 1:
        raise ValueError('x is empty.')
    if log_ratio.ndim != x.ndim or tuple(log_ratio.shape[:-1]) != tuple(x.shape[:-1]) or int(log_ratio.shape[-1]) < 1:
        raise ValueError('log_ratio should have the shape x.shape[:-1] + (K,).')
    if log_weights is not None and int(np.prod(log_weights.shape)) != n:
        raise ValueError('log_weights should hold one value per draw.')
    if getattr(x, 'is_cuda', False):
        import torch
        l = torch.as_tensor(log_ratio, device=x.device)
        return _device(x if x.ndim == 3 else x[None], l if l.ndim == 3 else l[None], log_weights)
    return _host(host_f64(x).reshape(n, d), host_f64(log_ratio).reshape(n, -1),
                 None if log_weights is None else host_f64(log_weights).reshape(-1))


# ---- the pipeline's data ---------------------------------------------------------------------------------------------------------------
def ratio_coefficients(y, y_new, prec=None, prec_diag=None):
    """(A (K, m), b (K,)) of l_k = A_k . f + b_k: A_k = P (y_k - y), b_k = -A_k . (y + y_k) / 2."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    yn = np.asarray(y_new, dtype=np.float64)
    yn = yn[None] if yn.ndim == 1 else yn
    if yn.ndim != 2 or yn.shape[1] != y.size or yn.shape[0] < 1:
        raise ValueError('y_new should be (K, %d) or (%d,).' % (y.size, y.size))
    if (prec is None) == (prec_diag is None):
        raise ValueError('give me exactly one of prec and prec_diag.')
    dy = yn - y[None, :]
    a = dy @ np.asarray(prec, dtype=np.float64).T if prec is not None else dy * np.asarray(prec_diag, dtype=np.float64).reshape(-1)[None, :]
    return a, -0.5 * np.einsum('km,km->k', a, yn + y[None, :])


def _prepare(who, density, x, y_new):
    """The checks of ``data_loo``, in its words, the density before the draws -> (x (n_chain, n_draw, d), dense arrays of the
    surrogate, A, b)."""
    from ..device import polymodel_dense_from_poly
    check_one_process(who)
    check_density(density)
    check_gpu_draws(who, x)
    su = density.surrogate
    x = shaped_draws(x, su.input_size)
    a, b = ratio_coefficients(density._y, y_new, density._prec, density._pdiag)
    return x, polymodel_dense_from_poly(su.poly_spec()), a, b


def _chunks(dense, big_k, chunk_bytes, width):
    """Scenarios per derived model: a multiple of 16 whose dense coefficient arrays stay under chunk_bytes (16 at the least)."""
    m = int(dense['m'])
    per = 8 * sum(int(np.size(dense[k])) // m for k in ('c0', 'lin', 'quad', 'cub2', 'cub3') if dense[k] is not None)
    size = max(width, int(chunk_bytes) // max(per, 1) // width * width)
    return [(k0, min(size, big_k - k0)) for k0 in range(0, big_k, size)]


def _ratio_columns(density, x, dense, a, b, chunk_bytes, width, sink):
    """Every scenario's column of A f + b in batches of at most ``width``: ``sink(rm, k0_global, k0_in_model, nb, lo, diff)`` evaluates."""
    from ..device import DevicePolyModel, linear_dense
    lo = diff = None
    for c0, ck in _chunks(dense, a.shape[0], chunk_bytes, width):
        # the ratio model takes the context's one polymodel slot; the surrogate's own device model uploads itself again at its next
        # use (DevicePolyModel.upload_if_needed)
        rm = DevicePolyModel.from_dense(linear_dense(dense, a[c0:c0 + ck], b[c0:c0 + ck]))
        if c0 == 0:
            lo, diff = input_map(rm.ctx, density.surrogate)
        for k0 in range(0, ck, width):
            sink(rm, c0 + k0, k0, min(width, ck - k0), lo, diff)


def data_log_ratio(density, x, y_new, chunk_bytes=64 << 20):
    """l_k(x) = log L(x | y_k) - log L(x | y) of a ``Chi2PipelineDensity`` at the ORIGINAL-space draws ``x``, a GPU tensor (n_chain,
    n_draw, d) or (n, d), for the data vectors ``y_new`` (K, m) or (m,) -> the (n_chain, n_draw, K) device tensor: ``psis`` and
    ``weighted_summary`` on one of its columns give that scenario's quantiles."""
    import torch
    from .. import _lib
    x, dense, a, b = _prepare('data_log_ratio', density, x, y_new)
    with torch.cuda.device(x.device):
        out = []

        def sink(rm, kg, k0, nb, lo, diff):
            if not out:
                out.append(rm.ctx.empty((int(x.shape[0]), int(x.shape[1]), a.shape[0])))
            rm.fun_columns(x, k0, nb, lo, diff, out=out[0][:, :, kg:])

        _ratio_columns(density, x, dense, a, b, chunk_bytes, _lib.DIAG_BATCH, sink)
        return out[0]


def data_reweight(density, x, y_new, log_weights=None, chunk_bytes=64 << 20):
    """The posterior of a ``Chi2PipelineDensity`` reweighted to the data vectors ``y_new`` at the draws ``x`` -> a ``Reweighted``.

    x : GPU tensor (n_chain, n_draw, d), or (n, d); the ORIGINAL space (the surrogate's ``_input_scales`` are the input map, as in
        ``data_loo``); float64 or float32, read in place.
    y_new : (K, m) or (m,) alternative data vectors; the covariance stays.
    log_weights : one log importance weight per draw, e.g. ``psis(...).log_weights``.
    chunk_bytes : the K ratios are a K-output PolyModel; they go to the device in chunks of a multiple of 16 scenarios whose dense
        coefficient arrays stay under this size."""
    import torch
    from .. import _lib
    x, dense, a, b = _prepare('data_reweight', density, x, y_new)
    n_chain, n_draw = int(x.shape[0]), int(x.shape[1])
    if log_weights is not None and int(np.prod(log_weights.shape)) != n_chain * n_draw:
        raise ValueError('log_weights should hold one value per draw.')
    if int(x.shape[2]) > _lib.MAX_DIM:
        raise NotImplementedError('more than %d parameters.' % _lib.MAX_DIM)
    with torch.cuda.device(x.device):
        state = {}

        def sink(rm, kg, k0, nb, lo, diff):
            if not state:
                state['st'] = _Stages(rm.ctx, x, log_weights)
                state['buf'] = rm.ctx.empty((n_chain, n_draw, _lib.DIAG_BATCH))
            rm.fun_columns(x, k0, nb, lo, diff, out=state['buf'])
            state['st'].run(state['buf'], nb)

        _ratio_columns(density, x, dense, -a, -b, chunk_bytes, _lib.DIAG_BATCH, sink)   # -l: the stages' ratio lb - ell is then lb + l
        return state['st'].result()
