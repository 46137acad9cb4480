"""Pointwise leave-one-out cross-validation by Pareto-smoothed importance sampling (PSIS-LOO) and WAIC (Vehtari, Gelman, Gabry 2017,
"Practical Bayesian model evaluation using leave-one-out cross-validation and WAIC") of the pipeline's data.  ``predictive`` says
whether the model fits the data as a whole; this says which data points the fit hangs on (``khat``, ``p_loo``), how well the model
predicts a point it was not shown (``elpd_loo``, ``pit``), and gives two models a predictive comparison (``DataLOO.compare``).

The pointwise terms of a ``Chi2PipelineDensity``.  y is the data, f(theta) the surrogate's m outputs, P the precision (``prec``, or
``diag(prec_diag)``).  With W = diag(P_ii)^(-1/2) P, z(theta) = W (y - f(theta)) and c_i = log(P_ii / 2 pi) / 2, the conditional of y_i
given all the other data points at theta is Gaussian with mean y_i - z_i / sqrt(P_ii) and variance 1 / P_ii (Buerkner, Gabry, Vehtari
2021, "Efficient leave-one-out cross-validation for Bayesian non-factorized normal and Student-t models"), so

  ell_i(theta) = log p(y_i | y_-i, theta) = c_i - z_i^2 / 2

and the importance ratio that removes point i from the posterior is 1 / p(y_i | y_-i, theta).  A diagonal P is the ordinary factorised
case.  The likelihood is the pipeline's: no prior, no decay term, as in ``predictive``.

Per column ell_s, s < n, with base log weights b_s normalised to logsumexp 0 (``log_weights``; without them b_s = -log n), w_s = exp(b_s):

  lpd        logsumexp_s(b_s + ell_s)
  p_waic     sum w (ell - sum w ell)^2 / (1 - sum w^2): the ddof = 1 variance under equal weights, as ``weighted_summary``'s sd
  elpd_waic  lpd - p_waic
  r_s        b_s - ell_s, or -ell_s without weights
  v_s, khat, sigma, n_tail     ``psis(r)`` exactly as utils/psis.py defines it; v_s are its ``log_weights``
  elpd_loo   logsumexp_s(v_s + ell_s)
  p_loo      lpd - elpd_loo
  ess_loo    1 / sum exp(2 v_s)
  pit        sum_s exp(v_s) Phi(z_s), the leave-one-out probability integral transform of y_i: uniform on [0, 1] over i for a calibrated
             model; only where z is known

Rows with b_s = -inf are not part of the sample, whatever they hold: they have r_s = -inf, count in n for the tail size as in ``psis``,
and are left out of every sum over s (where fewer than n_tail + 1 rows have any weight, ``psis`` hands smoothed weight to some of them:
it stays in the normalisation and in ess_loo, and out of elpd_loo and pit).  A non-finite ell in a row of non-zero weight makes every
figure of that column NaN, as does a column without a row of non-zero weight.  n < 25, or a tail without spread, gives khat = inf and
unsmoothed weights, as in ``psis``.

Totals over the k points: the sums ``elpd_loo_total``, ``p_loo_total``, ``elpd_waic_total``, ``p_waic_total``, ``se_* = sqrt(k var_i(.,
ddof = 1))`` and ``n_khat_bad``, the number of points with khat > 0.7.

Two routes compute the same numbers: NumPy arrays and CPU tensors take the host port below; a GPU tensor takes the device route
(csrc/bfhip_ploo.h) in batches of 16 columns -- two passes for the moments, a top-(n_tail + 1) radix select in place of a sort per
column, the fit of ``bfhip_psis`` on each column's tail, one pass for the sums.  ``data_loo`` never materialises the (n, m) outputs:
z(theta) is itself a PolyModel (``device.residual_dense``) whose ``fun_columns`` fills one (n, 16) buffer per batch, 128 bytes per draw
whatever m is.

Limits: a Gaussian likelihood with a fixed covariance; no prior or decay term in ell; strongly correlated data (conditioning on many
correlated neighbours) makes every point influential and pushes khat above 0.7 for most of them, which is the method's honest
answer; one process; ``data_loo`` reads device tensors only; n <= 2^31 - 1."""
import numpy as np

from ._pipeline_data import (PsisStages, base_log_weights, check_density, check_gpu_draws, check_one_process, dense_precision, host_f64,
                             input_map, logsumexp_host, shaped_draws, sum_and_se)
from .psis import _psis_host, tail_size

__all__ = ['data_loo', 'pointwise_loo', 'DataLOO']

_POINT = ('lpd', 'p_waic', 'elpd_waic', 'elpd_loo', 'p_loo', 'khat', 'sigma', 'ess_loo', 'pit')
_TOTAL = ('elpd_loo', 'p_loo', 'elpd_waic', 'p_waic')


class DataLOO:
    """What ``pointwise_loo`` and ``data_loo`` return.  Per point, (k,) arrays: ``outputs`` (the points' indices), ``lpd``, ``p_waic``,
    ``elpd_waic``, ``elpd_loo``, ``p_loo``, ``khat``, ``sigma``, ``n_tail`` (int), ``ess_loo`` and ``pit`` (NaN where z is not known).
    Totals: ``elpd_loo_total``, ``p_loo_total``, ``elpd_waic_total``, ``p_waic_total``, their ``se_*`` and ``n_khat_bad``; ``n`` draws."""

    def __init__(self, outputs, n, cols):
        self.outputs, self.n = np.asarray(outputs, dtype=np.int64), int(n)
        for name in _POINT:
            setattr(self, name, np.asarray(cols[name], dtype=np.float64))
        self.n_tail = np.asarray(cols['n_tail'], dtype=np.int64)
        for name in _TOTAL:
            total, se = sum_and_se(getattr(self, name))
            setattr(self, name + '_total', total)
            setattr(self, 'se_' + name, se)
        with np.errstate(all='ignore'):
            self.n_khat_bad = int((self.khat > 0.7).sum())

    def compare(self, other):
        """(difference of elpd_loo_total, self minus other; its standard error sqrt(k var_i(difference_i, ddof = 1))).  Both should
        hold the same points."""
        if not isinstance(other, DataLOO) or not np.array_equal(self.outputs, other.outputs):
            raise ValueError('the two results should hold the same points.')
        return sum_and_se(self.elpd_loo - other.elpd_loo)

    def __str__(self):
        k = len(self.outputs)
        rows = ['DataLOO: %d points at %d draws' % (k, self.n),
                '  elpd_loo %.6g (se %.3g), p_loo %.4g (se %.3g)' % (self.elpd_loo_total, self.se_elpd_loo, self.p_loo_total, self.se_p_loo),
                '  elpd_waic %.6g (se %.3g), p_waic %.4g (se %.3g)' % (self.elpd_waic_total, self.se_elpd_waic, self.p_waic_total,
                                                                      self.se_p_waic)]
        if k and np.isfinite(self.khat).any():
            i = int(np.nanargmax(np.where(np.isfinite(self.khat), self.khat, -np.inf)))
            rows.append('  khat > 0.7 at %d points; largest %.3g at point %d (ess_loo %.4g)'
                        % (self.n_khat_bad, self.khat[i], int(self.outputs[i]), self.ess_loo[i]))
        else:
            rows.append('  khat > 0.7 at %d points' % self.n_khat_bad)
        if k and np.isfinite(self.pit).any():
            rows.append('  pit: smallest %.3g, largest %.3g' % (np.nanmin(self.pit), np.nanmax(self.pit)))
        return '\n'.join(rows)

    __repr__ = __str__


# ---- the host port ---------------------------------------------------------------------------------------------------------------------
def _host_column(ell, lb, z):
    """Every figure of one column: ell (n,), lb (n,) normalised base log weights or None, z (n,) or None."""
    n = ell.size
    nan = np.nan
    out = dict(lpd=nan, p_waic=nan, elpd_waic=nan, elpd_loo=nan, p_loo=nan, khat=nan, sigma=nan, ess_loo=nan, pit=nan, n_tail=tail_size(n))
    keep = np.ones(n, dtype=bool) if lb is None else lb > -np.inf
    if not keep.any() or not np.isfinite(ell[keep]).all():
        return out
    with np.errstate(all='ignore'):
        b = np.full(n, -np.log(n)) if lb is None else lb
        ek, bk = ell[keep], b[keep]
        w = np.exp(bk) if lb is not None else np.full(ek.size, 1. / n)
        lpd = logsumexp_host(bk + ek)
        mean = (w * ek).sum()
        p_waic = (w * (ek - mean)**2).sum() / (1. - (w * w).sum())
        r = np.full(n, -np.inf)
        r[keep] = (bk if lb is not None else 0.) - ek
        v, khat, sigma, _, _, ess = _psis_host(r)
        elpd_loo = logsumexp_host(v[keep] + ek)
        out.update(lpd=lpd, p_waic=p_waic, elpd_waic=lpd - p_waic, elpd_loo=elpd_loo, p_loo=lpd - elpd_loo, khat=khat, sigma=sigma, ess_loo=ess)
        if z is not None:
            from scipy.special import ndtr
            out['pit'] = (np.exp(v[keep]) * ndtr(z[keep])).sum()
    return out


def _normalise_host(log_weights, n):
    if log_weights is None:
        return None
    g = np.asarray(log_weights, dtype=np.float64).reshape(-1)
    if g.size != n:
        raise ValueError('log_weights should hold one value per draw.')
    with np.errstate(all='ignore'):
        return g - logsumexp_host(g)


def _host(ell, log_weights, z):
    n, k = ell.shape
    lb = _normalise_host(log_weights, n)
    cols = [_host_column(np.ascontiguousarray(ell[:, c]), lb, None if z is None else np.ascontiguousarray(z[:, c])) for c in range(k)]
    return DataLOO(np.arange(k), n, {name: np.array([c[name] for c in cols]) for name in cols[0]})


# ---- the device route ------------------------------------------------------------------------------------------------------------------
class _Stages(PsisStages):
    """The three stages on one (n, 16) series buffer after another: ``run(buf, ld, nb, mode, c)`` queues a batch, ``result(outputs)``
    makes the one copy to the host."""

    def __init__(self, ctx, n, lb):
        super().__init__(ctx, n, lb)
        self.outs = []

    def run(self, buf, ld, nb, mode, c=None):
        from ..device import _ptr
        out, head, tail = self.front(buf, ld, nb, mode, c)
        self._lib.check(self.ctx._lib.bfhip_ploo_finish(*head, _ptr(self.keys), _ptr(self.idx), _ptr(out), *tail))
        self.outs.append(out)

    def result(self, outputs):
        o = self.collect(self.outs, self._lib.PLOO_NOUT)
        raw = {name: o[i] for i, name in enumerate(self._lib.PLOO_ROWS)}
        with np.errstate(all='ignore'):
            p_waic = raw['waic'] / (1. - raw['sw2'])
            cols = dict(lpd=raw['lpd'], p_waic=p_waic, elpd_waic=raw['lpd'] - p_waic, elpd_loo=raw['elpd_loo'],
                        p_loo=raw['lpd'] - raw['elpd_loo'], khat=raw['khat'], sigma=raw['sigma'], ess_loo=raw['ess_loo'], pit=raw['pit'],
                        n_tail=raw['n_tail'].astype(np.int64))
        return DataLOO(outputs, self.n, cols)


def _device(ell, log_weights):
    """ell (n_chain, n_draw, k) device tensor"""
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    from .diagnostics import _device_batches
    n_chain, n_draw, k = (int(v) for v in ell.shape)
    n = n_chain * n_draw
    if n > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 draws.')
    batches = _device_batches(ell, n)
    with torch.cuda.device(ell.device):
        ctx = get_context(ell.device.index)
        st = _Stages(ctx, n, base_log_weights(log_weights, ell, n))
        buf = ctx.empty((n, _lib.DIAG_BATCH))
        for xb, kb, nb in batches:
            _lib.check(ctx._lib.bfhip_wstat_columns(ctx.handle, n_chain, n_draw, int(xb.stride(0)), int(xb.stride(1)), _ptr(xb),
                                                    int(xb.dtype == torch.float32), 0, kb, nb, None, _ptr(buf)))
            st.run(buf, _lib.DIAG_BATCH, nb, _lib.PLOO_ELL)
        return st.result(np.arange(k))


def pointwise_loo(ell, log_weights=None, z=None):
    """PSIS-LOO and WAIC of every column of pointwise log likelihoods ``ell``, (n, k) or (n_chain, n_draw, k) -> a ``DataLOO``.
    ``log_weights``: one base log weight per draw (``ell.shape[:-1]``, or flat), not necessarily normalised, -inf for a draw that is
    not part of the sample.  ``z`` (host port only; ``ell``'s shape): the standardised conditional residuals, for ``pit``.  NumPy
    arrays and CPU tensors take the host port; a GPU tensor is reduced on its device in batches of 16 columns (float32 is read as
    float64, a strided view goes in without a copy) and gets its ``pit`` from ``data_loo``."""
    if ell.ndim not in (2, 3):
        raise ValueError('ell should be (n, k) or (n_chain, n_draw, k).')
    n, k = int(np.prod(ell.shape[:-1])), int(ell.shape[-1])
    if n < 1 or k < 1:
        raise ValueError('ell is empty.')
    if z is not None and tuple(z.shape) != tuple(ell.shape):
        raise ValueError('z should have the shape of ell.')
    if log_weights is not None and int(np.prod(log_weights.shape)) != n:
        raise ValueError('log_weights should hold one value per draw.')
    if getattr(ell, 'is_cuda', False):
        if z is not None:
            raise NotImplementedError('on the device pit comes from data_loo, which knows z.')
        return _device(ell if ell.ndim == 3 else ell[None], log_weights)
    return _host(host_f64(ell).reshape(n, k), None if log_weights is None else host_f64(log_weights),
                 None if z is None else host_f64(z).reshape(n, k))


# ---- the pipeline's data ---------------------------------------------------------------------------------------------------------------
def whitening_of(prec=None, prec_diag=None):
    """(W, c) of the conditional residuals: W = diag(P_ii)^(-1/2) P and c_i = log(P_ii / 2 pi) / 2."""
    p = dense_precision(prec, prec_diag)
    dg = np.diag(p)
    return p / np.sqrt(dg)[:, None], 0.5 * np.log(dg / (2. * np.pi))


def data_loo(density, x, log_weights=None, outputs=None):
    """PSIS-LOO and WAIC of the data points of a ``Chi2PipelineDensity`` at the draws ``x`` -> a ``DataLOO`` (with ``pit``).

    x : GPU tensor (n_chain, n_draw, d), or (n, d); the ORIGINAL space (the surrogate's ``_input_scales`` are the input map, as in
        ``predictive``); float64 or float32, read in place.
    log_weights : one log importance weight per draw, e.g. ``psis(...).log_weights``.
    outputs : indices of the data points (sorted, unique), default all."""
    import torch
    from .. import _lib
    from ..device import DevicePolyModel, polymodel_dense_from_poly, residual_dense
    from .predictive import output_plan
    check_one_process('data_loo')
    check_gpu_draws('data_loo', x)
    check_density(density)
    su = density.surrogate
    x = shaped_draws(x, su.input_size)
    n_chain, n_draw = int(x.shape[0]), int(x.shape[1])
    n = n_chain * n_draw
    idx, batches = output_plan(outputs, int(su.output_size), _lib.DIAG_BATCH)
    w, c = whitening_of(density._prec, density._pdiag)
    with torch.cuda.device(x.device):
        # the residual model takes the context's one polymodel slot; the surrogate's own device model uploads itself again at
        # its next use (DevicePolyModel.upload_if_needed)
        rm = DevicePolyModel.from_dense(residual_dense(polymodel_dense_from_poly(su.poly_spec()), density._y, w))
        ctx = rm.ctx
        lo, diff = input_map(ctx, su)
        st = _Stages(ctx, n, base_log_weights(log_weights, x, n))
        buf = ctx.empty((n_chain, n_draw, _lib.DIAG_BATCH))
        done = 0
        for calls in batches:
            ncol = 0
            for k0, nb, col in calls:
                rm.fun_columns(x, k0, nb, lo, diff, out=buf[:, :, col:])
                ncol = col + nb
            cb = np.zeros(_lib.DIAG_BATCH)
            cb[:ncol] = c[idx[done:done + ncol]]
            done += ncol
            st.run(buf, _lib.DIAG_BATCH, ncol, _lib.PLOO_Z, ctx.tensor(cb))
        return st.result(idx)
