"""Does a constraint come from the data or from the prior, and do the two disagree?  Power-scaling sensitivity (Kallioinen, Paananen,
Buerkner, Vehtari 2023, "Detecting and diagnosing prior and likelihood sensitivity with power-scaling"; the ``priorsense``
diagnostic): raise the prior, or the likelihood, to a power alpha close to 1, reweight the draws at hand by Pareto-smoothed importance
sampling, and measure how far every marginal moves.  What moves under the prior's power and not under the likelihood's is driven by
the prior; what moves under both is a conflict between prior and data.

Sample, weights and scenarios.  The draws are x (n, d).  The base log weights b_s are normalised to logsumexp 0 (``log_weights``;
without them b_s = -log n); a row with b_s = -inf is not part of the sample.  There are C component columns g_c(s), each the per-draw
log of one factor of the posterior, and A powers alpha_a.  Scenario (c, a) has the log ratio l = (alpha_a - 1) g_c, and everything
that reweight.py defines for a scenario is taken from it unchanged, through the same three stages: v_s, khat, sigma, n_tail, ess,
flags, log_evidence_ratio, mean, sd and mcse_mean.  u_s = exp(v_s) / sum over the rows of the sample; w_s = exp(b_s).

Sorted quantities of one parameter.  The rows of the sample sorted by value, stable and ascending (``bfhip_wstat_columns`` with w
masks the rows of zero weight to NaN, so they sort last: the sample is the first n_pos = wsum[2] positions).  x_(p), w_(p) and u_(p)
are value and weights at sorted position p;

  P_p = sum_{p' <= p} w_(p')      Q_p = sum_{p' <= p} u_(p')      h_p = x_(p+1) - x_(p), p = 0 .. n_pos - 2      M_p = (P_p + Q_p) / 2

Figures per parameter and scenario:

  bound = sum h_p (P_p + Q_p)
  J     = sum h_p [P_p log2(P_p / M_p) + Q_p log2(Q_p / M_p)],  0 log 0 = 0
  cjs   = sqrt(J / bound)
  ks    = max over p with h_p > 0 of |P_p - Q_p|

cjs is the symmetrised, normalised cumulative Jensen-Shannon distance of Nguyen & Vreeken (2015) as ``priorsense`` uses it (in the two
one-sided terms of that form +-(int Q - int P) / (2 ln 2) cancel in the sum).

Evaluating J.  Every term is non-negative.  With t = (Q - P) / (P + Q) the term is M [(1 - t) log1p(-t) + (1 + t) log1p(t)] / ln 2,
M t^2 / ln 2 to leading order; the bracket is taken in that form, and from its even series sum_k t^(2k) / (k (2k - 1)), nine terms,
below |t| = 1/8.  The numerator of t is the running sum of u - w, not the difference of two running sums: the naive form P log2 P -
P log2 M + ... cancels to first order and loses a digit for every factor of ten in alpha - 1.

Special cases.  u bit-equal to w gives cjs == 0 and ks == 0 exactly.  bound == 0 (one draw, or a constant parameter) gives NaN.  A
non-finite draw in a row of the sample makes that parameter NaN in every scenario.  A scenario with flag 1 or 4 is NaN in every
parameter.

Sensitivity per component and parameter.  alpha_lo is the largest power below 1, alpha_hi the smallest above 1;

  sensitivity   = (cjs_lo / |log2 alpha_lo| + cjs_hi / log2 alpha_hi) / 2      (``priorsense``'s (cjs_lo + cjs_hi) / (2 log2 alpha_hi) at
                                                                               its default powers 0.99 and 1.01)
  mean_gradient = (mean_hi - mean_lo) / (log2 alpha_hi - log2 alpha_lo) / sd_base;   sd_gradient the same expression on sd

``alphas`` must hold a value on each side of 1 and no 1.

Diagnosis, where components are named 'prior' and 'likelihood', with threshold = 0.05, the paper's value: prior and likelihood
sensitivity both above it 'prior-data conflict'; the prior's alone 'strong prior / weak likelihood'; otherwise '-'.

Two routes compute the same numbers: NumPy arrays and CPU tensors take the host port below; GPU tensors take the device route --
``reweight._Stages`` for the base table and the three stages of a batch of 16 scenarios, ``bfhip_rw_weights`` (csrc/bfhip_pscale.h) for
the batch's weights u, then per parameter one ``bfhip_diag_sort`` and per resident batch one ``bfhip_pscale_cjs`` (csrc/
bfhip_pscale.hip), a gather-scan of w and the 16 columns of u - w over the sort's permutation.

Limits: cjs integrates over the sample's own range [min x, max x], so it depends weakly on n; the threshold is a convention; powers far
from 1 fail as ``data_reweight`` does, and khat says so; mcse_mean and the smoothing ignore the autocorrelation of a chain; one
process; ``data_power_scale`` reads device tensors only; the decay term of a density belongs to neither component and is not scaled;
n <= 2^31 - 1."""
import numpy as np

from . import reweight as _rw
from ._pipeline_data import (check_density, check_gpu_draws, check_one_process, host_f64, input_map, logsumexp_host, shaped_draws)
from .psis import _psis_host

__all__ = ['power_scale', 'data_power_scale', 'PowerScale']

_LN2 = float(np.log(2.))
_CONFLICT, _STRONG, _NONE = 'prior-data conflict', 'strong prior / weak likelihood', '-'


class PowerScale:
    """What ``power_scale`` and ``data_power_scale`` return.  ``names`` of the C components, ``alphas`` (A,), ``n`` draws,
    ``threshold``; (d,) arrays ``mean_base`` and ``sd_base``; per scenario, (C, A) arrays: ``khat``, ``ess``, ``flags`` (int; 1 a
    non-finite ratio, 2 nothing smoothed, 4 no draw of non-zero weight) and ``log_evidence_ratio``; (C, A, d) arrays: ``cjs``, ``ks``,
    ``mean``, ``sd`` and ``mcse_mean``; (C, d) arrays: ``sensitivity``, ``mean_gradient`` and ``sd_gradient``; ``diagnosis``: d strings,
    or None without components named 'prior' and 'likelihood'; ``n_khat_bad``, the number of scenarios with khat > 0.7."""

    def __init__(self, names, alphas, n, threshold, rw, cjs, ks):
        c, a = len(names), len(alphas)
        d = int(np.size(rw.mean_base))
        self.names, self.alphas, self.n, self.threshold = list(names), np.array(alphas, dtype=np.float64), int(n), float(threshold)
        self.mean_base, self.sd_base = rw.mean_base, rw.sd_base
        for name in ('khat', 'ess', 'log_evidence_ratio'):
            setattr(self, name, getattr(rw, name).reshape(c, a))
        self.flags = rw.flags.reshape(c, a)
        for name in ('mean', 'sd', 'mcse_mean'):
            setattr(self, name, getattr(rw, name).reshape(c, a, d))
        self.cjs, self.ks = np.asarray(cjs, dtype=np.float64).reshape(c, a, d), np.asarray(ks, dtype=np.float64).reshape(c, a, d)
        self.n_khat_bad = rw.n_khat_bad
        below = np.where(self.alphas < 1., self.alphas, -np.inf)
        above = np.where(self.alphas > 1., self.alphas, np.inf)
        lo, hi = int(np.argmax(below)), int(np.argmin(above))
        l2lo, l2hi = np.log2(self.alphas[lo]), np.log2(self.alphas[hi])
        with np.errstate(all='ignore'):
            self.sensitivity = 0.5 * (self.cjs[:, lo] / abs(l2lo) + self.cjs[:, hi] / l2hi)
            self.mean_gradient = (self.mean[:, hi] - self.mean[:, lo]) / (l2hi - l2lo) / self.sd_base[None, :]
            self.sd_gradient = (self.sd[:, hi] - self.sd[:, lo]) / (l2hi - l2lo) / self.sd_base[None, :]
            self.diagnosis = None
            if 'prior' in self.names and 'likelihood' in self.names:
                sp = self.sensitivity[self.names.index('prior')] > self.threshold
                sl = self.sensitivity[self.names.index('likelihood')] > self.threshold
                self.diagnosis = [_CONFLICT if p and l else _STRONG if p else _NONE for p, l in zip(sp, sl)]

    def __str__(self):
        rows = ['PowerScale: %d components x %d powers, %d parameters at %d draws' % (len(self.names), len(self.alphas),
                                                                                      len(self.mean_base), self.n),
                '  khat > 0.7 at %d scenarios' % self.n_khat_bad]
        for i, name in enumerate(self.names):
            s = self.sensitivity[i]
            if np.isfinite(s).any():
                j = int(np.nanargmax(s))
                rows.append('  %s: largest sensitivity %.3g in parameter %d (mean gradient %.3g, sd gradient %.3g)'
                            % (name, s[j], j, self.mean_gradient[i, j], self.sd_gradient[i, j]))
            else:
                rows.append('  %s: no finite sensitivity' % name)
        if self.diagnosis is not None:
            for what in (_CONFLICT, _STRONG):
                hit = [j for j, v in enumerate(self.diagnosis) if v == what]
                if hit:
                    rows.append('  %s (sensitivity > %g): parameters %s' % (what, self.threshold, ', '.join(str(j) for j in hit)))
        return '\n'.join(rows)

    __repr__ = __str__


def _check_alphas(alphas):
    a = np.asarray(alphas, dtype=np.float64).reshape(-1)
    if a.size < 2 or not np.all(np.isfinite(a)) or not np.all(a > 0) or np.any(a == 1.) or not (np.any(a < 1.) and np.any(a > 1.)):
        raise ValueError('alphas should be positive, hold a value on each side of 1 and no 1.')
    return a


# ---- the host port ---------------------------------------------------------------------------------------------------------------------
def _bracket(t):
    """(1 - t) log1p(-t) + (1 + t) log1p(t), from its even series below |t| = 1/8"""
    with np.errstate(all='ignore'):
        s = t * t
        v = np.full_like(s, 1. / 153.)
        for c in (120., 91., 66., 45., 28., 15., 6., 1.):
            v = v * s + 1. / c
        a, b = 1. - t, 1. + t
        big = np.where(a == 0., 0., a * np.log1p(-t)) + np.where(b == 0., 0., b * np.log1p(t))
        return np.where(np.abs(t) < 0.125, v * s, big)


def ecdf_distance(v, wp, up):
    """(J, bound, cjs, ks), each (S,), of the sorted values v (p,) of the sample with the base weights wp (p,) and the S columns of
    weights up (p, S) in that order."""
    s = up.shape[1]
    nan = np.full(s, np.nan)
    if v.size and not np.isfinite(v).all():
        return nan, nan, nan, nan
    if v.size < 2:
        return np.zeros(s), np.zeros(s), nan, nan
    with np.errstate(all='ignore'):
        big_p = np.cumsum(wp)[:-1, None]
        big_d = np.cumsum(up - wp[:, None], axis=0)[:-1]
        h = np.diff(v)[:, None]
        tot = big_p + (big_p + big_d)   # P + Q
        t = np.clip(big_d / tot, -1., 1.)
        bound = (h * tot).sum(axis=0)
        big_j = (h * ((0.5 * tot) * _bracket(t))).sum(axis=0) / _LN2
        ks = np.where(h > 0., np.abs(big_d), 0.).max(axis=0)
        ok = bound != 0.
        return big_j, bound, np.where(ok, np.sqrt(big_j / np.where(ok, bound, 1.)), np.nan), np.where(ok & ~np.isnan(big_j), ks, np.nan)


def _ratios(g, alphas):
    """(n, C) components -> (n, C A) log ratios, scenario (c, a) in column c A + a"""
    with np.errstate(all='ignore'):
        return (g[:, :, None] * (alphas - 1.)[None, None, :]).reshape(g.shape[0], -1)


def _host(x, g, log_weights, alphas):
    """x (n, d), g (n, C) float64, log_weights (n,) or None -> (Reweighted, cjs (C A, d), ks (C A, d))"""
    n, d = x.shape
    l = _ratios(g, alphas)
    big_k = l.shape[1]
    rw = _rw._host(x, l, log_weights)
    with np.errstate(all='ignore'):
        lb = None if log_weights is None else log_weights - logsumexp_host(log_weights)
        keep = np.ones(n, dtype=bool) if lb is None else lb > -np.inf
        wb = np.exp(lb[keep]) if lb is not None else np.full(int(keep.sum()), 1. / n)
        u = np.full((int(keep.sum()), big_k), np.nan)
        for k in range(big_k):
            if rw.flags[k] & 5:
                continue
            r = np.full(n, -np.inf)
            r[keep] = l[keep, k] if lb is None else lb[keep] + l[keep, k]
            v = _psis_host(r)[0][keep]
            e = np.exp(v - v.max())   # (about the largest, as the device route has it: equal ratios are equal weights bit for bit)
            u[:, k] = e / e.sum()
        cjs, ks = np.full((big_k, d), np.nan), np.full((big_k, d), np.nan)
        for j in range(d):
            xk = x[keep, j]
            order = np.argsort(xk, kind='stable')
            _, _, cjs[:, j], ks[:, j] = ecdf_distance(xk[order], wb[order], u[order])
    return rw, cjs, ks


# ---- the device route ------------------------------------------------------------------------------------------------------------------
def _device(x, g, log_weights, alphas, max_bytes):
    """x (n_chain, n_draw, d) and g (n_chain, n_draw, C) device tensors -> (Reweighted, cjs (C A, d), ks (C A, d))"""
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    from .diagnostics import _device_batches
    n_chain, n_draw, n_comp = (int(v) for v in g.shape)
    n = n_chain * n_draw
    x = shaped_draws(x, x.shape[2])   # (refuses n > 2^31 - 1 before anything is allocated)
    d = int(x.shape[2])
    if d > _lib.MAX_DIM:
        raise NotImplementedError('more than %d parameters.' % _lib.MAX_DIM)
    n_alpha, width = len(alphas), _lib.DIAG_BATCH
    big_k = n_comp * n_alpha
    with torch.cuda.device(x.device):
        ctx = get_context(x.device.index)
        lib, h = ctx._lib, ctx.handle
        st = _rw._Stages(ctx, x, log_weights)
        gf = g.detach().reshape(n, n_comp).to(torch.float64)
        am1 = torch.as_tensor(alphas - 1., dtype=torch.float64, device=x.device)
        starts = list(range(0, big_k, width))
        resident = min(len(starts), max(1, int(max_bytes) // (8 * width * n)))
        buf, col = ctx.empty((n, width)), ctx.empty((n, width))
        ubufs = [ctx.empty((n, width)) for _ in range(resident)]
        keys, order = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int32)
        work = ctx.empty((_lib.pscale_work(n),))
        wout = ctx.empty((len(starts), _lib.RWW_NOUT, width))
        cj = ctx.empty((len(starts), d, _lib.CJS_NOUT, width))
        for g0 in range(0, len(starts), resident):
            group = [(g0 + i, k0, min(width, big_k - k0)) for i, k0 in enumerate(starts[g0:g0 + resident])]
            for i, k0, nb in group:
                ks = torch.arange(k0, k0 + nb, device=x.device)
                buf[:, :nb] = -(gf[:, ks // n_alpha] * am1[ks % n_alpha][None, :])   # -l: the stages' ratio lb - ell is then lb + l
                out, head, tail = st.run(buf, nb)
                _lib.check(lib.bfhip_rw_weights(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out), *tail, _ptr(ubufs[i - g0]), width,
                                                _ptr(wout[i])))
            j0 = 0
            for xb, kb, nbp in _device_batches(x, n):
                _lib.check(lib.bfhip_wstat_columns(h, n_chain, n_draw, int(xb.stride(0)), int(xb.stride(1)), _ptr(xb),
                                                   int(xb.dtype == torch.float32), 0, kb, nbp, _ptr(st.w), _ptr(col)))
                for b in range(nbp):
                    _lib.check(lib.bfhip_diag_sort(h, n, _ptr(col), b, _ptr(keys), _ptr(order)))
                    for i, k0, nb in group:
                        _lib.check(lib.bfhip_pscale_cjs(h, n, _ptr(keys), _ptr(order), _ptr(st.wsum), _ptr(st.w), _ptr(ubufs[i - g0]), width,
                                                        nb, _ptr(cj[i, j0 + b]), _ptr(work)))
                j0 += nbp
        rw = st.result()
        o = cj.cpu().numpy()   # the one copy of the distances to the host, after the last launch
    rows = _lib.CJS_ROWS
    cjs = np.concatenate([o[i, :, rows.index('cjs'), :min(width, big_k - k0)].T for i, k0 in enumerate(starts)], axis=0)
    ks = np.concatenate([o[i, :, rows.index('ks'), :min(width, big_k - k0)].T for i, k0 in enumerate(starts)], axis=0)
    bad = (rw.flags & 5) != 0
    cjs[bad], ks[bad] = np.nan, np.nan
    return rw, cjs, ks


def power_scale(x, log_components, log_weights=None, alphas=(0.99, 1.01), names=None, threshold=0.05, max_bytes=2 << 30):
    """Power-scaling sensitivity of the draws ``x``, (n, d) or (n_chain, n_draw, d), to each of the C factors of the posterior whose
    per-draw logs are the columns of ``log_components``, of shape ``x.shape[:-1] + (C,)`` -> a ``PowerScale``.

    log_weights : one base log weight per draw (``x.shape[:-1]``, or flat), not necessarily normalised, -inf for a draw that is not
        part of the sample.
    alphas : the powers; a value on each side of 1 and no 1.
    names : C names; components named 'prior' and 'likelihood' give the diagnosis.  Default 'component 0', ...
    threshold : of the diagnosis.
    max_bytes : the device route keeps the (n, 16) weight buffers of as many batches of 16 scenarios resident as fit in this size (one
        at the least) and sorts every parameter once per such group; a scenario's figures do not depend on the grouping.

    GPU tensors take the device route (float32 draws are read as float64, a strided view of the draws goes in without a copy); NumPy
    arrays and CPU tensors take the host port."""
    if x.ndim not in (2, 3):
        raise ValueError('x should be (n, d) or (n_chain, n_draw, d).')
    n, d = int(np.prod(x.shape[:-1])), int(x.shape[-1])
    if n < 1 or d < 1:
        raise ValueError('x is empty.')
    g = log_components
    if g.ndim != x.ndim or tuple(g.shape[:-1]) != tuple(x.shape[:-1]) or int(g.shape[-1]) < 1:
        raise ValueError('log_components should have the shape x.shape[:-1] + (C,).')
    if log_weights is not None and int(np.prod(log_weights.shape)) != n:
        raise ValueError('log_weights should hold one value per draw.')
    a = _check_alphas(alphas)
    n_comp = int(g.shape[-1])
    names = ['component %d' % i for i in range(n_comp)] if names is None else [str(v) for v in names]
    if len(names) != n_comp or len(set(names)) != n_comp:
        raise ValueError('names should hold %d different names.' % n_comp)
    if getattr(x, 'is_cuda', False):
        import torch
        gt = torch.as_tensor(g, device=x.device)
        rw, cjs, ks = _device(x if x.ndim == 3 else x[None], gt if gt.ndim == 3 else gt[None], log_weights, a, max_bytes)
    else:
        rw, cjs, ks = _host(host_f64(x).reshape(n, d), host_f64(g).reshape(n, n_comp),
                            None if log_weights is None else host_f64(log_weights).reshape(-1), a)
    return PowerScale(names, a, n, threshold, rw, cjs, ks)


# ---- the pipeline's prior and likelihood -----------------------------------------------------------------------------------------------
def prior_inputs(density):
    """The inputs of a ``Chi2PipelineDensity`` with a prior (prior_prec > 0), ascending; empty without one."""
    return [] if density._prior_prec is None else [int(i) for i in np.flatnonzero(density._prior_prec > 0)]


def component_names(density, prior_each=False):
    """The components ``data_power_scale`` builds: 'likelihood', 'prior' where some input has one, and with ``prior_each`` 'prior[i]'
    per such input."""
    who = prior_inputs(density)
    return ['likelihood'] + (['prior'] if who else []) + (['prior[%d]' % i for i in who] if prior_each else [])


def data_power_scale(density, x, log_weights=None, alphas=(0.99, 1.01), prior_each=False, threshold=0.05, max_bytes=2 << 30,
                     batch_bytes=1 << 30):
    """Power-scaling sensitivity of a ``Chi2PipelineDensity`` to its likelihood and its prior at the draws ``x`` -> a ``PowerScale``.

    x : GPU tensor (n_chain, n_draw, d), or (n, d); the ORIGINAL space, as in ``data_loo``; float64 or float32, read in place.
    log_weights : one log importance weight per draw, e.g. ``psis(...).log_weights``.
    prior_each : one further component per input with a prior, 'prior[i]': the diagonal prior is separable, so this shows whose
        prior matters.
    batch_bytes : size of a pass of the chi-square, as in ``predictive``.

    The components are built on the device: 'likelihood' = -chi2 / 2 (logp0 is a constant and drops out) and 'prior' =
    -sum_i prior_prec_i (x_i - prior_mu_i)^2 / 2.  A density without a prior has no 'prior' component and no diagnosis."""
    import torch
    from .. import _lib
    from .predictive import _chi2_of
    check_one_process('data_power_scale')
    check_density(density)
    check_gpu_draws('data_power_scale', x)
    su = density.surrogate
    x = shaped_draws(x, su.input_size)
    n_chain, n_draw, d = (int(v) for v in x.shape)
    if log_weights is not None and int(np.prod(log_weights.shape)) != n_chain * n_draw:
        raise ValueError('log_weights should hold one value per draw.')
    if d > _lib.MAX_DIM:
        raise NotImplementedError('more than %d parameters.' % _lib.MAX_DIM)
    a = _check_alphas(alphas)
    names = component_names(density, prior_each)
    with torch.cuda.device(x.device):
        dm = su.device_model()
        ctx = dm.ctx
        lo, diff = input_map(ctx, su)
        g = ctx.empty((n_chain, n_draw, len(names)))
        g[:, :, 0] = -0.5 * _chi2_of(density, dm, x, lo, diff, batch_bytes)
        who = prior_inputs(density)
        if who:
            mu, prec = ctx.tensor(density._prior_mu), ctx.tensor(density._prior_prec)
            dx = x.to(torch.float64) - mu
            each = -0.5 * (prec * (dx * dx))
            g[:, :, 1] = each[:, :, who].sum(dim=2)
            if prior_each:
                g[:, :, 2:] = each[:, :, who]
        rw, cjs, ks = _device(x, g, log_weights, a, max_bytes)
    return PowerScale(names, a, n_chain * n_draw, threshold, rw, cjs, ks)
