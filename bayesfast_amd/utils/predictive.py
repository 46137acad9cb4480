"""Posterior predictive summaries of a pipeline's outputs, on the device.

After ``sample()`` the draws of the INPUTS sit in the (chain, time, dimension) tensor.  ``predictive`` answers three questions about
the OUTPUTS of the multi-output surrogate under that posterior, without ever materialising the (n, m) tensor of their values:

- what the model predicts for each data point: the table of mean, sd, quantiles, ESS and R-hat of every output (``table``), and
  with a ``Chi2PipelineDensity`` its pull against the data, ``(mean - y) / sigma``;
- whether the model fits the data: the chi-square of every draw (``chi2``), its table, the best-fit draw and the posterior
  predictive p-value of the chi-square discrepancy (``ppp``);
- how much of the posterior sits outside the surrogate's extrapolation bound (``oob_share``), where every output is a linear
  extrapolation.

The outputs are walked in batches of W columns: ``DevicePolyModel.fun_columns`` (``bfhip_polymodel_columns``) evaluates a batch at
the draws, read in place from the chain tensor, into one (n_chain, n_draw, W) buffer, and that buffer goes to the existing device
tables as the tensor it is -- ``utils.summary`` without weights, ``utils.weighted_summary`` with them.  Their results do not depend
on the batch or column an output lands in, so neither does this table.  The working memory is the buffer and the tables' own
buffers, whatever m is.

``ppp``.  Under a Gaussian likelihood with a known covariance, the chi-square of a replicated data vector drawn at ANY parameter
value is chi-square distributed with m degrees of freedom.  The posterior predictive p-value of the chi-square discrepancy,
P(chi2(y_rep, theta) >= chi2(y, theta) | y), is therefore the posterior mean of the survival function Q(m / 2, chi2(y, theta) / 2),
and no replicate has to be drawn.  It holds for that likelihood only.

Limits: device tensors only (the package has no host evaluation of a ``PolyModel``), one process, n = n_chain n_draw <= 2^31 - 1,
at most 128 inputs; the chi-square is the likelihood's, without the prior or the decay term."""
import numpy as np

from ._pipeline_data import check_gpu_draws, input_map, shaped_draws
from .diagnostics import Summary

__all__ = ['predictive', 'Predictive', 'output_plan', 'batch_width']


# ---- the pure parts (tests/test_predictive_host.py) --------------------------------------------------------------------------------
def batch_width(batch_bytes, n, n_sel):
    """Columns of the buffer: ``batch_bytes // (8 n)``, at least 1, rounded down to a multiple of 16 from 16 on (the tables take 16
    columns at a time), and at most ``n_sel`` (everything at once when it fits)."""
    w = max(1, int(batch_bytes) // (8 * int(n)))
    if w >= 16:
        w -= w % 16
    return max(1, min(int(n_sel), w))


def output_plan(outputs, m, width):
    """The selection and its walk: ``outputs`` (None: all m) taken sorted and unique -> (the index array, the batches).  A batch is
    a list of calls (k0, nb, col): outputs k0 .. k0 + nb - 1, a contiguous run of the selection, go to the buffer's columns
    col .. col + nb - 1; a batch fills at most ``width`` columns, in the selection's order.  Out-of-range indices: ValueError."""
    m, width = int(m), int(width)
    if width < 1:
        raise ValueError('width should be positive.')
    if outputs is None:
        idx = np.arange(m, dtype=np.int64)
    else:
        a = np.asarray(outputs)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError('outputs should be integer indices.')
        idx = np.unique(a.astype(np.int64).reshape(-1))
        if idx.size and (idx[0] < 0 or idx[-1] >= m):
            raise ValueError('outputs should lie in [0, %d).' % m)
    batches = []
    for b0 in range(0, idx.size, width):
        part = idx[b0:b0 + width]
        cuts = np.flatnonzero(np.diff(part) != 1) + 1
        starts = np.concatenate([[0], cuts])
        ends = np.concatenate([cuts, [part.size]])
        batches.append([(int(part[s]), int(e - s), int(s)) for s, e in zip(starts, ends)])
    return idx, batches


def chi2_chunk(batch_bytes, m):
    """Draws per pass of the chi-square: ``max(64, batch_bytes // (8 m))``."""
    return max(64, int(batch_bytes) // (8 * int(m)))


def sigma_of(prec=None, prec_diag=None):
    """The data's standard deviations: ``prec_diag**-0.5``, or ``sqrt(diag(inv(prec)))``."""
    if (prec is None) == (prec_diag is None):
        raise ValueError('give me exactly one of prec and prec_diag.')
    if prec_diag is not None:
        return np.asarray(prec_diag, dtype=np.float64).reshape(-1)**-0.5
    return np.sqrt(np.diag(np.linalg.inv(np.asarray(prec, dtype=np.float64))))


def pull_of(mean, y, sigma):
    return (np.asarray(mean, dtype=np.float64) - np.asarray(y, dtype=np.float64)) / np.asarray(sigma, dtype=np.float64)


def _torch_of(a):
    import torch
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


def _weights_of(log_weights, like):
    """Raw weights exp(lw - max lw), float64, flat, where ``like`` lives; None without weights."""
    import torch
    if log_weights is None:
        return None
    g = _torch_of(log_weights).detach().to(like.device).reshape(-1).to(torch.float64)
    if g.numel() != like.numel():
        raise ValueError('log_weights should hold one value per draw.')
    return torch.exp(g - g.max())


def oob_share_of(outside, weights=None):
    """Share of the sample with the flag set -> (overall, per chain).  ``outside`` (n_chain, n_draw) bool (tensor or array);
    ``weights`` raw, non-negative, one per draw, or None.  Overall: count / n, or sum(w flag) / sum(w); per chain always unweighted."""
    import torch
    o = _torch_of(outside)
    if o.dim() == 1:
        o = o[None]
    o = o != 0
    chain = (o.sum(dim=1).to(torch.float64) / o.shape[1]).cpu().numpy()
    if weights is None:
        return float(int(o.sum().item()) / o.numel()), chain
    w = _torch_of(weights).to(o.device).reshape(-1).to(torch.float64)
    return float((torch.where(o.reshape(-1), w, torch.zeros_like(w)).sum() / w.sum()).item()), chain


def ppp_of(chi2, dof, weights=None):
    """The (weighted) mean of Q(dof / 2, chi2 / 2), the chi-square survival function, over the draws.  Rows of zero weight are not
    part of the sample; a NaN chi-square among the others makes it NaN."""
    import torch
    c = _torch_of(chi2).reshape(-1).to(torch.float64)
    p = torch.special.gammaincc(torch.full_like(c, 0.5 * float(dof)), 0.5 * c)
    p = torch.where(torch.isnan(c), c, p)
    if weights is None:
        return float(p.mean().item())
    w = _torch_of(weights).to(c.device).reshape(-1).to(torch.float64)
    return float((torch.where(w > 0, w * p, torch.zeros_like(p)).sum() / w.sum()).item())


def _concat_tables(parts):
    return Summary([(k, np.concatenate([p[k] for p in parts], axis=-1)) for k in parts[0].names])


# ---- the report ------------------------------------------------------------------------------------------------------------------------
class Predictive:
    """What ``predictive`` returns.  Always: ``outputs`` (the selected output indices), ``table`` (a ``Summary`` over them), ``beta``
    (device tensor (n_chain, n_draw): the bound radius of every draw), ``alpha`` (the bound, None without one), ``oob_share`` (share
    of the sample with beta > alpha, weighted when weights were given) and ``oob_share_chain`` ((n_chain,), unweighted).  For a
    ``Chi2PipelineDensity`` also ``y``, ``sigma`` and ``pull`` per selected output, ``chi2`` (device tensor (n_chain, n_draw), over
    ALL m outputs), ``chi2_table``, ``chi2_min``, ``best`` = (chain, draw), ``dof`` = m and ``ppp``; None otherwise."""

    def __init__(self, outputs, table, beta, alpha, oob_share, oob_share_chain, y=None, sigma=None, pull=None, chi2=None,
                 chi2_table=None, chi2_min=None, best=None, dof=None, ppp=None):
        self.outputs, self.table, self.beta, self.alpha = outputs, table, beta, alpha
        self.oob_share, self.oob_share_chain = oob_share, oob_share_chain
        self.y, self.sigma, self.pull = y, sigma, pull
        self.chi2, self.chi2_table, self.chi2_min, self.best, self.dof, self.ppp = chi2, chi2_table, chi2_min, best, dof, ppp

    def __str__(self):
        n_chain, n_draw = (int(v) for v in self.beta.shape)
        rows = ['Predictive: %d outputs at %d chains x %d draws' % (len(self.outputs), n_chain, n_draw)]
        if self.alpha is None:
            rows.append('  no extrapolation bound')
        else:
            rows.append('  outside the bound (beta > %.4g): %.3g of the sample; per chain up to %.3g'
                        % (self.alpha, self.oob_share, float(np.max(self.oob_share_chain))))
        if len(self.outputs) and 'rhat' in self.table.names:
            rows.append('  outputs: largest rhat %.4g, smallest ess_bulk %.4g' % (np.nanmax(self.table['rhat']), np.nanmin(self.table['ess_bulk'])))
        if self.chi2 is not None:
            rows.append('  chi2: best %.6g at chain %d, draw %d; mean %.6g; dof %d; ppp %.4g'
                        % (self.chi2_min, self.best[0], self.best[1], float(self.chi2_table['mean'][0]), self.dof, self.ppp))
            if len(self.outputs):
                i = int(np.nanargmax(np.abs(self.pull))) if np.isfinite(self.pull).any() else 0
                rows.append('  largest |pull|: %.3g at output %d' % (abs(self.pull[i]), int(self.outputs[i])))
        return '\n'.join(rows)

    __repr__ = __str__


def _chi2_of(density, dm, x, lo, diff, batch_bytes):
    """(f - y)^T prec (f - y) of every draw over all m outputs -> (n_chain, n_draw) device tensor, in passes of ``chi2_chunk`` draws
    through ``bfhip_polymodel_eval`` (no Jacobian) and ``bfhip_chi2_stage`` (no gradient).  The stage runs with logp0 = 0, so that
    turning its logp back, chi2 = 2 (logp0 - logp), is exact."""
    import torch
    from .. import _lib
    from ..device import _ptr
    ctx = dm.ctx
    n_chain, n_draw, d = (int(v) for v in x.shape)
    m = dm.m
    rows = chi2_chunk(batch_bytes, m)
    y = ctx.tensor(density._y)
    pr = None if density._prec is None else ctx.tensor(density._prec)
    pd = None if density._pdiag is None else ctx.tensor(density._pdiag)
    lp = ctx.empty((n_chain, n_draw))

    def run(xc, lpc):   # xc (k, d) a view or a copy; lpc (k,) contiguous
        xs = xc.to(torch.float64)
        if lo is not None:
            xs = (xs - lo) / diff
        f, _ = dm.fun_and_jac(xs.contiguous(), jac=False)
        _lib.check(ctx._lib.bfhip_chi2_stage(ctx.handle, int(xs.shape[0]), m, d, _ptr(f), None, _ptr(y), _ptr(pr), _ptr(pd), 0.,
                                             _ptr(lpc), None))

    if rows >= n_draw:   # whole chains at a time
        step = max(1, rows // n_draw)
        for c0 in range(0, n_chain, step):
            c1 = min(n_chain, c0 + step)
            run(x[c0:c1].reshape(-1, d), lp[c0:c1].reshape(-1))
    else:
        for c in range(n_chain):
            for t0 in range(0, n_draw, rows):
                run(x[c, t0:t0 + rows], lp[c, t0:t0 + rows])
    return -2. * lp


def predictive(model, x, log_weights=None, outputs=None, probs=(0.16, 0.5, 0.84), batch_bytes=1 << 30):
    """Posterior predictive summaries of the outputs of ``model`` at the draws ``x`` -> a ``Predictive``.

    model : a multi-output ``PolyModel`` (its inputs are x as given: the table and the bound part only) or a
        ``Chi2PipelineDensity`` (its surrogate with ``surrogate._input_scales`` as the input map, x in the ORIGINAL space; also the
        pull, the chi-square of every draw and ``ppp``).
    x : GPU tensor (n_chain, n_draw, d), or (n, d) taken as one chain; float64 or float32, read in place.
    log_weights : one log importance weight per draw ((n_chain, n_draw) or flat), e.g. ``psis(...).log_weights``; the table is then
        ``utils.weighted_summary``'s.
    outputs : indices of the outputs in the table (sorted, unique), default all.
    probs : the table's quantiles.
    batch_bytes : size of the (n_chain, n_draw, W) buffer the outputs are walked in, and of a pass of the chi-square."""
    import torch
    from .. import parallel
    from .diagnostics import summary
    from .psis import weighted_summary
    if parallel.world()[1] > 1:
        raise NotImplementedError('predictive covers one process: gather the chains first.')
    check_gpu_draws('predictive', x)
    density = model if hasattr(model, 'surrogate') and hasattr(model, '_y') else None
    su = model.surrogate if density is not None else model
    if not hasattr(su, 'poly_spec') or not hasattr(su, 'device_model'):
        raise ValueError('model should be a PolyModel or a Chi2PipelineDensity.')
    x = shaped_draws(x, su.input_size)
    n_chain, n_draw, m = int(x.shape[0]), int(x.shape[1]), int(su.output_size)
    n = n_chain * n_draw
    with torch.cuda.device(x.device):
        dm = su.device_model()
        ctx = dm.ctx
        alpha = float(dm._desc.alpha) if dm._desc.use_bound else None   # (an all-linear model ignores its bound)
        lo, diff = input_map(ctx, su) if density is not None else (None, None)
        w = _weights_of(log_weights, x[:, :, 0])
        idx_all, _ = output_plan(outputs, m, 1)
        width = batch_width(batch_bytes, n, max(1, idx_all.size))
        idx, batches = output_plan(outputs, m, width)
        buf = ctx.empty((n_chain, n_draw, max(width, 2)))
        beta, parts = None, []
        for calls in batches:
            ncol = 0
            for k0, nb, col in calls:
                r = dm.fun_columns(x, k0, nb, lo, diff, beta=beta is None, out=buf[:, :, col:])
                if beta is None:
                    beta = r[1]
                ncol = col + nb
            # A batch of one column goes to the tables next to a copy of itself.  Their Geyer sums run down the rows of a
            # (lags, columns) host array, which NumPy adds row by row for two columns or more and pairwise for one: a one-column
            # table differs from the same column's row of a wider table in the last bits of its ESS.
            if ncol == 1:
                buf[:, :, 1] = buf[:, :, 0]
            cols = buf[:, :, :max(ncol, 2)]
            part = summary(cols, probs) if w is None else weighted_summary(cols, weights=w, probs=probs)
            parts.append(part if ncol > 1 else Summary([(k, part[k][..., :1]) for k in part.names]))
        if beta is None:   # an empty selection: the bound part alone
            beta = dm.fun_columns(x, 0, 1, lo, diff, beta=True, out=buf[:, :, :1])[1]
        del buf
        table = _concat_tables(parts) if parts else Summary([])
        if alpha is None:
            share, share_chain = 0., np.zeros(n_chain)
        else:
            share, share_chain = oob_share_of(beta > alpha, w)
        if density is None:
            return Predictive(idx, table, beta, alpha, share, share_chain)
        chi2 = _chi2_of(density, dm, x, lo, diff, batch_bytes)
        c3 = chi2[:, :, None]
        chi2_table = summary(c3, probs) if w is None else weighted_summary(c3, weights=w, probs=probs)
        flat = chi2.reshape(-1)
        finite = torch.where(torch.isnan(flat), torch.full_like(flat, float('inf')), flat)
        if w is not None:
            finite = torch.where(w > 0, finite, torch.full_like(flat, float('inf')))
        best = int(torch.argmin(finite).item())
        sigma = sigma_of(density._prec, density._pdiag)
        y = np.array(density._y)
        pull = pull_of(table['mean'], y[idx], sigma[idx]) if idx.size else np.zeros(0)
        return Predictive(idx, table, beta, alpha, share, share_chain, y=y, sigma=sigma, pull=pull, chi2=chi2, chi2_table=chi2_table,
                          chi2_min=float(flat[best].item()), best=(best // n_draw, best % n_draw), dof=m, ppp=ppp_of(chi2, m, w))
