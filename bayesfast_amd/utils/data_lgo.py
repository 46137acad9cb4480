"""Leave-group-out cross-validation of the pipeline's data by Pareto-smoothed importance sampling: does the rest of the data vector
predict a given block of it -- one probe, one bin pair, one scale cut?  This is the conditional posterior-predictive consistency test
of Doux et al. 2021 ("Dark Energy Survey internal consistency tests of the joint cosmological probe analysis with posterior
predictive distributions"), and what K-fold cross-validation means for data with a dense covariance.  ``data_loo`` is leave-ONE-out;
a block's conditional is not a function of its pointwise z_i, because the covariance inside the block enters.

The terms of a ``Chi2PipelineDensity``.  y is the data, f(theta) the surrogate's m outputs, P the precision (``prec``, or
``diag(prec_diag)``), r(theta) = y - f(theta) and g = P r.  A group B is a set of b output indices and P_BB = L_B L_B^T, L_B the lower
Cholesky factor.  The conditional of y_B given all the other data points at theta is Gaussian with precision P_BB, and
y_B - mean = P_BB^-1 g_B, so

  z_B(theta) = L_B^-1 g_B       b values, linear in f: a PolyModel (``device.linear_dense`` with A = -L_B^-1 P[B, :], b = L_B^-1 P[B, :] y)
  q_B(theta) = |z_B|^2
  c_B        = sum log diag(L_B) - (b / 2) log 2 pi
  ell_B(theta) = log p(y_B | y_-B, theta) = c_B - q_B / 2

At any theta a replicated y_B drawn from that conditional has q_B ~ chi^2_b exactly, so Q(b / 2, q_B / 2), the regularised upper
incomplete gamma function, is its survival function and no replicate is drawn.  For b = 1 this is ``data_loo``'s c_i - z_i^2 / 2.

Per group's column ell_s, s < n, with base log weights b_s normalised to logsumexp 0 (``log_weights``; without them b_s = -log n),
w_s = exp(b_s), and v_s = ``psis(b - ell).log_weights`` the smoothed, normalised log weights that remove the group:

  lpd, p_waic, elpd_waic            as in ``data_loo``, on the column ell_B
  elpd_lgo                          logsumexp_s(v_s + ell_s)
  p_lgo                             lpd - elpd_lgo
  khat, sigma, n_tail, ess_lgo      as ``data_loo``'s khat, sigma, n_tail, ess_loo
  chi2_base, chi2_lgo               sum w_s q_s, sum exp(v_s) q_s
  ppp_base, ppp_lgo                 sum w_s Q(b / 2, q_s / 2), sum exp(v_s) Q(b / 2, q_s / 2)

``ppp_lgo`` is the posterior predictive p-value of the block given the rest: calibrated, unlike ``predictive``'s ``ppp``, which uses
the data twice.  A small value says that the block is in tension with what the other data and the model predict.  ``ppp_base`` and
``lpd`` are the same figures without importance sampling: they are exact when ``x`` was sampled from a density built without the block.

Rows with b_s = -inf are not part of the sample, whatever they hold: they have the ratio -inf, count in n for the tail size as in
``psis``, and are left out of every sum over s (where fewer than n_tail + 1 rows have any weight, ``psis`` hands smoothed weight to
some of them: it stays in the normalisation and in ess_lgo, and out of every other sum).  A non-finite ell in a row of non-zero weight
makes every figure of that column NaN, as does a column without a row of non-zero weight.  n < 25, or a tail without spread, gives
khat = inf and unsmoothed weights, as in ``psis``.

Totals over the K groups: ``elpd_lgo_total``, ``p_lgo_total``, ``se_* = sqrt(K var_B(., ddof = 1))`` and ``n_khat_bad``, the number of
groups with khat > 0.7.

Two routes compute the same numbers: NumPy arrays and CPU tensors of conditional chi-squares take the host port below
(``grouped_loo``); GPU tensors take the device route (csrc/bfhip_lgo.h).  ``data_lgo`` walks the groups in batches of 16 slots; the
z columns of a batch go through the derived model's ``fun_columns`` 16 at a time into one (n, 16) buffer, ``bfhip_lgo_accum`` folds
them into the batch's (n, 16) buffer of ell columns, the first two PSIS-LOO stages of ``data_loo`` run on it unchanged, and
``bfhip_lgo_finish`` turns the smoothed weights into the figures in one pass, with a device Q(a, x) in double precision
(csrc/bfhip_igamc.h).  Neither the (n, m) outputs nor an (n, sum of b) residual tensor is ever formed.

Limits: a Gaussian likelihood with a fixed covariance; the likelihood only -- no prior, no decay term; one process; ``data_lgo``
reads device tensors only; n <= 2^31 - 1 draws and at most 128 inputs.  Importance sampling removes a small block, not a probe that
carries the posterior: khat > 0.7 says so, and the honest answer then is to sample without the block and read ``lpd`` and
``ppp_base``."""
import numpy as np

from ._pipeline_data import (base_log_weights, check_density, check_gpu_draws, check_one_process, dense_precision, host_f64, input_map,
                             shaped_draws, sum_and_se)
from .data_loo import _Stages, _host_column, _normalise_host
from .psis import _psis_host

__all__ = ['data_lgo', 'grouped_loo', 'group_whitening_of', 'DataLGO']

_GROUP = ('lpd', 'p_waic', 'elpd_waic', 'elpd_lgo', 'p_lgo', 'khat', 'sigma', 'ess_lgo', 'chi2_base', 'chi2_lgo', 'ppp_base', 'ppp_lgo')
_TOTAL = ('elpd_lgo', 'p_lgo')


class DataLGO:
    """What ``grouped_loo`` and ``data_lgo`` return.  ``groups``: a list of K index arrays; ``size`` (K,) their numbers of points.  Per
    group, (K,) arrays: ``lpd``, ``p_waic``, ``elpd_waic``, ``elpd_lgo``, ``p_lgo``, ``khat``, ``sigma``, ``n_tail`` (int), ``ess_lgo``,
    ``chi2_base``, ``chi2_lgo``, ``ppp_base`` and ``ppp_lgo``.  Totals: ``elpd_lgo_total``, ``p_lgo_total``, their ``se_*`` and
    ``n_khat_bad``; ``n`` draws."""

    def __init__(self, groups, size, n, cols):
        self.groups = [np.asarray(g, dtype=np.int64) for g in groups]
        self.size, self.n = np.asarray(size, dtype=np.int64), int(n)
        for name in _GROUP:
            setattr(self, name, np.asarray(cols[name], dtype=np.float64))
        self.n_tail = np.asarray(cols['n_tail'], dtype=np.int64)
        for name in _TOTAL:
            total, se = sum_and_se(getattr(self, name))
            setattr(self, name + '_total', total)
            setattr(self, 'se_' + name, se)
        with np.errstate(all='ignore'):
            self.n_khat_bad = int((self.khat > 0.7).sum())

    def _same_groups(self, other):
        return (isinstance(other, DataLGO) and len(self.groups) == len(other.groups) and
                all(np.array_equal(a, b) for a, b in zip(self.groups, other.groups)))

    def compare(self, other):
        """(difference of elpd_lgo_total, self minus other; its standard error sqrt(K var_B(difference_B, ddof = 1))).  Both should
        hold the same groups."""
        if not self._same_groups(other):
            raise ValueError('the two results should hold the same groups.')
        return sum_and_se(self.elpd_lgo - other.elpd_lgo)

    def __str__(self):
        k = len(self.groups)
        rows = ['DataLGO: %d groups of %d points at %d draws' % (k, int(self.size.sum()), self.n),
                '  elpd_lgo %.6g (se %.3g), p_lgo %.4g (se %.3g)' % (self.elpd_lgo_total, self.se_elpd_lgo, self.p_lgo_total, self.se_p_lgo)]
        if k and np.isfinite(self.khat).any():
            i = int(np.nanargmax(np.where(np.isfinite(self.khat), self.khat, -np.inf)))
            rows.append('  khat > 0.7 at %d groups; largest %.3g at group %d of %d points (ess_lgo %.4g)'
                        % (self.n_khat_bad, self.khat[i], i, int(self.size[i]), self.ess_lgo[i]))
        else:
            rows.append('  khat > 0.7 at %d groups' % self.n_khat_bad)
        if k and np.isfinite(self.ppp_lgo).any():
            i = int(np.nanargmin(self.ppp_lgo))
            rows.append('  ppp_lgo: smallest %.3g at group %d (chi2_lgo %.4g at %d points), largest %.3g'
                        % (self.ppp_lgo[i], i, self.chi2_lgo[i], int(self.size[i]), np.nanmax(self.ppp_lgo)))
        return '\n'.join(rows)

    __repr__ = __str__


# ---- the host port ---------------------------------------------------------------------------------------------------------------------
def _host_group(q, dof, c, lb):
    """Every figure of one group: q (n,) conditional chi-squares, dof, the constant c of ell, lb (n,) normalised base log weights or
    None."""
    from scipy.special import gammaincc
    n = q.size
    with np.errstate(all='ignore'):
        ell = c - 0.5 * q
    col = _host_column(ell, lb, None)
    out = dict(lpd=col['lpd'], p_waic=col['p_waic'], elpd_waic=col['elpd_waic'], elpd_lgo=col['elpd_loo'], p_lgo=col['p_loo'],
               khat=col['khat'], sigma=col['sigma'], ess_lgo=col['ess_loo'], n_tail=col['n_tail'], chi2_base=np.nan, chi2_lgo=np.nan,
               ppp_base=np.nan, ppp_lgo=np.nan)
    if np.isnan(col['lpd']):
        return out
    keep = np.ones(n, dtype=bool) if lb is None else lb > -np.inf
    with np.errstate(all='ignore'):
        qk = q[keep]
        w = np.exp(lb[keep]) if lb is not None else np.full(qk.size, 1. / n)
        r = np.full(n, -np.inf)
        r[keep] = (lb[keep] if lb is not None else 0.) - ell[keep]
        e = np.exp(_psis_host(r)[0][keep])
        big_q = gammaincc(0.5 * dof, 0.5 * qk)
        out.update(chi2_base=(w * qk).sum(), chi2_lgo=(e * qk).sum(), ppp_base=(w * big_q).sum(), ppp_lgo=(e * big_q).sum())
    return out


def _collect(groups, dof, n, cols):
    return DataLGO(groups, dof, n, {name: np.array([c[name] for c in cols]) for name in cols[0]})


def _host(q, dof, const, log_weights, groups):
    n, k = q.shape
    lb = _normalise_host(log_weights, n)
    return _collect(groups, dof, n, [_host_group(np.ascontiguousarray(q[:, j]), float(dof[j]), float(const[j]), lb) for j in range(k)])


# ---- the device route ------------------------------------------------------------------------------------------------------------------
class _LgoStages(_Stages):
    """``data_loo``'s stages with the leave-group-out finish: ``run_groups(buf, nb, c, dof)`` queues a batch of nb group columns of
    ell, ``group_result(groups, size)`` makes the one copy to the host."""

    def __init__(self, ctx, n, lb):
        super().__init__(ctx, n, lb)
        self.lgo = []

    def run_groups(self, buf, nb, c, dof):
        import ctypes as C
        from ..device import _ptr
        L = self._lib
        out, head, tail = self.front(buf, L.DIAG_BATCH, nb, L.PLOO_ELL)
        lgo = self.ctx.empty((len(L.LGO_ROWS), L.DIAG_BATCH))
        L.check(self.ctx._lib.bfhip_lgo_finish(*head[:5], (C.c_double * int(nb))(*[float(v) for v in c]),
                                               (C.c_double * int(nb))(*[float(v) for v in dof]), _ptr(self.lb), _ptr(self.keys),
                                               _ptr(self.idx), _ptr(out), _ptr(lgo), *tail))   # head[:5]: handle, n, buf, ld, nb
        self.outs.append(out)
        self.lgo.append(lgo)

    def group_result(self, groups, size):
        base = self.result(np.arange(len(groups)))   # the PSIS-LOO rows, in DataLOO's names
        o = self.collect(self.lgo, len(self._lib.LGO_ROWS))
        cols = dict(lpd=base.lpd, p_waic=base.p_waic, elpd_waic=base.elpd_waic, elpd_lgo=base.elpd_loo, p_lgo=base.p_loo, khat=base.khat,
                    sigma=base.sigma, ess_lgo=base.ess_loo, n_tail=base.n_tail)
        cols.update({name: o[i] for i, name in enumerate(self._lib.LGO_ROWS)})
        return DataLGO(groups, size, self.n, cols)


def _device(q, dof, const, log_weights, groups):
    """q (n_chain, n_draw, K) device tensor"""
    import torch
    from .. import _lib
    from ..device import get_context
    n_chain, n_draw, k = (int(v) for v in q.shape)
    n = n_chain * n_draw
    if n > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 draws.')
    width = _lib.DIAG_BATCH
    with torch.cuda.device(q.device):
        ctx = get_context(q.device.index)
        st = _LgoStages(ctx, n, base_log_weights(log_weights, q, n, keep_neginf=True))
        buf = ctx.empty((n, width))
        qf = q.detach().reshape(n, k)
        ct = torch.as_tensor(const, dtype=torch.float64, device=q.device)
        for k0 in range(0, k, width):
            nb = min(width, k - k0)
            buf[:, :nb] = ct[None, k0:k0 + nb] - 0.5 * qf[:, k0:k0 + nb].to(torch.float64)   # ell; the finish takes q back from it
            st.run_groups(buf, nb, const[k0:k0 + nb], dof[k0:k0 + nb])
        return st.group_result(groups, dof)


def grouped_loo(q, dof, const=None, log_weights=None):
    """Leave-group-out figures of every column of conditional chi-squares ``q``, (n, K) or (n_chain, n_draw, K) -> a ``DataLGO``
    (its ``groups`` are empty index arrays: the columns are all it knows).  ``dof`` (K,): the groups' numbers of points; ``const``
    (K,): c_B, default 0 (it moves lpd and elpd_lgo alone).  ``log_weights``: one base log weight per draw (``q.shape[:-1]``, or flat),
    not necessarily normalised, -inf for a draw that is not part of the sample.  NumPy arrays and CPU tensors take the host port
    (``scipy.special.gammaincc``); a GPU tensor is reduced on its device in batches of 16 columns, where q is taken back from
    ell = c - q / 2."""
    if q.ndim not in (2, 3):
        raise ValueError('q should be (n, K) or (n_chain, n_draw, K).')
    n, k = int(np.prod(q.shape[:-1])), int(q.shape[-1])
    if n < 1 or k < 1:
        raise ValueError('q is empty.')
    dof = np.asarray(dof, dtype=np.float64).reshape(-1)
    const = np.zeros(k) if const is None else np.asarray(const, dtype=np.float64).reshape(-1)
    if dof.shape != (k,) or const.shape != (k,) or not np.all(dof > 0) or not np.all(np.isfinite(dof)) or not np.all(np.isfinite(const)):
        raise ValueError('dof (positive) and const should hold one finite value per column.')
    if log_weights is not None and int(np.prod(log_weights.shape)) != n:
        raise ValueError('log_weights should hold one value per draw.')
    groups = [np.zeros(0, dtype=np.int64)] * k
    if getattr(q, 'is_cuda', False):
        return _device(q if q.ndim == 3 else q[None], dof, const, log_weights, groups)
    return _host(host_f64(q).reshape(n, k), dof, const, None if log_weights is None else host_f64(log_weights), groups)


# ---- the pipeline's data ---------------------------------------------------------------------------------------------------------------
def _parse_groups(groups, m):
    """``groups`` in either form -> a list of K sorted int64 index arrays."""
    m = int(m)
    try:
        flat = np.asarray(groups)
    except ValueError:   # (ragged)
        flat = None
    if flat is not None and flat.ndim == 1 and flat.dtype != object and flat.size and np.issubdtype(flat.dtype, np.integer):
        # one label per output, -1: in no group
        if flat.size != m or flat.min() < -1:
            raise ValueError('a label array should hold one label >= -1 per output (%d).' % m)
        out = [np.flatnonzero(flat == lab).astype(np.int64) for lab in np.unique(flat[flat >= 0])]
        if not out:
            raise ValueError('no group.')
        return out
    if isinstance(groups, (str, bytes)) or not hasattr(groups, '__len__') or len(groups) < 1:
        raise ValueError('groups should be a sequence of index sequences or an integer label array of length %d.' % m)
    out, seen = [], np.zeros(m, dtype=bool)
    for g in groups:
        try:
            a = np.asarray(g)
        except ValueError:
            a = np.zeros(0)
        if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError('a group should be a non-empty sequence of integer indices.')
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() >= m:
            raise ValueError('group indices should lie in [0, %d).' % m)
        if np.any(np.diff(a) <= 0):
            raise ValueError('a group should be sorted and unique.')
        if seen[a].any():
            raise ValueError('groups should be disjoint.')
        seen[a] = True
        out.append(a)
    return out


def group_whitening_of(prec=None, prec_diag=None, groups=None):
    """(A, const, sizes, column_group) of the groups' conditional residuals, the analogue of ``data_loo.whitening_of``: the rows of
    A (sum of b, m) are L_B^-1 P[B, :] group after group, so that z = A (y - f) holds z_B for every group in turn; const (K,) are c_B
    = sum log diag(L_B) - (b / 2) log 2 pi; sizes (K,) the b; column_group (sum of b,) the group of every row of A.

    groups : a sequence of K index sequences, each non-empty, sorted and unique, mutually disjoint, within [0, m); or an integer
        label array of length m, -1 for a point in no group (the groups are the labels in ascending order).  Anything else: ValueError."""
    p = dense_precision(prec, prec_diag)
    if groups is None:
        raise ValueError('groups should be a sequence of index sequences or an integer label array.')
    from scipy.linalg import solve_triangular
    gs = _parse_groups(groups, p.shape[0])
    rows, const = [], []
    for g in gs:
        try:
            low = np.linalg.cholesky(p[np.ix_(g, g)])
        except np.linalg.LinAlgError:
            raise ValueError('the precision of a group is not positive definite.')
        rows.append(solve_triangular(low, p[g, :], lower=True))
        const.append(np.log(np.diag(low)).sum() - 0.5 * g.size * np.log(2. * np.pi))
    sizes = np.array([g.size for g in gs], dtype=np.int64)
    return np.concatenate(rows, axis=0), np.array(const), sizes, np.repeat(np.arange(len(gs)), sizes)


def data_lgo(density, x, groups, log_weights=None):
    """Leave-group-out cross-validation of groups of data points of a ``Chi2PipelineDensity`` at the draws ``x`` -> a ``DataLGO``.

    x : GPU tensor (n_chain, n_draw, d), or (n, d); the ORIGINAL space (the surrogate's ``_input_scales`` are the input map, as in
        ``data_loo``); float64 or float32, read in place.
    groups : K index sequences (each non-empty, sorted, unique; mutually disjoint), or an integer label array of length m with -1
        for a point in no group.
    log_weights : one log importance weight per draw, e.g. ``psis(...).log_weights``."""
    import ctypes as C
    import torch
    from .. import _lib
    from ..device import DevicePolyModel, polymodel_dense_from_poly, linear_dense, _ptr
    check_one_process('data_lgo')
    check_gpu_draws('data_lgo', x)
    check_density(density)
    su = density.surrogate
    x = shaped_draws(x, su.input_size)
    n_chain, n_draw, d = (int(v) for v in x.shape)
    n = n_chain * n_draw
    if d > _lib.MAX_DIM:
        raise NotImplementedError('more than %d inputs.' % _lib.MAX_DIM)
    a, const, sizes, colg = group_whitening_of(density._prec, density._pdiag, groups)
    gs = _parse_groups(groups, int(su.output_size))
    width = _lib.DIAG_BATCH
    first = np.concatenate([[0], np.cumsum(sizes)])   # a group's first column
    y = np.asarray(density._y, dtype=np.float64).reshape(-1)
    with torch.cuda.device(x.device):
        # the residual model takes the context's one polymodel slot; the surrogate's own device model uploads itself again at its
        # next use (DevicePolyModel.upload_if_needed)
        rm = DevicePolyModel.from_dense(linear_dense(polymodel_dense_from_poly(su.poly_spec()), -a, a @ y))
        ctx = rm.ctx
        lo, diff = input_map(ctx, su)
        st = _LgoStages(ctx, n, base_log_weights(log_weights, x, n, keep_neginf=True))
        zbuf = ctx.empty((n_chain, n_draw, width))
        acc = ctx.empty((n, width))
        for g0 in range(0, len(gs), width):
            ng = min(width, len(gs) - g0)
            cb = np.zeros(width)
            cb[:ng] = const[g0:g0 + ng]
            cc = (C.c_double * width)(*cb)
            for k0 in range(int(first[g0]), int(first[g0 + ng]), width):   # the batch's z columns, 16 at a time
                nb = min(width, int(first[g0 + ng]) - k0)
                rm.fun_columns(x, k0, nb, lo, diff, out=zbuf)
                slots = colg[k0:k0 + nb] - g0
                start = 0
                for s in np.unique(slots):
                    if first[g0 + s] >= k0:   # the group's first column is in this call
                        start |= 1 << int(s)
                _lib.check(ctx._lib.bfhip_lgo_accum(ctx.handle, n, _ptr(zbuf), width, nb, (C.c_int * nb)(*[int(s) for s in slots]), cc, start,
                                                    _ptr(acc), width))
            st.run_groups(acc, ng, const[g0:g0 + ng], sizes[g0:g0 + ng])
        return st.group_result(gs, sizes)
