"""Multivariate Gaussian kernel density estimate with weights: the counterpart of the reference's ``bayesfast.utils.kde``
(utils/kde.py:33-396, itself adapted from scipy's ``gaussian_kde``), with the n x m sum of kernels on the device.

For n data rows x_j (d values each) with weights w_j (sum 1), neff = 1 / sum w^2 and the bandwidth factor f -- Scott's
neff^(-1 / (d + 4)), Silverman's (neff (d + 2) / 4)^(-1 / (d + 4)), a scalar or a callable of the estimate, times ``bw_factor``:

  covariance  f^2 C, C = sum w (x - mean)(x - mean)^T / (1 - sum w^2), the weighted sample covariance (``np.cov``'s aweights);
              inv_cov its inverse
  pdf(x)      sum_j w_j exp(-(x - x_j)^T inv_cov (x - x_j) / 2) / sqrt(det(2 pi covariance))
  logpdf(x)   its logarithm as a true log-sum-exp: finite where ``pdf`` underflows to 0
  cdf(x)      sum_j w_j ndtr((x - x_j) / sqrt(covariance)), d = 1 only
  resample    rows drawn in proportion to the weights plus normal(0, covariance) noise

Query points are (m, d) rows (the reference's code; its docstring says otherwise), a (d,) vector is one point, and in one dimension
an (m,) vector is m points.  Two additions to the reference's interface:

  logpdf_loo()  the leave-self-out log density at the data rows themselves: row i's own kernel is left out and the remaining
                weights are renormalised, log w_j - log(1 - w_i).  A row of weight 1 gives -inf.  This is what an estimate
                EVALUATED AT ITS OWN DRAWS wants: the self term biases the density at a draw upward by w_i / norm, which in
                d >= 6 dominates everything else (``utils/shift.py``)
  log_weights=  the weights as logarithms, normalised by their log-sum-exp; -inf is a zero weight

Rows of zero weight are not part of the sample, whatever they hold.

How it is evaluated, on both routes: the data are centred at their weighted mean and whitened with the Cholesky factor A of
inv_cov = A A^T, z = (x - mean) A, so that the energy of a pair is |zq_i - z_j|^2 / 2 = (|zq_i|^2 + |z_j|^2) / 2 - zq_i . z_j: norms
and ONE (m, d) x (d, n) product.  After the centring the norms are O(d / f^2), and the energy carries an absolute error of about
eps (|zq_i|^2 + max_j |z_j|^2).

A GPU tensor as ``dataset`` takes the device route: mean, covariance, Cholesky factor and whitening through torch (d x d work and
one (n, d) product), the pairwise sum through ``bfhip_kde_logsum`` (csrc/bfhip_kde.h: float64 matrix cores, a running-maximum
log-sum-exp, an order of summation fixed by (n, d), so a query gives the same bits alone and in any batch).  Queries may be
tensors or arrays, results are device tensors.  At most ``BFHIP_MAX_DIM`` dimensions and 2^31 - 1 rows.  NumPy arrays and CPU
tensors take a host port of the same arithmetic, chunked over the queries so that memory stays bounded.

Kernel-weighted means.  The same pairs answer a second question: with p_ij = w_j exp(-|zq_i - z_j|^2 / 2) / sum_j' (the same), the
average sum_j p_ij v_j of any per-row quantity v over the rows near a query (``kde_wmean`` / ``bfhip_kde_wmean`` on the device,
``_wmean_host`` on the host, one pass either way).  Three methods are this sum with a different v:

  grad_logpdf(x)   the score of the estimate, A (sum_j p_ij z_j - zq_i) with v = z
  regress(values)  Nadaraya-Watson kernel regression E[values | x]; with ``loo=True`` the cross-validated prediction at the rows
  mean_shift(x0)   the iteration zq <- sum_j p_ij z_j, which climbs to a mode of the estimate (``utils/modes.py`` builds on it)"""
import numpy as np

__all__ = ['kde', 'kde_logsum', 'kde_wmean']

_HOST_CHUNK_BYTES = 1 << 27    # the host port's (queries x data) block of energies


def _is_cuda(a):
    return bool(getattr(a, 'is_cuda', False))


def _host(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, 'detach') else a)


def flat_draws(x, log_weights=None, params=None):
    """Per-chain draws ``x`` (n_chain, n_t, d), host or device, and their log weights ((n_chain, n_t), flat in that order, or None) as
    the rows (n_chain n_t, d) of the parameters ``params`` (indices; None: all) and the flat weights an estimate is built from."""
    x = x.reshape((-1, x.shape[-1]))
    if params is not None:
        x = x[:, [int(p) for p in params]]
    if log_weights is not None:
        log_weights = log_weights.reshape(-1)
    return x, log_weights


# ---- the pairwise sum: out[i] = log sum_j exp(logw[j] - |zq_i - z_j|^2 / 2) ---------------------------------------------------------
def _logsum_host(z, logw, zq, exclude_self=False):
    n, m = z.shape[0], zq.shape[0]
    with np.errstate(all='ignore'):
        off = logw == -np.inf
        if off.any():
            z = np.where(off[:, None], 0., z)
        c = logw - 0.5 * np.einsum('ij,ij->i', z, z)
        c[off] = -np.inf
        out = np.empty(m)
        step = max(1, _HOST_CHUNK_BYTES // (8 * n))
        for lo in range(0, m, step):
            q = zq[lo:lo + step]
            t = q @ z.T
            t += c[None, :]
            t -= 0.5 * np.einsum('ij,ij->i', q, q)[:, None]
            if exclude_self:
                t[np.arange(q.shape[0]), np.arange(lo, lo + q.shape[0])] = -np.inf
            top = t.max(axis=1)
            top = np.where(np.isfinite(top), top, 0.)
            out[lo:lo + step] = top + np.log(np.exp(t - top[:, None]).sum(axis=1))
    return out


def kde_logsum(z, logw, zq, exclude_self=False):
    """``bfhip_kde_logsum`` on device tensors: ``z`` (n, d) and ``zq`` (m, d) whitened float64 rows whose last stride is 1 (any row
    stride), ``logw`` (n,) contiguous or None; with ``exclude_self`` ``zq`` must be ``z`` itself.  A device tensor (m,)."""
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    for t in (z, zq):
        if t.dtype != torch.float64 or t.ndim != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or not t.is_cuda:
            raise ValueError('z and zq should be float64 device matrices with unit stride along a row.')
    if z.shape[1] != zq.shape[1]:
        raise ValueError('z and zq should have the same number of columns.')
    n, d = z.shape
    m = zq.shape[0]
    ldz = z.stride(0) if n > 1 else max(d, 1)
    ldq = zq.stride(0) if m > 1 else max(d, 1)
    if exclude_self:
        if zq.data_ptr() != z.data_ptr() or m != n:
            raise ValueError('exclude_self needs zq to be z.')
        ldq = ldz
    if logw is not None:
        if logw.dtype != torch.float64 or logw.shape != (n,) or not logw.is_contiguous() or logw.device != z.device:
            raise ValueError('logw should be a contiguous float64 vector of length n on the device of z.')
    with torch.cuda.device(z.device):
        ctx = get_context(z.device.index)
        out = ctx.empty((m,))
        nbytes = ctx._lib.bfhip_kde_work_bytes(n, m, d)
        work = ctx.empty((max(int(nbytes), 256),), dtype=torch.uint8)
        _lib.check(ctx._lib.bfhip_kde_logsum(ctx.handle, d, n, _ptr(z), ldz, _ptr(logw), m, _ptr(zq), ldq, int(bool(exclude_self)),
                                             _ptr(out), _ptr(work), work.numel()))
    return out


# ---- the kernel-weighted means: mean[i] = sum_j p_ij v_j, p_ij = softmax_j(logw[j] - |zq_i - z_j|^2 / 2) ----------------------------------
def _wmean_host(z, logw, zq, v, exclude_self=False):
    """The host port of ``bfhip_kde_wmean``: (logsum (m,), mean (m, k)) for ``v`` (n, k).  Rows of weight -inf are no part of the
    sample whatever ``z`` and ``v`` hold there; a query with no term has logsum -inf and a NaN mean."""
    n, m = z.shape[0], zq.shape[0]
    with np.errstate(all='ignore'):
        off = logw == -np.inf
        if off.any():
            z = np.where(off[:, None], 0., z)
            v = np.where(off[:, None], 0., v)
        c = logw - 0.5 * np.einsum('ij,ij->i', z, z)
        c = np.where(off, -np.inf, np.where(np.isfinite(c), c, np.nan))   # a bad weight or row poisons every output, as kd_rows_kernel has it
        logsum, mean = np.empty(m), np.empty((m, v.shape[1]))
        step = max(1, _HOST_CHUNK_BYTES // (8 * n))
        for lo in range(0, m, step):
            q = zq[lo:lo + step]
            t = q @ z.T
            t += c[None, :]
            t -= 0.5 * np.einsum('ij,ij->i', q, q)[:, None]
            if exclude_self:
                t[np.arange(q.shape[0]), np.arange(lo, lo + q.shape[0])] = -np.inf
            top = t.max(axis=1)
            top = np.where(np.isfinite(top), top, 0.)
            np.exp(t - top[:, None], out=t)
            s = t.sum(axis=1)
            logsum[lo:lo + step] = top + np.log(s)
            num = t @ v
            mean[lo:lo + step] = np.where(np.isfinite(num), num / s[:, None], np.nan)    # a bad value: NaN, whether p inf or 0 inf
    return logsum, mean


def kde_wmean(z, logw, zq, v, exclude_self=False):
    """``bfhip_kde_wmean`` on device tensors: (logsum (m,), mean (m, k)), mean[i] = sum_j p_ij v[j] with p_ij the normalised
    kernel weights of query i.  ``z``, ``logw``, ``zq`` and ``exclude_self`` as in ``kde_logsum``; ``v`` (n, k) is a float64
    device matrix with unit stride along a row, and may be ``z`` itself (nothing more is staged then).  More than
    ``BFHIP_MAX_DIM`` columns are taken in batches."""
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    for t in (z, zq, v):
        if t.dtype != torch.float64 or t.ndim != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or not t.is_cuda:
            raise ValueError('z, zq and v should be float64 device matrices with unit stride along a row.')
    if z.shape[1] != zq.shape[1]:
        raise ValueError('z and zq should have the same number of columns.')
    if v.shape[0] != z.shape[0] or v.shape[1] < 1 or v.device != z.device:
        raise ValueError('v should have one row per row of z, at least one column, and live on the device of z.')
    n, d = z.shape
    m, k = zq.shape[0], v.shape[1]
    ldz = z.stride(0) if n > 1 else max(d, 1)
    ldq = zq.stride(0) if m > 1 else max(d, 1)
    ldv = v.stride(0) if n > 1 else max(k, 1)
    if v.data_ptr() == z.data_ptr() and k == d:
        ldv = ldz
    if exclude_self:
        if zq.data_ptr() != z.data_ptr() or m != n:
            raise ValueError('exclude_self needs zq to be z.')
        ldq = ldz
    if logw is not None:
        if logw.dtype != torch.float64 or logw.shape != (n,) or not logw.is_contiguous() or logw.device != z.device:
            raise ValueError('logw should be a contiguous float64 vector of length n on the device of z.')
    with torch.cuda.device(z.device):
        ctx = get_context(z.device.index)
        logsum, mean = ctx.empty((m,)), ctx.empty((m, k))
        for c0 in range(0, k, _lib.MAX_DIM):
            kc = min(_lib.MAX_DIM, k - c0)
            nbytes = ctx._lib.bfhip_kde_wmean_work_bytes(n, m, d, kc)
            work = ctx.empty((max(int(nbytes), 256),), dtype=torch.uint8)
            _lib.check(ctx._lib.bfhip_kde_wmean(ctx.handle, d, n, _ptr(z), ldz, _ptr(logw), kc, _ptr(v[:, c0:]), ldv, m, _ptr(zq), ldq,
                                                int(bool(exclude_self)), _ptr(logsum), _ptr(mean[:, c0:]), k, _ptr(work), work.numel()))
    return logsum, mean


class kde:
    """Kernel density estimate of ``dataset`` ((n, d), or (n,) in one dimension) with Gaussian kernels; the module's docstring has
    the formulas.  ``bw_method``: 'scott' (also None), 'silverman', a scalar used as the factor, or a callable of the estimate;
    ``bw_factor`` multiplies it.  ``weights`` or ``log_weights``: one per row, normalised here.

    Attributes: ``dataset``, ``n``, ``d``, ``neff``, ``weights``, ``factor``, ``covariance``, ``inv_cov``.  On the device route
    ``dataset``, ``weights``, ``covariance`` and ``inv_cov`` are device tensors; ``neff`` and ``factor`` are floats on both."""

    def __init__(self, dataset, bw_method=None, bw_factor=None, weights=None, log_weights=None):
        self._dev = _is_cuda(dataset)
        if self._dev:
            import torch
            dataset = dataset.detach().to(torch.float64)
        else:
            dataset = np.asarray(_host(dataset), dtype=np.float64)
        if dataset.ndim == 1:
            dataset = dataset[:, None]
        elif dataset.ndim != 2:
            raise ValueError("`dataset` should be a 1-d or 2-d array.")
        if not (dataset.numel() if self._dev else dataset.size) > 1:
            raise ValueError("`dataset` input should have multiple elements.")
        self.dataset = dataset
        self.n, self.d = int(dataset.shape[0]), int(dataset.shape[1])
        if self._dev:
            from .. import _lib
            if self.d > _lib.MAX_DIM:
                raise NotImplementedError('more than %d dimensions on the device route.' % _lib.MAX_DIM)
            if self.n > 2**31 - 1:
                raise NotImplementedError('more than 2^31 - 1 rows.')
        if weights is not None and log_weights is not None:
            raise ValueError('give weights or log_weights, not both.')
        self._set_weights(weights, log_weights)
        self.bw_factor = 1. if bw_factor is None else bw_factor
        self.covariance_factor = self.scotts_factor
        self.set_bandwidth(bw_method=bw_method)

    # ---- weights -----------------------------------------------------------------------------------------------------------------------
    def _set_weights(self, weights, log_weights):
        n = self.n
        if self._dev:
            import torch
            dev = self.dataset.device
            if weights is None and log_weights is None:
                self._logw = torch.full((n,), -np.log(n), dtype=torch.float64, device=dev)
                self._weights = torch.full((n,), 1. / n, dtype=torch.float64, device=dev)
                self._neff = float(n)
                return
            given = torch.atleast_1d(torch.as_tensor(weights if weights is not None else log_weights, device=dev).detach().to(torch.float64))
            self._check_weights(given.ndim, given.shape[0])
            if weights is not None:
                w = given / given.sum()
                lw = torch.log(w)
            else:
                lw = given - torch.logsumexp(given, 0)
                w = torch.exp(lw)
            self._logw, self._weights = lw.contiguous(), w
            self._neff = float(1. / (w * w).sum())
            return
        if weights is None and log_weights is None:
            self._logw = np.full(n, -np.log(n))
            self._weights = np.full(n, 1. / n)
            self._neff = float(n)
            return
        given = np.atleast_1d(np.asarray(_host(weights if weights is not None else log_weights), dtype=np.float64))
        self._check_weights(given.ndim, given.shape[0])
        with np.errstate(all='ignore'):
            if weights is not None:
                w = given / np.sum(given)
                lw = np.log(w)
            else:
                top = given.max()
                lw = given - (top + np.log(np.exp(given - top).sum()))
                w = np.exp(lw)
        self._logw, self._weights = lw, w
        self._neff = float(1. / np.sum(w**2))

    def _check_weights(self, ndim, length):
        if ndim != 1:
            raise ValueError("`weights` input should be one-dimensional.")
        if length != self.n:
            raise ValueError("`weights` input should be of length n")

    @property
    def weights(self):
        return self._weights

    @property
    def neff(self):
        return self._neff

    # ---- bandwidth -------------------------------------------------------------------------------------------------------------------
    def scotts_factor(self):
        """neff^(-1 / (d + 4))"""
        return np.power(self.neff, -1. / (self.d + 4))

    def silverman_factor(self):
        """(neff (d + 2) / 4)^(-1 / (d + 4))"""
        return np.power(self.neff * (self.d + 2.) / 4., -1. / (self.d + 4.))

    def set_bandwidth(self, bw_method=None):
        """'scott', 'silverman', a scalar (used as ``factor`` before ``bw_factor``) or a callable of this estimate; None keeps the
        current rule.  Later evaluations use the new bandwidth."""
        if bw_method is None:
            pass
        elif isinstance(bw_method, str) and bw_method == 'scott':
            self.covariance_factor = self.scotts_factor
        elif isinstance(bw_method, str) and bw_method == 'silverman':
            self.covariance_factor = self.silverman_factor
        elif np.isscalar(bw_method) and not isinstance(bw_method, str):
            self._bw_method = 'use constant'
            self.covariance_factor = lambda: bw_method
        elif callable(bw_method):
            self._bw_method = bw_method
            self.covariance_factor = lambda: self._bw_method(self)
        else:
            raise ValueError("`bw_method` should be 'scott', 'silverman', a scalar or a callable.")
        self._compute_covariance()

    def _compute_covariance(self):
        self.factor = float(self.covariance_factor() * self.bw_factor)
        f2 = self.factor**2
        if not hasattr(self, '_data_covariance'):
            x, w = self.dataset, self._weights
            if self._dev:
                import torch
                on = (w > 0)[:, None]
                xs = torch.where(on, x, torch.zeros_like(x))
                self._mean = (w[:, None] * xs).sum(0)
                r = torch.where(on, x - self._mean, torch.zeros_like(x))
                self._data_covariance = (r.T @ (w[:, None] * r)) / (1. - (w * w).sum())
                self._data_inv_cov = torch.linalg.inv(self._data_covariance)
            else:
                with np.errstate(all='ignore'):
                    on = (w > 0)[:, None]
                    xs = np.where(on, x, 0.)
                    self._mean = (w[:, None] * xs).sum(0)
                    r = np.where(on, x - self._mean, 0.)
                    self._data_covariance = (r.T @ (w[:, None] * r)) / (1. - np.sum(w**2))
                    self._data_inv_cov = np.linalg.inv(self._data_covariance)
        self.covariance = self._data_covariance * f2
        self.inv_cov = self._data_inv_cov / f2
        if self._dev:
            import torch
            ic = 0.5 * (self.inv_cov + self.inv_cov.T)
            self._white = torch.linalg.cholesky(ic)
            self._log_norm = 0.5 * (self.d * np.log(2. * np.pi) + float(torch.linalg.slogdet(self.covariance)[1]))
            z = (self.dataset - self._mean) @ self._white
            self._z = torch.where((self._weights > 0)[:, None], z, torch.zeros_like(z)).contiguous()
        else:
            self._white = np.linalg.cholesky(0.5 * (self.inv_cov + self.inv_cov.T))
            self._log_norm = 0.5 * (self.d * np.log(2. * np.pi) + np.linalg.slogdet(self.covariance)[1])
            with np.errstate(all='ignore'):
                z = (self.dataset - self._mean) @ self._white
            self._z = np.where((self._weights > 0)[:, None], z, 0.)

    # ---- evaluation ------------------------------------------------------------------------------------------------------------------
    def _points(self, x):
        """The queries as an (m, d) float64 matrix of this estimate's route."""
        if self._dev:
            import torch
            x = torch.as_tensor(x.detach() if hasattr(x, 'detach') else np.asarray(x, dtype=np.float64), device=self.dataset.device).to(torch.float64)
        else:
            x = np.asarray(_host(x), dtype=np.float64)
        if x.ndim == 0:
            x = x.reshape(1)
        points = x[:, None] if x.ndim == 1 else x
        if points.ndim != 2:
            raise ValueError("points have dimension %s, dataset has dimension %s" % (tuple(points.shape[1:]), self.d))
        m, d = points.shape
        if d != self.d:
            if d == 1 and m == self.d:
                points = points.reshape((1, self.d))     # a (d,) vector: one point
            else:
                raise ValueError("points have dimension %s, dataset has dimension %s" % (d, self.d))
        return points

    def _whiten(self, points):
        return (points - self._mean) @ self._white

    def logpdf(self, x):
        """The log density at the points ``x``: (m,)."""
        zq = self._whiten(self._points(x))
        if self._dev:
            return kde_logsum(self._z, self._logw, zq.contiguous()) - self._log_norm
        return _logsum_host(self._z, self._logw, zq) - self._log_norm

    def pdf(self, x):
        """The density at the points ``x``: (m,)."""
        lp = self.logpdf(x)
        return lp.exp() if self._dev else np.exp(lp)

    __call__ = pdf

    def logpdf_loo(self):
        """The leave-self-out log density at the data rows: (n,).  Row i's own kernel is left out and the other weights are
        renormalised by 1 - w_i; a row of weight 1 gives -inf."""
        if self._dev:
            import torch
            s = kde_logsum(self._z, self._logw, self._z, exclude_self=True)
            full = self._weights >= 1.
            rest = torch.log1p(-torch.where(full, torch.zeros_like(s), self._weights))
            return torch.where(full, torch.full_like(s, -np.inf), s - rest - self._log_norm)
        s = _logsum_host(self._z, self._logw, self._z, exclude_self=True)
        with np.errstate(all='ignore'):
            return np.where(self._weights >= 1., -np.inf, s - np.log1p(-self._weights) - self._log_norm)

    # ---- kernel-weighted means ----------------------------------------------------------------------------------------------------------
    def _wmean(self, zq, v, exclude_self=False):
        if self._dev:
            return kde_wmean(self._z, self._logw, self._z if exclude_self else zq.contiguous(), v, exclude_self)
        return _wmean_host(self._z, self._logw, zq, v, exclude_self)

    def grad_logpdf(self, x):
        """The score of the estimate, the gradient of ``logpdf`` at the points ``x`` in the original coordinates: (m, d)."""
        zq = self._whiten(self._points(x))
        return (self._wmean(zq, self._z)[1] - zq) @ self._white.T

    def regress(self, values, x=None, loo=False):
        """Kernel regression (Nadaraya-Watson) of one value (n,) or k values (n, k) per row: E[values | x] at the points ``x``, (m,)
        or (m, k); ``x=None`` means at the data rows.  ``loo=True`` needs ``x=None`` and leaves each row's own kernel out, which is
        the cross-validated prediction that picks a bandwidth; a row of weight 1 gives NaN.  Rows of zero weight carry no value,
        whatever ``values`` holds there."""
        if self._dev:
            import torch
            v = torch.as_tensor(values.detach() if hasattr(values, 'detach') else np.asarray(values, dtype=np.float64),
                                device=self.dataset.device).to(torch.float64)
        else:
            v = np.asarray(_host(values), dtype=np.float64)
        flat = v.ndim == 1
        if flat:
            v = v[:, None]
        if v.ndim != 2 or v.shape[0] != self.n or v.shape[1] < 1:
            raise ValueError("`values` should hold one value, or one row of values, per row of the dataset.")
        if loo and x is not None:
            raise ValueError('loo=True predicts at the data rows: x should be None.')
        if self._dev:
            v = v.contiguous()
        zq = self._z if x is None else self._whiten(self._points(x))
        out = self._wmean(zq, v, exclude_self=bool(loo))[1]
        return out[:, 0] if flat else out

    def _mean_shift_white(self, zq, tol, max_iter):
        """Mean shift of whitened points: (zq, logsum at zq, iterations, converged per point).  The largest step is looked at once
        per 8 iterations, so the device route synchronises with the host once per 8 kernel calls."""
        n_iter, max_iter = 0, int(max_iter)
        step = None
        while n_iter < max_iter:
            for _ in range(min(8, max_iter - n_iter)):
                new = self._wmean(zq, self._z)[1]
                d = new - zq
                step = (d * d).sum(1)
                zq = new
                n_iter += 1
            if bool((step < tol * tol).all()):
                break
        if self._dev:
            import torch
            logsum = kde_logsum(self._z, self._logw, zq.contiguous())
            conv = step < tol * tol if step is not None else torch.zeros(zq.shape[0], dtype=torch.bool, device=zq.device)
        else:
            logsum = _logsum_host(self._z, self._logw, zq)
            conv = step < tol * tol if step is not None else np.zeros(zq.shape[0], dtype=bool)
        return zq, logsum, n_iter, conv

    def mean_shift(self, x0, tol=1e-8, max_iter=1000):
        """Climbs from the points ``x0`` to modes of the estimate by the mean-shift iteration x <- sum_j p_j(x) x_j, which is a
        gradient ascent of ``logpdf`` with the estimate's own step.  Returns ``(x, logpdf, n_iter, converged)``: the end points
        (m, d) in the original coordinates, the log density there, the iterations made (all points iterate together) and, per
        point, whether its last step was below ``tol`` in whitened units.  The rate is linear, about 1 / (1 + factor^2) per
        iteration near a Gaussian mode, so a very small bandwidth needs thousands of iterations."""
        zq, logsum, n_iter, conv = self._mean_shift_white(self._whiten(self._points(x0)), float(tol), max_iter)
        if self._dev:
            import torch
            x = torch.linalg.solve_triangular(self._white.T, zq.T, upper=True).T + self._mean
        else:
            x = np.linalg.solve(self._white.T, zq.T).T + self._mean
        return x, logsum - self._log_norm, n_iter, conv

    def cdf(self, x):
        """The cumulative distribution at the points ``x`` of a one-dimensional estimate: (m,)."""
        if self.d != 1:
            raise NotImplementedError("currently only supports cdf for 1-d kde")
        points = self._points(x)[:, 0]
        if self._dev:
            import torch
            from .. import _lib
            from ..device import get_context, _ptr
            on = self._weights > 0
            data = torch.where(on, self.dataset[:, 0], torch.zeros_like(self._weights)).contiguous()
            w = self._weights.contiguous()
            h = self.covariance.reshape(1).sqrt().contiguous()
            out = torch.empty_like(points)
            step = 1 << 20    # the entry point counts its queries in an int
            with torch.cuda.device(data.device):
                ctx = get_context(data.device.index)
                for lo in range(0, points.shape[0], step):
                    p = points[lo:lo + step].contiguous()
                    o = torch.empty_like(p)
                    _lib.check(ctx._lib.bfhip_kde_cdf(ctx.handle, 1, self.n, _ptr(data), _ptr(w), _ptr(h), p.shape[0], _ptr(p), _ptr(o)))
                    out[lo:lo + step] = o
            return out
        from scipy.special import ndtr
        h = float(np.sqrt(self.covariance[0, 0]))
        on = self._weights > 0
        data, w = self.dataset[on, 0], self._weights[on]
        out = np.empty(points.shape[0])
        step = max(1, _HOST_CHUNK_BYTES // (8 * max(1, data.size)))
        for lo in range(0, points.shape[0], step):
            out[lo:lo + step] = ndtr((points[lo:lo + step, None] - data[None, :]) / h) @ w
        return out

    def resample(self, size=None, seed=None):
        """``size`` rows (default int(neff)) drawn from the estimate: (size, d).  ``seed`` makes the draw repeatable (a NumPy
        ``default_rng`` on the host port, a torch generator on the device route; the two give different rows)."""
        if size is None:
            size = int(self.neff)
        size = int(size)
        if self._dev:
            import torch
            dev = self.dataset.device
            gen = torch.Generator(device=dev)
            if seed is None:
                gen.seed()
            else:
                gen.manual_seed(int(seed))
            cw = torch.cumsum(self._weights, 0)
            u = torch.rand(size, dtype=torch.float64, device=dev, generator=gen) * cw[-1]
            idx = torch.searchsorted(cw, u, right=True).clamp_(max=self.n - 1)
            noise = torch.randn(size, self.d, dtype=torch.float64, device=dev, generator=gen)
            chol = torch.linalg.cholesky(0.5 * (self.covariance + self.covariance.T))
            return self.dataset[idx] + noise @ chol.T
        rng = np.random.default_rng(seed)
        idx = rng.choice(self.n, size=size, p=self._weights / self._weights.sum())
        chol = np.linalg.cholesky(0.5 * (self.covariance + self.covariance.T))
        return self.dataset[idx] + rng.standard_normal((size, self.d)) @ chol.T
