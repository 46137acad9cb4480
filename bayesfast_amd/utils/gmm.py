"""A Gaussian mixture fitted to the draws by expectation-maximisation: how many modes, which draw and which chain belongs to which,
and a closed-form density to evaluate and to draw from, where a kernel density estimate runs out of dimensions.  Nothing like it is
in the reference.

For n rows x_i (d values each) with weights w_i and K components (pi_k, mu_k, Sigma_k), Sigma_k^-1 = A_k A_k^T (A_k the transposed
inverse of the Cholesky factor of Sigma_k) and logc_k = log pi_k + log|det A_k| - d/2 log 2 pi:

  t_ik      logc_k - |(x_i - mu_k) A_k|^2 / 2, the energy formed from the DIFFERENCE (never the expanded quadratic form)
  logpdf_i  log sum_k exp(t_ik), a true log-sum-exp: finite where every exp(t_ik) underflows
  r_ik      exp(t_ik - logpdf_i), the responsibilities (soft labels), sum_k r_ik = 1
  E step    N_k = sum_i w_i r_ik, S1_k = sum_i w_i r_ik (x_i - c), S2_k = sum_i w_i r_ik (x_i - c)(x_i - c)^T about the weighted
            mean c of the sample, and sum_i w_i logpdf_i, sum_i w_i: ONE pass over the draws (``gmm_step``)
  M step    pi_k = N_k / sum N,  mu_k = c + S1_k / N_k,  Sigma_k = S2_k / N_k - (S1_k / N_k)(S1_k / N_k)^T + reg_covar I
  log_likelihood   sum w logpdf / sum w of the LAST E step, i.e. of the parameters before the last M step (scikit-learn's
            ``lower_bound_`` convention); the iteration stops when it changes by less than ``tol``.  The host route looks at it
            after every iteration; the device route reads it only every ``check_every`` iterations (one host synchronisation per
            ``check_every`` kernel calls), so a device fit stops at a multiple of ``check_every`` and may make up to
            ``check_every - 1`` iterations more than the host's
  neff      1 / sum w^2 for normalised weights (n without weights); n_parameters = K - 1 + K d + K d (d + 1) / 2
  bic, aic  -2 neff log_likelihood + n_parameters log neff,  -2 neff log_likelihood + 2 n_parameters

A component whose N_k falls below d + 1 effective rows (N_k neff / sum w) has collapsed: its mean and covariance stop updating
from then on (its weight keeps following N_k), and it is counted in ``n_collapsed``; it is not hidden and not re-seeded.

Initialisation, on the HOST on both routes so that both start from the same numbers: a systematic subsample of at most 4096 rows in
proportion to the weights (``modes.systematic_rows``, ``np.random.default_rng(seed)``), whitened by the subsample's own covariance
(which estimates the whole sample's); there k-means++ seeding, ONE hard assignment, and per cluster the weight, mean and covariance
(a cluster with fewer than 2 d rows takes the subsample's covariance).  ``means_init`` (``Modes.x`` fits), ``weights_init`` and
``covariances_init`` each replace their part; given means replace the seeding.

A GPU tensor takes the device route: every iteration is one ``bfhip_gmm_step`` call (csrc/bfhip_gmm.h: the E step and the K weighted
Gram matrices on the float64 matrix cores, the rows read at whatever row stride they have, sums in an order fixed by (n, d, K), so a fit is bitwise
repeatable), the M step is d x d work in torch; results are device tensors.  NumPy arrays and CPU tensors take ``_step_host``, a
NumPy port of the same arithmetic.

Limits.  EM finds a LOCAL optimum, and k-means++ among many noise dimensions starts badly (at d = 27 with two components 4 sd apart
along one axis about one seed in three ends in a poor optimum): use ``n_init`` or ``means_init``.  The BIC is a convention, and
``neff`` ignores the autocorrelation of the chains, so it overstates the evidence for more components in strongly correlated
chains.  One process.  At most ``BFHIP_MAX_DIM`` parameters, 32 components and 2^31 - 1 rows on the device route.

``logpdf`` and ``resample`` make the fit a proposal for ``evidence.importance`` / ``bridge`` on a multimodal posterior."""
import numpy as np

from .kde import flat_draws, _host, _is_cuda

__all__ = ['gmm', 'GaussianMixture', 'gmm_step']

MAX_K = 32      # BFHIP_GMM_MAX_K
_INIT_ROWS = 4096


# ---- one pass over the draws ---------------------------------------------------------------------------------------------------------
def _step_host(x, logw, centre, mean, whiten, logc, stats=True, logpdf=True, resp=True):
    """The host port of ``bfhip_gmm_step``: (stats, logpdf, resp), None where not asked for.  ``stats`` is N (K), S1 (K, d), S2
    (K, d, d) about ``centre``, then sum w logpdf and sum w, flat; S2 is exactly symmetric.  ``logpdf`` and ``resp`` do not look at
    ``logw``; a non-finite row has NaN there.  In ``stats`` a row of weight -inf is no part of the sample whatever it holds; a NaN
    or +inf weight, or a non-finite row of weight above -inf, makes every entry NaN."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    K = mean.shape[0]
    with np.errstate(all='ignore'):
        t = np.empty((n, K))
        for k in range(K):
            y = (x - mean[k]) @ whiten[k]
            t[:, k] = logc[k] - 0.5 * np.einsum('ij,ij->i', y, y)
        t[~np.isfinite(x).all(axis=1)] = np.nan
        top = t.max(axis=1)
        top = np.where(np.isfinite(top), top, 0.)
        lp = top + np.log(np.exp(t - top[:, None]).sum(axis=1))
        r = np.exp(t - lp[:, None])
        st = None
        if stats:
            lw = np.zeros(n) if logw is None else np.asarray(logw, dtype=np.float64)
            off = lw == -np.inf
            w = np.where(off, 0., np.where(lw < np.inf, np.exp(lw), np.nan))
            wr = np.where(off[:, None], 0., w[:, None] * r)
            xc = np.where(off[:, None], 0., x - centre)
            st = np.empty(K * (1 + d + d * d) + 2)
            st[:K] = wr.sum(axis=0)
            st[K:K + K * d] = (wr.T @ xc).reshape(-1)
            s2 = st[K * (1 + d):K * (1 + d) + K * d * d].reshape(K, d, d)
            for k in range(K):
                full = xc.T @ (wr[:, k, None] * xc)
                s2[k] = np.triu(full) + np.triu(full, 1).T
            st[-2] = np.where(off, 0., w * lp).sum()
            st[-1] = np.where(off, 0., w + 0. * lp).sum()      # a non-finite row that carries weight: NaN
    return st, (lp if logpdf else None), (r if resp else None)


def _step_device(x, logw, centre, mean, whiten, logc, stats=True, logpdf=True, resp=True):
    import torch
    from .. import _lib
    from ..device import get_context, _ptr
    if x.dtype != torch.float64 or x.ndim != 2 or (x.shape[1] > 1 and x.stride(1) != 1) or not x.is_cuda:
        raise ValueError('x should be a float64 device matrix with unit stride along a row.')
    n, d = x.shape
    if n < 1 or d < 1:
        raise ValueError('x should have at least one row and one column.')
    for t in (centre, mean, whiten, logc):
        if t.dtype != torch.float64 or not t.is_contiguous() or t.device != x.device:
            raise ValueError('centre, mean, whiten and logc should be contiguous float64 tensors on the device of x.')
    if mean.ndim != 2 or mean.shape[1] != d or mean.shape[0] < 1:
        raise ValueError('mean should be (k, d).')
    k = mean.shape[0]
    if centre.shape != (d,) or whiten.shape != (k, d, d) or logc.shape != (k,):
        raise ValueError('centre should be (d,), whiten (k, d, d) and logc (k,).')
    if logw is not None:
        if logw.dtype != torch.float64 or logw.shape != (n,) or not logw.is_contiguous() or logw.device != x.device:
            raise ValueError('logw should be a contiguous float64 vector of length n on the device of x.')
    if not (stats or logpdf or resp):
        raise ValueError('ask for stats, logpdf or resp.')
    if d > _lib.MAX_DIM:
        raise NotImplementedError('more than %d dimensions on the device route.' % _lib.MAX_DIM)
    if k > MAX_K:
        raise NotImplementedError('more than %d components on the device route.' % MAX_K)
    if n > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 rows.')
    ldx = x.stride(0) if n > 1 else max(d, 1)
    with torch.cuda.device(x.device):
        ctx = get_context(x.device.index)
        st = ctx.empty((k * (1 + d + d * d) + 2,)) if stats else None
        lp = ctx.empty((n,)) if logpdf else None
        r = ctx.empty((n, k)) if resp else None
        nbytes = ctx._lib.bfhip_gmm_work_bytes(n, d, k)
        work = ctx.empty((max(int(nbytes), 256),), dtype=torch.uint8)
        _lib.check(ctx._lib.bfhip_gmm_step(ctx.handle, d, k, n, _ptr(x), ldx, _ptr(logw), _ptr(centre), _ptr(mean), _ptr(whiten), _ptr(logc),
                                           _ptr(st), _ptr(lp), _ptr(r), k, _ptr(work), work.numel()))
    return st, lp, r


def gmm_step(x, logw, centre, mean, whiten, logc, stats=True, logpdf=True, resp=True):
    """One pass over the rows ``x`` (n, d) for the mixture (``mean`` (K, d), ``whiten`` (K, d, d) with Sigma_k^-1 = A_k A_k^T,
    ``logc`` (K,)): ``(stats, logpdf, resp)`` as the module's docstring defines them, None where not asked for.  ``logw`` (n,) or
    None; ``centre`` (d,).  Device tensors (float64, unit stride along a row, any row stride; the parameters contiguous) go to
    ``bfhip_gmm_step`` and give device tensors; arrays and CPU tensors take the host port."""
    if _is_cuda(x):
        return _step_device(x, logw, centre, mean, whiten, logc, stats, logpdf, resp)
    a = lambda v: None if v is None else np.asarray(_host(v), dtype=np.float64)
    return _step_host(a(x), a(logw), a(centre), a(mean), a(whiten), a(logc), stats, logpdf, resp)


# ---- the parameters the step takes, from (pi, mu, Sigma) ---------------------------------------------------------------------------------
def _derive(weights, covariances):
    """(whiten (K, d, d), logc (K,)) on the route of the arguments: A_k = L_k^-T with Sigma_k = L_k L_k^T."""
    d = covariances.shape[-1]
    if _is_cuda(covariances):
        import torch
        L = torch.linalg.cholesky_ex(covariances)[0]      # no host synchronisation; a failed factor gives NaN downstream
        eye = torch.eye(d, dtype=torch.float64, device=covariances.device).expand(covariances.shape)
        A = torch.linalg.solve_triangular(L, eye, upper=False).swapaxes(-1, -2).contiguous()
        logdet = torch.log(L.diagonal(0, -2, -1)).sum(-1)
        return A, (torch.log(weights) - logdet - 0.5 * d * np.log(2. * np.pi)).contiguous()
    from scipy.linalg import solve_triangular
    A = np.empty_like(covariances)
    logdet = np.empty(covariances.shape[0])
    with np.errstate(all='ignore'):
        for k, cov in enumerate(covariances):
            try:
                L = np.linalg.cholesky(cov)
                A[k] = solve_triangular(L, np.eye(d), lower=True).T
                logdet[k] = np.log(np.diagonal(L)).sum()
            except (np.linalg.LinAlgError, ValueError):
                A[k], logdet[k] = np.nan, np.nan
        return A, np.log(weights) - logdet - 0.5 * d * np.log(2. * np.pi)


def _m_step(xp, st, K, d, centre, eye, reg_covar, neff, means, covariances, dead):
    """The M step on the statistics of one pass: (log_likelihood, weights, means, covariances, dead), in float64 on the route of
    ``st`` (``xp`` is numpy or torch)."""
    N = st[:K]
    S1 = st[K:K + K * d].reshape(K, d)
    S2 = st[K * (1 + d):K * (1 + d) + K * d * d].reshape(K, d, d)
    W = st[-1]
    ll = st[-2] / W
    dead = dead | (N * (neff / W) < d + 1)
    m = S1 / N[:, None]
    weights = N / N.sum()
    means = xp.where(dead[:, None], means, centre + m)
    covariances = xp.where(dead[:, None, None], covariances, S2 / N[:, None, None] - m[:, :, None] * m[:, None, :] + reg_covar * eye)
    return ll, weights, means, covariances, dead


# ---- initialisation (host, both routes) --------------------------------------------------------------------------------------------------
def _initial(sub, K, rng, reg_covar, means_init, weights_init, covariances_init):
    """(weights, means, covariances) from the subsample ``sub`` (m, d): k-means++ in the subsample's whitened coordinates, one hard
    assignment, per-cluster moments."""
    m, d = sub.shape
    mu = sub.mean(axis=0)
    r = sub - mu
    cov = r.T @ r / max(m, 1) + reg_covar * np.eye(d)
    try:
        white = np.linalg.inv(np.linalg.cholesky(cov)).T
    except np.linalg.LinAlgError:
        white = np.eye(d)
    z = r @ white
    if means_init is not None:
        means = np.array(means_init, dtype=np.float64).reshape(K, d)
        cz = (means - mu) @ white
    else:
        first = int(rng.integers(m))
        idx = [first]
        d2 = ((z - z[first])**2).sum(axis=1)
        for _ in range(1, K):
            tot = d2.sum()
            nxt = int(rng.choice(m, p=d2 / tot)) if tot > 0. else int(rng.integers(m))
            idx.append(nxt)
            d2 = np.minimum(d2, ((z - z[nxt])**2).sum(axis=1))
        cz = z[idx]
        means = None
    lab = np.argmin(((z[:, None, :] - cz[None, :, :])**2).sum(axis=2), axis=1)
    weights = np.empty(K)
    mean_c = np.empty((K, d))
    covs = np.empty((K, d, d))
    for k in range(K):
        rows = sub[lab == k]
        weights[k] = max(rows.shape[0], 1) / float(m)
        mean_c[k] = rows.mean(axis=0) if rows.shape[0] else mu
        if rows.shape[0] >= 2 * d and rows.shape[0] >= 2:
            rk = rows - mean_c[k]
            covs[k] = rk.T @ rk / rows.shape[0] + reg_covar * np.eye(d)
        else:
            covs[k] = cov
    weights /= weights.sum()
    if means is None:
        means = mean_c
    if weights_init is not None:
        weights = np.array(weights_init, dtype=np.float64).reshape(K)
        weights = weights / weights.sum()
    if covariances_init is not None:
        covs = np.array(covariances_init, dtype=np.float64).reshape(K, d, d)
    return weights, means, covs


class GaussianMixture:
    """What ``gmm`` fitted.  K components sorted by weight, descending.

    weights (K,), means (K, d), covariances (K, d, d): device tensors on the device route, arrays on the host route;
    log_likelihood, n_iter, converged, n_collapsed, neff, n_parameters, bic, aic: Python numbers; history (n_iter,) the
    log_likelihood of every iteration (NumPy); n, d, n_components.  A selection over several component counts also has
    ``candidates`` (every fit) and ``bic_path`` (rows of n_components, log_likelihood, n_parameters, bic, aic).  From
    ``TraceTuple.gmm``: chain_share (n_chain, K), chain_component (n_chain,), chain_split (n_chain,)."""

    candidates = None
    bic_path = None
    chain_share = None
    chain_component = None
    chain_split = None

    def __init__(self, x, logw, weights, means, covariances, log_likelihood, history, n_iter, converged, n_collapsed, neff):
        self._x, self._logw = x, logw
        self._dev = _is_cuda(x)
        self.n, self.d = int(x.shape[0]), int(x.shape[1])
        if self._dev:
            import torch
            order = torch.argsort(weights, descending=True, stable=True)
        else:
            order = np.argsort(-weights, kind='stable')
        self.weights, self.means, self.covariances = weights[order], means[order], covariances[order]
        K, d = int(weights.shape[0]), self.d
        self.n_components = K
        self.log_likelihood = float(log_likelihood)
        self.history = np.asarray(history, dtype=np.float64)
        self.n_iter, self.converged, self.n_collapsed, self.neff = int(n_iter), bool(converged), int(n_collapsed), float(neff)
        self.n_parameters = K - 1 + K * d + K * d * (d + 1) // 2
        self.bic = -2. * self.neff * self.log_likelihood + self.n_parameters * np.log(self.neff)
        self.aic = -2. * self.neff * self.log_likelihood + 2. * self.n_parameters
        if self._dev:
            self.means, self.covariances = self.means.contiguous(), self.covariances.contiguous()
        self._whiten, self._logc = _derive(self.weights, self.covariances)
        self._centre = self.means[0] if not self._dev else self.means[0].contiguous()

    def __repr__(self):
        w = _host(self.weights)
        return 'GaussianMixture(n_components=%d, weights=%s, log_likelihood=%.6g, bic=%.6g, n_iter=%d, converged=%s, n_collapsed=%d)' % (
            self.n_components, np.array2string(w, precision=3), self.log_likelihood, self.bic, self.n_iter, self.converged, self.n_collapsed)

    def _points(self, x):
        if self._dev:
            import torch
            x = torch.as_tensor(x.detach() if hasattr(x, 'detach') else np.asarray(x, dtype=np.float64), device=self._x.device).to(torch.float64)
        else:
            x = np.asarray(_host(x), dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape((1, -1)) if x.shape[0] == self.d else x[:, None]
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError('points have dimension %s, the mixture has dimension %d' % (tuple(x.shape[1:]), self.d))
        if self._dev and x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        return x

    def _eval(self, x, logpdf, resp):
        x = self._x if x is None else self._points(x)
        return gmm_step(x, None, self._centre, self.means, self._whiten, self._logc, stats=False, logpdf=logpdf, resp=resp)

    def logpdf(self, x):
        """The log density of the mixture at the points ``x`` ((m, d), or (d,) for one point): (m,)."""
        return self._eval(x, True, False)[1]

    def pdf(self, x):
        """The density at the points ``x``: (m,)."""
        lp = self.logpdf(x)
        return lp.exp() if self._dev else np.exp(lp)

    __call__ = pdf

    def responsibilities(self, x=None):
        """r_ik at the points ``x``, or at the data rows with None: (m, K), rows that sum to 1."""
        return self._eval(x, False, True)[2]

    def labels(self, x=None):
        """The component of the largest responsibility, at the points ``x`` or at the data rows: (m,) integers."""
        return self.responsibilities(x).argmax(1)

    def resample(self, size, seed=None):
        """``size`` rows drawn from the mixture: (size, d).  ``seed`` makes the draw repeatable (a NumPy ``default_rng`` on the
        host route, a torch generator on the device route; the two give different rows)."""
        size = int(size)
        if self._dev:
            import torch
            dev = self._x.device
            gen = torch.Generator(device=dev)
            if seed is None:
                gen.seed()
            else:
                gen.manual_seed(int(seed))
            comp = torch.multinomial(self.weights / self.weights.sum(), size, replacement=True, generator=gen)
            noise = torch.randn(size, self.d, dtype=torch.float64, device=dev, generator=gen)
            chol = torch.linalg.cholesky_ex(self.covariances)[0]
            return self.means[comp] + torch.einsum('nab,nb->na', chol[comp], noise)
        rng = np.random.default_rng(seed)
        comp = rng.choice(self.n_components, size=size, p=self.weights / self.weights.sum())
        chol = np.linalg.cholesky(self.covariances)
        return self.means[comp] + np.einsum('nab,nb->na', chol[comp], rng.standard_normal((size, self.d)))

    def component_of_chain(self, shape):
        """For data rows that are the draws of ``shape = (n_chain, n_t)`` chains, flat in that order: ``(chain_share (n_chain, K),
        chain_component (n_chain,), chain_split (n_chain,))`` as NumPy arrays -- the mean responsibility of a chain's draws
        (weighted by the draws' weights, if any), its argmax, and whether the largest share is below 0.9."""
        n_chain, n_t = int(shape[0]), int(shape[1])
        if n_chain * n_t != self.n:
            raise ValueError('shape does not match the %d data rows.' % self.n)
        r = self.responsibilities().reshape((n_chain, n_t, self.n_components))
        if self._logw is not None:
            w = (self._logw.exp() if self._dev else np.exp(self._logw)).reshape((n_chain, n_t, 1))
            zero = w == 0
            if self._dev:
                import torch
                r = torch.where(zero, torch.zeros_like(r), r * w)
            else:
                with np.errstate(all='ignore'):
                    r = np.where(zero, 0., r * w)
            share = r.sum(1) / w.sum(1)
        else:
            share = r.sum(1) / n_t
        share = np.asarray(_host(share), dtype=np.float64)
        comp = share.argmax(axis=1)
        return share, comp, share.max(axis=1) < 0.9


def _fit(x, logw, logw_host, centre, neff, K, seed, tol, max_iter, reg_covar, means_init, weights_init, covariances_init, check_every):
    dev = _is_cuda(x)
    n, d = int(x.shape[0]), int(x.shape[1])
    rng = np.random.default_rng(seed)
    m = min(n, _INIT_ROWS)
    from .modes import systematic_rows
    with np.errstate(all='ignore'):
        wsel = np.ones(n) if logw_host is None else np.exp(logw_host - logw_host.max())
    rows = systematic_rows(wsel, m, rng)
    if dev:
        import torch
        sub = x[torch.as_tensor(rows, device=x.device)].cpu().numpy()
    else:
        sub = x[rows]
    w0, m0, c0 = _initial(np.asarray(sub, dtype=np.float64), K, rng, reg_covar, means_init, weights_init, covariances_init)
    if dev:
        import torch
        xp = torch
        as_route = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=x.device)
        eye = torch.eye(d, dtype=torch.float64, device=x.device)
        dead = torch.zeros(K, dtype=torch.bool, device=x.device)
    else:
        xp = np
        as_route = lambda a: np.array(a, dtype=np.float64)
        eye = np.eye(d)
        dead = np.zeros(K, dtype=bool)
    weights, means, covs = as_route(w0), as_route(m0), as_route(c0)
    history = []
    n_iter, converged, max_iter, check_every = 0, False, int(max_iter), max(1, int(check_every)) if dev else 1
    with np.errstate(all='ignore'):
        while n_iter < max_iter and not converged:
            for _ in range(min(check_every, max_iter - n_iter)):
                whiten, logc = _derive(weights, covs)
                st = gmm_step(x, logw, centre, means if not dev else means.contiguous(), whiten, logc, True, False, False)[0]
                ll, weights, means, covs, dead = _m_step(xp, st, K, d, centre, eye, reg_covar, neff, means, covs, dead)
                history.append(ll)
                n_iter += 1
            last = float(history[-1])
            prev = float(history[-2]) if len(history) > 1 else -np.inf
            if not np.isfinite(last):
                break
            converged = abs(last - prev) < tol
    hist = np.asarray(_host(xp.stack(history)) if dev else history, dtype=np.float64) if history else np.zeros(0)
    return GaussianMixture(x, logw, weights, means, covs, hist[-1] if hist.size else np.nan, hist, n_iter, converged,
                           int(dead.sum()), neff)


def gmm(x, n_components=2, log_weights=None, params=None, n_init=1, seed=0, tol=1e-7, max_iter=200, reg_covar=1e-6, means_init=None,
        weights_init=None, covariances_init=None, check_every=8):
    """Fits a mixture of ``n_components`` Gaussians to the rows ``x`` ((n, d), or per-chain draws (n_chain, n_t, d); host or device)
    by expectation-maximisation: a ``GaussianMixture``.  The module's docstring has the formulas and the limits.

    ``n_components`` may be a sequence: every count is fitted and the fit of lowest BIC is returned, with all fits in
    ``.candidates`` and the table in ``.bic_path``.  ``log_weights``: one per row ((n_chain, n_t) or flat), normalised here, -inf a
    row that is no part of the sample.  ``params`` selects parameters by index.  ``n_init`` > 1 repeats the fit with the seeds
    ``seed``, ``seed + 1``, ... and keeps the highest ``log_likelihood``.  ``means_init`` (K, d), ``weights_init`` (K,) and
    ``covariances_init`` (K, d, d) replace their part of the initialisation (one component count only)."""
    dev = _is_cuda(x)
    if x.ndim not in (2, 3):
        raise ValueError('x should be (n, d) or (n_chain, n_t, d).')
    if dev:
        import torch
        x = x.detach().to(torch.float64)
        if log_weights is not None:
            log_weights = torch.as_tensor(log_weights.detach() if hasattr(log_weights, 'detach') else np.asarray(log_weights, dtype=np.float64),
                                          device=x.device).to(torch.float64)
    else:
        x = np.asarray(_host(x), dtype=np.float64)
        if log_weights is not None:
            log_weights = np.asarray(_host(log_weights), dtype=np.float64)
    x, log_weights = flat_draws(x, log_weights, params)
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 2:
        raise ValueError('x should have at least two rows.')
    if log_weights is not None and tuple(log_weights.shape) != (n,):
        raise ValueError('log_weights should hold one value per row.')
    counts = [int(k) for k in np.atleast_1d(n_components)]
    if not counts or min(counts) < 1:
        raise ValueError('n_components should be at least 1.')
    if len(counts) > 1 and (means_init is not None or weights_init is not None or covariances_init is not None):
        raise ValueError('means_init, weights_init and covariances_init fit one component count.')
    if dev:
        from .. import _lib
        if d > _lib.MAX_DIM:
            raise NotImplementedError('more than %d dimensions on the device route.' % _lib.MAX_DIM)
        if max(counts) > MAX_K:
            raise NotImplementedError('more than %d components on the device route.' % MAX_K)
        if n > 2**31 - 1:
            raise NotImplementedError('more than 2^31 - 1 rows.')
        if x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
    # normalised weights, neff and the centre of the moments
    logw = logw_host = None
    with np.errstate(all='ignore'):
        if log_weights is None:
            neff = float(n)
            centre = x.mean(0)
        elif dev:
            import torch
            logw = (log_weights - torch.logsumexp(log_weights, 0)).contiguous()
            w = logw.exp()
            neff = float(1. / (w * w).sum())
            centre = (w[:, None] * torch.where((w > 0)[:, None], x, torch.zeros_like(x))).sum(0)
            logw_host = log_weights.cpu().numpy()
        else:
            top = log_weights.max()
            logw = log_weights - (top + np.log(np.exp(log_weights - top).sum()))
            w = np.exp(logw)
            neff = float(1. / np.sum(w * w))
            centre = (w[:, None] * np.where((w > 0)[:, None], x, 0.)).sum(axis=0)
            logw_host = log_weights
    if dev:
        centre = centre.contiguous()
    fits = []
    for K in counts:
        best = None
        for j in range(max(1, int(n_init))):
            f = _fit(x, logw, logw_host, centre, neff, K, int(seed) + j, float(tol), max_iter, float(reg_covar), means_init, weights_init,
                     covariances_init, check_every)
            if best is None or (f.log_likelihood > best.log_likelihood) or not np.isfinite(best.log_likelihood):
                best = f
        fits.append(best)
    if len(fits) == 1:
        return fits[0]
    bic = np.array([f.bic if np.isfinite(f.bic) else np.inf for f in fits])
    out = fits[int(np.argmin(bic))]
    out.candidates = fits
    out.bic_path = np.array([[f.n_components, f.log_likelihood, f.n_parameters, f.bic, f.aic] for f in fits], dtype=np.float64)
    return out
