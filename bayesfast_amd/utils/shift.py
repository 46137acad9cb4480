"""Do two posteriors agree?  The parameter-difference test of Raveri & Doux 2021 ("Non-Gaussian estimates of tensions in
cosmological parameters", Phys. Rev. D 104, 043504) on two separately sampled chains a and b over shared parameters.

If the chains are independent, the differences delta = x_a - x_b of independently drawn rows are draws of the difference
distribution, and the two posteriors agree to the extent that delta = 0 is a typical point of it:

  prob     = P(p(delta) > p(0)), the mass of the difference distribution above the density contour through zero, with p the kernel
             density estimate (``utils/kde.py``) of the difference sample: the share of difference samples whose log density
             exceeds that at zero
  n_sigma  = sqrt(2) erfinv(prob), the two-sided Gaussian equivalent

``loo=True`` (the default) evaluates the density AT the difference samples leave-self-out (``kde.logpdf_loo``).  With the self
term, as tensiometer's form has it, every sample's own kernel adds w / norm to its density and nothing to that at zero; that bias
grows with dimension: measured on two Gaussians with 4000 difference samples and Silverman's factor, d = 6 with the means 2 sigma
apart gave 0.25 +- 0.05 where the exact value is 0.153 (leave-self-out: 0.157 +- 0.032), and d = 6 at 3.5 sigma and d = 10 at
3 sigma gave exactly 1 where the exact values are 0.778 and 0.188.  Use ``loo=False`` only to reproduce tensiometer's figure.

Limits:
  * the estimate degrades with dimension (the bandwidth of a d-dimensional KDE shrinks as n^(-1 / (d + 4))): report on a few shared
    parameters through ``params``, and look at the Gaussian cross-check next to it;
  * its noise is that of the SINGLE value p(0), which falls only with ``n_pairs``: this is what the device route is for;
  * the two chains are assumed independent of each other (two data sets, not two runs on the same data);
  * one process; at most ``BFHIP_MAX_DIM`` parameters on the device route.

Device tensors take the device route (pairs gathered and subtracted on the device, the n_pairs^2 kernel sum through
``bfhip_kde_logsum``); arrays and CPU tensors the host port.  The index pairs come from a seeded ``np.random.default_rng`` on both
routes, so the two evaluate the same difference sample."""
import numpy as np

from .kde import kde, _is_cuda, _host

__all__ = ['parameter_shift', 'ParameterShift']


class ParameterShift:
    """``prob`` and ``prob_err``, ``n_sigma`` and ``saturated``, ``logpdf_zero``, ``logpdf`` (the n_pairs log densities at the
    difference samples: a device tensor on the device route), ``n_pairs``, ``factor`` (the bandwidth factor), ``d``, and the
    Gaussian cross-check from the two chains' moments alone: ``mean_shift`` (d,), ``cov_shift`` (d, d), ``gaussian_chi2``,
    ``gaussian_prob``, ``gaussian_n_sigma``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return ('ParameterShift(d=%d, n_pairs=%d, prob=%.4g +- %.2g, n_sigma=%.3g%s, gaussian_prob=%.4g, gaussian_n_sigma=%.3g)'
                % (self.d, self.n_pairs, self.prob, self.prob_err, self.n_sigma, ' (saturated)' if self.saturated else '',
                   self.gaussian_prob, self.gaussian_n_sigma))


def _n_sigma(prob):
    from scipy.special import erfinv
    return float(np.sqrt(2.) * erfinv(prob))


def _prepare(x, log_weights, params, name):
    """(rows (n, d) on their route, normalised weights (n,) as a host array or None)."""
    dev = _is_cuda(x)
    if not dev:
        x = np.asarray(_host(x), dtype=np.float64)
    else:
        import torch
        x = x.detach().to(torch.float64)
    if x.ndim == 1:
        x = x[:, None]
    x = x.reshape((-1, x.shape[-1]))
    if params is not None:
        idx = [int(p) for p in params]
        if not idx or min(idx) < 0 or max(idx) >= x.shape[1]:
            raise ValueError('params should be indices of the parameters of %s.' % name)
        x = x[:, idx]
    w = None
    if log_weights is not None:
        lw = np.asarray(_host(log_weights), dtype=np.float64).reshape(-1)
        if lw.size != x.shape[0]:
            raise ValueError('log_weights_%s should hold one value per row of x_%s.' % (name, name))
        with np.errstate(all='ignore'):
            w = np.exp(lw - lw.max())
        if not np.all(np.isfinite(w)) or not w.sum() > 0:
            raise ValueError('log_weights_%s should be finite or -inf, with at least one entry above -inf.' % name)
        w = w / w.sum()
    return x, w


def _moments(x, w):
    """Weighted mean and covariance (ddof as ``np.cov``'s aweights) as host arrays."""
    if _is_cuda(x):
        import torch
        wt = torch.full((x.shape[0],), 1. / x.shape[0], dtype=torch.float64, device=x.device) if w is None else torch.as_tensor(w, device=x.device)
        xs = torch.where((wt > 0)[:, None], x, torch.zeros_like(x))
        mean = (wt[:, None] * xs).sum(0)
        r = torch.where((wt > 0)[:, None], x - mean, torch.zeros_like(x))
        cov = (r.T @ (wt[:, None] * r)) / (1. - (wt * wt).sum())
        return mean.cpu().numpy(), cov.cpu().numpy()
    wt = np.full(x.shape[0], 1. / x.shape[0]) if w is None else w
    with np.errstate(all='ignore'):
        xs = np.where((wt > 0)[:, None], x, 0.)
        mean = (wt[:, None] * xs).sum(0)
        r = np.where((wt > 0)[:, None], x - mean, 0.)
        return mean, (r.T @ (wt[:, None] * r)) / (1. - np.sum(wt**2))


def parameter_shift(x_a, x_b, log_weights_a=None, log_weights_b=None, params=None, n_pairs=65536, bw_method='silverman', bw_factor=None,
                    loo=True, seed=0):
    """The parameter-difference test between the draws ``x_a`` (n_a, d) and ``x_b`` (n_b, d) of two independent chains over the
    same parameters (any leading shape is flattened): a ``ParameterShift``.

    ``n_pairs`` index pairs are drawn with ``np.random.default_rng(seed)``, uniformly or -- with ``log_weights_a`` /
    ``log_weights_b``, one per row -- in proportion to the normalised weights, independently for a and b, so that the difference
    sample delta = x_a[i] - x_b[j] has equal weights either way.  The kernel density estimate of delta (``bw_method``,
    ``bw_factor`` as ``kde``) is evaluated at every delta -- leave-self-out with ``loo=True``, with the self term with
    ``loo=False`` (tensiometer's form: biased upward in more than a few dimensions, for reproducing its figure only) -- and at
    zero.  ``params`` selects the shared parameters by index.

    ``prob`` is the share of difference samples with a log density above that at zero; ``prob_err`` = sqrt(prob (1 - prob) /
    n_pairs) is the BINOMIAL part of its error only: the noise of the single value p(0), which moves every comparison together,
    is not in it and is the larger part at small ``n_pairs``.  ``n_sigma`` = sqrt(2) erfinv(prob) with prob clipped to
    1 - 1 / (2 n_pairs); ``saturated`` says that the clip happened (then n_sigma is a lower limit).  The Gaussian cross-check uses
    the chains' moments alone: ``mean_shift`` = mean_a - mean_b, ``cov_shift`` = cov_a + cov_b, ``gaussian_chi2`` =
    mean^T cov^-1 mean, ``gaussian_prob`` its chi-square cdf with d degrees of freedom and ``gaussian_n_sigma``.

    The estimate degrades with dimension: report on a few shared parameters.  The chains are assumed independent.  One process;
    at most ``BFHIP_MAX_DIM`` parameters on the device route (device tensors; arrays take the host port)."""
    n_pairs = int(n_pairs)
    if n_pairs < 2:
        raise ValueError('n_pairs should be at least 2.')
    if _is_cuda(x_a) != _is_cuda(x_b):
        if _is_cuda(x_a):
            import torch
            x_b = torch.as_tensor(_host(x_b), device=x_a.device)
        else:
            import torch
            x_a = torch.as_tensor(_host(x_a), device=x_b.device)
    xa, wa = _prepare(x_a, log_weights_a, params, 'a')
    xb, wb = _prepare(x_b, log_weights_b, params, 'b')
    if xa.shape[1] != xb.shape[1]:
        raise ValueError('x_a and x_b should have the same parameters: %d and %d columns.' % (xa.shape[1], xb.shape[1]))
    d = int(xa.shape[1])
    rng = np.random.default_rng(seed)
    ia = rng.choice(xa.shape[0], size=n_pairs, p=wa)
    ib = rng.choice(xb.shape[0], size=n_pairs, p=wb)
    dev = _is_cuda(xa)
    if dev:
        import torch
        if xb.device != xa.device:
            xb = xb.to(xa.device)
        delta = xa[torch.as_tensor(ia, device=xa.device)] - xb[torch.as_tensor(ib, device=xa.device)]
        zero = torch.zeros((1, d), dtype=torch.float64, device=xa.device)
    else:
        delta = xa[ia] - xb[ib]
        zero = np.zeros((1, d))
    est = kde(delta, bw_method=bw_method, bw_factor=bw_factor)
    lp = est.logpdf_loo() if loo else est.logpdf(delta)
    lp0 = est.logpdf(zero)
    if dev:
        prob = float((lp > lp0).sum()) / n_pairs
        lp0 = float(lp0[0])
    else:
        lp0 = float(lp0[0])
        prob = float(np.count_nonzero(lp > lp0)) / n_pairs
    cap = 1. - 1. / (2. * n_pairs)
    saturated = prob > cap

    from scipy.stats import chi2
    ma, ca = _moments(xa, wa)
    mb, cb = _moments(xb, wb)
    mean, cov = ma - mb, ca + cb
    g_chi2 = float(mean @ np.linalg.solve(cov, mean))
    g_prob = float(chi2.cdf(g_chi2, d))
    return ParameterShift(prob=prob, prob_err=float(np.sqrt(prob * (1. - prob) / n_pairs)), n_sigma=_n_sigma(min(prob, cap)),
                          saturated=bool(saturated), logpdf_zero=lp0, logpdf=lp, n_pairs=n_pairs, factor=est.factor, d=d,
                          mean_shift=mean, cov_shift=cov, gaussian_chi2=g_chi2, gaussian_prob=g_prob,
                          gaussian_n_sigma=_n_sigma(min(g_prob, 1. - 2.**-53)))
