"""The modes of a sample: where they are, what share of the mass sits in each, and which seeds climb to which.

R-hat says that chains disagree; it does not say how.  ``modes`` runs the mean-shift iteration of ``utils.kde`` (``kde.mean_shift``:
x <- sum_j p_j(x) x_j with the kernel weights p_j of the estimate, in whitened coordinates; on a GPU tensor every iteration is one
``bfhip_kde_wmean`` call and the points stay on the device) from ``n_seeds`` rows of the sample and merges the end points:

  seeds     rows drawn in proportion to the weights by systematic resampling on the host (one uniform number from
            ``np.random.default_rng(seed)``, then ``n_seeds`` equally spaced points of the cumulative weights), on both routes, so
            that a mode's share of the seeds estimates the mass of its basin
  merging   the converged end points in descending ``logpdf``, ties by seed number: a point joins the first mode within
            ``merge_tol`` (whitened units) of it, otherwise it founds one.  Points that did not converge within ``max_iter`` get the
            label -1 and are counted in ``n_not_converged``, not hidden in a mode
  shares    share = seeds of the mode / converged seeds, ``share_err`` = sqrt(share (1 - share) / converged seeds), the binomial error

What it finds are the modes of THE ESTIMATE at ITS bandwidth, whitened by the covariance of the WHOLE sample, which an elongated
bimodal sample inflates: at Scott's factor two well separated Gaussians come with one or two spurious one-seed modes
(``n_minor``), and a wider kernel (``bw_factor=2``) that removes them merges the two in five dimensions.  Choose a few parameters
through ``params`` and read ``n_minor``.  Plain mean shift converges linearly, at a rate of about 1 / (1 + factor^2) per iteration."""
import numpy as np

from .kde import kde, flat_draws, _host

__all__ = ['modes', 'modes_by_chain', 'Modes']


class Modes:
    """What ``modes`` found.  K modes sorted by share, descending; all arrays are NumPy arrays on both routes.

    x (K, d) the modes in the original coordinates (of the selected ``params``); logpdf (K,) the estimate's log density there;
    share, share_err (K,); label (n_seeds,) the mode of every seed, -1 where the iteration did not converge; seed_index
    (n_seeds,) the seeds' rows of the sample; n_iter the iterations made; n_not_converged; n_modes the modes with share >=
    ``min_share`` and n_minor the others; factor the bandwidth factor of the estimate.  ``modes_by_chain`` adds chain_mode
    (n_chain,), the majority label of a chain's seeds (ties to the lower label, -1 where none converged), and chain_split
    (n_chain,), whether the chain's converged seeds disagree."""

    chain_mode = None
    chain_split = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'Modes(n_modes=%d, n_minor=%d, share=%s, n_iter=%d, n_not_converged=%d)' % (
            self.n_modes, self.n_minor, np.array2string(self.share, precision=3), self.n_iter, self.n_not_converged)


def systematic_rows(weights, n_draws, rng):
    """``n_draws`` row numbers in proportion to ``weights`` (NumPy, not necessarily normalised) by systematic resampling:
    the points (u + i) / n_draws of the cumulative weights, u one uniform number of ``rng``.  Ascending."""
    cw = np.cumsum(np.asarray(weights, dtype=np.float64))
    u = (rng.uniform() + np.arange(int(n_draws))) / int(n_draws) * cw[-1]
    return np.minimum(np.searchsorted(cw, u, side='right'), cw.size - 1)


def merge_points(zq, logpdf, converged, merge_tol):
    """The greedy merge of whitened end points: (labels (m,), founders), labels in the order the modes were founded."""
    label = np.full(zq.shape[0], -1, dtype=np.int64)
    found = []
    with np.errstate(all='ignore'):
        idx = np.flatnonzero(converged & np.isfinite(logpdf))
        for i in idx[np.lexsort((idx, -logpdf[idx]))]:
            if found:
                dist = np.sqrt(((zq[found] - zq[i])**2).sum(axis=1))
                near = np.flatnonzero(dist <= merge_tol)
                if near.size:
                    label[i] = near[0]
                    continue
            label[i] = len(found)
            found.append(i)
    return label, np.asarray(found, dtype=np.int64)


def modes_from_seeds(est, seed_index, tol=1e-8, max_iter=1000, merge_tol=1e-3, min_share=0.02):
    """``Modes`` of the estimate ``est`` from the rows ``seed_index`` (host integers) of its own dataset."""
    seed_index = np.asarray(seed_index, dtype=np.int64)
    if est._dev:
        import torch
        z0 = est._z[torch.as_tensor(seed_index, device=est._z.device)]
    else:
        z0 = est._z[seed_index]
    zq, logsum, n_iter, conv = est._mean_shift_white(z0, float(tol), max_iter)
    if est._dev:
        import torch
        x = torch.linalg.solve_triangular(est._white.T, zq.T, upper=True).T + est._mean
    else:
        x = np.linalg.solve(est._white.T, zq.T).T + est._mean
    zq, x, conv = _host(zq), _host(x), _host(conv).astype(bool)
    logpdf = _host(logsum) - est._log_norm
    label, found = merge_points(zq, logpdf, conv, float(merge_tol))
    n_conv = int(np.count_nonzero(label >= 0))
    count = np.bincount(label[label >= 0], minlength=found.size)
    order = np.argsort(-count, kind='stable')            # by share; ties keep the order of logpdf
    rank = np.empty(found.size, dtype=np.int64)
    rank[order] = np.arange(found.size)
    label = np.where(label >= 0, rank[np.maximum(label, 0)], -1) if found.size else label
    share = count[order] / max(n_conv, 1)
    return Modes(x=x[found[order]], logpdf=logpdf[found[order]], share=share, share_err=np.sqrt(share * (1. - share) / max(n_conv, 1)),
                 label=label, seed_index=seed_index, n_iter=int(n_iter), n_not_converged=int(seed_index.size - n_conv),
                 n_modes=int(np.count_nonzero(share >= min_share)), n_minor=int(np.count_nonzero(share < min_share)),
                 factor=est.factor)


def modes(x, log_weights=None, params=None, n_seeds=1024, bw_method=None, bw_factor=None, tol=1e-8, max_iter=1000, merge_tol=1e-3,
          min_share=0.02, seed=0):
    """The modes of the kernel density estimate of the sample ``x`` (n, d) (a GPU tensor takes the device route) with log weights
    ``log_weights``, over the parameters ``params`` (indices; None: all): a ``Modes``.  ``bw_method`` and ``bw_factor`` as in
    ``utils.kde``; ``tol`` and ``merge_tol`` are in whitened units; the module's docstring has the method and its limits."""
    if params is not None:
        x = x[:, [int(p) for p in params]]
    est = kde(x, bw_method=bw_method, bw_factor=bw_factor, log_weights=log_weights)
    rows = systematic_rows(_host(est.weights), n_seeds, np.random.default_rng(seed))
    return modes_from_seeds(est, rows, tol, max_iter, merge_tol, min_share)


def modes_by_chain(x, log_weights=None, per_chain=4, params=None, seed=0, bw_method=None, bw_factor=None, **kw):
    """``modes`` of the per-chain draws ``x`` (n_chain, n_t, d), host or device, seeded from every chain, and which chains sit in
    which mode: ``per_chain`` evenly spaced draws of every chain or, with ``log_weights`` ((n_chain, n_t) or flat in that order),
    ``per_chain`` rows resampled within the chain in proportion to the weights (a chain without weight seeds from its first draw).
    ``kw`` are ``tol``, ``max_iter``, ``merge_tol`` and ``min_share``.  The ``Modes`` also has ``chain_mode`` and ``chain_split``."""
    n_chain, n_t, per_chain = int(x.shape[0]), int(x.shape[1]), int(per_chain)
    if per_chain < 1:
        raise ValueError('per_chain should be at least 1.')
    x, log_weights = flat_draws(x, log_weights, params)
    est = kde(x, log_weights=log_weights, bw_method=bw_method, bw_factor=bw_factor)
    if log_weights is None:
        t = ((np.arange(per_chain) + 0.5) * n_t / per_chain).astype(np.int64)
        rows = (np.arange(n_chain)[:, None] * n_t + t[None, :]).reshape(-1)
    else:
        rng = np.random.default_rng(seed)
        w = _host(est.weights).reshape(n_chain, n_t)
        rows = np.concatenate([c * n_t + (systematic_rows(w[c], per_chain, rng) if w[c].sum() > 0. else np.zeros(per_chain, np.int64))
                               for c in range(n_chain)])
    out = modes_from_seeds(est, rows, **kw)
    label = out.label.reshape(n_chain, per_chain)
    out.chain_mode = np.full(n_chain, -1, dtype=np.int64)
    out.chain_split = np.zeros(n_chain, dtype=bool)
    for c in range(n_chain):
        got = label[c][label[c] >= 0]
        if got.size:
            out.chain_mode[c] = int(np.argmax(np.bincount(got)))     # the first of equal counts: the lower label
            out.chain_split[c] = bool(np.any(got != got[0]))
    return out
