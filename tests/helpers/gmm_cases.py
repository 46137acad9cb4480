"""Shared by tests/test_gmm_host.py and tests/test_gpu_gmm.py: data, mixture parameters and the bound of one ``gmm_step``.

The bound, in the form tests/test_gpu_kde.py derives.  An energy |(x - mu) A|^2 / 2 from differences and one product carries about
eps E of absolute error, E the largest energy of the case, so every exp(t_ik) -- and with it every responsibility, and the
log-sum-exp -- has a relative (the logarithm: absolute) error of at most eps 64 (1 + E), and a sum of n terms adds n eps relative to
the sum of the terms' magnitudes:
    |got - ref| <= eps (64 (1 + E) + n) sum |terms|,     eps = 2.2e-16,
with sum |terms| = 1 for logpdf and resp, sum_i |w_i r_ik| for N_k, sum_i |w_i r_ik (x_i - c)_a| for S1_k[a],
sum_i |w_i r_ik (x_i - c)_a (x_i - c)_b| for S2_k[a][b], sum_i |w_i logpdf_i| and sum_i w_i for the last two, all from the reference."""
import numpy as np

EPS = 2.2e-16


def mixture(seed, sep, n=4000, d=3):
    """The project's two-Gaussian test sample (tests/test_kde_wmean_host.py): 30 % of the rows moved by ``sep`` along axis 0."""
    rng = np.random.default_rng(seed)
    lab = rng.uniform(size=n) < 0.3
    x = rng.standard_normal((n, d))
    x[lab, 0] += sep
    return x, lab


def random_spd(rng, d, cond=100.):
    """A random symmetric positive definite matrix with eigenvalues between 1 / sqrt(cond) and sqrt(cond)."""
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    ev = np.exp(rng.uniform(-0.25 * np.log(cond), 0.25 * np.log(cond), size=d)) if d > 1 else np.ones(1)
    s = (q * ev) @ q.T
    return 0.5 * (s + s.T)


def random_params(rng, d, K, spread=3.):
    """(weights, means, covariances, whiten, logc): whiten[k] = L_k^-T, Sigma_k = L_k L_k^T, as ``gmm_step`` takes them."""
    weights = rng.uniform(0.5, 1.5, size=K)
    weights /= weights.sum()
    means = rng.standard_normal((K, d)) * spread / np.sqrt(d)
    covs = np.stack([random_spd(rng, d) for _ in range(K)])
    whiten = np.empty_like(covs)
    logc = np.empty(K)
    for k in range(K):
        L = np.linalg.cholesky(covs[k])
        whiten[k] = np.linalg.inv(L).T
        logc[k] = np.log(weights[k]) - np.log(np.diagonal(L)).sum() - 0.5 * d * np.log(2. * np.pi)
    return weights, means, covs, whiten, logc


def step_case(n, d, K, seed=0, weights=True):
    """Rows drawn around the components' means (so that every component owns some), log weights, the centre and the parameters."""
    rng = np.random.default_rng([seed, n, d, K])
    pi, means, covs, whiten, logc = random_params(rng, d, K)
    comp = rng.integers(K, size=n)
    x = means[comp] + rng.standard_normal((n, d)) * 1.2
    logw = np.log(rng.uniform(size=n)) if weights else None
    if logw is not None:
        logw -= np.log(np.exp(logw).sum())
    w = np.ones(n) if logw is None else np.exp(logw)
    centre = (w[:, None] * x).sum(axis=0) / w.sum()
    return dict(x=x, logw=logw, centre=centre, mean=means, whiten=whiten, logc=logc, pi=pi, covs=covs)


def step_bounds(x, logw, centre, mean, whiten, logc, ref_logpdf, ref_resp):
    """(bound of logpdf and resp (a number), bound of every entry of stats) from the reference's values."""
    n, d = x.shape
    K = mean.shape[0]
    E = max(float((((x - mean[k]) @ whiten[k])**2).sum(axis=1).max()) * 0.5 for k in range(K))
    f = EPS * (64. * (1. + E) + n)
    w = np.ones(n) if logw is None else np.where(logw == -np.inf, 0., np.exp(logw))
    wr = np.abs(w[:, None] * ref_resp)
    xc = np.abs(x - centre)
    st = np.empty(K * (1 + d + d * d) + 2)
    st[:K] = wr.sum(axis=0)
    st[K:K + K * d] = (wr.T @ xc).reshape(-1)
    for k in range(K):
        st[K * (1 + d) + k * d * d:K * (1 + d) + (k + 1) * d * d] = (xc.T @ (wr[:, k, None] * xc)).reshape(-1)
    st[-2] = np.abs(w * ref_logpdf).sum()
    st[-1] = w.sum()
    return f, f * st
