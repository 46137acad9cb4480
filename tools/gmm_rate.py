#!/usr/bin/env python3
"""One EM iteration of the Gaussian mixture (csrc/bfhip_gmm.h: ``bfhip_gmm_step`` through utils/gmm.py) and a whole ``gmm()`` call on
draws of a four-component mixture generated on the device, at 4096 chains x 1000 draws x 27 parameters and at 65536 x 27, K = 4 (and
K = 1, 2, 16 for the iteration), all in one run and alternating within every window:

  - ``gmm_step`` with all statistics (the E step, the K weighted Gram matrices, the merge), and with ``logpdf`` alone;
  - the M step on the statistics (torch, d x d work);
  - the route a user had before on the same GPU: per component ``solve_triangular`` of the centred rows, ``logsumexp`` over the
    components, then ``x.T @ (r_k x)`` per component -- and the largest relative difference of its statistics from the kernel's;
  - the same with the triangular solve replaced by one product with the inverse factor, ``(x - mu_k) @ A_k``: the fastest form of
    that route, and the fairer comparison;
  - ``gmm()`` itself, the whole call with its host initialisation, with the iterations it made.

Wall clock around a synchronise; ``--windows`` windows of ``--reps`` calls each after a warm-up call; the median window, the smallest
and the largest.  There is no threshold.

  python3 tools/gmm_rate.py [--windows 5] [--reps 3] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _alternate(fns, windows, reps, torch):
    """Every function once as a warm-up, then ``windows`` rounds in which each is timed over ``reps`` calls in turn."""
    res = {k: fn() for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / reps)
    return times, res


def _draws(n, d, torch):
    """n rows of four Gaussians (shares 0.4, 0.3, 0.2, 0.1) with their own correlations, centres 5 sd apart along two axes."""
    g = torch.Generator(device='cuda').manual_seed(n + d)
    kw = dict(generator=g, device='cuda', dtype=torch.float64)
    x = torch.randn((n, d), **kw)
    comp = torch.multinomial(torch.tensor([0.4, 0.3, 0.2, 0.1], device='cuda', dtype=torch.float64), n, replacement=True, generator=g)
    centres = torch.zeros((4, d), device='cuda', dtype=torch.float64)
    centres[1, 0], centres[2, 1], centres[3, 0], centres[3, 1] = 5., 5., 5., 5.
    for k in range(4):
        mix = torch.randn((d, d), **kw) / (2. * d**0.5) + torch.eye(d, device='cuda', dtype=torch.float64)
        rows = comp == k
        x[rows] = x[rows] @ mix + centres[k]
    return x, centres


def _torch_step(x, w, centre, means, chol, logc, torch, whiten=None):
    """The statistics of one pass through torch alone: the energies by a triangular solve with the Cholesky factors, or, with
    ``whiten``, by one product with the inverse factors A_k (the faster route)."""
    K = means.shape[0]
    t = torch.empty((x.shape[0], K), device=x.device, dtype=torch.float64)
    for k in range(K):
        if whiten is None:
            y = torch.linalg.solve_triangular(chol[k], (x - means[k]).T, upper=False)
            t[:, k] = logc[k] - 0.5 * (y * y).sum(0)
        else:
            y = (x - means[k]) @ whiten[k]
            t[:, k] = logc[k] - 0.5 * (y * y).sum(1)
    lp = torch.logsumexp(t, 1)
    wr = torch.exp(t - lp[:, None])
    if w is not None:
        wr = wr * w[:, None]
    xc = x - centre
    s2 = torch.stack([xc.T @ (wr[:, k, None] * xc) for k in range(K)])
    total = lp.sum() if w is None else (w * lp).sum()
    return torch.cat([wr.sum(0), (wr.T @ xc).reshape(-1), s2.reshape(-1), total.reshape(1),
                      torch.full((1,), float(x.shape[0]), device=x.device, dtype=torch.float64) if w is None else w.sum().reshape(1)])


def measure(shape, d, a, torch):
    import numpy as np
    from bayesfast_amd.utils import gmm, gmm_step
    from bayesfast_amd.utils.gmm import _derive, _m_step
    n = int(np.prod(shape))
    x, centres = _draws(n, d, torch)
    centre = x.mean(0).contiguous()
    eye = torch.eye(d, device='cuda', dtype=torch.float64)
    for K in (a.components if a.components else (4, 1, 2, 16)):
        g = torch.Generator(device='cuda').manual_seed(K)
        means = (centres[torch.arange(K, device='cuda') % 4] + 0.3 * torch.randn((K, d), generator=g, device='cuda', dtype=torch.float64)).contiguous()
        covs = (eye * 1.5).expand(K, d, d).contiguous()
        weights = torch.full((K,), 1. / K, device='cuda', dtype=torch.float64)
        whiten, logc = _derive(weights, covs)
        chol = torch.linalg.cholesky(covs)
        dead = torch.zeros(K, dtype=torch.bool, device='cuda')
        st0 = gmm_step(x, None, centre, means, whiten, logc, True, False, False)[0]
        fns = {
            'gmm_step stats': lambda: gmm_step(x, None, centre, means, whiten, logc, True, False, False)[0],
            'gmm_step logpdf alone': lambda: gmm_step(x, None, centre, means, whiten, logc, False, True, False)[1],
            'M step (torch, d x d)': lambda: _m_step(torch, st0, K, d, centre, eye, 1e-6, float(n), means, covs, dead)[0],
            'torch solve_triangular, logsumexp, x.T @ (r_k x)': lambda: _torch_step(x, None, centre, means, chol, logc, torch),
            'torch (x - mu_k) @ A_k, logsumexp, x.T @ (r_k x)': lambda: _torch_step(x, None, centre, means, chol, logc, torch, whiten),
        }
        times, res = _alternate(fns, a.windows, a.reps, torch)
        ref = res['torch solve_triangular, logsumexp, x.T @ (r_k x)']
        diff = float(((res['gmm_step stats'] - ref).abs() / ref.abs().clamp_min(1e-300)).max())
        base = statistics.median(times['gmm_step stats'])
        for k, t in times.items():
            med = statistics.median(t)
            print(json.dumps({'call': k, 'n': n, 'd': d, 'K': K, 'median_s': med, 'min_s': min(t), 'max_s': max(t), 'windows_s': t,
                              'over_gmm_step': med / base, 'stats_rel_diff_torch': diff}), flush=True)
    xs = x.reshape(tuple(shape) + (d,))
    for kw in (dict(n_components=4), dict(n_components=4, tol=0., max_iter=32)):
        out = None
        ts = []
        for _ in range(1 + a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = gmm(xs, seed=0, **kw)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts = ts[1:]
        print(json.dumps({'call': 'gmm() whole call', 'n': n, 'd': d, 'options': {k: v for k, v in kw.items()}, 'n_iter': out.n_iter,
                          'converged': out.converged, 'weights': [float(v) for v in out.weights.cpu()], 'log_likelihood': out.log_likelihood,
                          'median_s': statistics.median(ts), 'min_s': min(ts), 'max_s': max(ts), 'windows_s': ts,
                          's_per_iteration': statistics.median(ts) / max(out.n_iter, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='65536 x 27 only')
    ap.add_argument('--components', type=int, nargs='*', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('gmm_rate.py needs a GPU.')
    shapes = [((65536,), 27)] if a.small else [((4096, 1000), 27), ((65536,), 27)]
    for shape, d in shapes:
        measure(shape, d, a, torch)


if __name__ == '__main__':
    main()
