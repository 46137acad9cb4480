#!/usr/bin/env python3
"""``kde.logpdf_loo()`` and ``parameter_shift`` (csrc/bfhip_kde.h through utils/kde.py and utils/shift.py) on correlated normal draws
generated on the device, at (n, d) = (65536, 27) and (16384, 6):

  - ``logpdf_loo`` on the device route: wall clock around a synchronise, ``--windows`` windows of ``--reps`` calls after a warm-up
    call; the median window, the smallest and the largest (the spread), and the kernel pairs per second that the median means;
  - the route a user had before on the same GPU, with the same whitened rows: ``torch.mm`` of a chunk of queries against the data,
    the norms, the diagonal set to -inf and ``torch.logsumexp`` (``--torch-route cdist`` takes ``torch.cdist`` instead of the
    product); the same windows, and the largest difference of the two routes' results;
  - one ``parameter_shift`` with n_pairs = n at the first shape: the whole call, index draws and moments included;
  - the host port of ``logpdf_loo`` on the CPU at ``--host-n`` rows of the same data, once.

There is no threshold: nobody had measured either side.

  python3 tools/kde_rate.py [--windows 5] [--reps 3] [--host-n 8192] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _windows(fn, windows, reps, torch):
    fn()   # warm-up: code objects, the allocator's blocks
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return out, r


def _torch_loo(est, route, torch, chunk_bytes=1 << 30):
    """The leave-self-out log density through torch alone, on the estimate's own whitened rows."""
    z, lw = est._z, est._logw
    n = z.shape[0]
    zh = 0.5 * (z * z).sum(1)
    out = torch.empty(n, dtype=torch.float64, device=z.device)
    step = max(1, chunk_bytes // (8 * n))
    for lo in range(0, n, step):
        q = z[lo:lo + step]
        if route == 'cdist':
            t = lw[None, :] - 0.5 * torch.cdist(q, z)**2
        else:
            t = q @ z.T
            t += (lw - zh)[None, :]
            t -= zh[lo:lo + step, None]
        idx = torch.arange(q.shape[0], device=z.device)
        t[idx, lo + idx] = -float('inf')
        out[lo:lo + step] = torch.logsumexp(t, 1)
    return out - torch.log1p(-est.weights) - est._log_norm


def measure(n, d, a, torch, shift):
    from bayesfast_amd.utils import kde, parameter_shift
    g = torch.Generator(device='cuda').manual_seed(n + d)
    mix = torch.randn((d, d), generator=g, device='cuda', dtype=torch.float64) / d**0.5 + torch.eye(d, device='cuda', dtype=torch.float64)
    x = torch.randn((n, d), generator=g, device='cuda', dtype=torch.float64) @ mix
    est = kde(x, 'silverman')
    t_dev, r_dev = _windows(est.logpdf_loo, a.windows, a.reps, torch)
    med = statistics.median(t_dev)
    print(json.dumps({'route': 'bfhip_kde_logsum', 'call': 'logpdf_loo', 'n': n, 'd': d, 'factor': est.factor, 'median_s': med,
                      'min_s': min(t_dev), 'max_s': max(t_dev), 'windows_s': t_dev, 'reps': a.reps, 'pairs_per_s': n * n / med}),
          flush=True)
    t_ref, r_ref = _windows(lambda: _torch_loo(est, a.torch_route, torch), a.windows, a.reps, torch)
    mref = statistics.median(t_ref)
    print(json.dumps({'route': 'torch ' + a.torch_route + ' + logsumexp', 'call': 'logpdf_loo', 'n': n, 'd': d, 'median_s': mref,
                      'min_s': min(t_ref), 'max_s': max(t_ref), 'windows_s': t_ref, 'reps': a.reps, 'pairs_per_s': n * n / mref,
                      'ratio_to_kernel': mref / med, 'max_abs_difference': float((r_dev - r_ref).abs().max())}), flush=True)
    if shift:
        y = torch.randn((n, d), generator=g, device='cuda', dtype=torch.float64) @ mix * 0.8 + 0.3
        t_ps, r = _windows(lambda: parameter_shift(x, y, n_pairs=n), a.windows, 1, torch)
        print(json.dumps({'route': 'bfhip_kde_logsum', 'call': 'parameter_shift', 'n_pairs': n, 'd': d, 'median_s': statistics.median(t_ps),
                          'min_s': min(t_ps), 'max_s': max(t_ps), 'windows_s': t_ps, 'prob': r.prob, 'gaussian_prob': r.gaussian_prob}),
              flush=True)
    nh = min(a.host_n, n)
    xh = x[:nh].cpu().numpy()
    t0 = time.perf_counter()
    kde(xh, 'silverman').logpdf_loo()
    th = time.perf_counter() - t0
    print(json.dumps({'route': 'host port', 'call': 'kde + logpdf_loo', 'n': nh, 'd': d, 'seconds': th, 'pairs_per_s': nh * nh / th,
                      'cpus': len(os.sched_getaffinity(0))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-n', type=int, default=8192)
    ap.add_argument('--torch-route', choices=('mm', 'cdist'), default='mm')
    ap.add_argument('--small', action='store_true', help='one small shape only: a rehearsal of the script')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('kde_rate: no GPU (there is no CPU measurement of a device route)')
    shapes = ((2048, 5),) if a.small else ((65536, 27), (16384, 6))
    for i, (n, d) in enumerate(shapes):
        measure(n, d, a, torch, shift=i == 0)


if __name__ == '__main__':
    main()
