#!/usr/bin/env python3
"""The kernel-weighted means (csrc/bfhip_kde.h: ``bfhip_kde_wmean`` through utils/kde.py) on correlated normal draws generated on the
device, at (n, d) = (65536, 27) and (16384, 6), n queries against n rows, all in one run and alternating within every window:

  - ``kde_wmean`` with v = z and ``exclude_self`` (the leave-self-out mean-shift step of every row);
  - the same with a separate v of one column and of d columns (what staging V costs, and what the second product costs);
  - ``logpdf_loo()`` at the same shape (``bfhip_kde_logsum``: the first product and the exponential alone);
  - the route a user had before on the same GPU: chunked ``torch.softmax(q z^T + c, 1) @ z`` with the diagonal at -inf, and the
    largest difference of its means from the kernel's;
  - one ``utils.modes`` call on the first shape's rows (1024 seeds), the whole call.

Wall clock around a synchronise; ``--windows`` windows of ``--reps`` calls each after a warm-up call; the median window, the smallest
and the largest.  There is no threshold.

  python3 tools/kde_wmean_rate.py [--windows 5] [--reps 3] [--small]     one JSON line per measurement"""
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


def _torch_wmean_loo(z, lw, torch, chunk_bytes=1 << 30):
    n = z.shape[0]
    zh = 0.5 * (z * z).sum(1)
    out = torch.empty_like(z)
    step = max(1, chunk_bytes // (8 * n))
    for lo in range(0, n, step):
        q = z[lo:lo + step]
        t = q @ z.T
        t += (lw - zh)[None, :]
        idx = torch.arange(q.shape[0], device=z.device)
        t[idx, lo + idx] = -float('inf')
        out[lo:lo + step] = torch.softmax(t, 1) @ z
    return out


def measure(n, d, a, torch, with_modes):
    from bayesfast_amd.utils import kde, modes
    from bayesfast_amd.utils.kde import kde_wmean
    g = torch.Generator(device='cuda').manual_seed(n + d)
    mix = torch.randn((d, d), generator=g, device='cuda', dtype=torch.float64) / d**0.5 + torch.eye(d, device='cuda', dtype=torch.float64)
    x = torch.randn((n, d), generator=g, device='cuda', dtype=torch.float64) @ mix
    est = kde(x, 'silverman')
    z, lw = est._z, est._logw
    v1 = torch.randn((n, 1), generator=g, device='cuda', dtype=torch.float64)
    vd = z.clone()
    fns = {
        'kde_wmean v = z exclude_self': lambda: kde_wmean(z, lw, z, z, True)[1],
        'kde_wmean v = z': lambda: kde_wmean(z, lw, vd, z, False)[1],
        'kde_wmean v separate, k = 1': lambda: kde_wmean(z, lw, z, v1, True)[1],
        'kde_wmean v separate, k = d': lambda: kde_wmean(z, lw, z, vd, True)[1],
        'logpdf_loo': est.logpdf_loo,
        'torch softmax(q z^T + c) @ z': lambda: _torch_wmean_loo(z, lw, torch),
    }
    times, res = _alternate(fns, a.windows, a.reps, torch)
    base = statistics.median(times['logpdf_loo'])
    diff = float((res['kde_wmean v = z exclude_self'] - res['torch softmax(q z^T + c) @ z']).abs().max())
    for k, t in times.items():
        med = statistics.median(t)
        print(json.dumps({'call': k, 'n': n, 'd': d, 'factor': est.factor, 'median_s': med, 'min_s': min(t), 'max_s': max(t), 'windows_s': t,
                          'reps': a.reps, 'pairs_per_s': n * n / med, 'ratio_to_logpdf_loo': med / base,
                          'max_abs_difference_kernel_torch': diff}), flush=True)
    if with_modes:
        modes(x, bw_factor=2., max_iter=16)      # warm-up
        t = []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mo = modes(x, bw_factor=2.)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        print(json.dumps({'call': 'modes, 1024 seeds, bw_factor 2', 'n': n, 'd': d, 'median_s': statistics.median(t), 'min_s': min(t),
                          'max_s': max(t), 'windows_s': t, 'n_iter': mo.n_iter, 'n_modes': mo.n_modes, 'n_minor': mo.n_minor,
                          'n_not_converged': mo.n_not_converged}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='one small shape only: a rehearsal of the script')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('kde_wmean_rate: no GPU (there is no CPU measurement of a device route)')
    shapes = ((2048, 5),) if a.small else ((65536, 27), (16384, 6))
    for i, (n, d) in enumerate(shapes):
        measure(n, d, a, torch, with_modes=i == 0)


if __name__ == '__main__':
    main()
