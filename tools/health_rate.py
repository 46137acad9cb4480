#!/usr/bin/env python3
"""``TraceTuple.health()`` (csrc/bfhip_health.hip and bfhip_acor_moments through utils/health.py) on draws and a statistics table
generated on the device: 4096 chains x 1100 iterations (100 of warm-up, so the reader takes a ``[:, 100:]`` view: 1000 selected rows)
x 64 parameters.

  - ``tt.health()``: wall clock around a synchronise, the median of the repeats after a warm-up call; the same on the statistics
    alone (no draws); and the two kernels alone between device events, with the bytes of the selected rows they read (once: the
    second pass of each comes from cache or not, the figure does not say) per second;
  - the route there was before: ``tt.stat(name)`` for diverging, tree_depth, tree_size and energy -- the first of them copies the
    whole table to the host -- and the same counts and E-BFMI in NumPy (the host cache is dropped before every repeat).

There is no threshold: the comparison (host route, same machine) is informative only.

  python3 tools/health_rate.py [--reps 5] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 100


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _events(fn, reps, torch):
    times = []
    for _ in range(reps + 1):     # (the first is the warm-up)
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(z) * 1e-3)
    return times[1:]


def make_trace(n_chain, n_iter, d, torch):
    """Device tensors in the NUTS layout: iid draws, logp of the unit Gaussian, energies logp + chi^2_d / 2, depths 0 .. 10 with
    2^depth - 1 leaves, one transition in a hundred divergent."""
    from bayesfast_amd import _lib
    from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn((n_chain, n_iter, d), generator=g, device='cuda', dtype=torch.float64)
    st = torch.zeros((n_chain, n_iter, _lib.STAT_STRIDE), device='cuda', dtype=torch.float64)
    col = _lib.NSTATS.index
    st[:, :, col('logp')] = -0.5 * (x * x).sum(dim=2)
    st[:, :, col('energy')] = -st[:, :, col('logp')] + 0.5 * torch.randn((n_chain, n_iter, d), generator=g, device='cuda',
                                                                       dtype=torch.float64).square_().sum(dim=2)
    depth = torch.randint(0, 11, (n_chain, n_iter), generator=g, device='cuda')
    st[:, :, col('tree_depth')] = depth.to(torch.float64)
    st[:, :, col('tree_size')] = (2**depth - 1).clamp_(min=1).to(torch.float64)
    st[:, :, col('mean_tree_accept')] = torch.rand((n_chain, n_iter), generator=g, device='cuda', dtype=torch.float64)
    st[:, :, col('step_size')] = 0.3
    st[:, :, col('diverging')] = (torch.rand((n_chain, n_iter), generator=g, device='cuda') < 0.01).to(torch.float64)
    trace = NTrace(n_chain=n_chain, n_iter=n_iter, n_warmup=WARMUP)
    return TraceTuple(trace, x, st, x, st[:, :, col('logp')].contiguous())


def measure(n_chain, n_iter, d, reps, torch):
    import numpy as np
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context, _ptr
    tt = make_trace(n_chain, n_iter, d, torch)
    n = n_iter - WARMUP
    stat_bytes, draw_bytes = n_chain * n * _lib.STAT_STRIDE * 8, n_chain * n * d * 8
    h = tt.health()     # warm-up: code objects
    t_all = [_wall(tt.health, torch)[0] for _ in range(reps)]
    print(json.dumps({'reader': 'TraceTuple.health', 'shape': [n_chain, n, d], 's': statistics.median(t_all), 'all_s': t_all,
                      'selected_bytes': stat_bytes + draw_bytes, 'selected_bytes_per_s': (stat_bytes + draw_bytes) / statistics.median(t_all),
                      'flagged': int(h.flagged.sum()), 'share_divergent': h.share_divergent, 'bfmi_median': h.bfmi_median}), flush=True)
    from bayesfast_amd.utils import sampler_health
    st_v, x_v = tt.device('stats')[:, WARMUP:], tt.device('samples')[:, WARMUP:]
    t_st = [_wall(lambda: sampler_health(st_v), torch)[0] for _ in range(reps)]
    print(json.dumps({'reader': 'sampler_health, statistics alone', 'shape': [n_chain, n, _lib.STAT_STRIDE], 's': statistics.median(t_st),
                      'all_s': t_st, 'selected_bytes': stat_bytes, 'selected_bytes_per_s': stat_bytes / statistics.median(t_st)}), flush=True)
    # the kernels alone
    ctx = get_context(0)
    itab = ctx.empty((n_chain, _lib.HEALTH_I_N), dtype=torch.int64)
    ftab = ctx.empty((n_chain, _lib.HEALTH_F_N))
    t_k = _events(lambda: _lib.check(ctx._lib.bfhip_health_chains(ctx.handle, n_chain, n, int(st_v.stride(0)), _ptr(st_v), 0, 10, _ptr(itab),
                                                                  _ptr(ftab))), reps, torch)
    print(json.dumps({'kernel': 'bfhip_health_chains', 'chains': n_chain, 'rows': n, 's': statistics.median(t_k), 'all_s': t_k,
                      'selected_bytes': stat_bytes, 'selected_bytes_per_s': stat_bytes / statistics.median(t_k)}), flush=True)
    mean, inv = ctx.empty((n_chain, d)), ctx.empty((n_chain, d))
    t_m = _events(lambda: _lib.check(ctx._lib.bfhip_acor_moments(ctx.handle, n_chain, n, d, int(x_v.stride(0)), _ptr(x_v), _ptr(mean),
                                                                 _ptr(inv))), reps, torch)
    print(json.dumps({'kernel': 'bfhip_acor_moments', 'series': n_chain * d, 'rows': n, 's': statistics.median(t_m), 'all_s': t_m,
                      'selected_bytes': draw_bytes, 'selected_bytes_per_s': draw_bytes / statistics.median(t_m)}), flush=True)

    # the route there was before: host copies of the columns, then NumPy
    def before():
        tt._host.clear()
        div, depth = tt.stat('diverging')[:, WARMUP:], tt.stat('tree_depth')[:, WARMUP:]
        size, en = tt.stat('tree_size')[:, WARMUP:], tt.stat('energy')[:, WARMUP:]
        n_div, n_sat, n_leap = (div != 0).sum(axis=1), (depth >= 10).sum(axis=1), size.sum(axis=1)
        bfmi = (np.diff(en, axis=1)**2).sum(axis=1) / ((en - en.mean(axis=1, keepdims=True))**2).sum(axis=1)
        return n_div, n_sat, n_leap, bfmi
    t_b, out = [], None
    for _ in range(max(2, min(reps, 3))):
        t, out = _wall(before, torch)
        t_b.append(t)
    same = bool((out[0] == h.n_divergent).all() and (out[1] == h.n_max_treedepth).all() and (out[2] == h.n_leapfrog).all()
                and np.allclose(out[3], h.bfmi, rtol=1e-10))
    print(json.dumps({'route': 'tt.stat() host copies + NumPy', 'shape': [n_chain, n, _lib.STAT_STRIDE], 's': statistics.median(t_b),
                      'all_s': t_b, 'copied_bytes': n_chain * n_iter * _lib.STAT_STRIDE * 8, 'selected_bytes': stat_bytes,
                      'selected_bytes_per_s': stat_bytes / statistics.median(t_b), 'same_figures': same,
                      'cpus': len(os.sched_getaffinity(0))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='a small shape only: a rehearsal of the script')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('health_rate: no GPU (there is no CPU measurement of a device route)')
    if a.small:
        return measure(32, 300, 8, a.reps, torch)
    measure(4096, 1100, 64, a.reps, torch)


if __name__ == '__main__':
    main()
