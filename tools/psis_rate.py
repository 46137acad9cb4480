#!/usr/bin/env python3
"""``psis`` and ``weighted_summary`` (csrc/bfhip_psis.hip through utils/psis.py) at the headline's output size, 4096 chains x 1500
kept iterations x 64 dimensions of iid normal draws generated on the device, with the log ratios of the Gaussian pair p = N(0, 1),
q = N(0, 0.8^2) on the first dimension, and at one small shape:

  - each call on the device route: wall clock around a synchronise, the median of the repeats after a warm-up call;
  - the same two calls through the host port: the device-to-host copy of what the port needs (median of the repeats) and the port,
    once; ``--host-dims`` takes fewer parameters, and the line then says that the table's time is extrapolated.

There is no threshold: the comparison (host port, same machine) is informative only.

  python3 tools/psis_rate.py [--reps 5] [--host-dims 64] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(shape, reps, host_dims, torch):
    from bayesfast_amd.utils import psis, weighted_summary
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(shape, generator=g, device='cuda', dtype=torch.float64)
    x[:, :, 0] *= 0.8
    lr = -0.5 * x[:, :, 0]**2 + 0.5 * (x[:, :, 0] / 0.8)**2   # log p - log q up to a constant
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = psis(lr)   # warm-up: code objects, rocPRIM's configuration, the context's workspace
    weighted_summary(x, log_weights=r.log_weights)
    torch.cuda.synchronize()
    work = torch.cuda.max_memory_allocated() - base
    t_psis = [_wall(lambda: psis(lr), torch)[0] for _ in range(reps)]
    t_tab = [_wall(lambda: weighted_summary(x, log_weights=r.log_weights), torch)[0] for _ in range(reps)]
    print(json.dumps({'device_route': True, 'shape': shape, 'psis_s': statistics.median(t_psis), 'psis_all_s': t_psis,
                      'weighted_summary_s': statistics.median(t_tab), 'weighted_summary_all_s': t_tab, 'khat': r.khat, 'ess': r.ess,
                      'torch_working_bytes': work, 'sample_bytes': x.numel() * 8}), flush=True)
    copies_lr = [_wall(lambda: lr.cpu(), torch)[0] for _ in range(max(reps, 3))]
    copies_x = []
    for _ in range(max(reps, 3)):
        t, host = _wall(lambda: x.cpu(), torch)
        copies_x.append(t)
    host, lr_h = host.numpy(), lr.cpu().numpy()
    t0 = time.perf_counter()
    rh = psis(lr_h)
    port_psis = time.perf_counter() - t0
    nd = min(host_dims, shape[2])
    t0 = time.perf_counter()
    weighted_summary(host[:, :, :nd], log_weights=rh.log_weights)
    port_tab = time.perf_counter() - t0
    print(json.dumps({'host_port': True, 'shape': shape, 'psis_d2h_copy_s': statistics.median(copies_lr), 'psis_port_s': port_psis,
                      'psis_s': statistics.median(copies_lr) + port_psis, 'table_d2h_copy_s': statistics.median(copies_x),
                      'table_port_dims': nd, 'table_port_s': port_tab,
                      'weighted_summary_s': statistics.median(copies_x) + port_tab / nd * shape[2], 'table_extrapolated': nd < shape[2],
                      'khat': rh.khat, 'cpus': len(os.sched_getaffinity(0))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-dims', type=int, default=64)
    ap.add_argument('--small', action='store_true', help='the small shape only: a rehearsal of the script')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('psis_rate: no GPU (there is no CPU measurement of a device route)')
    for shape in ((64, 500, 8),) + (() if a.small else ((4096, 1500, 64),)):
        measure(shape, a.reps, a.host_dims, torch)


if __name__ == '__main__':
    main()
