#!/usr/bin/env python3
"""The device route of the convergence diagnostics (csrc/bfhip_diag.hip through utils/diagnostics.py) at the headline's output
size, 4096 chains x 1000 kept iterations x 64 dimensions of iid normal draws generated on the device:

  - ``summary`` on the device route: wall clock around a synchronise, the median of the repeats after a warm-up call;
  - its phases (column passes, sorts, rank kernel, chain moments, lag blocks), from a run of their own in which the route
    synchronises around every phase (``stats=``), medians again; 'other' is the call minus the phases (host arithmetic on the
    (m, 16)-sized arrays, allocation);
  - the same table through the host port: the device-to-host copy of the whole tensor (median of the repeats) and the port on
    all 64 parameters, once (about a minute and a half; ``--host-dims`` takes fewer, and the line then says that the table's
    time is extrapolated).

  python3 tools/diag_rate.py [--reps 5] [--host-dims 64] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ('columns', 'sort', 'rank', 'moments', 'lags')


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-dims', type=int, default=64)
    ap.add_argument('--small', action='store_true', help='256 x 1000 x 64: a rehearsal of the script, not a measurement')
    a = ap.parse_args()
    import torch
    from bayesfast_amd.utils.diagnostics import summary, _table
    if not torch.cuda.is_available():
        raise SystemExit('diag_rate: no GPU (there is no CPU measurement of a device route)')
    shape = (256, 1000, 64) if a.small else (4096, 1000, 64)
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(shape, generator=g, device='cuda', dtype=torch.float64)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    summary(x)   # warm-up: code objects, rocPRIM's configuration, the context's workspace
    torch.cuda.synchronize()
    work = torch.cuda.max_memory_allocated() - base
    calls = [_wall(lambda: summary(x), torch)[0] for _ in range(a.reps)]
    print(json.dumps({'device_route': True, 'shape': shape, 'summary_s': statistics.median(calls), 'all_s': calls,
                      'torch_working_bytes': work, 'sample_bytes': x.numel() * 8}), flush=True)
    runs = []
    for _ in range(a.reps):
        st = {}
        t, _ = _wall(lambda: _table(x, (0.05, 0.5, 0.95), (0.05, 0.95), stats=st), torch)
        st['other'] = t - sum(st.get(k, 0.) for k in PHASES)
        st['call'] = t
        runs.append(st)
    print(json.dumps({'device_phases_s': {k: statistics.median(r.get(k, 0.) for r in runs) for k in PHASES + ('other', 'call')},
                      'note': 'synchronised around every phase'}), flush=True)
    copies = []
    for _ in range(max(a.reps, 3)):
        t, host = _wall(lambda: x.cpu(), torch)
        copies.append(t)
    host = host.numpy()
    nd = min(a.host_dims, shape[2])
    t0 = time.perf_counter()
    summary(host[:, :, :nd])
    port = time.perf_counter() - t0
    print(json.dumps({'host_port': True, 'd2h_copy_s': statistics.median(copies), 'port_dims': nd, 'port_s': port,
                      'port_s_per_dim': port / nd, 'table_s': statistics.median(copies) + port / nd * shape[2], 'table_extrapolated': nd < shape[2],
                      'cpus': len(os.sched_getaffinity(0))}), flush=True)


if __name__ == '__main__':
    main()
