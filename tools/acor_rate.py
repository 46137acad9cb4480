#!/usr/bin/env python3
"""The device integrated autocorrelation time (csrc/bfhip_acor.hip) at the headline's output size, 4096 chains x 1000 kept
iterations x 64 dimensions, on AR(1) series generated on the device: a short window (phi = 0.5, one block of 64 lags) and a long
one (phi = 0.98, tau about 99: several doubling blocks).  Device times with events, per call and per kernel (the moments pass and
one 64-lag block), against the two floors of a 64-lag block (the 2.1 GB read at 6.3 TB/s; its FMAs at the 78.6 TFLOP/s FP64
rate); the host port's time on a slice it can hold; then a rocprofv3 --kernel-trace --stats run of its own, whose kernel
statistics are copied to profiles/acor_rate_kernel_stats.csv.

  python3 tools/acor_rate.py              all of it; one JSON line per measurement, the profile's path last
  python3 tools/acor_rate.py --gpu-only   the device times only (what runs under the profiler)"""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_W, N_T, N_D = 4096, 1000, 64
HBM_BPS, FP64_FLOPS = 6.3e12, 78.6e12


def ar1_device(phi, n_w=N_W, n_t=N_T, n_d=N_D, seed=1):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn((n_w, n_t, n_d), generator=g, device='cuda', dtype=torch.float64)
    s = (1 - phi * phi)**0.5
    for t in range(1, n_t):   # in place: x[t] = phi x[t - 1] + s e[t]
        x[:, t].mul_(s).add_(x[:, t - 1], alpha=phi)
    return x


def _events_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def device_times(phi, reps=5):
    import torch
    from bayesfast_amd.utils.acor import integrated_time_sharded, _DeviceLagSums
    x = ar1_device(phi)
    st = {}
    tau = integrated_time_sharded(x, N_W, quiet=True, stats=st)
    call_ms = _events_ms(lambda: integrated_time_sharded(x, N_W, quiet=True), reps)
    t0 = time.perf_counter()
    for _ in range(reps):
        integrated_time_sharded(x, N_W, quiet=True)
    wall_ms = (time.perf_counter() - t0) / reps * 1e3
    ls = _DeviceLagSums()
    ls(x, 0, 64)
    lag_ms = _events_ms(lambda: ls(x, 0, 64), reps)
    ls2 = _DeviceLagSums()
    mom_ms = _events_ms(lambda: (setattr(ls2, 'moments', None), ls2(x, 0, 1)), reps) - _events_ms(lambda: ls2(x, 0, 1), reps)
    fma = N_W * N_D * sum(N_T - t for t in range(64))
    floors = {'read_ms': x.numel() * 8 / HBM_BPS * 1e3, 'fma_ms': fma * 2 / FP64_FLOPS * 1e3}
    out = {'phi': phi, 'shape': [N_W, N_T, N_D], 'tau_mean': float(np.mean(tau)), 'blocks': st['blocks'], 'lags': st['lags'],
           'call_ms': call_ms, 'call_wall_ms': wall_ms, 'lag_block64_ms': lag_ms, 'moments_ms': mom_ms, 'floors': floors,
           'block64_over_floor': lag_ms / max(floors.values())}
    del x
    torch.cuda.empty_cache()
    return out


def host_time(n_d=4):
    from bayesfast_amd.utils.acor import integrated_time
    rng = np.random.default_rng(2)
    x = rng.normal(size=(N_W, N_T, n_d))
    t0 = time.perf_counter()
    integrated_time(x, quiet=True)
    s = time.perf_counter() - t0
    return {'host_port': True, 'shape': [N_W, N_T, n_d], 'seconds': s, 'seconds_per_dimension': s / n_d}


def main():
    gpu_only = '--gpu-only' in sys.argv
    for phi in (0.5, 0.98):
        print(json.dumps(device_times(phi, reps=2 if gpu_only else 5)), flush=True)
    if gpu_only:
        return
    print(json.dumps(host_time()), flush=True)
    prof = shutil.which('rocprofv3')
    if not prof:
        print(json.dumps({'profile': None, 'reason': 'rocprofv3 not found'}))
        return
    out_dir = os.path.join(ROOT, 'profiles', 'acor_rate')
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([prof, '--kernel-trace', '--stats', '-d', out_dir, '-o', 'acor_rate', '--output-format', 'csv', '--',
                        sys.executable, os.path.abspath(__file__), '--gpu-only'], cwd=ROOT, capture_output=True, text=True)
    stats = []
    for base, _, files in os.walk(out_dir):
        stats += [os.path.join(base, f) for f in files if f.endswith('kernel_stats.csv')]
    if stats:
        shutil.copy(sorted(stats)[0], os.path.join(ROOT, 'profiles', 'acor_rate_kernel_stats.csv'))
    print(json.dumps({'profile': sorted(stats), 'rc': r.returncode}))


if __name__ == '__main__':
    main()
