#!/usr/bin/env python3
"""The pipeline density's streamed form (bfhip_pld.h: pld_eval_stream_q8) at the shapes it exists for: NUTS leapfrog steps/s of
4096 chains in the fused sampler (bf_sampler_kernel<W, true, false, 11, 0>) and, beside them, the tuned CPU port's rate on the
same specs on the host cores this process may use (tools/benchlib/cpu.py), then a rocprofv3 --kernel-trace --stats summary of a
short device run, kept under profiles/.

  python3 tools/pld_stream_rate.py              all of it; one JSON line per shape, the profile's path last
  python3 tools/pld_stream_rate.py --gpu-only   the device rates only (what runs under the profiler)
  python3 tools/pld_stream_rate.py --no-cpu     without the CPU baselines"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SHAPES = [(457, 64, 64), (120, 128, 64)]   # (m, d, nq): 2,145 and 2,209 monomials


def device_rate(m, d, nq, n_chain=4096, n_warm=40, n_timed=20):
    import torch
    from bayesfast_amd.device import get_context, DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd.workloads import random_pipeline_spec, flops_per_leapfrog_spec
    from bayesfast_amd import _lib
    ctx = get_context(0)
    spec = random_pipeline_spec(m, d, nq, seed=m + d)
    dd = DeviceDensity(spec, ctx)
    rng = np.random.default_rng(1)
    ch = DeviceChains(dd, rng.normal(size=(n_chain, d)) * 0.1, seed=1)
    ch.run(n_warm, 'NUTS', n_warmup=n_warm, max_treedepth=8, check=False)
    lf0 = ch.total_leapfrog
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(ctx.stream)
    _, st = ch.run(n_timed, 'NUTS', n_warmup=n_warm, max_treedepth=8, check=False)
    e1.record(ctx.stream)
    torch.cuda.synchronize()
    ch.raise_on_error()
    t = e0.elapsed_time(e1) * 1e-3
    nl = ch.total_leapfrog - lf0
    fl = flops_per_leapfrog_spec(spec)
    return spec, {'m': m, 'd': d, 'n_quad': nq, 'n_monomials': 1 + d + nq * (nq + 1) // 2, 'chains': n_chain, 'kernel': _lib.last_kernel(),
                  'leapfrog_per_s': nl / t, 'seconds': t, 'leapfrog_steps': nl, 'mean_tree_size': float(st[:, :, 3].float().mean()),
                  'flops_per_leapfrog': fl, 'TFLOPs': nl * fl / t / 1e12}


def main():
    gpu_only = '--gpu-only' in sys.argv
    no_cpu = gpu_only or '--no-cpu' in sys.argv
    for m, d, nq in SHAPES:
        spec, out = device_rate(m, d, nq)
        if not no_cpu:
            from benchlib import cpu
            out['cpu'] = cpu.adapted_rate(spec, d, 20, seed=1, target_seconds=10.)
        print(json.dumps(out), flush=True)
    if gpu_only:
        return
    prof = shutil.which('rocprofv3')
    if not prof:
        print(json.dumps({'profile': None, 'reason': 'rocprofv3 not found'}))
        return
    out_dir = os.path.join(ROOT, 'profiles', 'pld_stream')
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([prof, '--kernel-trace', '--stats', '-d', out_dir, '-o', 'pld_stream', '--output-format', 'csv', '--',
                        sys.executable, os.path.abspath(__file__), '--gpu-only'], cwd=ROOT, capture_output=True, text=True)
    stats = []
    for base, _, files in os.walk(out_dir):
        stats += [os.path.join(base, f) for f in files if f.endswith('kernel_stats.csv')]
    print(json.dumps({'profile': sorted(stats), 'rc': r.returncode}))


if __name__ == '__main__':
    main()
