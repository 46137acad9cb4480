#!/usr/bin/env python3
"""``marginals`` (csrc/bfhip_marg.hip through utils/marginals.py) on iid normal draws generated on the device, with the log weights
of the Gaussian pair p = N(0, 1), q = N(0, 0.8^2) on the first dimension; all pairs, 64 bins per axis:

  - 256 chains x 1500 draws x 64 parameters: the device route (wall clock around a synchronise, the median of the repeats after a
    warm-up call) and the host port on the same input: the device-to-host copy of the draws (median) and the port, once;
    ``--host-pairs`` takes fewer pairs, and the line then says that the port's time is extrapolated in the pairs;
  - 4096 x 1500 x 64, the headline's output: the device route alone;
  - per size ``bfhip_marg_hist2d`` alone between device events on the bin indices of that input, the median of the repeats: time,
    LDS atomic adds per second (rows x pairs / time) and index bytes per second, both as the kernel asks for them (every pair group
    reads every index row: rows x ld x groups) and as the matrix is big (rows x ld).  Three more index matrices of the same shape
    say where the time goes: nothing in range (the index traffic and the loop alone: no atomic, nothing to flush), every draw in one
    bin (the most contended atomics, the smallest flush) and bins drawn uniformly (the least contended, the largest flush).

There is no threshold: the comparison (host port, same machine) is informative only.

  python3 tools/marginals_rate.py [--reps 5] [--host-pairs 64] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS2D = 64


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _pairs_per_group(ld, bins):
    """mg2_shape of csrc/bfhip_marg.hip: the pairs whose uint64 histograms fit the CU's LDS next to the row tile."""
    fixed = (16384 // ld) * (ld // 4 + 1) * 4 + 2 * 16 * 4
    return max(1, min(16, (163840 - fixed) // (bins * bins * 8)))


def pair_kernel(x, lw, reps, torch):
    """bfhip_marg_hist2d alone, on the indices of x and on three synthetic index matrices."""
    import numpy as np
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    from bayesfast_amd.utils.marginals import _DevicePasses, _bin_constants, weight_shift
    ps = _DevicePasses(x, lw.reshape(-1), 'log')
    n, d, w = ps.n, ps.d, _lib.DIAG_BATCH
    lib, h = ps.ctx._lib, ps.ctx.handle
    top = ps.weight_top()
    ps.quantise(top[0], weight_shift(n))
    e = ps.extent().cpu().numpy()
    lo, hi = -e[0], e[1]
    inv2 = _bin_constants(lo, hi, BINS2D)[0]
    ld = 16
    while ld < d:
        ld *= 2
    idx = torch.empty((n, ld), dtype=torch.uint8, device=x.device)
    for b, (xb, kb, nb) in enumerate(ps._batches()):
        ps._columns(xb, kb, nb)
        c = [torch.as_tensor(np.ascontiguousarray(v[b * w:b * w + nb]), device=x.device) for v in (lo, hi, inv2)]
        _lib.check(lib.bfhip_marg_index(h, n, _ptr(ps.buf), _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), nb, BINS2D, _ptr(idx), ld, b * w))
    pairs = np.stack(np.triu_indices(d, 1), axis=1).astype(np.int32)
    pairs_d = torch.as_tensor(pairs, device=x.device)
    n_pair = len(pairs)
    hist = torch.zeros((n_pair * BINS2D * BINS2D,), dtype=torch.int64, device=x.device)
    groups = -(-n_pair // _pairs_per_group(ld, BINS2D))
    g = torch.Generator(device='cuda').manual_seed(2)
    variants = [('draws', idx), ('nothing_in_range', torch.full_like(idx, 255)), ('one_bin', torch.full_like(idx, 31)),
                ('uniform_bins', torch.randint(0, BINS2D, idx.shape, generator=g, device=x.device, dtype=torch.uint8))]
    for name, ix in variants:
        times = []
        for r in range(reps + 1):     # (the first is the warm-up)
            hist.zero_()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.bfhip_marg_hist2d(h, n, _ptr(ix), ld, _ptr(pairs_d), n_pair, _ptr(ps.q), BINS2D, _ptr(hist)))
            z.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(z) * 1e-3)
        t = statistics.median(times[1:])
        print(json.dumps({'kernel': 'bfhip_marg_hist2d', 'indices': name, 'rows': n, 'ld': ld, 'pairs': n_pair, 'bins2d': BINS2D,
                          'pair_groups': groups, 's': t, 'all_s': times[1:], 'row_pairs_per_s': n * n_pair / t,
                          'index_bytes_asked_per_s': n * ld * groups / t, 'index_matrix_bytes_per_s': n * ld / t,
                          'nonzero_bins': int((hist != 0).sum())}), flush=True)


def measure(shape, reps, host_pairs, torch):
    import numpy as np
    from bayesfast_amd.utils import marginals
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(shape, generator=g, device='cuda', dtype=torch.float64)
    x[:, :, 0] *= 0.8
    lw = -0.5 * x[:, :, 0]**2 + 0.5 * (x[:, :, 0] / 0.8)**2   # log p - log q up to a constant
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m = marginals(x, log_weights=lw, bins2d=BINS2D)   # warm-up: code objects, the LDS attribute of the kernels
    torch.cuda.synchronize()
    work = torch.cuda.max_memory_allocated() - base
    t_dev = [_wall(lambda: marginals(x, log_weights=lw, bins2d=BINS2D), torch)[0] for _ in range(reps)]
    t_1d = [_wall(lambda: marginals(x, log_weights=lw, pairs=None), torch)[0] for _ in range(reps)]
    print(json.dumps({'device_route': True, 'shape': shape, 'pairs': len(m.pairs), 'bins2d': BINS2D, 'marginals_s': statistics.median(t_dev),
                      'marginals_all_s': t_dev, 'marginals_1d_only_s': statistics.median(t_1d), 'torch_working_bytes': work,
                      'sample_bytes': x.numel() * 8, 'result_bytes': m.mass1d.nbytes + m.mass2d.nbytes}), flush=True)
    pair_kernel(x, lw, reps, torch)
    if host_pairs <= 0:
        return
    copies = []
    for _ in range(max(reps, 3)):
        t, host = _wall(lambda: x.cpu(), torch)
        copies.append(t)
    host, lw_h = host.numpy(), lw.cpu().numpy()
    pairs = np.stack(np.triu_indices(shape[2], 1), axis=1)
    n_host = min(host_pairs, len(pairs))
    t0 = time.perf_counter()
    mh = marginals(host, log_weights=lw_h, bins2d=BINS2D, pairs=None)
    port_1d = time.perf_counter() - t0
    t0 = time.perf_counter()
    mh = marginals(host, log_weights=lw_h, bins2d=BINS2D, pairs=pairs[:n_host])
    port = time.perf_counter() - t0
    per_pair = (port - port_1d) / n_host
    print(json.dumps({'host_port': True, 'shape': shape, 'd2h_copy_s': statistics.median(copies), 'port_1d_only_s': port_1d,
                      'port_pairs': n_host, 'port_s': port, 'marginals_s': statistics.median(copies) + port_1d + per_pair * len(pairs),
                      'extrapolated_in_pairs': n_host < len(pairs), 'same_1d_masses': bool((mh.mass1d == m.mass1d).all()),
                      'cpus': len(os.sched_getaffinity(0))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-pairs', type=int, default=64)
    ap.add_argument('--small', action='store_true', help='a small shape only: a rehearsal of the script')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('marginals_rate: no GPU (there is no CPU measurement of a device route)')
    if a.small:
        return measure((16, 200, 20), a.reps, a.host_pairs, torch)
    measure((256, 1500, 64), a.reps, a.host_pairs, torch)
    measure((4096, 1500, 64), a.reps, 0, torch)


if __name__ == '__main__':
    main()
