#!/usr/bin/env python3
"""``PolyModel.fit`` against ``PolyModel.fit_loo`` (csrc/bfhip_loo.hip through modules/poly.py) at the two fitted shapes of the
benchmark, on standard-normal fit points:

  - the 64-d quadratic (P = 2145, n = 4290) and the 128-d cubic-cross surrogate (P = 9201, n = 18 402);
  - each call's wall clock around a synchronise, the median of the repeats after a warm-up call (the bound is off: its statistics
    are host work that both calls share);
  - the solve alone through the C ABI, ``bfhip_lstsq`` against ``bfhip_lstsq_loo`` on the same design, between two stream events:
    the difference is the leave-one-out part (one residual pass, the leverage kernel, the residual and sum kernels), credited with
    the n P^2 operations of the forward substitution and set against the FP64 matrix peak of 78.6 TFLOP/s.

There is no threshold.

  python3 tools/fit_loo_rate.py [--reps 5] [--small]     one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_MATRIX = 78.6e12


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _events(fn, reps, ctx, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(ctx.stream)
        fn()
        e1.record(ctx.stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def measure(name, d, configs, reps, torch, np):
    from bayesfast_amd import PolyModel, _lib
    from bayesfast_amd.device import get_context, _ptr
    mod = PolyModel(configs(), input_size=d, output_size=1, bound_options=dict(use_bound=False))
    P = mod.n_param
    n = 2 * P
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, d))
    y = (np.sin(x[:, 0]) + x[:, 1]**2 + 0.1 * rng.standard_normal(n))[:, None]
    mod.fit(x, y)   # warm-up: code objects, the context's scratch
    rep = mod.fit_loo(x, y)
    t_fit = [_wall(lambda: mod.fit(x, y), torch)[0] for _ in range(reps)]
    t_loo = [_wall(lambda: mod.fit_loo(x, y), torch)[0] for _ in range(reps)]
    print(json.dumps({'shape': name, 'd': d, 'P': P, 'n': n, 'fit_s': statistics.median(t_fit), 'fit_all_s': t_fit,
                      'fit_loo_s': statistics.median(t_loo), 'fit_loo_all_s': t_loo, 'sum_h_minus_P': float(rep.leverage[0].sum() - P),
                      'max_h': float(rep.leverage[0].max()), 'q2': float(rep.q2[0]), 'r2': float(rep.r2[0])}), flush=True)
    # the solve alone, on a design of the same shape
    ctx = get_context()
    L = ctx._lib
    A = torch.randn((n, P), dtype=torch.float64, device=ctx.device)
    B = torch.randn((n, 1), dtype=torch.float64, device=ctx.device)
    G, c, work = ctx.empty((P, P)), ctx.empty((P, 1)), ctx.empty((n + P,))
    info = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    h, e, s = ctx.empty((n,)), ctx.empty((n, 1)), ctx.empty((1, _lib.LOO_NSUM))
    n_ws = min(-(-n // _lib.LOO_TILE) * -(-P // 64) * 64 * _lib.LOO_TILE, _lib.LOO_WS_MAX)
    ws = ctx.empty((n_ws,))
    head = (ctx.handle, n, P, 1, _ptr(A), P, _ptr(B), _ptr(G), _ptr(c), 2, _ptr(work), _ptr(info))
    plain = lambda: _lib.check(L.bfhip_lstsq(*head))
    loo = lambda: _lib.check(L.bfhip_lstsq_loo(*head, _ptr(h), _ptr(e), _ptr(s), None, _ptr(ws), n_ws))
    plain()
    loo()
    t_plain, t_full = _events(plain, reps, ctx, torch), _events(loo, reps, ctx, torch)
    dt = statistics.median(t_full) - statistics.median(t_plain)
    print(json.dumps({'shape': name, 'P': P, 'n': n, 'lstsq_s': statistics.median(t_plain), 'lstsq_all_s': t_plain,
                      'lstsq_loo_s': statistics.median(t_full), 'lstsq_loo_all_s': t_full, 'loo_part_s': dt,
                      'loo_TFLOPs': n * float(P)**2 / dt / 1e12, 'share_of_fp64_matrix_peak': n * float(P)**2 / dt / PEAK_FP64_MATRIX,
                      'workspace_bytes': 8 * n_ws, 'sum_h_minus_P': float(h.sum() - P)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='a small shape only: a rehearsal of the script')
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fit_loo_rate: no GPU (there is no CPU measurement of a device route)')
    from bayesfast_amd import PolyConfig
    m16 = np.arange(16)
    quad = lambda: 'quadratic'
    cross = lambda: [PolyConfig('linear'), PolyConfig('quadratic'), PolyConfig('cubic-2', input_mask=m16), PolyConfig('cubic-3', input_mask=m16)]
    if a.small:
        measure('16-d quadratic', 16, quad, a.reps, torch, np)
        return
    measure('64-d quadratic', 64, quad, a.reps, torch, np)
    measure('128-d cubic-cross', 128, cross, a.reps, torch, np)


if __name__ == '__main__':
    main()
