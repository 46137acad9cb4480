#!/usr/bin/env python3
"""``PolyModel.fit_ridge`` (csrc/bfhip_ridge.hip through modules/ridge.py) on standard-normal fit points, L = 15 penalties (the
default grid), at shapes on both sides of n = P:

  - 27 inputs, quadratic, 457 outputs (P = 406): n = 812 and n = 300;
  - 64 inputs, quadratic (P = 2145): n = 4290 and n = 1500;
  - the 128-input cubic-cross surrogate (P = 9201): n = 18 402 and n = 4000.

Per shape, one JSON line with
  - the whole call, and ``fit_loo`` where it is legal (n >= P): wall clock around a synchronise, the median of the repeats after a
    warm-up call (the bound is off: its statistics are host work);
  - on random operands of the same sizes, between two stream events: the eigen-decomposition (``torch.linalg.eigh`` of the smaller
    side), the rotation (``bfhip_ridge_rotate``, primal side only, and the same product through ``torch.matmul`` beside it),
    ``bfhip_ridge_path`` for the 15 penalties, and the same path through torch with the (r, m L) right operand materialised
    (leverages, fitted values, SSE and PRESS).  The path kernel is credited with 2 n r (m + 1) L operations and set against the
    FP64 matrix peak of 78.6 TFLOP/s.

There is no threshold.

  python3 tools/fit_ridge_rate.py [--reps 3] [--shapes 0,1,2,3,4,5] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_MATRIX = 78.6e12
L_PATH = 15


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _events(fn, reps, ctx, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()   # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record(ctx.stream)
        fn()
        e1.record(ctx.stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(out)


def measure(name, d, m, n, configs, reps, torch, np):
    from bayesfast_amd import PolyModel, _lib
    from bayesfast_amd.device import get_context, _ptr
    from bayesfast_amd.modules.ridge import DEFAULT_RIDGE
    mod = PolyModel(configs(), input_size=d, output_size=m, bound_options=dict(use_bound=False))
    P = mod.n_param
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, d))
    y = np.stack([np.sin(q * x[:, 0]) + x[:, 1]**2 for q in range(m)], axis=1) + 0.1 * rng.standard_normal((n, m))
    out = {'shape': name, 'd': d, 'm': m, 'P': P, 'n': n, 'L': L_PATH, 'side': 'primal' if n >= P - 1 else 'dual'}
    rep = mod.fit_ridge(x, y)   # warm-up: code objects, the solver's workspaces
    t = [_wall(lambda: mod.fit_ridge(x, y), torch) for _ in range(reps)]
    out.update(fit_ridge_s=statistics.median(t), fit_ridge_all_s=t, rho=float(rep.ridge[0]), at_edge=bool(rep.at_edge[0]),
               dof=float(rep.dof[0, rep.ridge_index[0]]), q2_mean=float(np.mean(rep.q2)), r2_mean=float(np.mean(rep.r2)))
    if n >= P:
        loo = mod.fit_loo(x, y)
        t = [_wall(lambda: mod.fit_loo(x, y), torch) for _ in range(reps)]
        out.update(fit_loo_s=statistics.median(t), fit_loo_q2_mean=float(np.mean(loo.q2)))
    # the parts, on random operands of the same sizes
    ctx = get_context()
    lib = ctx._lib
    dual = n < P - 1
    r, side = (n - 1, n) if dual else (P - 1, P - 1)
    M = torch.randn((side, side + 8), dtype=torch.float64, device=ctx.device)
    M = M @ M.T
    out['eigh_s'] = _events(lambda: torch.linalg.eigh(M), max(1, reps // 2), ctx, torch)
    del M
    Z = torch.randn((n, r), dtype=torch.float64, device=ctx.device) / np.sqrt(2. * r)
    if not dual:
        A = torch.randn((n, r), dtype=torch.float64, device=ctx.device)
        V = torch.randn((r, r), dtype=torch.float64, device=ctx.device)
        out['rotate_s'] = _events(lambda: _lib.check(lib.bfhip_ridge_rotate(ctx.handle, n, r, r, _ptr(A), r, _ptr(V), r, _ptr(Z), r)),
                                  reps, ctx, torch)
        out['rotate_TFLOPs'] = 2. * n * r * r / out['rotate_s'] / 1e12
        out['torch_matmul_s'] = _events(lambda: torch.matmul(A, V, out=Z), reps, ctx, torch)   # (the same product through the BLAS)
        Z = torch.randn((n, r), dtype=torch.float64, device=ctx.device) / np.sqrt(2. * r)
        del A, V
    Lam = 1. + torch.rand((r,), dtype=torch.float64, device=ctx.device)   # (every 1 - h stays positive)
    T, Bp = (torch.randn(s, dtype=torch.float64, device=ctx.device) for s in ((r, m), (n, m)))
    lams = ctx.tensor(n * np.array(DEFAULT_RIDGE), torch.float64)
    h, sums = ctx.empty((n, L_PATH)), ctx.empty((L_PATH, m, _lib.LOO_NSUM))
    nw = _lib.ridge_work(n, r, m, L_PATH)
    work = ctx.empty((nw,))
    path = lambda: _lib.check(lib.bfhip_ridge_path(ctx.handle, n, r, m, L_PATH, _ptr(Z), r, _ptr(Lam), _ptr(T), _ptr(lams), _ptr(Bp), _ptr(Bp),
                                                   None, None, 0, 0, _ptr(h), _ptr(sums), None, None, _ptr(work), nw))
    out['path_s'] = _events(path, reps, ctx, torch)
    ops = 2. * n * r * (m + 1) * L_PATH
    out.update(path_TFLOPs=ops / out['path_s'] / 1e12, path_share_of_fp64_matrix_peak=ops / out['path_s'] / PEAK_FP64_MATRIX)

    def through_torch():
        g = 1. / (Lam[:, None] + lams[None, :])                                  # (r, L)
        W = (T[:, :, None] * g[:, None, :]).reshape(r, m * L_PATH)               # the right operand, materialised
        S = Bp[:, :, None] - (Z @ W).view(n, m, L_PATH)
        dd = 1. - (Z * Z) @ g
        return (S * S).sum(0), ((S / dd[:, None, :])**2).sum(0)

    out['torch_path_s'] = _events(through_torch, reps, ctx, torch)
    sse, press = through_torch()
    out['path_vs_torch_press'] = float(((sums[:, :, 1].T - press).abs() / press.abs()).max())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='0,1,2,3,4,5')
    ap.add_argument('--small', action='store_true', help='two small shapes only: a rehearsal of the script')
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fit_ridge_rate: no GPU (there is no CPU measurement of a device route)')
    from bayesfast_amd import PolyConfig
    m16 = np.arange(16)
    quad = lambda: 'quadratic'
    cross = lambda: [PolyConfig('linear'), PolyConfig('quadratic'), PolyConfig('cubic-2', input_mask=m16), PolyConfig('cubic-3', input_mask=m16)]
    if a.small:
        measure('8-d quadratic', 8, 3, 120, quad, a.reps, torch, np)
        measure('8-d quadratic', 8, 3, 30, quad, a.reps, torch, np)
        return
    shapes = [('27-d quadratic', 27, 457, 812, quad), ('27-d quadratic', 27, 457, 300, quad), ('64-d quadratic', 64, 1, 4290, quad),
              ('64-d quadratic', 64, 1, 1500, quad), ('128-d cubic-cross', 128, 1, 18402, cross), ('128-d cubic-cross', 128, 1, 4000, cross)]
    for k in (int(v) for v in a.shapes.split(',')):
        name, d, m, n, cfg = shapes[k]
        measure(name, d, m, n, cfg, a.reps, torch, np)


if __name__ == '__main__':
    main()
