#!/usr/bin/env python3
"""The Laplace approximation of the PIPELINE density (csrc/bfhip_pld_hess.hip) measured on the DES shape
(``workloads.des_like_pipeline``: 27 inputs, 457 outputs, fitted as examples/des_like_pipeline.py fits its round 0), all in one process:

  1. ``Laplace.run`` on the device route (``bfhip_pipeline_laplace_opt``: the whole Newton iteration in one launch, analytic Hessian),
     with the full and with the Gauss-Newton matrix;
  2. ``Laplace.run`` on the host route (scipy 'trust-exact', per-step launches, the Hessian differenced from 4 d gradients in one
     launch) -- the only route this density had before the kernel existed;
  3. the Hessian kernel alone (``bfhip_pipeline_logp_hess``) for 1 and 256 points, outputs preallocated;
  4. the same kernels on a larger resident shape (``random_pipeline_spec(500, 64, 9)``: 64 inputs, 500 outputs compressed to 110 rows)
     for 1, 256 and 4096 points.

A single launch here lasts tens of microseconds, the size of the launch and event overhead, so a timed window holds INNER
back-to-back launches between two HIP events (per-launch time = window / INNER: launch overhead overlaps with execution, the figure
is the sustained cost of a launch in a stream), and a wall-time window RUNS_PER_WINDOW calls of ``run`` between two device
synchronisations.  A warm-up window first (it also grows the work buffer), then REPS windows, the routes alternated; median, min and
max over the windows.  One JSON line per measurement.

  python3 tools/pipeline_laplace_rate.py"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 7
INNER = 50             # launches per event window
RUNS_PER_WINDOW = 10   # Laplace.run calls per wall-time window


def _spread(v):
    v = sorted(v)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def _events_ms(fn, reps=REPS):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / INNER)
    return out[1:]   # (the first window is warm-up)


def fitted_density(seed=0):
    """The example's density after its round-0 fit, and a start in the sampling space."""
    import bayesfast_amd as bfa
    from bayesfast_amd.workloads import des_like_pipeline
    w = des_like_pipeline()
    d, m = w['d'], w['m']
    lo, hi = w['para_range'][:, 0], w['para_range'][:, 1]
    rng = np.random.default_rng(seed)
    su = bfa.PolyModel([bfa.PolyConfig('linear'), bfa.PolyConfig('quadratic', input_mask=w['nonlinear'])], input_size=d, output_size=m,
                       input_scales=w['para_range'])
    den = bfa.Chi2PipelineDensity(su, w['data'], prec_diag=np.ones(m), logp0=w['norm'], prior_mu=w['prior_mu'], prior_prec=w['prior_prec'],
                                  prior_c0=w['prior_c0'], input_scales=w['para_range'], hard_bounds=True)
    u0 = (w['x_true'] - lo) / (hi - lo)
    x_fit = lo + (hi - lo) * np.clip(u0 + 0.08 * rng.normal(size=(4 * su.n_param, d)), 0.02, 0.98)
    den.fit(x_fit, w['logp'](x_fit), y=w['model'](x_fit))
    return den, den.from_original(x_fit[0])


def _wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(RUNS_PER_WINDOW):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / RUNS_PER_WINDOW, out


def run_rates(den, x0):
    from bayesfast_amd.utils import Laplace
    routes = {'device_full': Laplace(n_sample=2000), 'device_gauss_newton': Laplace(n_sample=2000, hess_options={'gauss_newton': True}),
              'host_trust_exact': Laplace(optimize_method='trust-exact', n_sample=2000)}
    res, ms = {}, {k: [] for k in routes}
    for k, lap in routes.items():
        lap.run(den, x0)   # warm-up: uploads, allocations, scipy's imports
    for _ in range(REPS):   # alternated in one process
        for k, lap in routes.items():
            t, res[k] = _wall_ms(lambda: lap.run(den, x0))
            ms[k].append(t)
    out = {'workload': 'des_like_pipeline: 27 inputs, 457 outputs, round-0 fit', 'n_sample': 2000, 'windows': REPS,
           'runs_per_window': RUNS_PER_WINDOW}
    for k in routes:
        o = res[k].opt_result
        out[k] = {'wall_ms': _spread(ms[k]), 'nit': int(o.nit), 'success': bool(o.success), 'f_max': float(res[k].f_max)}
    out['x_max_difference_device_full_vs_host'] = float(np.max(np.abs(res['device_full'].x_max - res['host_trust_exact'].x_max)))
    out['cov_relative_difference_device_full_vs_host'] = float(np.max(np.abs(res['device_full'].cov - res['host_trust_exact'].cov)) /
                                                               np.max(np.abs(res['host_trust_exact'].cov)))
    out['host_over_device_full'] = out['host_trust_exact']['wall_ms']['median'] / out['device_full']['wall_ms']['median']
    return out


def kernel_rates(dev, x0, n, workload):
    import torch
    from bayesfast_amd import _lib
    dev.upload_if_needed()
    ctx, d = dev.ctx, dev.d
    x = torch.as_tensor(x0 + 0.05 * np.random.default_rng(1).normal(size=(n, d)), device=ctx.device)
    logp, grad, hess = ctx.empty((n,)), ctx.empty((n, d)), ctx.empty((n, d, d))
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {'workload': workload, 'kernel': 'bfhip_pipeline_logp_hess', 'n': n,
           'note': 'per-launch time of %d back-to-back launches between two events, outputs preallocated' % INNER}
    for name, kind in (('full', _lib.HESS_FULL), ('gauss_newton', _lib.HESS_GAUSS_NEWTON)):
        ms = _events_ms(lambda: _lib.check(ctx._lib.bfhip_pipeline_logp_hess(ctx.handle, n, p(x), 0, kind, p(logp), p(grad), p(hess))))
        out[name + '_ms'] = _spread(ms)
    ms = _events_ms(lambda: _lib.check(ctx._lib.bfhip_logp_grad(ctx.handle, n, p(x), 0, p(logp), p(grad))))
    out['bfhip_logp_grad_ms'] = _spread(ms)   # the gradient kernel on the same points, for scale
    opts = _lib.LaplaceOpts(200, 1e-5)
    xo, info = ctx.empty((n, d)), ctx.empty((n, 4))
    ms = _events_ms(lambda: _lib.check(ctx._lib.bfhip_pipeline_laplace_opt(ctx.handle, C.byref(opts), _lib.HESS_FULL, n, p(x), p(xo), p(logp),
                                                                          p(hess), p(info))))
    it = info.cpu().numpy()
    out['bfhip_pipeline_laplace_opt'] = {'ms': _spread(ms), 'iterations_mean': float(it[:, 0].mean()), 'iterations_max': int(it[:, 0].max()),
                                         'status_counts': np.bincount(it[:, 1].astype(int), minlength=4).tolist()}
    return out


def main():
    den, x0 = fitted_density()
    print(json.dumps(run_rates(den, x0)), flush=True)
    for n in (1, 256):
        print(json.dumps(kernel_rates(den.device(), x0, n, 'des_like_pipeline 27 x 457')), flush=True)
    from bayesfast_amd.device import DeviceDensity, get_context
    from bayesfast_amd.workloads import random_pipeline_spec
    big = DeviceDensity(random_pipeline_spec(500, 64, 9, seed=3), get_context(0))
    for n in (1, 256, 4096):
        print(json.dumps(kernel_rates(big, np.zeros(64), n, 'random_pipeline_spec(500, 64, 9)')), flush=True)


if __name__ == '__main__':
    main()
