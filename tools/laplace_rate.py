#!/usr/bin/env python3
"""The device Laplace approximation (csrc/bfhip_laplace.hip) measured: the analytic Hessian kernel against its HBM write bound, and
``Laplace.run`` on the device route against the host loop the parent API allowed.

  1. ``bfhip_logp_hess`` at d = 64 and 128, n = 4096 points: device-synchronised event times, five repeats, against 8 n d^2 bytes at
     the plain-store rate of the chip (6.1 TB/s): a share of the write bound.
  2. ``Laplace.run`` on the 64-d headline surrogate (``correlated_gaussian_spec(64)``, the surrogate of smoke() and of the bench's
     headline) and on a 128-d surrogate with masked cubic-2 / cubic-3 terms, both behind hard bounds: the device route with 1, 256
     and 4096 starts, alternated in one process with the HOST LOOP restricted to what the API had before this kernel existed -- scipy's
     Newton-CG with per-point ``SurrogateDensity.logp`` / ``.grad`` and a Hessian from per-point central differences of the gradient
     (2 d calls, each a launch and a synchronisation) -- and with this package's own host route (scipy 'trust-exact', the
     difference Hessian in ONE launch of 4 d points), the fairer second number.
  3. Iterations per start (``info``), so that the cost per iteration can be stated.

  python3 tools/laplace_rate.py              all of it, one JSON line per measurement; then a rocprofv3 --kernel-trace --stats run
                                             of its own (kernel statistics copied to profiles/laplace_rate_kernel_stats.csv)
  python3 tools/laplace_rate.py --gpu-only   the device launches only (what runs under the profiler)"""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STORE_BPS = 6.1e12   # plain 8-byte-per-lane stores, whole chip
REPS = 5


def _events_ms(fn, reps=REPS):
    """Warm-up call, then ``reps`` separately timed calls: [ms] * reps."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def _spread(v):
    v = sorted(v)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def bounded_spec(d, cubic):
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, _ = correlated_gaussian_spec(d)
    spec = dict(spec, ranges=np.tile(np.array([-3., 5.]), (d, 1)), hard_bounds=np.ones((d, 2), np.uint8), link=None)
    if cubic:
        rng = np.random.default_rng(17)
        n = 16
        m = np.arange(n)
        a3 = np.zeros((1, n, n, n))
        for j in range(n):
            for k in range(j + 1, n):
                for l in range(k + 1, n):
                    a3[0, j, k, l] = 0.005 * rng.normal()
        po = dict(spec['poly'])
        po['configs'] = list(po['configs']) + [dict(order='cubic-2', input_mask=m, output_mask=np.arange(1), coef=0.005 * rng.normal(size=(1, n, n))),
                                               dict(order='cubic-3', input_mask=m, output_mask=np.arange(1), coef=a3)]
        spec['poly'] = po
    return spec


def _density(spec):
    from bayesfast_amd.core.density import SurrogateDensity
    from bayesfast_amd.device import DeviceDensity, get_context

    class SpecDensity(SurrogateDensity):
        def __init__(self):
            self._dev = DeviceDensity(spec, get_context(0))

        def spec(self):
            return spec

        def device(self, ctx=None):
            return self._dev

    return SpecDensity()


def hess_rate(d, n=4096):
    from bayesfast_amd.workloads import correlated_gaussian_spec
    from bayesfast_amd.device import DeviceDensity, get_context
    import torch
    spec, _ = correlated_gaussian_spec(d)
    dd = DeviceDensity(spec, get_context(0))
    x = torch.as_tensor(np.random.default_rng(1).normal(size=(n, d)), device='cuda')
    # the launch alone, into preallocated outputs (DeviceDensity.logp_grad_hess adds three allocations per call)
    import ctypes as C
    from bayesfast_amd import _lib
    dd.upload_if_needed()
    ctx = dd.ctx
    logp, grad, hess = ctx.empty((n,)), ctx.empty((n, d)), ctx.empty((n, d, d))
    p = lambda t: C.c_void_p(t.data_ptr())
    ms = _events_ms(lambda: _lib.check(ctx._lib.bfhip_logp_hess(ctx.handle, n, p(x), 0, p(logp), p(grad), p(hess))))
    bound_ms = 8. * n * d * d / STORE_BPS * 1e3
    return {'kernel': 'bfhip_logp_hess', 'd': d, 'n': n, 'ms': _spread(ms), 'write_bound_ms': bound_ms,
            'share_of_write_bound': bound_ms / _spread(ms)['median'], 'note': 'event time of the launch alone, outputs preallocated'}


def host_loop(den, x0, tol=1e-5):
    """What the API allowed before: per-point logp / grad, the Hessian by 2 d per-point gradient calls."""
    from scipy.optimize import minimize
    d = x0.size
    n_call = [0]

    def f(x):
        n_call[0] += 1
        return -float(den.logp(x, original_space=False))

    def g(x):
        n_call[0] += 1
        return -np.asarray(den.grad(x, original_space=False))

    def h(x):
        H = np.empty((d, d))
        for j in range(d):
            e = np.zeros(d)
            e[j] = 1e-4 * max(1., abs(x[j]))
            H[:, j] = (g(x + e) - g(x - e)) / (2. * e[j])
        return 0.5 * (H + H.T)

    t0 = time.perf_counter()
    opt = minimize(f, x0, method='Newton-CG', jac=g, hess=h, tol=tol)
    cov_h = h(opt.x)
    return (time.perf_counter() - t0) * 1e3, opt, n_call[0], cov_h


def laplace_rates(d, cubic, reps=REPS, host=True):
    import torch
    from bayesfast_amd.utils import Laplace
    spec = bounded_spec(d, cubic)
    den = _density(spec)
    rng = np.random.default_rng(3)
    lap = Laplace(n_sample=2000)
    out = {'workload': '%d-d %s surrogate behind hard bounds' % (d, 'cubic' if cubic else 'quadratic'), 'd': d}
    x1 = rng.normal(size=d)
    run_ms, host_ms, route_ms = [], [], []
    # this package's own host route: scipy with the difference Hessian taken in ONE launch ('trust-exact' keeps it off the device route)
    host_route = Laplace(optimize_method='trust-exact', n_sample=2000)
    lap.run(den, x1)
    for _ in range(reps):   # alternated in one process
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = lap.run(den, x1)
        run_ms.append((time.perf_counter() - t0) * 1e3)
        if host:
            ms, opt, n_call, _ = host_loop(den, x1)
            host_ms.append(ms)
            t0 = time.perf_counter()
            res_h = host_route.run(den, x1)
            route_ms.append((time.perf_counter() - t0) * 1e3)
    out['device_route_1_start_wall_ms'] = _spread(run_ms)
    out['iterations_1_start'] = int(res.opt_result.nit)
    if host:
        out['host_loop_wall_ms'] = _spread(host_ms)
        out['host_loop_density_calls'] = n_call
        out['host_loop_nit'] = int(opt.nit)
        out['host_over_device'] = _spread(host_ms)['median'] / _spread(run_ms)['median']
        out['own_host_route_wall_ms'] = _spread(route_ms)
        out['own_host_route_nit'] = int(res_h.opt_result.nit)
        out['own_host_route_over_device'] = _spread(route_ms)['median'] / _spread(run_ms)['median']
        out['x_max_difference'] = float(np.max(np.abs(opt.x - res.x_max)))
    for n_start in (1, 256, 4096):
        x0 = torch.as_tensor(rng.normal(size=(n_start, d)), device='cuda')
        dev = den.device()
        ms = _events_ms(lambda: dev.maximize(x0, xtol=1e-5), reps)
        info = dev.maximize(x0, xtol=1e-5)['info'].cpu().numpy()
        out['maximize_%d_starts' % n_start] = {'kernel_ms': _spread(ms), 'iterations_mean': float(info[:, 0].mean()),
                                               'iterations_max': int(info[:, 0].max()), 'status_counts': np.bincount(info[:, 1].astype(int), minlength=4).tolist(),
                                               'ms_per_iteration_of_the_slowest_start': _spread(ms)['median'] / max(1, int(info[:, 0].max()))}
    return out


def main():
    gpu_only = '--gpu-only' in sys.argv
    for d in (64, 128):
        print(json.dumps(hess_rate(d)), flush=True)
    for d, cubic in ((64, False), (128, True)):
        print(json.dumps(laplace_rates(d, cubic, reps=2 if gpu_only else REPS, host=not gpu_only)), flush=True)
    if gpu_only:
        return
    prof = shutil.which('rocprofv3')
    if not prof:
        print(json.dumps({'profile': None, 'reason': 'rocprofv3 not found'}))
        return
    out_dir = os.path.join(ROOT, 'profiles', 'laplace_rate')
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([prof, '--kernel-trace', '--stats', '-d', out_dir, '-o', 'laplace_rate', '--output-format', 'csv', '--',
                        sys.executable, os.path.abspath(__file__), '--gpu-only'], cwd=ROOT, capture_output=True, text=True)
    stats = []
    for base, _, files in os.walk(out_dir):
        stats += [os.path.join(base, f) for f in files if f.endswith('kernel_stats.csv')]
    if stats:
        shutil.copy(sorted(stats)[0], os.path.join(ROOT, 'profiles', 'laplace_rate_kernel_stats.csv'))
    print(json.dumps({'profile': sorted(stats), 'rc': r.returncode}))


if __name__ == '__main__':
    main()
