#!/usr/bin/env python3
"""Profiles of the density (csrc/bfhip_profile.hip; ``bayesfast_amd.utils.profile``) measured on the DES shape
(``workloads.des_like_pipeline``: 27 inputs, 457 outputs, fitted as examples/des_like_pipeline.py fits its round 0) and on the 64-d
headline surrogate behind hard bounds (``correlated_gaussian_spec(64)``, as tools/laplace_rate.py bounds it), all in one process:

  1. ``profile`` with the 1-D profiles only, and with ``pairs='all'`` (21 x 21 points per pair): wall time of the whole call (its
     launches, the host's grid bookkeeping and the copies back), and from the result the number of grid points, the mean and the
     largest number of accepted Newton iterations per grid point, and the points that did not converge;
  2. the two launches alone (the 1-D lines: 2 d workgroups, latency-bound by construction; the 2-D lines: two per pair and grid
     value, the launch that fills the machine), event-timed on preallocated outputs;
  3. for comparison the route that existed before: ``scipy.optimize.minimize`` (BFGS) over the free coordinates of one grid point
     with the device's ``logp_and_grad`` (one launch per function value, minus the log-Jacobian on the host), on a sample of 20 grid
     points of the 1-D profiles, each started at its neighbour's optimum as the device lines are.

A warm-up call first (it also grows the work buffer), then REPS calls; median, min and max.  One JSON line per measurement.

  python3 tools/profile_rate.py"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

REPS = 5
N_HOST = 20


def _spread(v):
    v = sorted(v)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def _wall_ms(fn, reps=REPS):
    import torch
    out = fn()   # warm-up
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return _spread(ms), out


def _counts(p, two_d):
    it = np.concatenate([p.n_iter2d[q].ravel() for q in p.pairs]) if two_d else np.concatenate([p.n_iter[i] for i in p.params])
    st = np.concatenate([p.status2d[q].ravel() for q in p.pairs]) if two_d else np.concatenate([p.status[i] for i in p.params])
    run = st != 4
    return {'grid_points': int(run.sum()), 'iterations_mean': float(it[run].mean()), 'iterations_max': int(it[run].max()),
            'status_counts': np.bincount(st, minlength=5).tolist()}


def profile_rates(den, x_0, workload, gauss_newton=False):
    from bayesfast_amd.utils import profile
    out = {'workload': workload, 'n_grid': 21, 'span': 4., 'reps': REPS}
    ms, p1 = _wall_ms(lambda: profile(den, x_0=x_0, gauss_newton=gauss_newton))
    out['profile_1d'] = dict(wall_ms=ms, **_counts(p1, False))
    ms, p2 = _wall_ms(lambda: profile(den, x_0=x_0, pairs='all', gauss_newton=gauss_newton))
    out['profile_1d_and_all_pairs'] = dict(wall_ms=ms, pairs=len(p2.pairs), **_counts(p2, True))
    out['improved_at'] = len(p2.improved_at)
    out['us_per_2d_grid_point'] = 1e3 * (out['profile_1d_and_all_pairs']['wall_ms']['median'] - out['profile_1d']['wall_ms']['median']) / \
        out['profile_1d_and_all_pairs']['grid_points']
    return out, p1


def _lines_of(dev, p1, two_d):
    """fixed, walk, start, values (NumPy, sampling coordinates) of the launches ``profile`` makes for the result p1."""
    d = dev.d
    to_s = (lambda x: dev.constraint('from_original', x).cpu().numpy()) if dev.spec.get('ranges') is not None else (lambda x: np.array(x))
    xm = to_s(p1.x_max[None])[0]
    opt = {i: to_s(p1.x[i]) for i in p1.params}
    fixed, walk, start, vals = [], [], [], []
    if not two_d:
        for i in p1.params:
            g = opt[i][:, i]
            for side in (np.flatnonzero(g >= xm[i]), np.flatnonzero(g < xm[i])[::-1]):
                m = np.zeros(d, np.uint8)
                m[i] = 1
                fixed.append(m), walk.append(i), start.append(xm), vals.append(g[side])
    else:
        for a, i in enumerate(p1.params):
            for j in p1.params[a + 1:]:
                g = opt[j][:, j]
                for s in opt[i]:
                    for side in (np.flatnonzero(g >= s[j]), np.flatnonzero(g < s[j])[::-1]):
                        m = np.zeros(d, np.uint8)
                        m[[i, j]] = 1
                        fixed.append(m), walk.append(j), start.append(s), vals.append(g[side])
    n_val = max(len(v) for v in vals)
    V = np.full((len(vals), n_val), np.nan)
    for k, v in enumerate(vals):
        V[k, :len(v)] = v
    return np.array(fixed), np.array(walk, np.int32), np.array(start), V


def launch_rates(dev, p1, workload, gauss_newton=False):
    """The 1-D and the 2-D launch alone, rebuilt from the 1-D result as ``profile`` builds them, on preallocated outputs."""
    import torch
    from bayesfast_amd import _lib
    dev.upload_if_needed()
    ctx, d = dev.ctx, dev.d
    pipeline = dev.spec.get('chi2') is not None
    p = lambda t: C.c_void_p(t.data_ptr())
    opts = _lib.LaplaceOpts(50, 1e-6)
    out = {'workload': workload, 'note': 'event time of the launch alone (it includes the read-back of the mask that checks it), outputs preallocated'}
    for name, two_d in (('lines_1d', False), ('lines_2d_all_pairs', True)):
        fixed, walk, start, vals = _lines_of(dev, p1, two_d)
        n, n_val = vals.shape
        t = [ctx.tensor(fixed, torch.uint8), ctx.tensor(walk, torch.int32), ctx.tensor(start, torch.float64), ctx.tensor(vals, torch.float64)]
        x, logp, info = ctx.empty((n, n_val, d)), ctx.empty((n, n_val)), ctx.empty((n, n_val, 4))
        if pipeline:
            kind = _lib.HESS_GAUSS_NEWTON if gauss_newton else _lib.HESS_FULL
            fn = lambda: _lib.check(ctx._lib.bfhip_pipeline_profile_lines(ctx.handle, C.byref(opts), kind, _lib.PROFILE_ORIGINAL, n, n_val, p(t[0]),
                                                                          p(t[1]), p(t[2]), p(t[3]), p(x), p(logp), p(info)))
        else:
            fn = lambda: _lib.check(ctx._lib.bfhip_profile_lines(ctx.handle, C.byref(opts), _lib.PROFILE_ORIGINAL, n, n_val, p(t[0]), p(t[1]),
                                                                 p(t[2]), p(t[3]), p(x), p(logp), p(info)))
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        st = info.cpu().numpy()[..., 1]
        pts = int((st != 4).sum())
        out[name] = {'lines': n, 'n_val': n_val, 'grid_points': pts, 'ms': _spread(ms), 'us_per_grid_point': 1e3 * _spread(ms)['median'] / pts}
    return out


def host_route(dev, p1, workload):
    """scipy's BFGS over the free coordinates with one ``logp_and_grad`` launch per function value, at N_HOST grid points of the 1-D
    profiles, each from its inward neighbour's optimum."""
    from scipy.optimize import minimize
    d = dev.d
    has_t = dev.spec.get('ranges') is not None
    to_s = (lambda x: dev.constraint('from_original', x).cpu().numpy()) if has_t else (lambda x: np.array(x))
    both = np.asarray(dev.spec['hard_bounds'], dtype=bool).all(axis=1) if has_t else np.zeros(d, bool)
    rg = (dev.spec['ranges'][:, 1] - dev.spec['ranges'][:, 0]) if has_t else np.ones(d)
    assert bool(both.all()) == has_t   # (two-sided hard bounds on every coordinate, or no transform: the two workloads here)

    def fg(x):   # the original objective and its gradient from the sampling-space launch (all-logit or no transform here)
        f, g = dev.logp_and_grad(x, False)
        f, g = float(f.cpu()), g.cpu().numpy()
        if has_t:
            s = 1. / (1. + np.exp(-x))
            f -= float(np.sum(np.where(both, np.log(rg * s * (1. - s)), 0.)))
            g = g - np.where(both, 1. - 2. * s, 0.)
        return f, g

    rng = np.random.default_rng(0)
    ms, n_eval, err = [], [], []
    for _ in range(N_HOST):
        i = int(rng.choice(p1.params))
        k = int(rng.integers(0, p1.values[i].size))
        c = (p1.values[i].size - 1) // 2
        if k == c:
            k += 1
        xs = to_s(p1.x[i])
        start, target = xs[k - 1 if k > c else k + 1].copy(), xs[k]
        start[i] = target[i]
        free = np.arange(d) != i
        count = [0]

        def neg(z):
            count[0] += 1
            x = start.copy()
            x[free] = z
            f, g = fg(x)
            return -f, -g[free]

        t0 = time.perf_counter()
        opt = minimize(neg, start[free], jac=True, method='BFGS', options={'gtol': 1e-6})
        ms.append((time.perf_counter() - t0) * 1e3)
        n_eval.append(count[0])
        err.append(float(abs(-opt.fun - p1.logp[i][k])))
    return {'workload': workload, 'route': "scipy.optimize.minimize(BFGS) over the free coordinates, one logp_and_grad launch per value",
            'grid_points': N_HOST, 'ms_per_grid_point': _spread(ms), 'launches_per_grid_point_mean': float(np.mean(n_eval)),
            'max_abs_difference_of_the_profile_value': float(np.max(err))}


def main():
    from pipeline_laplace_rate import fitted_density
    from laplace_rate import bounded_spec, _density
    den, x0 = fitted_density()
    name = 'des_like_pipeline: 27 inputs, 457 outputs, round-0 fit'
    for gn in (True, False):
        res, p1 = profile_rates(den, den.to_original(x0), name + (', Gauss-Newton matrix' if gn else ''), gn)
        print(json.dumps(res), flush=True)
        print(json.dumps(launch_rates(den.device(), p1, res['workload'], gn)), flush=True)
    print(json.dumps(host_route(den.device(), p1, name)), flush=True)   # (against the full matrix's profile)
    spec = bounded_spec(64, False)
    sden = _density(spec)
    name = 'correlated_gaussian_spec(64) behind hard bounds [-3, 5]'
    res, p1 = profile_rates(sden, np.zeros(64), name)
    print(json.dumps(res), flush=True)
    print(json.dumps(launch_rates(sden.device(), p1, name)), flush=True)
    print(json.dumps(host_route(sden.device(), p1, name)), flush=True)


if __name__ == '__main__':
    main()
