#!/usr/bin/env python3
"""The posterior predictive summaries (bayesfast_amd/utils/predictive.py, csrc/bfhip_poly.hip: bfhip_polymodel_columns) at 4096
chains x 1000 draws, at two shapes: the DES shape (27 inputs, 457 outputs, quadratic) and 64 inputs x 500 outputs.  The draws are a
seeded normal around the bound's centre, scaled so that a few percent of them lie outside the bound.

  - ``predictive`` on the pipeline density: wall clock around a synchronise after a warm-up call, and its split into the columns
    kernel, the tables and the chi-square pass (each timed on its own, synchronised);
  - the route without it: ``fun_and_jac(jac=False)`` of all draws into (n, m), then ``summary`` of that tensor.  The two routes are
    alternated in one process, ``--reps`` times each, and every repeat is printed (the spread is the noise);
  - both routes' peak extra device memory (``torch.cuda.max_memory_allocated`` minus the level before), ``predictive`` at 64
    selected outputs and at all of them;
  - the columns kernel's time per point and output next to ``bfhip_polymodel_eval``'s without Jacobian at the same shape, each over
    a window of at least a second.

  python3 tools/predictive_rate.py [--reps 3] [--small] [--shape des|d64|both] [--kernel-only]     one JSON line per measurement

``--kernel-only`` keeps the last item alone; with ``BFHIP_LIBRARY`` pointing at a library whose ``bfhip_poly.hip`` was compiled with
``-DBF_PC_TILES=a,b,c,d`` it measures other numbers of 16-point tiles per wave (at T = 1, 2, 4, 8)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _window(fn, torch, least=1.0):
    """Seconds per call of fn over a window of at least ``least`` seconds (after one warm-up call)."""
    fn()
    n = 1
    while True:
        t, _ = _wall(lambda: [fn() for _ in range(n)], torch)
        if t >= least:
            return t / n
        n = max(n + 1, int(n * 1.5 * least / max(t, 1e-6)))


def _peak(fn, torch):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def make_density(d, m, seed):
    """A quadratic surrogate with random coefficients and a bound, and a Gaussian likelihood around its value at the centre."""
    from bayesfast_amd import PolyModel, PolyConfig, Chi2PipelineDensity
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(d, d))
    poly = dict(input_size=d, output_size=m, use_bound=True, mu=rng.normal(size=d) * 0.1, hess=a @ a.T / d + np.eye(d), alpha=1.,
                f_mu=np.zeros(m),
                configs=[dict(order='linear', input_mask=np.arange(d), output_mask=np.arange(m), coef=rng.normal(size=(m, d + 1))),
                         dict(order='quadratic', input_mask=np.arange(d), output_mask=np.arange(m),
                              coef=rng.normal(size=(m, d, d)) * (0.5 / np.sqrt(d)))])

    class _Fixed(PolyModel):
        def poly_spec(self, use_bound=None):
            return poly

    su = _Fixed([PolyConfig(c['order'], input_mask=c['input_mask'], output_mask=c['output_mask']) for c in poly['configs']],
                input_size=d, output_size=m)
    lin, quad = poly['configs'][0]['coef'], poly['configs'][1]['coef']
    mu = poly['mu']
    y = lin[:, 0] + lin[:, 1:] @ mu + np.einsum('i,oij,j->o', mu, np.triu(np.ones((d, d))) * quad, mu)
    poly['f_mu'] = y.copy()
    return su, Chi2PipelineDensity(su, y + rng.normal(size=m) * 0.05, prec_diag=np.full(m, 400.)), poly


def run_shape(name, d, m, n_chain, n_draw, reps, torch, kernel_only=False):
    su, den, poly = make_density(d, m, 11 + d)
    dm = su.device_model()
    # draws x = mu + s L^-T z with H = L L^T: beta = s |z|; s puts the 97th percentile of |z| (chi, d degrees) on alpha
    g = torch.Generator(device='cuda').manual_seed(5)
    z = torch.randn((n_chain, n_draw, d), generator=g, device='cuda', dtype=torch.float64)
    l_inv = torch.as_tensor(np.linalg.inv(np.linalg.cholesky(poly['hess'])), device='cuda')   # x - mu = s L^-T z = s (z^T L^-1)^T
    s = float(poly['alpha']) / float(np.sqrt(d) + 1.33)
    x = (torch.as_tensor(poly['mu'], device='cuda') + s * (z.reshape(-1, d) @ l_inv)).reshape(n_chain, n_draw, d).contiguous()
    del z
    n = n_chain * n_draw
    shape = dict(shape=name, d=d, m=m, n_chain=n_chain, n_draw=n_draw)
    xf = x.reshape(n, d)
    if not kernel_only:
        run_routes(shape, su, den, dm, x, xf, reps, torch)
    run_kernels(shape, dm, x, xf, reps, torch)


def run_routes(shape, su, den, dm, x, xf, reps, torch):
    from bayesfast_amd.utils import predictive, summary
    from bayesfast_amd.utils.predictive import _chi2_of, batch_width, output_plan
    ctx = dm.ctx
    n_chain, n_draw, d = (int(v) for v in x.shape)
    n, m = n_chain * n_draw, dm.m
    res = predictive(den, x)   # warm-up of every kernel of the route
    print(json.dumps(dict(shape, oob_share=res.oob_share, ppp=res.ppp, chi2_min=res.chi2_min, width=batch_width(1 << 30, n, m))), flush=True)

    def materialised():
        f, _ = dm.fun_and_jac(xf, jac=False)
        return summary(f.reshape(n_chain, n_draw, m), (0.16, 0.5, 0.84))

    pred_s, mat_s = [], []
    materialised()
    for _r in range(reps):      # alternated
        pred_s.append(_wall(lambda: predictive(den, x), torch)[0])
        mat_s.append(_wall(materialised, torch)[0])
    print(json.dumps(dict(shape, predictive_s=pred_s, materialised_s=mat_s,
                          note='materialised = fun_and_jac(jac=False) into (n, m) + summary; it has no chi-square pass')), flush=True)
    # the split of predictive: columns kernel over all outputs, the tables, the chi-square pass
    width = batch_width(1 << 30, n, m)
    buf = ctx.empty((n_chain, n_draw, width))
    _, batches = output_plan(None, m, width)

    def columns_all():
        for calls in batches:
            for k0, nb, col in calls:
                dm.fun_columns(x, k0, nb, out=buf[:, :, col:])

    def tables_all():
        for calls in batches:
            summary(buf[:, :, :calls[-1][2] + calls[-1][1]], (0.16, 0.5, 0.84))

    columns_all()
    t_cols = [_wall(columns_all, torch)[0] for _r in range(reps)]
    t_tabs = [_wall(tables_all, torch)[0] for _r in range(reps)]
    t_chi2 = [_wall(lambda: _chi2_of(den, dm, x, None, None, 1 << 30), torch)[0] for _r in range(reps)]
    print(json.dumps(dict(shape, columns_s=t_cols, tables_s=t_tabs, chi2_pass_s=t_chi2)), flush=True)
    del buf
    # peak extra device memory
    torch.cuda.empty_cache()
    peaks = dict(predictive_64_outputs=_peak(lambda: predictive(den, x, outputs=np.arange(min(64, m))), torch),
                 predictive_all_outputs=_peak(lambda: predictive(den, x), torch),
                 materialised=_peak(materialised, torch))
    print(json.dumps(dict(shape, peak_extra_bytes=peaks, f_bytes=8 * n * m, sample_bytes=8 * n * d)), flush=True)


def run_kernels(shape, dm, x, xf, reps, torch):
    """Kernel against kernel: per point and output, windows of at least a second."""
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = dm.ctx
    n_chain, n_draw, d = (int(v) for v in x.shape)
    n, m = n_chain * n_draw, dm.m
    nb = min(16 * (m // 16), 256)
    outc = ctx.empty((n_chain, n_draw, nb))
    t_col = _window(lambda: dm.fun_columns(x, 0, nb, out=outc), torch)
    del outc
    n_ev = min(n, (1 << 30) // (8 * m))
    f = ctx.empty((n_ev, m))
    xe = xf[:n_ev].contiguous()
    dm.upload_if_needed()
    t_ev = _window(lambda: _lib.check(ctx._lib.bfhip_polymodel_eval(ctx.handle, n_ev, _ptr(xe), _ptr(f), None)), torch)
    reps_k = []
    for _r in range(reps):
        outc = ctx.empty((n_chain, n_draw, nb))
        a = _window(lambda: dm.fun_columns(x, 0, nb, out=outc), torch, 0.5)
        del outc
        b = _window(lambda: _lib.check(ctx._lib.bfhip_polymodel_eval(ctx.handle, n_ev, _ptr(xe), _ptr(f), None)), torch, 0.5)
        reps_k.append((a / (n * nb) * 1e12, b / (n_ev * m) * 1e12))
    print(json.dumps(dict(shape, library=os.path.basename(_lib.LIB_PATH), columns_ps_per_value=t_col / (n * nb) * 1e12, eval_nojac_ps_per_value=t_ev / (n_ev * m) * 1e12,
                          columns_call=dict(points=n, outputs=nb), eval_call=dict(points=n_ev, outputs=m),
                          alternated_ps_per_value=reps_k)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='64 chains x 200 draws: a rehearsal of the script, not a measurement')
    ap.add_argument('--shape', default='both', choices=('des', 'd64', 'both'))
    ap.add_argument('--kernel-only', action='store_true',
                    help='only the kernel-against-kernel windows (with BFHIP_LIBRARY: a build with other tiles per wave, -DBF_PC_TILES=...)')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('predictive_rate: no GPU (there is no CPU measurement of a device route)')
    n_chain, n_draw = (64, 200) if a.small else (4096, 1000)
    if a.shape in ('des', 'both'):
        run_shape('des', 27, 457, n_chain, n_draw, a.reps, torch, a.kernel_only)
    if a.shape in ('d64', 'both'):
        run_shape('d64', 64, 500, n_chain, n_draw, a.reps, torch, a.kernel_only)


if __name__ == '__main__':
    main()
