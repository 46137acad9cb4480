#!/usr/bin/env python3
"""Pointwise PSIS-LOO and WAIC of the pipeline's data (bayesfast_amd/utils/data_loo.py, csrc/bfhip_ploo.h) at the DES shape: 27 inputs,
457 outputs, 4096 chains x 1000 draws (``make_density`` of tools/predictive_rate.py; the draws are a seeded sample of the Laplace
approximation of that density's posterior, so that the conditional residuals are of order one).

  - ``data_loo`` on the pipeline density: wall clock around a synchronise after a warm-up call, ``--reps`` times;
  - its stages on one batch of 16 outputs, each timed on its own (synchronised): the residual model's ``fun_columns``,
    ``bfhip_ploo_moments``, ``bfhip_ploo_tail`` (the select), ``bfhip_ploo_finish``;
  - the route without the select: the existing ``psis()`` (``bfhip_psis``: a full radix sort of its n values) on the ratios of each of
    the same 16 columns of the same buffer, the ratios formed by torch on the device beforehand and not timed;
  - the ratio of the two per batch, and both scaled to the 29 batches of the shape.

  python3 tools/data_loo_rate.py [--reps 3] [--small]     one JSON line per measurement

No threshold is set.  ``--small`` runs 256 x 250 draws and 40 outputs (a check that the tool runs)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    import torch
    from predictive_rate import make_density
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel, polymodel_dense_from_poly, residual_dense, _ptr
    from bayesfast_amd.utils import data_loo, psis
    from bayesfast_amd.utils.data_loo import whitening_of, _Stages
    d, m, n_chain, n_draw = (27, 40, 256, 250) if args.small else (27, 457, 4096, 1000)
    su, den, poly = make_density(d, m, 11 + d)
    # draws from the Laplace approximation of this density's posterior around the bound's centre: with J the outputs' Jacobian at mu
    # and P = prec_diag, x ~ N(mu + C J^T P (y - f(mu)), C), C = (J^T P J)^-1 -- the conditional residuals are then of order one
    lin, quad, mu = poly['configs'][0]['coef'], poly['configs'][1]['coef'], poly['mu']
    qu = np.triu(np.ones((d, d))) * quad
    jac = lin[:, 1:] + np.einsum('oij,j->oi', qu + np.transpose(qu, (0, 2, 1)), mu)
    cov = np.linalg.inv(jac.T @ (den._pdiag[:, None] * jac))
    centre = mu + cov @ (jac.T @ (den._pdiag * (den._y - poly['f_mu'])))
    g = torch.Generator(device='cuda').manual_seed(5)
    z = torch.randn((n_chain * n_draw, d), generator=g, device='cuda', dtype=torch.float64)
    x = (torch.as_tensor(centre, device='cuda') + z @ torch.as_tensor(np.linalg.cholesky(cov).T.copy(), device='cuda'))
    x = x.reshape(n_chain, n_draw, d).contiguous()
    del z
    n = n_chain * n_draw
    shape = dict(d=d, m=m, n_chain=n_chain, n_draw=n_draw, batches=(m + 15) // 16)
    res = data_loo(den, x)   # warm-up of every kernel of the route
    print(json.dumps(dict(shape, elpd_loo=res.elpd_loo_total, p_loo=res.p_loo_total, khat_max=float(np.nanmax(res.khat)),
                          n_khat_bad=res.n_khat_bad, pit_range=[float(res.pit.min()), float(res.pit.max())])), flush=True)
    for rep in range(args.reps):
        t, _ = _wall(lambda: data_loo(den, x), torch)
        print(json.dumps(dict(shape, what='data_loo', rep=rep, seconds=t)), flush=True)
    # the stages on the first batch
    w, c = whitening_of(den._prec, den._pdiag)
    rm = DevicePolyModel.from_dense(residual_dense(polymodel_dense_from_poly(su.poly_spec()), den._y, w))
    ctx = rm.ctx
    lib, h = ctx._lib, ctx.handle
    buf = ctx.empty((n_chain, n_draw, 16))
    st = _Stages(ctx, n, None)
    cd = ctx.tensor(np.ascontiguousarray(c[:16]))
    out = ctx.empty((_lib.PLOO_NOUT, 16))
    head = (h, n, _ptr(buf), 16, 16, _lib.PLOO_Z, _ptr(cd), None)
    tail = (_ptr(st.work), st.work.numel())
    stages = [('fun_columns', lambda: rm.fun_columns(x, 0, 16, out=buf)),
              ('moments', lambda: _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), *tail))),
              ('tail', lambda: _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(st.keys), _ptr(st.idx), *tail))),
              ('finish', lambda: _lib.check(lib.bfhip_ploo_finish(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out), *tail)))]
    for name, fn in stages:
        fn()
    sel = []
    for rep in range(args.reps):
        row = {}
        for name, fn in stages:
            row[name], _ = _wall(fn, torch)
        sel.append(sum(row[k] for k in ('moments', 'tail', 'finish')))
        print(json.dumps(dict(shape, what='stages of one batch', rep=rep, **row)), flush=True)
    khat_sel = out[4].cpu().numpy().copy()
    # the parent's route: psis() per column, a full sort each
    rm.fun_columns(x, 0, 16, out=buf)
    ratios = (0.5 * buf.reshape(n, 16)**2 - cd).t().contiguous()   # r = -ell = z^2 / 2 - c, a row per column
    khat_ps = np.array([psis(ratios[b]).khat for b in range(16)])   # (and the warm-up)
    full = []
    for rep in range(args.reps):
        t, _ = _wall(lambda: [psis(ratios[b]) for b in range(16)], torch)
        full.append(t)
        print(json.dumps(dict(shape, what='psis() on the 16 columns of the batch', rep=rep, seconds=t)), flush=True)
    print(json.dumps(dict(shape, what='summary', select_batch=min(sel), psis_batch=min(full), ratio_psis_over_select=min(full) / min(sel),
                          select_all_batches=min(sel) * shape['batches'], psis_all_batches=min(full) * shape['batches'],
                          khat_max_abs_difference=float(np.max(np.abs(khat_sel - khat_ps))))), flush=True)


if __name__ == '__main__':
    main()
