#!/usr/bin/env python3
"""Leave-group-out cross-validation of the pipeline's data (bayesfast_amd/utils/data_lgo.py, csrc/bfhip_lgo.h) at the DES shape: 27
inputs, 457 outputs, 4096 chains x 1000 draws, 20 groups of mixed sizes (1 to 60 adjacent outputs, 411 in all; ``make_density`` of
tools/predictive_rate.py and the seeded draws of tools/data_loo_rate.py).

  - ``data_lgo`` on the pipeline density: wall clock around a synchronise after a warm-up call, ``--reps`` times;
  - its stages, each timed on its own (synchronised): the derived model's ``fun_columns`` on 16 columns, ``bfhip_lgo_accum`` of those 16
    columns, and on the first batch of 16 groups ``bfhip_ploo_moments``, ``bfhip_ploo_tail`` and ``bfhip_lgo_finish``, beside
    ``bfhip_ploo_finish`` on the same batch;
  - the route that existed before these entry points: every group's z materialised with ``fun_columns``, ``torch`` row sums,
    ``pointwise_loo`` on the device for the K columns of ell, and per group ``psis()`` to rebuild the weights under which
    ``torch.special.gammaincc`` and q are averaged;
  - both times, and the largest differences of khat, elpd_lgo and ppp_lgo between the two routes.

  python3 tools/data_lgo_rate.py [--reps 3] [--small]     one JSON line per measurement

No threshold is set.  ``--small`` runs 256 x 250 draws and 40 outputs in 6 groups (a check that the tool runs)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SIZES = (1, 2, 3, 5, 8, 12, 16, 17, 20, 24, 30, 33, 40, 45, 50, 10, 6, 4, 25, 60)


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
    from bayesfast_amd.device import DevicePolyModel, polymodel_dense_from_poly, linear_dense, _ptr
    from bayesfast_amd.utils import data_lgo, group_whitening_of, pointwise_loo, psis
    from bayesfast_amd.utils.data_lgo import _LgoStages
    d, m, n_chain, n_draw, sizes = (27, 40, 256, 250, (1, 2, 3, 5, 8, 17)) if args.small else (27, 457, 4096, 1000, SIZES)
    su, den, poly = make_density(d, m, 11 + d)
    lin, quad, mu = poly['configs'][0]['coef'], poly['configs'][1]['coef'], poly['mu']
    qu = np.triu(np.ones((d, d))) * quad
    jac = lin[:, 1:] + np.einsum('oij,j->oi', qu + np.transpose(qu, (0, 2, 1)), mu)
    cov = np.linalg.inv(jac.T @ (den._pdiag[:, None] * jac))
    chol = np.linalg.cholesky(cov)
    centre = mu + cov @ (jac.T @ (den._pdiag * (den._y - poly['f_mu'])))
    g = torch.Generator(device='cuda').manual_seed(5)
    z = torch.randn((n_chain * n_draw, d), generator=g, device='cuda', dtype=torch.float64)
    x = (torch.as_tensor(centre, device='cuda') + z @ torch.as_tensor(chol.T.copy(), device='cuda'))
    x = x.reshape(n_chain, n_draw, d).contiguous()
    del z
    n = n_chain * n_draw
    first = np.concatenate([[0], np.cumsum(sizes)])
    groups = [list(range(int(first[k]), int(first[k + 1]))) for k in range(len(sizes))]
    shape = dict(d=d, m=m, n_chain=n_chain, n_draw=n_draw, groups=len(groups), points=int(first[-1]))
    res = data_lgo(den, x, groups)   # warm-up of every kernel of the route
    print(str(res), file=sys.stderr)
    print(json.dumps(dict(shape, khat_max=float(np.nanmax(res.khat)), n_khat_bad=res.n_khat_bad, ppp_lgo_min=float(np.nanmin(res.ppp_lgo)),
                          ppp_lgo_max=float(np.nanmax(res.ppp_lgo)))), flush=True)
    whole = []
    for rep in range(args.reps):
        t, _ = _wall(lambda: data_lgo(den, x, groups), torch)
        whole.append(t)
        print(json.dumps(dict(shape, what='data_lgo', rep=rep, seconds=t)), flush=True)
    # the stages: 16 columns, and the first batch of 16 groups
    a, const, sz, colg = group_whitening_of(den._prec, den._pdiag, groups)
    dense = polymodel_dense_from_poly(su.poly_spec())
    rm = DevicePolyModel.from_dense(linear_dense(dense, -a, a @ den._y))
    ctx = rm.ctx
    lib, h = ctx._lib, ctx.handle
    lo = diff = None
    if su._input_scales is not None:
        lo = ctx.tensor(np.ascontiguousarray(su._input_scales[:, 0]), torch.float64)
        diff = ctx.tensor(np.ascontiguousarray(su._input_scales_diff), torch.float64)
    ng = min(16, len(groups))
    zbuf = ctx.empty((n_chain, n_draw, 16))
    acc = ctx.empty((n, 16))
    st = _LgoStages(ctx, n, None)
    out, out2, lgo = ctx.empty((_lib.PLOO_NOUT, 16)), ctx.empty((_lib.PLOO_NOUT, 16)), ctx.empty((len(_lib.LGO_ROWS), 16))
    cc, dd = (C.c_double * 16)(*const[:ng]), (C.c_double * 16)(*[float(v) for v in sz[:ng]])
    for k0 in range(0, int(first[ng]), 16):   # the batch's ell columns, as data_lgo fills them
        nb = min(16, int(first[ng]) - k0)
        rm.fun_columns(x, k0, nb, lo, diff, out=zbuf)
        slots = colg[k0:k0 + nb]
        start = sum(1 << int(s) for s in np.unique(slots) if first[s] >= k0)
        _lib.check(lib.bfhip_lgo_accum(h, n, _ptr(zbuf), 16, nb, (C.c_int * nb)(*[int(s) for s in slots]), cc, start, _ptr(acc), 16))
    scratch = ctx.empty((n, 16))
    slot16 = (C.c_int * 16)(*range(16))
    head = (h, n, _ptr(acc), 16, ng, _lib.PLOO_ELL, None, None)
    tail = (_ptr(st.work), st.work.numel())

    def ploo_finish():
        out2.copy_(out)
        _lib.check(lib.bfhip_ploo_finish(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out2), *tail))

    stages = [('fun_columns', lambda: rm.fun_columns(x, 0, 16, lo, diff, out=zbuf)),
              ('lgo_accum', lambda: _lib.check(lib.bfhip_lgo_accum(h, n, _ptr(zbuf), 16, 16, slot16, cc, 0xffff, _ptr(scratch), 16))),
              ('moments', lambda: _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), *tail))),
              ('tail', lambda: _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(st.keys), _ptr(st.idx), *tail))),
              ('lgo_finish', lambda: _lib.check(lib.bfhip_lgo_finish(h, n, _ptr(acc), 16, ng, cc, dd, None, _ptr(st.keys), _ptr(st.idx), _ptr(out),
                                                                     _ptr(lgo), *tail))),
              ('ploo_finish', ploo_finish)]
    for name, fn in stages:
        fn()
    best = {}
    for rep in range(args.reps):
        row = {}
        for name, fn in stages:
            row[name], _ = _wall(fn, torch)
            best[name] = min(best.get(name, np.inf), row[name])
        print(json.dumps(dict(shape, what='stages: 16 columns, one batch of %d groups' % ng, rep=rep, **row)), flush=True)
    del scratch, acc, zbuf

    # the route that existed before: z of every group materialised, torch row sums, pointwise_loo, psis() and torch's gammaincc per group
    def old_route():
        ell = ctx.empty((n_chain, n_draw, len(groups)))
        qs = []
        for k, grp in enumerate(groups):
            b = len(grp)
            zg = ctx.empty((n_chain, n_draw, b))
            for k0 in range(0, b, 16):
                rm.fun_columns(x, int(first[k]) + k0, min(16, b - k0), lo, diff, out=zg[:, :, k0:])
            q = (zg * zg).sum(dim=2)
            del zg
            ell[:, :, k] = const[k] - 0.5 * q
            qs.append(q)
        loo = pointwise_loo(ell)
        chi2, ppp = np.zeros(len(groups)), np.zeros(len(groups))
        for k, q in enumerate(qs):
            wgt = torch.exp(psis(-ell[:, :, k]).log_weights.reshape(-1))
            qf = q.reshape(-1)
            big_q = torch.special.gammaincc(torch.full_like(qf, 0.5 * len(groups[k])), 0.5 * qf)
            chi2[k], ppp[k] = float((wgt * qf).sum()), float((wgt * big_q).sum())
        return loo, chi2, ppp

    old_route()   # warm-up
    old = []
    for rep in range(args.reps):
        t, (loo, chi2, ppp) = _wall(old_route, torch)
        old.append(t)
        print(json.dumps(dict(shape, what='fun_columns + row sums + pointwise_loo + psis() + torch gammaincc', rep=rep, seconds=t)), flush=True)
    print(json.dumps(dict(shape, what='summary', data_lgo=min(whole), old_route=min(old), ratio_old_over_new=min(old) / min(whole),
                          fun_columns_16=best['fun_columns'], lgo_accum_16=best['lgo_accum'], moments_batch=best['moments'],
                          tail_batch=best['tail'], lgo_finish_batch=best['lgo_finish'], ploo_finish_batch=best['ploo_finish'],
                          khat_max_abs_difference=float(np.nanmax(np.abs(loo.khat - res.khat))),
                          elpd_max_abs_difference=float(np.nanmax(np.abs(loo.elpd_loo - res.elpd_lgo))),
                          ppp_max_abs_difference=float(np.nanmax(np.abs(ppp - res.ppp_lgo))),
                          chi2_max_rel_difference=float(np.nanmax(np.abs(chi2 / res.chi2_lgo - 1.))))), flush=True)


if __name__ == '__main__':
    main()
