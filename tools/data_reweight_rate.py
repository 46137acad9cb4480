#!/usr/bin/env python3
"""The posterior reweighted to alternative data vectors (bayesfast_amd/utils/reweight.py, csrc/bfhip_rw.h) at the DES shape: 27 inputs,
457 outputs, 4096 chains x 1000 draws, K = 64 data vectors (``make_density`` of tools/predictive_rate.py and the seeded draws of
tools/data_loo_rate.py; data vector k is the data moved by J L u_k s_k, which moves the Laplace posterior by s_k = 0.05 .. 0.5 sd along
the unit direction u_k).

  - ``data_reweight`` on the pipeline density: wall clock around a synchronise after a warm-up call, ``--reps`` times;
  - its stages on one batch of 16 scenarios, each timed on its own (synchronised): the ratio model's ``fun_columns``,
    ``bfhip_ploo_moments``, ``bfhip_ploo_tail``, ``bfhip_rw_finish``; beside them ``bfhip_ploo_finish`` on the same batch and a plain
    pass over the draws (``bfhip_wstat_columns`` + ``bfhip_wstat_moments`` on the 27 parameters under one set of weights);
  - the route without the new stage, per scenario: ``fun_columns`` on a one-output ratio model, ``psis()`` (a full sort) and
    ``weighted_summary()`` (a sort per parameter), timed on ``--baseline`` scenarios and scaled to K;
  - the ratio of the two, and the largest differences of khat and of the means between the two routes.

  python3 tools/data_reweight_rate.py [--reps 3] [--baseline 2] [--small]     one JSON line per measurement

No threshold is set.  ``--small`` runs 256 x 250 draws, 40 outputs and K = 20 (a check that the tool runs)."""
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
    ap.add_argument('--baseline', type=int, default=2)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    import torch
    from predictive_rate import make_density
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel, polymodel_dense_from_poly, linear_dense, _ptr
    from bayesfast_amd.utils import data_reweight, psis, weighted_summary
    from bayesfast_amd.utils.reweight import ratio_coefficients, _Stages
    d, m, n_chain, n_draw, big_k = (27, 40, 256, 250, 20) if args.small else (27, 457, 4096, 1000, 64)
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
    rng = np.random.default_rng(3)
    u = rng.standard_normal((big_k, d))
    u *= (np.linspace(0.05, 0.5, big_k) / np.sqrt((u * u).sum(axis=1)))[:, None]
    y_new = den._y + (u @ chol.T) @ jac.T
    shape = dict(d=d, m=m, n_chain=n_chain, n_draw=n_draw, K=big_k, batches=(big_k + 15) // 16)
    res = data_reweight(den, x, y_new)   # warm-up of every kernel of the route
    print(str(res), file=sys.stderr)
    print(json.dumps(dict(shape, khat_max=float(np.nanmax(res.khat)), n_khat_bad=res.n_khat_bad, ess_min=float(np.nanmin(res.ess)),
                          largest_shift=float(np.nanmax(np.abs(res.shift))), largest_shift_mcse=float(np.nanmax(res.shift_mcse)))), flush=True)
    whole = []
    for rep in range(args.reps):
        t, _ = _wall(lambda: data_reweight(den, x, y_new), torch)
        whole.append(t)
        print(json.dumps(dict(shape, what='data_reweight', rep=rep, seconds=t)), flush=True)
    # the stages on the first batch
    a, b = ratio_coefficients(den._y, y_new, den._prec, den._pdiag)
    dense = polymodel_dense_from_poly(su.poly_spec())
    rm = DevicePolyModel.from_dense(linear_dense(dense, -a[:16], -b[:16]))
    ctx = rm.ctx
    lib, h = ctx._lib, ctx.handle
    nb = min(16, big_k)
    buf = ctx.empty((n_chain, n_draw, 16))
    st = _Stages(ctx, x, None)
    out = ctx.empty((_lib.PLOO_NOUT, 16))
    out2 = ctx.empty((_lib.PLOO_NOUT, 16))
    rw = ctx.empty((_lib.RW_SUMS + 2 * (1 + 2 * d), 16))
    head = (h, n, _ptr(buf), 16, nb, _lib.PLOO_ELL, None, None)
    tail = (_ptr(st.work), st.work.numel())
    w = torch.full((n,), 1. / n, dtype=torch.float64, device=x.device)
    wbuf, wout, wwork = ctx.empty((n, 16)), ctx.empty((5, 16)), ctx.empty((_lib.WSTAT_WORK,))

    def plain_pass():
        for k0 in range(0, d, 16):
            _lib.check(lib.bfhip_wstat_columns(h, n_chain, n_draw, int(x.stride(0)), int(x.stride(1)), _ptr(x), 0, 0, k0, min(16, d - k0),
                                               _ptr(w), _ptr(wbuf)))
            _lib.check(lib.bfhip_wstat_moments(h, n, _ptr(wbuf), _ptr(w), None, _ptr(wout), _ptr(wwork)))

    def ploo_finish():
        out2.copy_(out)
        _lib.check(lib.bfhip_ploo_finish(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out2), *tail))

    stages = [('fun_columns', lambda: rm.fun_columns(x, 0, nb, out=buf)),
              ('moments', lambda: _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), *tail))),
              ('tail', lambda: _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(st.keys), _ptr(st.idx), *tail))),
              ('rw_finish', lambda: _lib.check(lib.bfhip_rw_finish(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out), *tail, n_chain, n_draw,
                                                                   int(x.stride(0)), int(x.stride(1)), _ptr(x), 0, 0, d, _ptr(st.centre),
                                                                   _ptr(rw), _ptr(st.rw_work), st.rw_work.numel()))),
              ('ploo_finish', ploo_finish), ('plain_pass', plain_pass)]
    for name, fn in stages:
        fn()
    best = {}
    for rep in range(args.reps):
        row = {}
        for name, fn in stages:
            row[name], _ = _wall(fn, torch)
            best[name] = min(best.get(name, np.inf), row[name])
        print(json.dumps(dict(shape, what='stages of one batch', rep=rep, **row)), flush=True)
    # the route without the new stage, scenario by scenario
    lo = diff = None
    if su._input_scales is not None:
        lo = ctx.tensor(np.ascontiguousarray(su._input_scales[:, 0]), torch.float64)
        diff = ctx.tensor(np.ascontiguousarray(su._input_scales_diff), torch.float64)

    def old_route(k):
        one = DevicePolyModel.from_dense(linear_dense(dense, a[k:k + 1], b[k:k + 1]))
        l = one.fun_columns(x, 0, 1, lo, diff)
        ps = psis(l)
        return ps, weighted_summary(x, log_weights=ps.log_weights.reshape(n_chain, n_draw))

    ks = list(range(big_k - 1, big_k - 1 - args.baseline, -1))
    old_route(ks[0])   # warm-up
    old = []
    dk = dm = 0.
    for k in ks:
        t, (ps, tab) = _wall(lambda: old_route(k), torch)
        old.append(t)
        dk = max(dk, abs(ps.khat - res.khat[k]))
        dm = max(dm, float(np.max(np.abs(tab['mean'] - res.mean[k]) / res.sd_base)))
        print(json.dumps(dict(shape, what='fun_columns + psis() + weighted_summary() of one scenario', scenario=k, seconds=t)), flush=True)
    print(json.dumps(dict(shape, what='summary', data_reweight=min(whole), old_route_one_scenario=min(old), old_route_all=min(old) * big_k,
                          ratio_old_over_new=min(old) * big_k / min(whole), rw_finish_batch=best['rw_finish'],
                          ploo_stages_batch=best['moments'] + best['tail'], ploo_finish_batch=best['ploo_finish'],
                          plain_pass=best['plain_pass'], khat_max_abs_difference=float(dk), mean_max_difference_in_sd=dm)), flush=True)


if __name__ == '__main__':
    main()
