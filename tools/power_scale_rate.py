#!/usr/bin/env python3
"""Power-scaling sensitivity (bayesfast_amd/utils/power_scale.py, csrc/bfhip_pscale.h, csrc/bfhip_pscale.hip) at the DES shape: 27
inputs, 457 outputs, 4096 chains x 1000 draws (``make_density`` of tools/predictive_rate.py with a Gaussian prior of one Laplace sd on
the 20 last inputs, and the seeded Laplace draws of tools/data_reweight_rate.py without that prior).

  - ``Chi2PipelineDensity.power_scale`` as called by default (likelihood and prior at two powers: one batch of 4 scenarios) and with
    ``prior_each=True`` (22 components: three batches): wall clock around a synchronise after a warm-up call, ``--reps`` times;
  - the stages on one batch of 16 scenarios, each timed on its own (synchronised): ``bfhip_rw_weights``, one ``bfhip_diag_sort``, one
    ``bfhip_pscale_cjs``; beside them ``bfhip_rw_finish`` and ``bfhip_wstat_cumweights``, the one-column scan of the same shape;
  - the same ECDF distance of the 16 columns through ``torch`` on the same GPU (``u[order]``, ``torch.cumsum``, elementwise), with the
    largest difference of cjs between the two;
  - the ratio of the two.

  python3 tools/power_scale_rate.py [--reps 3] [--small]     one JSON line per measurement

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


def torch_cjs(torch, keys_val, order, n_pos, w, u):
    """cjs (16,) of the definitions by torch's own kernels: a gather of the rows, two running sums, elementwise terms"""
    o = order[:n_pos].long()
    wp, up = w[o], u[o]
    big_p = torch.cumsum(wp, 0)[:-1, None]
    big_d = torch.cumsum(up - wp[:, None], 0)[:-1]
    h = (keys_val[1:n_pos] - keys_val[:n_pos - 1])[:, None]
    tot = big_p + (big_p + big_d)
    t = torch.clamp(big_d / tot, -1., 1.)
    a, b = 1. - t, 1. + t
    zero = torch.zeros_like(t)
    f = torch.where(a == 0, zero, a * torch.log1p(-t)) + torch.where(b == 0, zero, b * torch.log1p(t))
    return torch.sqrt((h * (0.5 * tot) * f).sum(0) / np.log(2.) / (h * tot).sum(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    import torch
    from predictive_rate import make_density
    from bayesfast_amd import _lib, Chi2PipelineDensity
    from bayesfast_amd.device import _ptr
    from bayesfast_amd.utils.reweight import _Stages
    d, m, n_chain, n_draw = (27, 40, 256, 250) if args.small else (27, 457, 4096, 1000)
    su, den0, poly = make_density(d, m, 11 + d)
    lin, quad, mu = poly['configs'][0]['coef'], poly['configs'][1]['coef'], poly['mu']
    qu = np.triu(np.ones((d, d))) * quad
    jac = lin[:, 1:] + np.einsum('oij,j->oi', qu + np.transpose(qu, (0, 2, 1)), mu)
    cov = np.linalg.inv(jac.T @ (den0._pdiag[:, None] * jac))
    chol = np.linalg.cholesky(cov)
    centre = mu + cov @ (jac.T @ (den0._pdiag * (den0._y - poly['f_mu'])))
    prior_prec = np.where(np.arange(d) >= d - 20, 1. / np.diag(cov), 0.)
    den = Chi2PipelineDensity(su, den0._y, prec_diag=den0._pdiag, prior_mu=centre + 0.5 * np.sqrt(np.diag(cov)), prior_prec=prior_prec)
    g = torch.Generator(device='cuda').manual_seed(5)
    z = torch.randn((n_chain * n_draw, d), generator=g, device='cuda', dtype=torch.float64)
    x = (torch.as_tensor(centre, device='cuda') + z @ torch.as_tensor(chol.T.copy(), device='cuda'))
    x = x.reshape(n_chain, n_draw, d).contiguous()
    del z
    n = n_chain * n_draw
    shape = dict(d=d, m=m, n_chain=n_chain, n_draw=n_draw)
    calls = {}
    for name, kw in (('power_scale', {}), ('power_scale, prior_each', dict(prior_each=True))):
        res = den.power_scale(x, **kw)   # warm-up of every kernel of the route
        print(str(res), file=sys.stderr)
        print(json.dumps(dict(shape, what=name, components=len(res.names), scenarios=int(res.khat.size), khat_max=float(np.nanmax(res.khat)),
                              largest_sensitivity={k: float(np.nanmax(res.sensitivity[i])) for i, k in enumerate(res.names[:2])},
                              diagnosed=sum(v != '-' for v in res.diagnosis))), flush=True)
        for rep in range(args.reps):
            t, _ = _wall(lambda: den.power_scale(x, **kw), torch)
            calls[name] = min(calls.get(name, np.inf), t)
            print(json.dumps(dict(shape, what=name, rep=rep, seconds=t)), flush=True)
    # the stages on one batch of 16 scenarios: the prior of 8 inputs at two powers
    from bayesfast_amd.device import get_context
    ctx = get_context(x.device.index)
    lib, h = ctx._lib, ctx.handle
    st = _Stages(ctx, x, None)
    xf = x.reshape(n, d)
    each = -0.5 * torch.as_tensor(prior_prec[-8:], device='cuda') * (xf[:, -8:] - torch.as_tensor(den._prior_mu[-8:], device='cuda'))**2
    buf = ctx.empty((n, 16))
    buf[:, :8], buf[:, 8:] = 0.01 * each, -0.01 * each   # -l of the powers 0.99 and 1.01
    out = ctx.empty((_lib.PLOO_NOUT, 16))
    rw = ctx.empty((_lib.RW_SUMS + 2 * (1 + 2 * d), 16))
    u, wout, cout = ctx.empty((n, 16)), ctx.empty((_lib.RWW_NOUT, 16)), ctx.empty((_lib.CJS_NOUT, 16))
    col, cum = ctx.empty((n, 16)), ctx.empty((n,))
    keys, order = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int32)
    work = ctx.empty((max(_lib.pscale_work(n), (n + _lib.WSTAT_TILE - 1) // _lib.WSTAT_TILE),))
    head = (h, n, _ptr(buf), 16, 16, _lib.PLOO_ELL, None, None)
    tail = (_ptr(st.work), st.work.numel())
    _lib.check(lib.bfhip_ploo_moments(*head, _ptr(out), *tail))
    _lib.check(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(st.keys), _ptr(st.idx), *tail))
    _lib.check(lib.bfhip_wstat_columns(h, n_chain, n_draw, int(x.stride(0)), int(x.stride(1)), _ptr(x), 0, 0, d - 16, 16, _ptr(st.w), _ptr(col)))
    stages = [('rw_finish', lambda: _lib.check(lib.bfhip_rw_finish(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out), *tail, n_chain, n_draw,
                                                                   int(x.stride(0)), int(x.stride(1)), _ptr(x), 0, 0, d, _ptr(st.centre),
                                                                   _ptr(rw), _ptr(st.rw_work), st.rw_work.numel()))),
              ('rw_weights', lambda: _lib.check(lib.bfhip_rw_weights(*head, _ptr(st.keys), _ptr(st.idx), _ptr(out), *tail, _ptr(u), 16,
                                                                     _ptr(wout)))),
              ('diag_sort', lambda: _lib.check(lib.bfhip_diag_sort(h, n, _ptr(col), 15, _ptr(keys), _ptr(order)))),
              ('pscale_cjs', lambda: _lib.check(lib.bfhip_pscale_cjs(h, n, _ptr(keys), _ptr(order), _ptr(st.wsum), _ptr(st.w), _ptr(u), 16,
                                                                     16, _ptr(cout), _ptr(work)))),
              ('wstat_cumweights', lambda: _lib.check(lib.bfhip_wstat_cumweights(h, n, _ptr(order), _ptr(st.w), _ptr(cum), _ptr(work))))]
    for name, fn in stages:
        fn()
    vals = col[:, 15][order.long()]
    stages.append(('torch', lambda: torch_cjs(torch, vals, order, n, st.w, u)))
    ref = stages[-1][1]()
    fn = dict(stages)['pscale_cjs']
    fn()
    diff = float((cout[_lib.CJS_ROWS.index('cjs')] / ref - 1.).abs().max())
    best = {}
    for rep in range(args.reps):
        row = {}
        for name, fn in stages:
            row[name], _ = _wall(fn, torch)
            best[name] = min(best.get(name, np.inf), row[name])
        print(json.dumps(dict(shape, what='stages of one batch', rep=rep, **row)), flush=True)
    gathered = 2. * n * (128 + 8 + 4 + 8)   # two passes over the rows of u with w, the permutation and the keys
    print(json.dumps(dict(shape, what='summary', power_scale=calls['power_scale'], power_scale_prior_each=calls['power_scale, prior_each'],
                          rw_weights_batch=best['rw_weights'], rw_finish_batch=best['rw_finish'], diag_sort=best['diag_sort'],
                          pscale_cjs=best['pscale_cjs'], wstat_cumweights=best['wstat_cumweights'], torch_cjs=best['torch'],
                          ratio_torch_over_kernel=best['torch'] / best['pscale_cjs'], pscale_cjs_tb_per_s=gathered / best['pscale_cjs'] / 1e12,
                          cjs_max_relative_difference=diff)), flush=True)


if __name__ == '__main__':
    main()
