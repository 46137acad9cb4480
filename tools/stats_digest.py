#!/usr/bin/env python3
"""One SHA-256 per output array of every entry point of the post-sampling statistics kernels (csrc/bfhip_sit.hip's evidence part and
polar factor, bfhip_refit.hip, bfhip_acor.hip, bfhip_diag.hip, bfhip_psis.hip) on seeded inputs: sizes 1, 255, 256, 257 and one past
each grid cap (65537, 131073, 262145); NaN of both signs, +-inf, -inf only, ties, columns of -0.0 and of a constant, zero weights.
Every reduction there has an order fixed by the shape, so two builds that compute the same thing print the same JSON:

  BFHIP_LIBRARY=<other libbfhip.so> python3 tools/stats_digest.py > a.json;  python3 tools/stats_digest.py > b.json;  cmp a.json b.json"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bayesfast_amd import _lib
from bayesfast_amd.device import get_context, _ptr

SIZES, KINDS, W = (1, 255, 256, 257, 65537, 131073, 262145), ('plain', 'special', 'ninf', 'minf'), _lib.DIAG_BATCH
f64, f32, i64, i32 = torch.float64, torch.float32, torch.int64, torch.int32
ctx, rng, OUT = get_context(0), np.random.default_rng(7), {}


def dev(a, dt=f64):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda').to(dt)


def zeros(*shape, dt=f64):
    return torch.zeros(shape, dtype=dt, device='cuda')


def call(name, *args):
    args = [_ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *args))


def put(key, *arrays):
    for i, a in enumerate(arrays):
        OUT['%s/%d' % (key, i)] = hashlib.sha256(a.cpu().numpy().tobytes()).hexdigest()


def vec(n, kind='plain'):
    """n normal values; all but 'plain' rounded (ties); 'special' holds both NaNs, both infinities and -0, 'ninf' only -inf"""
    v = np.round(rng.normal(size=n), 12 if kind == 'plain' else 2)
    if kind == 'special':
        for start, step, value in ((0, 7, np.nan), (2, 9, -np.nan), (3, 11, np.inf), (5, 13, -np.inf), (6, 17, -0.0)):
            v[start::step] = value
    elif kind == 'ninf':
        v[:] = -np.inf
    elif kind == 'minf':
        v[2::5] = -np.inf
    return v


def table(n_chain, n_draw, dt):
    """(chain, draw, 20): a view strided in chain and row, with special columns in both batches of 16"""
    x = rng.normal(size=(n_chain, n_draw + 3, 23))
    v = x[:, :, 2:22]
    for col, value in ((0, -0.0), (1, 4.25), (16, -0.0), (17, 0.1)):
        v[..., col] = value
    v[..., 15] = np.round(v[..., 15], 1)
    v[..., 2] = vec(v[..., 2].size, 'special').reshape(v[..., 2].shape)
    v[:, 3::4, 3] = v[:, 2::9, 18] = -np.inf
    return dev(x, dt)[:, 1:1 + n_draw, 2:22]


def sort_columns(key, n, buf, nb, then):
    """sorts columns 0, 1, 3 and the last of the batch; ``then(b, keys, order)`` runs what follows a sort and returns its outputs"""
    keys, order = zeros(n, dt=i64), zeros(n, dt=i32)
    for b in sorted({0, min(1, nb - 1), min(3, nb - 1), nb - 1}):
        call('bfhip_diag_sort', n, buf, b, keys, order)
        put('%s/sort%d' % (key, b), keys, order, *then(b, keys, order))


for n in SIZES:
    for kind in KINDS:
        a, b, c, d = dev(vec(n, kind)), dev(vec(n + 2, kind)), dev(vec(n, kind)), dev(vec(n + 2, kind))
        out2, out3, terms, f1, f2, w, wt = zeros(2), zeros(3), zeros(n), zeros(n + 2), zeros(n), zeros(n), zeros(n)
        keys, order, lw, out8 = zeros(n, dt=i64), zeros(n, dt=i64), zeros(n), zeros(8)
        work = zeros(_lib.psis_work_bytes(n), dt=torch.uint8)
        call('bfhip_bridge_sums', n, a, n + 2, b, 0.3, out2)
        call('bfhip_bridge_terms', n, a, c, n + 2, b, d, 0.3, f1, f2)
        call('bfhip_logmeanexp_stats', n, a, c, out3, terms)
        call('bfhip_sort_keys', n, a, keys, order)
        put('flat/%d/%s' % (n, kind), out2, f1, f2, out3, terms, keys, order)
        call('bfhip_order_keys', n, c, keys)
        call('bfhip_psis', n, a, c if kind == 'plain' else None, lw, out8, work, work.numel())
        put('flat/%d/%s/psis' % (n, kind), keys, lw, out8)
        for k_trunc in (0.25, -1.):
            call('bfhip_importance_weights', n, a, c, k_trunc, w, wt)
            put('flat/%d/%s/iw%g' % (n, kind, k_trunc), w, wt)
for n in (1, 255, 256, 257, 40000):   # (40000: more than one split of the data)
    for kind in KINDS:   # dimension 0 plain, 1 and 2 of the kind; weights and points of the kind too
        data, out = dev(np.stack([vec(n), vec(n, kind), vec(n, kind)])), zeros(3, 9)
        call('bfhip_kde_cdf', 3, n, data, dev(np.abs(vec(n, kind)) / n), dev([0.3, 0.5, 1.1]), 9, dev(vec(27, kind).reshape(3, 9)), out)
        put('kde/%d/%s' % (n, kind), out)
for d in (5, 16, 64):
    for kind in ('plain', 'special'):
        X, work = zeros(d, d), zeros(2 * d * d + 32 + 11)
        call('bfhip_polar_ns', d, dev(vec(d * d, kind).reshape(d, d)), X, 32, work, work[-1:])
        put('polar/%d/%s' % (d, kind), X, work[-1:])
for h, dt in ((1, f64), (85, f32), (128, f64), (257, f64), (257, f32)):   # 6 h rows: 6, 510, 768 (3 x 256), 1542
    x, c, m = table(3, 2 * h + 1, dt), dev(rng.normal(size=W)), 6
    for k0, nb in ((0, 16), (16, 4)):
        for mode in (0, 1, 2):   # plain, |x - c|, x <= c
            key = 'diag/%d/%s/%d/%d' % (h, dt, k0, mode)
            buf, lo, hi, mean, inv = zeros(m, h, W), zeros(m, W), zeros(m, W), zeros(m, W), zeros(m, W)
            lag, work = zeros(2, 70, W), zeros(m * 70 * W)
            call('bfhip_diag_columns', 3, h, x.stride(0), x.stride(1), x, int(dt == f32), 1, k0, nb, mode, c, buf)
            call('bfhip_diag_extent', m, h, buf, lo, hi)
            call('bfhip_acor_moments', m, h, W, h * W, buf, mean, inv)
            for i, t0 in enumerate((0, 64)):
                call('bfhip_acor_lag_sums', m, h, W, h * W, buf, mean, inv, t0, 70, work, lag[i])
            put(key, buf, lo, hi, mean, inv, lag)

            def rank(b, keys, order):
                call('bfhip_diag_rank', m * h, keys, order, b, buf)
                return (buf,)
            sort_columns(key, m * h, buf, nb, rank)
x = rng.normal(size=(5, 257, 3))   # the autocorrelation time's own layout, n_d = 3; dimension 1 special, dimension 2 all -0
x[..., 1], x[..., 2] = vec(5 * 257, 'special').reshape(5, 257), -0.0
x, mean, inv, lag = dev(x), zeros(5, 3), zeros(5, 3), zeros(300, 3)
call('bfhip_acor_moments', 5, 257, 3, 257 * 3, x, mean, inv)
call('bfhip_acor_lag_sums', 5, 257, 3, 257 * 3, x, mean, inv, 0, 300, zeros(5 * 300 * 3), lag)
put('acor/5x257x3', mean, inv, lag)
for (n_chain, n_draw), dt in (((1, 1), f64), ((3, 85), f32), ((2, 128), f64), ((1, 257), f32), ((5, 52429), f64)):
    n = n_chain * n_draw
    w = np.abs(rng.normal(size=n))
    w[1::3] = 0.
    w, probs, x = dev(w / w.sum()), dev([0., 0.05, 0.5, 0.95, 1.]), table(n_chain, n_draw, dt)
    work, wsum = zeros(max(_lib.WSTAT_WORK, (n + _lib.WSTAT_TILE - 1) // _lib.WSTAT_TILE)), zeros(4)
    call('bfhip_wstat_moments', n, None, w, wsum, None, work)
    for k0, nb, wv in ((0, 16, w), (16, 4, w), (0, 16, None)):
        key = 'wstat/%d/%s/%d/%s' % (n, dt, k0, wv is None)
        buf, out, qout, cum = zeros(n, W), zeros(5, W), zeros(5, W), zeros(n)
        call('bfhip_wstat_columns', n_chain, n_draw, x.stride(0), x.stride(1), x, int(dt == f32), 0, k0, nb, wv, buf)
        call('bfhip_wstat_moments', n, buf, w, None, out, work)
        put(key, buf, out, wsum)

        def quantiles(b, keys, order):
            call('bfhip_wstat_cumweights', n, order, w, cum, work)
            call('bfhip_wstat_quantiles', n, keys, order, w, cum, wsum, 5, probs, b, qout)
            return cum, qout
        sort_columns(key, n, buf, nb, quantiles)
torch.cuda.synchronize()
print(json.dumps(OUT, indent=0, sort_keys=True))
