#!/usr/bin/env python3
"""One SHA-256 per output array (samples, statistics, sc, vec, the random state; mat under the full-rank metric; u and the weights of the
tempered kernels) of a short run of every sampler kernel family and feature set the dispatcher reaches: a few chains, 40 iterations,
n_warmup = 30, adapt_window = 5, update_window = 3, doubling -- so the metric's window rolls twice with refreshes in between and the step
size adapts throughout.  A chain's arithmetic has a fixed order, so two builds that compute the same thing print the same JSON:

  BFHIP_LIBRARY=<other libbfhip.so> python3 tools/sampler_digest.py > a.json;  python3 tools/sampler_digest.py > b.json;  cmp a.json b.json

Each entry also names the kernel that ran (`kernel`), so that the JSON shows what it covers."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bayesfast_amd import _lib
from bayesfast_amd.chains import DeviceChains
from bayesfast_amd.device import get_context, DeviceDensity
from bayesfast_amd.workloads import correlated_gaussian_spec

N_ITER, N_WARMUP, N_CHAIN = 40, 30, 5
RUN_KW = dict(n_warmup=N_WARMUP, update_window=3, doubling=True)
OUT, DEFAULTS = {}, {}


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def with_decay(spec):
    po = spec['poly']
    return dict(spec, use_decay=True, decay_mu=po['mu'] + 0.05, decay_hess=po['hess'], decay_alpha2=(0.8 * po['alpha'])**2, decay_gamma=0.1)


def with_bounds(spec):
    """behind the constraint transform: all four kinds of bounds"""
    d = spec['d']
    lo = np.full(d, -9.) + np.arange(d) * 0.01
    kinds = np.array([[1, 1], [1, 0], [0, 1], [0, 0]] * ((d + 3) // 4), dtype=np.uint8)[:d]
    return dict(spec, ranges=np.stack([lo, lo + 18.], 1), hard_bounds=kinds)


def with_cubic(spec, n2, n3, amp):
    """cubic-2 and cubic-3 configs on the first n2 and n3 inputs"""
    rng = np.random.default_rng(5)
    c3 = np.zeros((1, n3, n3, n3))
    j, k, l = np.meshgrid(*[np.arange(n3)] * 3, indexing='ij')
    c3[0][(j < k) & (k < l)] = 0.03 * amp * rng.normal(size=int(((j < k) & (k < l)).sum()))
    one = np.array([0])
    configs = list(spec['poly']['configs']) + [
        dict(order='cubic-2', input_mask=np.arange(n2), output_mask=one, coef=0.02 * amp * rng.normal(size=(1, n2, n2))),
        dict(order='cubic-3', input_mask=np.arange(n3), output_mask=one, coef=c3)]
    return dict(spec, poly=dict(spec['poly'], configs=configs))


def case(key, spec, sampler='NUTS', layout='wave', scale=1., chain_kw=None, tempered=False, expect=None, **debug):
    d = spec['d']
    rng = np.random.default_rng(2)
    x0 = rng.normal(size=(N_CHAIN, d)) * scale
    try:
        for k, v in debug.items():
            _lib.debug_set(k, v)
        dc = DeviceChains(DeviceDensity(spec, ctx), x0, seed=11, adapt_window=5,
                          **{k: v for k, v in (chain_kw or {}).items() if k != 'adapt_metric'})
        if tempered:
            out = dc.run_tempered(N_ITER, np.zeros(d), np.eye(d) * 1.5, logxi=0.2, u_0=rng.normal(size=N_CHAIN), **RUN_KW)
            out, names, kernel = out + (dc.tu,), ('samples', 'stats', 'stats_t', 'u'), _lib.last_kernel()
        else:
            kw = dict(RUN_KW, n_int_step=8, launch_iters=None, layout=layout)
            if chain_kw and 'adapt_metric' in chain_kw:
                kw['adapt_metric'] = chain_kw['adapt_metric']
            out, names, kernel = dc.run(N_ITER, sampler, **kw), ('samples', 'stats'), _lib.last_kernel()
    finally:
        for k in debug:
            _lib.debug_set(k, DEFAULTS[k])
    if expect is not None and expect not in kernel:   # (the entry's `kernel` says what ran instead)
        print('%s: expected %s, the dispatcher ran %s' % (key, expect, kernel), file=sys.stderr)
    OUT[key] = dict(kernel=kernel, **{n: sha(t) for n, t in zip(names, out)}, sc=sha(dc.sc), vec=sha(dc.vec), rng=sha(dc.rng))
    if dc.mat is not None:
        OUT[key]['mat'] = sha(dc.mat)


def main():
    global ctx
    ctx = get_context(0)
    DEFAULTS.update({k: _lib.debug_get(k) for k in ('no_group', 'no_pipe', 'lone', 'lone_form', 'wave_cpg', 'tnuts_generic')})
    g = {d: correlated_gaussian_spec(d)[0] for d in (10, 24, 40, 64, 128)}
    cov8 = correlated_gaussian_spec(8)[1]
    WAVE, SLICED = dict(no_group=1), dict(no_group=1, no_pipe=1)
    # ---- the sliced kernel ----
    for d in (10, 40, 64):
        case('sliced/plain/%d' % d, g[d], expect='bf_sampler_kernel', **SLICED)
    case('sliced/fs3', with_decay(g[64]), expect='bf_sampler_kernel', **SLICED)
    case('sliced/fs5', with_bounds(g[64]), scale=0.3, expect='bf_sampler_kernel', **SLICED)
    case('sliced/fs7', with_bounds(with_decay(g[64])), scale=0.3, expect='bf_sampler_kernel', **SLICED)
    case('sliced/generic_decay/24', with_decay(g[24]), expect='bf_sampler_kernel', **SLICED)
    case('sliced/cubic/24', with_cubic(g[24], 20, 16, 0.15), scale=0.5, expect='bf_sampler_kernel', **SLICED)
    case('sliced/cubic/128', with_cubic(g[128], 20, 16, 0.05), scale=0.5, layout='auto', expect='bf_sampler_kernel')
    case('sliced/plain/128', g[128], layout='auto', expect='bf_sampler_kernel')
    g8 = correlated_gaussian_spec(8)[0]
    case('sliced/full/adapting', g8, chain_kw=dict(metric='full'), expect='bf_sampler_kernel', **WAVE)
    case('sliced/full/fixed', g8, chain_kw=dict(metric=cov8, adapt_metric=False), expect='bf_sampler_kernel', **WAVE)
    case('sliced/full/adapting/128', g[128], chain_kw=dict(metric='full'), layout='auto', expect='bf_sampler_kernel')
    case('sliced/full/hmc', g8, sampler='HMC', chain_kw=dict(metric=cov8), expect='bf_sampler_kernel', **WAVE)
    for d in (10, 64):
        case('sliced/hmc/%d' % d, g[d], sampler='HMC', expect='bf_sampler_kernel', **WAVE)
    case('sliced/hmc/fs7', with_bounds(with_decay(g[64])), sampler='HMC', scale=0.3, expect='bf_sampler_kernel', **WAVE)
    # ---- the pipelined kernel (sixteen chains per workgroup: the latency kernel takes few chains otherwise) ----
    PIPE = dict(no_group=1, lone=0, wave_cpg=16)
    for d in (10, 24, 40, 64):
        case('pipe/plain/%d' % d, g[d], expect='bf_nuts_pipe_kernel', **PIPE)
    case('pipe/tr', with_bounds(g[64]), scale=0.3, expect='bf_nuts_pipe_kernel<4, true', **PIPE)
    case('pipe/dec1', with_decay(g[64]), expect='bf_nuts_pipe_kernel<4, false, 1', **PIPE)
    # (the decay term's centre and matrix are the bound's own arrays: one product serves both)
    case('pipe/dec2', dict(with_decay(g[64]), decay_mu=g[64]['poly']['mu']), expect='bf_nuts_pipe_kernel<4, false, 2', **PIPE)
    # ---- the latency kernel, its three forms ----
    for form in (0, 1, 2):
        for d in (10, 40):
            case('lone/form%d/%d' % (form, d), g[d], expect='bf_lone_kernel', no_group=1, lone=2, lone_form=form)
    case('lone/tr', with_bounds(g[64]), scale=0.3, expect='bf_lone_kernel', no_group=1, lone=2)
    case('lone/dec', with_decay(g[64]), expect='bf_lone_kernel', no_group=1, lone=2)
    # ---- the group kernel ----
    for d in (10, 24, 40, 64):
        case('group/nuts/%d' % d, g[d], layout='group', expect='bf_group_kernel')
    case('group/nuts/decay', with_decay(g[64]), layout='group', expect='bf_group_kernel')
    case('group/nuts/bounds', with_bounds(g[64]), layout='group', scale=0.3, expect='bf_group_kernel')
    case('group/nuts/decay_bounds', with_bounds(with_decay(g[40])), layout='group', scale=0.3, expect='bf_group_kernel')
    case('group/hmc', g[64], sampler='HMC', layout='group', expect='bf_group_kernel')
    case('group/hmc/decay_bounds', with_bounds(with_decay(g[40])), sampler='HMC', layout='group', scale=0.3, expect='bf_group_kernel')
    # ---- the split kernel: W = 1, 2, 4 ----
    for d in (10, 24, 40, 64):
        case('split/%d' % d, g[d], layout='split', expect='bf_split_kernel')
    # ---- both tempered kernels, both metrics ----
    for d in (10, 24, 64):
        case('tempered/tuned/%d' % d, g[d], tempered=True, scale=0.3, expect='bf_tnuts_kernel')
        case('tempered/generic/%d' % d, g[d], tempered=True, scale=0.3, expect='bf_tnuts_gen_kernel', tnuts_generic=1)
    case('tempered/tuned/decay_bounds', with_bounds(with_decay(g[24])), tempered=True, scale=0.3, expect='bf_tnuts_kernel<2, true, true>')
    case('tempered/generic/128', g[128], tempered=True, scale=0.3, expect='bf_tnuts_gen_kernel<8>')
    case('tempered/generic/full/adapting', g8, tempered=True, scale=0.3, chain_kw=dict(metric=cov8 * 0.9), expect='bf_tnuts_gen_kernel')
    case('tempered/generic/full/adapting/128', g[128], tempered=True, scale=0.3, chain_kw=dict(metric='full'),
         expect='bf_tnuts_gen_kernel<8>')


if __name__ == '__main__':
    try:
        main()
    finally:   # (after an error: what ran until then)
        print(json.dumps(OUT, indent=0, sort_keys=True))
