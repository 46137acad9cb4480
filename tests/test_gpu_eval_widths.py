"""bfhip_logp_grad and bfhip_leapfrog (csrc/bfhip_eval.hip) through the C ABI, at every padded width and LDS layout, across the
grid-stride loop and on the pipeline density's two-dimensions-per-lane step -- against the extended-precision reference of
helpers/eval_reference.py, with tolerances K 2^-52 scale (``ROUNDING`` of helpers/eval_cases.py; test_eval_reference_host.py
measures K and shows that the comparison sees one entry wrong by 1e-9).  There is no free-standing absolute tolerance.

Which instantiation a case runs, from the dispatch of bfhip_logp_grad / bfhip_leapfrog:

    d = 2, 16 | 17, 32 | 33, 64    bf_*_kernel<T = 1 | 2 | 4, staged>; 'quadratic', 'su_folded' (folded at upload) are the plain
                                   instantiation, every other feature set the general one
    d = 65, 127                    'quadratic', 'su_folded': bf_*_coop128_kernel; everything else -- 'link' and the four derived
                                   sets included, which are not the common surrogate -- bf_*_kernel<8, unstaged, general>

and which LDS layout of bf_stage_model (pd | S | H | Hd, a matrix left out where its feature is off, the cubic stage behind) at the
staged widths d <= 64:

    pd S H           'quadratic', 'link', 'su_*', 'transform'        pd S H Hd      'decay_own', 'transform_decay_link'
    pd S H + stage   'cubic', 'su_kept_cubic'                        all of them    'everything'
    pd S             'no_bound' (nothing behind the gap)             pd             'linear_only' (an all-linear surrogate never
    pd H + stage     'cubic_no_quad': H in S's place, the stage                     applies its bound)
                     one matrix earlier                              pd S Hd        'decay_no_bound': Hd in H's place

('decay_shared' uploads the bound's own matrix as the decay term's.)  At d = 65 and 127 nothing is staged; the same specs run the
general instantiation's global-memory path there.

Every test prints its largest error in units of 2^-52 scale next to K before it asserts.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import eval_cases as ec  # noqa: E402
import eval_reference as er  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = ec.GUARD


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


# ---- plumbing: guarded device arrays and the two C entry points ------------------------------------------------------------------
def guarded(ctx, a=None, shape=None):
    """A device array of shape (n + GUARD, ...) whose first n rows hold ``a`` (or, with ``shape``, the NaN payload too: an output)
    and whose guard rows hold ec.NAN_BITS."""
    import torch
    a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    shape = a.shape if a is not None else shape
    host = np.full((shape[0] + GUARD,) + tuple(shape[1:]), ec.NAN_BITS, dtype=np.uint64)
    if a is not None:
        host[:shape[0]] = a.view(np.uint64)
    return ctx.tensor(host.view(np.int64), torch.int64).view(torch.float64)   # (moved as integers: the payload's bits arrive as they are)


def fetch(t, n):
    """(the first n rows, whether the guard rows still hold the payload)"""
    import torch
    host = t.view(torch.int64).cpu().numpy().view(np.float64)
    return host[:n].copy(), bool(np.all(host[n:].view(np.uint64) == ec.NAN_BITS))


def run_logp_grad(ctx, n, x, original_space, with_grad=True):
    """bfhip_logp_grad on the current density: (logp (n,), grad (n, d) or None, guards intact)"""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    d = x.shape[1]
    xt = ctx.tensor(np.ascontiguousarray(x), torch.float64)
    lp, g = guarded(ctx, shape=(n,)), (guarded(ctx, shape=(n, d)) if with_grad else None)
    _lib.check(ctx._lib.bfhip_logp_grad(ctx.handle, n, _ptr(xt), int(original_space), _ptr(lp), _ptr(g)))
    ctx.synchronize()
    lp, ok = fetch(lp, n)
    if with_grad:
        g, ok2 = fetch(g, n)
        ok = ok and ok2
    return lp, g, ok


def run_leapfrog(ctx, st, with_velocity=True):
    """bfhip_leapfrog on the current density: ({q, p, grad, logp, energy[, v]}, guards intact)"""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    n, d = st['q'].shape
    q, p, g = (guarded(ctx, st[k]) for k in ('q', 'p', 'grad'))
    lp, en = guarded(ctx, shape=(n,)), guarded(ctx, shape=(n,))
    v = guarded(ctx, shape=(n, d)) if with_velocity else None
    eps, var = ctx.tensor(np.ascontiguousarray(st['eps']), torch.float64), ctx.tensor(np.ascontiguousarray(st['var']), torch.float64)
    _lib.check(ctx._lib.bfhip_leapfrog(ctx.handle, n, _ptr(eps), _ptr(var), _ptr(q), _ptr(p), _ptr(g), _ptr(lp), _ptr(en), _ptr(v)))
    ctx.synchronize()
    out, ok = {}, True
    for k, t in (('q', q), ('p', p), ('grad', g), ('logp', lp), ('energy', en)) + ((('v', v),) if with_velocity else ()):
        out[k], intact = fetch(t, n)
        ok = ok and intact
    return out, ok


def same_bits(a, b):
    return a.shape == b.shape and bool(np.all(np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)))


# ---- 1. evaluation matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.EVAL_FEATURES)
@pytest.mark.parametrize('d', ec.WIDTHS)
def test_logp_grad_every_width_and_feature_set(ctx, d, name):
    """53 points (a tile inside the bound, one with a single point outside, one outside, a ragged mixed one; with a decay term on
    both sides of its surface and between the two), both spaces where the spec has a transform: logp and gradient within
    K 2^-52 scale of the reference, the 16 guard rows past n untouched, and logp the same bits without a gradient."""
    from bayesfast_amd.device import DeviceDensity
    spec = ec.spec_for(d, name)
    xo, xs, outside = ec.eval_points(d, name)
    ec.check_eval_inputs(spec, xo, xs, outside)
    DeviceDensity(spec, ctx)
    K = ec.rounding_for(d)
    failures = []
    for x, original in ([(xo, False)] if xs is None else [(xo, True), (xs, False)]):
        label = 'eval d=%d %s %s' % (d, name, 'original' if original else 'sampling')
        lp, g, intact = run_logp_grad(ctx, ec.N_EVAL, x, original)
        lp_only, _, intact2 = run_logp_grad(ctx, ec.N_EVAL, x, original, with_grad=False)
        _, bad = ec.compare(label, ec.eval_parts(lp, g, er.logp_and_grad(spec, x, original_space=original)), K)
        failures += [(label, b) for b in bad]
        if not (intact and intact2):
            failures.append((label, 'guard rows written'))
        if not same_bits(lp, lp_only):
            failures.append((label, 'logp differs without a gradient'))
    assert not failures, failures


# ---- 2. leapfrog matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.LEAPFROG_FEATURES)
@pytest.mark.parametrize('d', ec.WIDTHS)
def test_leapfrog_every_width_and_feature_set(ctx, d, name):
    """37 chains, per-chain step sizes of both signs (one exactly 0), per-chain and per-dimension variances, with and without
    velocity_out: q, p, grad, logp, energy and velocity within K 2^-52 scale of the reference step, the chain with eps = 0 keeps q
    and p bit for bit, guard rows intact on every in/out array."""
    from bayesfast_amd.device import DeviceDensity
    spec, st = ec.spec_for(d, name), ec.leapfrog_state(d, name)
    assert st['eps'][7] == 0. and (st['eps'] > 0).any() and (st['eps'] < 0).any()
    DeviceDensity(spec, ctx)
    K = ec.rounding_for(d)
    ref = er.leapfrog(spec, st['var'], st['eps'], st['q'], st['p'], st['grad'])
    failures = []
    first = None
    for with_velocity in (True, False):
        label = 'leapfrog d=%d %s %s' % (d, name, 'velocity' if with_velocity else 'no velocity')
        got, intact = run_leapfrog(ctx, st, with_velocity)
        _, bad = ec.compare(label, ec.leapfrog_parts(got, ref, velocity=with_velocity), K)
        failures += [(label, b) for b in bad]
        if not intact:
            failures.append((label, 'guard rows written'))
        if not (same_bits(got['q'][7], st['q'][7]) and same_bits(got['p'][7], st['p'][7])):
            failures.append((label, 'the chain with eps = 0 moved'))
        if first is None:
            first = got
        elif not all(same_bits(first[k], got[k]) for k in got):
            failures.append((label, 'the step depends on velocity_out'))
    assert not failures, failures


# ---- 3. the grid-stride loop -------------------------------------------------------------------------------------------------------
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def stride_case(kind):
    """(spec, n, first row of the second pass, sampling-space points (n, d), K): the smallest batch whose last tiles a wave reaches
    on its second trip through ``for (tile ...; tile += gridDim.x * waves)``."""
    from bayesfast_amd.workloads import correlated_gaussian_spec
    cu = n_cu()
    if kind == 'coop100':      # bf_*_coop128_kernel: min(n_tiles, n_cu) workgroups of one tile each
        spec, _ = correlated_gaussian_spec(100)
        n, second = 16 * cu + 21, 16 * cu
        rng = np.random.default_rng(4100)
        x = rng.normal(size=(n, 100)) * rng.choice([0.9, 1.9], size=n)[:, None]
        po = spec['poly']
        beta = np.sqrt(np.einsum('ni,ij,nj->n', x - po['mu'], po['hess'], x - po['mu']))
        out = beta > po['alpha']
    else:                      # bf_*_kernel: at most 2 n_cu workgroups of four waves, a tile per wave
        d, name = {'plain16': (16, 'quadratic'), 'general17': (17, 'everything')}[kind]
        spec = ec.spec_for(d, name)
        n, second = 128 * cu + 69, 128 * cu
        rng = np.random.default_rng(4000 + d)
        rho = rng.choice(ec.INSIDE + ec.OUTSIDE, size=n)
        xo = ec.ray_points(spec, rho, rng)
        x = ec.lc.from_original(spec, xo) if ec.has_transform(spec) else xo
        out = ec.lc.bound_ratio(spec, x, False)[0] > 1.
    for rows in (slice(0, 16), slice(second, n)):   # both branches in the first tile and on the second pass
        assert out[rows].any() and not out[rows].all()
    assert np.all(np.abs(x) < 12.)
    return spec, n, second, x, ec.rounding_for(int(spec['d']))


def stride_rows(n, second, rng):
    """(the rows evaluated again in a batch of their own, reversed: the first tile, every tile of the second pass -- the last two
    tiles among them; about 300 rows for the reference: those and a spread over the first pass)"""
    again = np.concatenate((np.arange(16), np.arange(second, n)))[::-1].copy()
    assert second + 16 < n and n - second < 5 * 16   # more than one tile, and fewer than a full round, on the second pass
    spread = np.sort(rng.choice(np.arange(16, second), size=300 - again.size, replace=False))
    return again, np.concatenate((again[::-1], spread))


@pytest.mark.parametrize('kind', ['plain16', 'general17', 'coop100'])
def test_logp_grad_second_pass_of_the_tile_loop(ctx, kind):
    """bf_logp_grad_kernel (plain at d = 16, general with the cubic stage at d = 17) at n = 128 n_cu + 69 and
    bf_logp_grad_coop128_kernel (d = 100) at n = 16 n_cu + 21: the rows of the first tile and of every tile reached on the second
    pass come back bit-identical from a batch of their own in reversed order (a result does not depend on tile, lane or pass), 300
    rows over both passes are within tolerance of the reference, guard rows intact."""
    from bayesfast_amd.device import DeviceDensity
    spec, n, second, x, K = stride_case(kind)
    again, check = stride_rows(n, second, np.random.default_rng(1))
    DeviceDensity(spec, ctx)
    lp, g, intact = run_logp_grad(ctx, n, x, False)
    lp2, g2, intact2 = run_logp_grad(ctx, again.size, x[again], False)
    _, bad = ec.compare('stride eval %s n=%d' % (kind, n), ec.eval_parts(lp[check], g[check], er.logp_and_grad(spec, x[check])), K)
    assert not bad, bad
    assert intact and intact2
    assert same_bits(lp[again], lp2) and same_bits(g[again], g2), 'a point\'s result depends on where in the batch it sits'


@pytest.mark.parametrize('kind', ['plain16', 'general17', 'coop100'])
def test_leapfrog_second_pass_of_the_tile_loop(ctx, kind):
    """The same for bf_leapfrog_kernel and bf_leapfrog_coop128_kernel: per-chain step sizes and variances, velocity written."""
    from bayesfast_amd.device import DeviceDensity
    spec, n, second, q, K = stride_case(kind)
    again, check = stride_rows(n, second, np.random.default_rng(2))
    d = q.shape[1]
    rng = np.random.default_rng(3)
    st = dict(q=q, p=rng.normal(size=(n, d)), var=rng.uniform(0.5, 2., size=(n, d)),
              eps=rng.uniform(0.02, 0.12, size=n) * rng.choice([-1., 1.], size=n))
    DeviceDensity(spec, ctx)
    _, g0, _ = run_logp_grad(ctx, n, q, False)    # the start gradient: an input (whatever it is, both sides take the same one)
    st['grad'] = g0
    sub = lambda rows: {k: np.ascontiguousarray(v[rows]) for k, v in st.items()}
    got, intact = run_leapfrog(ctx, st)
    got2, intact2 = run_leapfrog(ctx, sub(again))
    c = sub(check)
    ref = er.leapfrog(spec, c['var'], c['eps'], c['q'], c['p'], c['grad'])
    _, bad = ec.compare('stride leapfrog %s n=%d' % (kind, n), ec.leapfrog_parts({k: v[check] for k, v in got.items()}, ref), K)
    assert not bad, bad
    assert intact and intact2
    for k in got:
        assert same_bits(got[k][again], got2[k]), 'a chain\'s %s depends on where in the batch it sits' % k


# ---- 4. the pipeline density's step at d > 64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,d,nq', [(40, 96, 6), (100, 128, 9)])
def test_pipeline_leapfrog_step_beyond_64_inputs(ctx, m, d, nq):
    """bf_leapfrog_half_kernel<2> (two dimensions per lane) around the pipeline density's evaluation, behind the transform: n = 45
    and n = 1 .. 5 chains (the last workgroup of four waves part-empty), per-chain step sizes and variances, against the oracle's
    step at the tolerances of test_gpu_pipeline.py::test_pipeline_leapfrog_step_matches_the_oracle (a long-double pipeline
    reference is out of scope); velocity, logp and energy too, guard rows intact."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.workloads import random_pipeline_spec
    from oracle import oracle as orc
    spec = random_pipeline_spec(m, d, nq, seed=m + d, transform=True)
    DeviceDensity(spec, ctx)
    rng = np.random.default_rng(m)
    worst = {}
    for n in (45, 1, 2, 3, 4, 5):
        q, p = rng.normal(size=(n, d)) * 0.4, rng.normal(size=(n, d))
        st = dict(q=q, p=p, var=rng.uniform(0.5, 2., size=(n, d)), eps=rng.uniform(0.02, 0.05, size=n) * rng.choice([-1., 1.], size=n),
                  grad=orc.logp_and_grad(spec, q)[1])
        got, intact = run_leapfrog(ctx, st)
        assert intact, n
        rows = [orc.leapfrog(spec, st['var'][i], st['eps'][i], q[i], p[i], st['grad'][i]) for i in range(n)]
        want = {k: np.array([r[k] for r in rows]) for k in got}
        tol = dict(q=(1e-10, 1e-11), p=(1e-9, 1e-9), grad=(1e-9, 1e-8), v=(1e-9, 1e-9), logp=(1e-10, 1e-9), energy=(1e-10, 1e-9))
        for k, (rtol, atol) in tol.items():
            worst[k] = max(worst.get(k, 0.), float(np.max(np.abs(got[k] - want[k]) / (atol + rtol * np.abs(want[k])))))
    print('pipeline step m=%d d=%d: largest error as a fraction of the tolerance  %s' % (m, d, '  '.join('%s %.3g' % kv for kv in worst.items())))
    assert all(np.isfinite(v) and v <= 1. for v in worst.values()), worst
