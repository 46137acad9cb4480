"""The constraint transform near its bounds, in every kernel family, against an extended-precision reference.

A posterior pressed against a hard bound puts |x_trans| at tens to hundreds.  The reference's statements (and every copy of them the
library had) lose the logistic kind's 1 - t there: T''/T' is wrong by 4e-8 at x_trans = 20 and log|T'| by 1e-3 at 30, -inf from 37.
These tests hold a point near a bound to the tolerance the suite holds a point in the middle of its range to:

    stand-alone logp / grad / leapfrog / Hessian    1e-11   (test_logp_grad_golden)
    bfhip_constraint                                 1e-14 to_original*, 1e-12 from_original*   (test_constraint_transforms_golden)
    sampler statistics and recovered gradients       1e-8    (the head tolerance of the oracle comparisons)

each relative to max(1, |reference|) per component.  The reference is ``helpers/constraint_reference.py`` (mpmath, written from the
definitions); the oracle restates the reference project's arithmetic and cannot arbitrate here.

Sampler kernels expose no gradient.  One NUTS iteration with max_treedepth = 1 and no warm-up is one leapfrog step from the start
point, q1 = q0 + s eps (p0 + s eps/2 g0) with s = +-1 the tree's direction, so g0 = 2 (q1 - q0 - s eps p0) / eps^2 where p0 is the
chain's first momentum draw (the documented xoshiro / SplitMix64 / Box-Muller stream, drawn through the oracle's generator, which
the oracle tests pin); s is the sign that reproduces the unconstrained coordinates, whose gradient the reference gives
independently.  The recovery divides the rounding of q1 (|q| <= 40: 7e-15) by eps^2 / 2 = 2e-4: 4e-11, far inside 1e-8.  A chain
whose proposal was rejected returns q0 and gives the 'logp' statistic only.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(HERE, 'helpers'),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import constraint_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_EVAL, TOL_SAMPLER = 1e-11, 1e-8
EPS = 0.02       # the leapfrog step of the sampler cases
N = 32
_cache = {}


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _err(got, ref):
    return np.abs(got - ref) / np.maximum(1., np.abs(ref))


def _case(d, su=None, limit=700.):
    """spec, points (probe values of different kinds on neighbouring lanes on every second point), reference logp and grad"""
    key = (d, su, limit)
    if key not in _cache:
        spec = cr.narrow_bounded_spec(d, input_scales=su)
        x = cr.probe_points(spec, N, limit=limit, mix_lanes=True)
        assert cr.probes_covered(spec, x, limit=limit)
        lp, g, _ = cr.logp_grad_hess(spec, x, want_hess=False)
        _cache[key] = (spec, x, lp, g)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------------
# stand-alone entry points
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,su', [(8, None), (8, 'folded'), (8, 'kept'), (20, None), (64, None), (128, None)])
def test_logp_and_grad_at_the_probe_points(ctx, d, su):
    """``bfhip_logp_grad`` in the sampling space; d = 128 behind the transform is ``launch_logp_grad<8, false>``, not the cooperative
    kernel of the plain surrogate."""
    from bayesfast_amd.device import DeviceDensity
    spec, x, rl, rg = _case(d, su)
    lp, g = DeviceDensity(spec, ctx).logp_and_grad(x)
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    el, eg = _err(lp, rl), _err(g, rg)
    print('d %d su %s: logp %.3g (point %d) grad %.3g (x = %g)' % (d, su, np.nanmax(el), np.nanargmax(el), np.nanmax(eg), x.ravel()[np.nanargmax(eg)]))
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    assert el.max() <= TOL_EVAL and eg.max() <= TOL_EVAL


def test_logp_is_not_a_finite_wrong_number_beyond_the_exponent_range(ctx):
    """|x_trans| = 800: exp(-800) is zero and so is the Jacobian; logp is -inf or NaN, never finite -- at every stand-alone entry
    point: ``logp_and_grad``, ``leapfrog`` (a step of length zero), ``logp_grad_hess`` and the pipeline density's kernel."""
    from bayesfast_amd.device import DeviceDensity

    def points(spec):
        kinds, d = cr.kinds_of(spec['hard_bounds']), int(spec['d'])
        pts = []
        for i in np.nonzero(kinds)[0][:6]:
            for v in (800., -800.):
                pts.append(np.zeros(d))
                pts[-1][i] = v
        return np.array(pts)

    spec, _, _, _ = _case(8)
    pts = points(spec)
    n = pts.shape[0]
    dd = DeviceDensity(spec, ctx)
    lp, _ = dd.logp_and_grad(pts)
    assert not np.any(np.isfinite(lp.cpu().numpy())), lp
    lp, _, _ = dd.logp_grad_hess(pts)
    assert not np.any(np.isfinite(lp.cpu().numpy())), lp
    q, p, g = ctx.tensor(pts.copy()), ctx.tensor(np.zeros((n, 8))), ctx.tensor(np.zeros((n, 8)))
    lp, _ = dd.leapfrog(ctx.tensor(np.zeros(n)), ctx.tensor(np.ones((n, 8))), q, p, g)
    assert np.array_equal(q.cpu().numpy(), pts) and not np.any(np.isfinite(lp.cpu().numpy())), lp
    pspec = _pipeline_case()
    lp, _ = DeviceDensity(pspec, ctx).logp_and_grad(points(pspec))
    assert not np.any(np.isfinite(lp.cpu().numpy())), lp


def test_leapfrog_one_step(ctx):
    """``bfhip_leapfrog`` from the probe points: q1 = q0 + eps (p0 + eps/2 g0) exactly as stated, logp and grad at q1 against the
    reference AT the q1 the kernel returns."""
    from bayesfast_amd.device import DeviceDensity
    spec, x, rl, rg = _case(8)
    d = 8
    dd = DeviceDensity(spec, ctx)
    rng = np.random.default_rng(3)
    p0 = rng.normal(size=(N, d))
    q, p, g = ctx.tensor(x.copy()), ctx.tensor(p0.copy()), ctx.tensor(rg.copy())
    eps, var = ctx.tensor(np.full(N, EPS)), ctx.tensor(np.ones((N, d)))
    logp, energy = dd.leapfrog(eps, var, q, p, g)
    q1, p1, g1, lp1 = (t.cpu().numpy() for t in (q, p, g, logp))
    np.testing.assert_allclose(q1, x + EPS * (p0 + 0.5 * EPS * rg), rtol=1e-13, atol=1e-13)
    r1, rg1, _ = cr.logp_grad_hess(spec, q1, want_hess=False)
    el, eg = _err(lp1, r1).max(), _err(g1, rg1).max()
    ep = _err(p1, p0 + 0.5 * EPS * rg + 0.5 * EPS * rg1).max()
    print('leapfrog: logp %.3g grad %.3g p %.3g' % (el, eg, ep))
    assert el <= TOL_EVAL and eg <= TOL_EVAL and ep <= TOL_EVAL
    np.testing.assert_allclose(energy.cpu().numpy(), 0.5 * np.sum(p1 * p1, axis=1) - lp1, rtol=1e-13)


def test_logp_grad_hess_at_the_probe_points(ctx):
    """``bfhip_logp_hess`` (the Laplace code's kernel) at d = 8, with the input scales kept as a device-side step too."""
    from bayesfast_amd.device import DeviceDensity
    for su in (None, 'kept'):
        spec, x, _, _ = _case(8, su)
        rl, rg, rh = cr.logp_grad_hess(spec, x)
        lp, g, h = (t.cpu().numpy() for t in DeviceDensity(spec, ctx).logp_grad_hess(x))
        el, eg, eh = _err(lp, rl).max(), _err(g, rg).max(), _err(h, rh).max()
        print('hess su %s: logp %.3g grad %.3g hess %.3g' % (su, el, eg, eh))
        assert el <= TOL_EVAL and eg <= TOL_EVAL and eh <= TOL_EVAL


def test_constraint_entry_point(ctx):
    """``bfhip_constraint``, which = 0..5.  to_original* at every probe value; from_original* on points whose t = (x - lo) / rg lies
    within a few ulp of 0 and of 1 -- finite, and equal to the reference evaluated at the t the kernel forms (the definition takes t
    as an intermediate; the difference between that t and the exact quotient is the input's conditioning, not the kernel's) -- and
    exactly on a bound, where the ``bad`` flag is set and ``SurrogateDensity.from_original`` raises."""
    import mpmath as mp
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd import PolyModel, SurrogateDensity
    spec, x, _, _ = _case(8)
    lo, hi = -1., 2.
    kinds = cr.kinds_of(spec['hard_bounds'])
    dd = DeviceDensity(spec, ctx)
    out = {w: dd.constraint(w, x).cpu().numpy() for w in ('to_original', 'to_original_grad', 'to_original_grad2')}
    ref = np.array([[[float(v) for v in cr.to_original(x[p, i], kinds[i], lo, hi)] for i in range(8)] for p in range(N)])
    for c, w in enumerate(('to_original', 'to_original_grad', 'to_original_grad2')):
        e = _err(out[w], ref[:, :, c])
        print('%s: %.3g at x = %g' % (w, e.max(), x.ravel()[np.argmax(e)]))
        assert e.max() <= 1e-14
        if c:   # the derivatives span 600 orders of magnitude at the probes: relative accuracy as well
            pr = (np.abs(x) >= 3.) & (np.abs(ref[:, :, c]) > 1e-300)
            assert np.max(np.abs(out[w][pr] - ref[:, :, c][pr]) / np.abs(ref[:, :, c][pr])) <= 1e-14
    # from_original: t a few ulp from 0 and from 1.  (The kernel, like the definition's statements, decides on the rounded t: an x one
    # ulp inside the upper bound whose quotient rounds to 1 is out of bound to both; such candidates are the on-the-bound cases.)
    xo = np.tile(0.5 * np.ones(8), (12, 1))
    edge, on_bound = [], [lo, hi]
    a, b = lo, hi
    for _ in range(8):
        a, b = np.nextafter(a, np.inf), np.nextafter(b, -np.inf)
        for v in (a, b):
            t = (v - lo) / (hi - lo)
            (edge if 0. < t < 1. else on_bound).append(v)
    assert sum(v < 0. for v in edge) >= 3 and sum(v > 0. for v in edge) >= 3
    r = 0
    for i in range(8):
        for v in edge[:6]:
            if (kinds[i] == 1) or (kinds[i] == 2 and v < 0.) or (kinds[i] == 3 and v > 0.):
                xo[r % 12, i] = v
                r += 1
    got = {w: dd.constraint(w, xo).cpu().numpy() for w in ('from_original', 'from_original_grad', 'from_original_grad2')}
    with mp.workdps(60):
        for p in range(12):
            for i in range(8):
                t = mp.mpf(float((xo[p, i] - lo) / (hi - lo)))   # the quotient as the definition's statements round it
                rg = mp.mpf(hi - lo)
                if kinds[i] == 1:
                    want = (mp.log(t / (1 - t)), 1 / (t * (1 - t)) / rg, (2 * t - 1) / (t * (1 - t))**2 / rg**2)
                elif kinds[i] == 2:
                    want = (mp.log(t), 1 / t / rg, -1 / t**2 / rg**2)
                elif kinds[i] == 3:
                    want = (mp.log(1 - t), -1 / (1 - t) / rg, -1 / (1 - t)**2 / rg**2)
                else:
                    want = (t, 1 / rg, mp.mpf(0))
                for c, w in enumerate(('from_original', 'from_original_grad', 'from_original_grad2')):
                    g, wv = got[w][p, i], float(want[c])
                    assert np.isfinite(g) and abs(g - wv) <= 1e-12 * max(1., abs(wv)), (w, p, i, xo[p, i], g, wv)
    # in the middle of the range the exact reference (no intermediate) to 1e-12
    mid = np.random.default_rng(1).uniform(-0.9, 1.9, size=(N, 8))
    gm = dd.constraint('from_original', mid).cpu().numpy()
    rm = np.array([[float(cr.from_original(mid[p, i], kinds[i], lo, hi)[0]) for i in range(8)] for p in range(N)])
    assert _err(gm, rm).max() <= 1e-12
    # exactly on the bound
    den = SurrogateDensity(PolyModel('quadratic', input_size=8, output_size=1), input_scales=spec['ranges'], hard_bounds=spec['hard_bounds'])
    for i, v in [(0, v) for v in on_bound] + [(1, lo), (2, hi)]:
        bad = np.full(8, 0.5)
        bad[i] = v
        with pytest.raises(ValueError):
            dd.constraint('from_original', bad)
        with pytest.raises(ValueError):
            den.from_original(bad)
    ok = np.full(8, 0.5)
    ok[1], ok[2] = hi + 5., lo - 5.   # (the one-sided kinds' open side)
    assert np.all(np.isfinite(dd.constraint('from_original', ok).cpu().numpy()))


def _pipeline_case():
    """``random_pipeline_spec(33, 16, 16, transform=True)`` with the hard-bound kinds cycling, and points with the probe values"""
    from bayesfast_amd.workloads import random_pipeline_spec
    spec = random_pipeline_spec(33, 16, 16, transform=True)
    spec['hard_bounds'] = np.array([[1, 1], [1, 0], [0, 1], [0, 0]], dtype=np.uint8)[np.arange(16) % 4]
    return spec


def _pipeline_reference(dens, spec, x):
    """logp and grad of the pipeline density in the sampling space: the surrogate, likelihood and prior part from the stand-alone
    kernel's ORIGINAL-space evaluation at T(x) (not under test here: no transform runs), the transform's T, T', log|T'| and T''/T'
    from the reference.  (T(x) is rounded to a double on the way: an ulp of T, 1e-16 of a smooth function's value.)"""
    n, d = x.shape
    kinds, rgs = cr.kinds_of(spec['hard_bounds']), np.asarray(spec['ranges'])
    T, J, lj, gj = (np.empty((n, d)) for _ in range(4))
    for p in range(n):
        for i in range(d):
            t = cr.to_original(x[p, i], kinds[i], rgs[i, 0], rgs[i, 1])
            l = cr.log_jac(x[p, i], kinds[i], rgs[i, 0], rgs[i, 1])
            T[p, i], J[p, i], lj[p, i], gj[p, i] = float(t[0]), float(t[1]), float(l[0]), float(l[1])
    lo, go = (t.cpu().numpy() for t in dens.logp_and_grad(T, original_space=True))
    return lo + lj.sum(1), go * J + gj


def test_pipeline_density_logp_and_grad(ctx):
    """``bfhip_pld.hip``'s stand-alone kernel in the sampling space at the probe points of every kind."""
    from bayesfast_amd.device import DeviceDensity
    spec = _pipeline_case()
    x = cr.probe_points(spec, N, mix_lanes=True)
    assert cr.probes_covered(spec, x)
    dens = DeviceDensity(spec, ctx)
    rl, rg = _pipeline_reference(dens, spec, x)
    lp, g = (t.cpu().numpy() for t in dens.logp_and_grad(x))
    el, eg = _err(lp, rl), _err(g, rg)
    print('pipeline density: logp %.3g grad %.3g (x = %g)' % (el.max(), eg.max(), x.ravel()[np.argmax(eg)]))
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    assert el.max() <= TOL_EVAL and eg.max() <= TOL_EVAL


# ------------------------------------------------------------------------------------------------------------------------
# every sampler family's own evaluation
# ------------------------------------------------------------------------------------------------------------------------

SEED = 4
FAMILIES = {
    # name: (d, su, layout, switches, the kernel's name starts with)
    'group': (8, None, 'group', {}, 'bf_group_kernel<1, true'),
    'sliced': (8, None, 'wave', dict(no_group=1, lone=0, tail_relaunch=0, wave_cpg=16, no_pipe=1), 'bf_sampler_kernel<1, true'),
    'sliced_su': (8, 'kept', 'wave', dict(no_group=1, lone=0, tail_relaunch=0, wave_cpg=16, no_pipe=1), 'bf_sampler_kernel<1, true'),
    'pipelined': (8, None, 'wave', dict(no_group=1, lone=0, tail_relaunch=0, wave_cpg=16, no_pipe=0), 'bf_nuts_pipe_kernel<1, true'),
    'lone': (8, None, 'wave', dict(no_group=1, lone=2, tail_relaunch=0, wave_cpg=0, no_pipe=0), 'bf_lone_kernel<1, true'),
    'wave128': (128, None, 'wave', {}, 'bf_sampler_kernel<8, true'),
}


def _momenta(n, d, seed):
    """the first momentum draw of chain i: d normals of the stream (seed, i) (unit metric)"""
    from oracle import oracle as orc
    p0 = np.empty((n, d))
    for i in range(n):
        r, keep = orc.make_rng('xoshiro', seed=seed, stream=i)
        orc.lib().bfo_rng_normal(r, p0[i].ctypes.data_as(orc._dp), d)
    return p0


def _one_step(ctx, name):
    """one NUTS iteration of depth 1 from the probe points (|x_trans| <= 40) in the family `name`:
    spec, q0, q1, the 'logp' statistic, the step, the kernel's name"""
    key = ('run', name)
    if key in _cache:
        return _cache[key]
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    d, su, layout, switches, kernel = FAMILIES[name]
    spec, x, rl, rg = _case(d, su, limit=40.)
    dens = DeviceDensity(spec, ctx)
    for k, v in switches.items():   # (the autouse fixture of conftest.py puts the switches back)
        _lib.debug_set(k, v)
    dc = DeviceChains(dens, x, seed=SEED, step_size=EPS * d**0.25)
    s, st = dc.run(1, 'NUTS', n_warmup=0, max_treedepth=1, max_change=1e6, layout=layout, launch_iters=None)
    got = _lib.last_kernel()
    assert got.startswith(kernel), got
    s, st = s.cpu().numpy()[:, 0], st.cpu().numpy()[:, 0]
    np.testing.assert_allclose(st[:, _lib.NSTATS.index('step_size')], EPS, rtol=1e-14)   # (the statistic: the step the tree used)
    _cache[key] = (spec, x, s, st[:, _lib.NSTATS.index('logp')], rg, got)
    return _cache[key]


def _recovered(x, q1, p0):
    """the gradient at q0 from one leapfrog step, the chains it is defined for (the proposal was accepted), and the direction"""
    moved = np.any(q1 != x, axis=1)
    g = {s: 2. * (q1 - x - s * EPS * p0) / EPS**2 for s in (1., -1.)}
    return g, moved


def _check_family(ctx, name):
    spec, x, q1, logp, rg, kernel = _one_step(ctx, name)
    d = x.shape[1]
    # (a) the 'logp' statistic at the returned sample
    rl1, _, _ = cr.logp_grad_hess(spec, q1, want_hess=False)
    el = _err(logp, rl1)
    assert np.all(np.isfinite(logp)), (name, x[~np.isfinite(logp)])
    # (b) the gradient at the start point
    g, moved = _recovered(x, q1, _momenta(N, d, SEED))
    free = cr.kinds_of(spec['hard_bounds']) == 0
    eg = np.zeros(N)
    for c in np.nonzero(moved)[0]:
        e = {s: _err(g[s][c], rg[c]) for s in g}
        s = min(e, key=lambda s: e[s][free].max())   # the direction: the sign that reproduces the unconstrained coordinates
        eg[c] = e[s].max()
    print('%-10s %s: logp %.3g, recovered gradient %.3g on %d of %d chains' % (name, kernel, el.max(), eg.max(), moved.sum(), N))
    assert el.max() <= TOL_SAMPLER
    assert moved.sum() >= 3 * N // 4, 'only %d of %d chains moved' % (moved.sum(), N)
    assert eg.max() <= TOL_SAMPLER, (name, np.argmax(eg), x[np.argmax(eg)])


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_sampler_family(ctx, name):
    _check_family(ctx, name)


def test_families_agree(ctx):
    """'Layouts agree to rounding' where it was false: on the same start points and streams every d = 8 family returns the same
    samples and 'logp' statistics within twice the tolerance against the reference."""
    names = [n for n in sorted(FAMILIES) if FAMILIES[n][0] == 8 and FAMILIES[n][1] is None]
    runs = {n: _one_step(ctx, n) for n in names}
    p0 = _momenta(N, 8, SEED)
    for a in names:
        for b in names:
            if a < b:
                (_, x, qa, la, rg, _), (_, _, qb, lb, _, _) = runs[a], runs[b]
                assert np.array_equal(np.any(qa != x, axis=1), np.any(qb != x, axis=1)), (a, b)
                assert _err(la, lb).max() <= 2 * TOL_SAMPLER, (a, b)
                ga, _ = _recovered(x, qa, p0)
                gb, moved = _recovered(x, qb, p0)
                assert _err(ga[1.][moved], gb[1.][moved]).max() <= 2 * TOL_SAMPLER, (a, b)


# ---- pipeline density: the wave forms and the group form ---------------------------------------------------------------

PLD_FORMS = {
    # name: (layout, pld_waves, the kernel that has to run)
    'wave': ('wave', 0, 'bf_sampler_kernel<1, true, false, 10, 0>'),     # eight waves, compile-time feature set
    'wave16': ('wave', 16, 'bf_sampler_kernel<1, true, false, 8, 0>'),   # sixteen waves
    'group': ('group', 0, 'bf_group_kernel<1, true, 12>'),
}


@pytest.mark.parametrize('form', sorted(PLD_FORMS))
def test_pipeline_density_sampler(ctx, form):
    """The sampler kernels' pipeline-density instantiations (the sliced kernel's, with the inlined exponential and logarithm, in
    both wave counts; the group kernel's) from the probe points up to +-40: the 'logp' statistic at the returned sample and the
    gradient recovered at the start point, against the reference's transform around the stand-alone kernel's original-space
    evaluation (``_pipeline_reference``)."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    layout, waves, want = PLD_FORMS[form]
    spec = _pipeline_case()
    d = 16
    # (the one-sided kinds' +3 puts T forty range widths out, where the 33 quadratic outputs make a step of any useful size diverge:
    # it stays on four chains, which the share below allows to stay where they are)
    x = cr.probe_points(spec, N, limit=40., mix_lanes=True, up_rows=(1, 9, 17, 25))
    assert cr.probes_covered(spec, x, limit=40.)
    dens = DeviceDensity(spec, ctx)
    _lib.debug_set('pld_waves', waves)   # (the autouse fixture of conftest.py puts the switch back)
    dc = DeviceChains(dens, x, seed=SEED, step_size=EPS * d**0.25)
    s, st = dc.run(1, 'NUTS', n_warmup=0, max_treedepth=1, max_change=1e6, layout=layout, launch_iters=None)
    kernel = _lib.last_kernel()
    assert kernel == want, kernel
    s, st = s.cpu().numpy()[:, 0], st.cpu().numpy()[:, 0]
    logp = st[:, _lib.NSTATS.index('logp')]
    _cache[('pld', form)] = (x, s, logp)
    ref, _ = _pipeline_reference(dens, spec, s)
    moved = np.any(s != x, axis=1)
    el = _err(logp, ref).max()
    _, g0 = _pipeline_reference(dens, spec, x)
    g, _ = _recovered(x, s, _momenta(N, d, SEED))
    eg = max(min(_err(g[sg][c], g0[c]).max() for sg in g) for c in np.nonzero(moved)[0])
    print('pipeline density %s %s: logp %.3g gradient %.3g, %d of %d chains moved' % (form, kernel, el, eg, moved.sum(), N))
    assert np.all(np.isfinite(logp))
    assert el <= TOL_SAMPLER and eg <= TOL_SAMPLER
    assert moved.sum() >= 3 * N // 4


# ---- tempered kernels -------------------------------------------------------------------------------------------------

U0 = 8.   # the tempering coordinate at the start: beta = 1 / (1 + exp(-u)) = 0.9997, the step is the target's but for 3e-4 of the base's


@pytest.mark.parametrize('generic', [0, 1])
def test_tempered_kernels(ctx, generic):
    """The tuned (bfhip_tnuts.hip) and the generic (bfhip_tnuts_gen.hip) tempered kernel, one iteration of depth 1 from the probe
    points.  (a) The 'logp' statistic is the target's logp at the returned sample.  (b) The tempered step (integration.py:153-222)
    is a half drift, a kick by the mixed force at the mid point, a half drift:

        q_m = q0 + s eps/2 p0,   u_m = u0 + s eps/2 v0,   beta = 1 / (1 + exp(-u_m)),
        F = beta grad logp(q_m) + (1 - beta) grad log N(q_m; 0, 0.3 I),   q1 = q_m + s eps/2 (p0 + s eps F)

    so F = 2 (q1 - q0 - s eps p0) / eps^2 as for the other families, with p0 the chain's first draw (d normals) and v0 its second (one
    normal) of the documented stream, both through the oracle's generator.  F is compared with the reference's gradient at q_m in
    that mixture; the base density's part is known in closed form.  The sign s is the one that reproduces the unconstrained
    coordinates.  (The one-sided kinds' +3 sits on four chains only: the tempered integrator's energy error there is 1e3 at this step
    and the proposal is never taken.)"""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    from oracle import oracle as orc
    d = 8
    spec = cr.narrow_bounded_spec(d)
    x = cr.probe_points(spec, N, limit=40., mix_lanes=True, up_rows=(1, 9, 17, 25))
    assert cr.probes_covered(spec, x, limit=40.)
    _lib.debug_set('tnuts_generic', generic)
    dc = DeviceChains(DeviceDensity(spec, ctx), x, seed=SEED, step_size=EPS * d**0.25)
    s, st, stt = dc.run_tempered(1, np.zeros(d), np.eye(d) * 0.3, logxi=0.3, u_0=np.full(N, U0), n_warmup=0, max_treedepth=1,
                                 max_change=1e6)
    kernel = _lib.last_kernel()
    assert kernel == ('bf_tnuts_gen_kernel<1>' if generic else 'bf_tnuts_kernel<1, true, false>'), kernel
    s, st = s.cpu().numpy()[:, 0], st.cpu().numpy()[:, 0]
    logp = st[:, _lib.NSTATS.index('logp')]
    np.testing.assert_allclose(st[:, _lib.NSTATS.index('step_size')], EPS, rtol=1e-14)
    _cache[('tempered', generic)] = (x, s, logp)
    rl, _, _ = cr.logp_grad_hess(spec, s, want_hess=False)
    moved = np.any(s != x, axis=1)
    # the two draws
    p0, v0 = np.empty((N, d)), np.empty(N)
    for i in range(N):
        r, keep = orc.make_rng('xoshiro', seed=SEED, stream=i)
        orc.lib().bfo_rng_normal(r, p0[i].ctypes.data_as(orc._dp), d)
        one = np.empty(1)
        orc.lib().bfo_rng_normal(r, one.ctypes.data_as(orc._dp), 1)
        v0[i] = one[0]
    free = cr.kinds_of(spec['hard_bounds']) == 0
    F, _ = _recovered(x, s, p0)
    eg = np.zeros(N)
    for sg in (1., -1.):
        qm = x + sg * 0.5 * EPS * p0
        beta = 1. / (1. + np.exp(-(U0 + sg * 0.5 * EPS * v0)))
        _, gt, _ = cr.logp_grad_hess(spec, qm, want_hess=False)
        Fr = beta[:, None] * gt + (1. - beta[:, None]) * (-qm / 0.3)
        e = _err(F[sg], Fr)
        if sg == 1.:
            e_plus = e
    for c in np.nonzero(moved)[0]:
        ec = e_plus[c] if e_plus[c][free].max() <= e[c][free].max() else e[c]   # the direction that reproduces the free coordinates
        eg[c] = ec.max()
    print('tempered %s: logp %.3g, recovered force %.3g on %d of %d chains' % (kernel, _err(logp, rl).max(), eg.max(), moved.sum(), N))
    assert np.all(np.isfinite(logp))
    assert _err(logp, rl).max() <= TOL_SAMPLER
    assert moved.sum() >= 3 * N // 4, 'only %d of %d chains moved' % (moved.sum(), N)
    assert eg.max() <= TOL_SAMPLER, (np.argmax(eg), x[np.argmax(eg)])


def test_pipeline_forms_and_tempered_kernels_agree(ctx):
    """The cross-family promise for the families that have their own start points: the three pipeline-density forms with each other,
    the tuned tempered kernel with the generic one -- samples (hence the forces) and 'logp' statistics within twice the tolerance."""
    for keys in ([('pld', f) for f in sorted(PLD_FORMS)], [('tempered', 0), ('tempered', 1)]):
        for k in keys:
            if k not in _cache:   # (run alone: produce the runs)
                (test_pipeline_density_sampler if k[0] == 'pld' else test_tempered_kernels)(ctx, k[1])
        for a in keys:
            for b in keys:
                if a < b:
                    (x, qa, la), (_, qb, lb) = _cache[a], _cache[b]
                    assert np.array_equal(np.any(qa != x, axis=1), np.any(qb != x, axis=1)), (a, b)
                    assert _err(la, lb).max() <= 2 * TOL_SAMPLER, (a, b)
                    fa, fb = 2. * (qa - x) / EPS**2, 2. * (qb - x) / EPS**2
                    assert _err(fa, fb).max() <= 2 * TOL_SAMPLER, (a, b)
