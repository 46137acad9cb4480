"""The extended-precision reference of the density evaluation and the leapfrog step (helpers/eval_reference.py), checked on the
CPU before test_gpu_eval_widths.py holds the HIP kernels to it:

1. it reproduces the fixtures the reference package produced (golden/density.npz, golden/sampler.npz), at the tolerances
   test_gpu_eval.py applies to the device on the same fixtures, and its constraint transform agrees with the 60-digit
   helpers/constraint_reference.py;
2. the ``ROUNDING`` table of helpers/eval_cases.py is ten times what the float64 C oracle's error against it measures, in units
   of 2^-52 scale, on the very inputs of the GPU tests;
3. the comparison the GPU tests use rejects the oracle's output for a spec with ONE entry changed by 1e-9 relative, field by field
   -- it stands in for mutating the kernels.
"""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import eval_cases as ec  # noqa: E402
import eval_reference as er  # noqa: E402

G = os.path.join(HERE, 'golden')


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- 1. the reference is right ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['plain', 'decay', 'scales', 'su', 'full', 'd64'])
def test_reference_reproduces_the_density_fixtures(case):
    """Density.logp_and_grad fixtures of the reference package (core/density.py:724-754), both spaces."""
    from specio import rebuild_spec
    z = np.load(os.path.join(G, 'density.npz'))
    spec = rebuild_spec(z, case + '.')
    spaces = [('trans', False)] + ([('orig', True)] if case + '.x_orig' in z.files else [])
    for key, original in spaces:
        lp, g, _, _ = er.logp_and_grad(spec, z['%s.x_%s' % (case, key)], original_space=original)
        np.testing.assert_allclose(_f64(lp), z['%s.logp_%s' % (case, key)], rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(_f64(g), z['%s.grad_%s' % (case, key)], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize('name', ['full5', 'plain16', 'd64'])
def test_reference_reproduces_the_leapfrog_fixtures(name):
    """CpuLeapfrogIntegrator._step fixtures (integration.py:68-95): two consecutive states."""
    from specio import rebuild_spec
    samp = np.load(os.path.join(G, 'sampler.npz'))
    spec = rebuild_spec(samp, name + '.')
    var, eps = samp[name + '.lf.var'], samp[name + '.lf.eps']
    for a, b, e in (('s0', 's1', eps[0]), ('s1', 's2', eps[1])):
        q, p, g = (samp['%s.lf.%s.%s' % (name, a, f)] for f in ('q', 'p', 'q_grad'))
        r = er.leapfrog(spec, var, [e], q, p, g)
        for f, k in (('q', 'q'), ('p', 'p'), ('velocity', 'v'), ('q_grad', 'grad')):
            np.testing.assert_allclose(_f64(r[k][0])[0], samp['%s.lf.%s.%s' % (name, b, f)], rtol=1e-10, atol=1e-11)
        for f in ('logp', 'energy'):
            np.testing.assert_allclose(_f64(r[f][0])[0], samp['%s.lf.%s.%s' % (name, b, f)], rtol=1e-11, atol=1e-11)


def test_constraint_form_agrees_with_the_60_digit_reference():
    """The cancellation-free logistic form and the one-sided kinds against helpers/constraint_reference.py (mpmath): T, T',
    log|T'| and its derivative to 1e-17 relative (longdouble rounds at 1e-19), out to |x| = 40 where t (1 - t) has no digits left."""
    import mpmath as mp
    import constraint_reference as cr
    ranges = np.array([[-1.25, 2.5], [0.3, 7.], [-60., -58.5], [2., 3.]])
    kinds = np.array([1, 2, 3, 0])
    xs = [-40., -12., -3.3, -0.4, 0., 0.7, 2.9, 11.5, 36.5, 40.]
    x = np.array([[v if (k == 1 or abs(v) < 13.) else v / 10. for k in kinds] for v in xs])
    T, J, lj, gj = er.constraint(x, kinds, ranges)
    worst = 0.
    for i in range(x.shape[0]):
        for j, k in enumerate(kinds):
            t0, t1, _ = cr.to_original(x[i, j], int(k), ranges[j, 0], ranges[j, 1])
            l0, l1, _ = cr.log_jac(x[i, j], int(k), ranges[j, 0], ranges[j, 1])
            # (J'' / J = 1 - 2 t of the logistic kind is a difference of numbers of size 1: its error is taken against 1)
            for got, want, floor in ((T.v[i, j], t0, 0.), (J.v[i, j], t1, 0.), (lj.v[i, j], l0, 1.), (gj.v[i, j], l1, 1.)):
                want = np.longdouble(mp.nstr(want, 30))
                worst = max(worst, float(abs(got - want) / max(abs(want), floor)))
    print('constraint: largest relative error %.3g' % worst)
    assert worst < 1e-17


# ---- 2. ROUNDING ---------------------------------------------------------------------------------------------------------------
def eval_runs(d, name):
    """[(points, original_space)] of one cell of the evaluation matrix: both spaces where the spec has a transform."""
    xo, xs, outside = ec.eval_points(d, name)
    ec.check_eval_inputs(ec.spec_for(d, name), xo, xs, outside)
    return [(xo, False)] if xs is None else [(xo, True), (xs, False)]


def oracle_leapfrog(spec, st):
    from oracle import oracle as orc
    rows = [orc.leapfrog(spec, st['var'][i], st['eps'][i], st['q'][i], st['p'][i], st['grad'][i]) for i in range(len(st['eps']))]
    return {k: np.array([r[k] for r in rows]) for k in ('q', 'p', 'v', 'grad', 'logp', 'energy')}


def measure_width(d):
    """Largest error of the C oracle against the reference at width d, in units of 2^-52 scale, per figure."""
    from oracle import oracle as orc
    worst = dict.fromkeys(ec.FIGURES, 0.)
    for name in ec.EVAL_FEATURES:
        spec = ec.spec_for(d, name)
        for x, original in eval_runs(d, name):
            lp, g = orc.logp_and_grad(spec, x, original_space=original)
            for _, fig, got, ref, scale in ec.eval_parts(lp, g, er.logp_and_grad(spec, x, original_space=original)):
                worst[fig] = max(worst[fig], ec.units(got, ref, scale))
    for name in ec.LEAPFROG_FEATURES:
        spec, st = ec.spec_for(d, name), ec.leapfrog_state(d, name)
        ref = er.leapfrog(spec, st['var'], st['eps'], st['q'], st['p'], st['grad'])
        for _, fig, got, r, scale in ec.leapfrog_parts(oracle_leapfrog(spec, st), ref):
            worst[fig] = max(worst[fig], ec.units(got, r, scale))
    return worst


@pytest.mark.parametrize('d', ec.WIDTHS)
def test_rounding_table_is_ten_times_the_measurement(d):
    """K of every figure is ten times the oracle's largest error at this width, rounded to two digits, and no K 2^-52 exceeds 1e-11,
    the project's T0 figure -- above that the scale would be hiding something.  (The inputs are the same bits on every host,
    eval_cases.q32; re-measured on two hosts with different CPUs the table came out the same to four digits.)"""
    worst = measure_width(d)
    print('d = %3d   measured  %s' % (d, '  '.join('%s %.3g' % (f, worst[f]) for f in ec.FIGURES)))
    print('          10 x      %s' % '  '.join('%s %.2g' % (f, 10. * worst[f]) for f in ec.FIGURES))
    for f in ec.FIGURES:
        K = ec.ROUNDING[d][f]
        assert K == ec.two_digits(10. * worst[f]), (d, f, K, 10. * worst[f])
        assert K * ec.EPS <= 1e-11, (d, f, K)


# ---- 3. the comparison can see a wrong term ----------------------------------------------------------------------------------------
def _bump(a, idx=None):
    """one entry times (1 + 1e-9)"""
    if idx is None:
        return float(a) * (1. + 1e-9)
    a[idx] = a[idx] * (1. + 1e-9)
    assert a[idx] != 0.
    return a


ALL_FIELDS = ('quad', 'mu', 'hess', 'alpha', 'cubic', 'decay_alpha2', 'su_diff', 'range_end')
# Every field on the plainest feature set that has it, where the scale is that of the formula itself; then all of them at once on
# 'everything'.  One entry of mu is left out there: behind the kept input scaling (offsets of 40 to 50 widths) every coordinate of
# the surrogate's input carries a rounding error of 50 x 2^-52 ~ 1e-14, worst case 127 of them add up along the gradient, and a
# 1e-9 change of mu_j ~ 0.03 moves ONE coordinate of the projected point by 3e-11 (1 - alpha / beta): at d = 127 that is the size of
# the rounding bound itself, whatever the comparison.
PERTURBATION_CASES = (('quadratic', ('quad', 'mu', 'hess', 'alpha')), ('cubic', ('cubic',)), ('decay_own', ('decay_alpha2',)),
                      ('su_kept', ('su_diff',)), ('transform', ('range_end',)),
                      ('everything', tuple(f for f in ALL_FIELDS if f != 'mu')))


def perturbed_specs(spec, fields):
    """(field, spec with ONE entry of that field changed by 1e-9 relative)"""
    d = int(spec['d'])
    order = {cf['order']: i for i, cf in enumerate(spec['poly']['configs'])}
    j = d // 2
    out = []
    for field in fields:
        s = copy.deepcopy(spec)
        po = s['poly']
        if field == 'quad':
            _bump(po['configs'][order['quadratic']]['coef'], (0, j, j))
        elif field == 'mu':
            _bump(po['mu'], int(np.argmax(np.abs(po['mu']))))
        elif field == 'hess':
            _bump(po['hess'], (j, j))
        elif field == 'alpha':
            po['alpha'] = _bump(po['alpha'])
        elif field == 'cubic':
            c = po['configs'][order['cubic-2']]['coef']
            _bump(c, np.unravel_index(int(np.argmax(np.abs(c))), c.shape))
        elif field == 'decay_alpha2':
            s['decay_alpha2'] = _bump(s['decay_alpha2'])
        elif field == 'su_diff':
            _bump(s['su_diff'], j)
        else:
            _bump(s['ranges'], (j - j % 4, 1))   # the upper end of a coordinate with both bounds hard
        out.append((field, s))
    return out


@pytest.mark.parametrize('d', ec.WIDTHS)
def test_comparison_rejects_one_perturbed_entry(d):
    """The oracle's output for an unperturbed spec passes the GPU tests' comparison; for a spec with one entry of the quadratic
    coefficients, mu, hess, alpha, a cubic coefficient, decay_alpha2, su_diff or a range end off by 1e-9 relative it does not."""
    from oracle import oracle as orc
    K = ec.rounding_for(d)
    seen = set()
    for name, fields in PERTURBATION_CASES:
        spec = ec.spec_for(d, name)
        xo, xs, outside = ec.eval_points(d, name)
        ec.check_eval_inputs(spec, xo, xs, outside)
        x = xo if xs is None else xs
        ref = er.logp_and_grad(spec, x)
        lp, g = orc.logp_and_grad(spec, x)
        _, bad = ec.compare('d=%d %s unperturbed' % (d, name), ec.eval_parts(lp, g, ref), K)
        assert not bad
        for field, s in perturbed_specs(spec, fields):
            lp, g = orc.logp_and_grad(s, x)
            _, bad = ec.compare('d=%d %s %s' % (d, name, field), ec.eval_parts(lp, g, ref), K)
            assert bad, 'a 1e-9 change of %s went unnoticed on %s' % (field, name)
            seen.add(field)
    assert seen == set(ALL_FIELDS)
