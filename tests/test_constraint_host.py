"""The constraint transform's one helper (``csrc/bfhip_constraint.h``), compiled for the host, against an extended-precision reference.

Every kernel family and the Hessian code evaluate this helper, so a sweep of it on the CPU covers the arithmetic that the GPU tests
(``test_gpu_constraint_edges.py``) then find again in each family.  The claim: a coordinate pressed against a hard bound
(|x_trans| of tens to hundreds) is as accurate as one in the middle of its range.

Tolerances are those of ``test_constraint_transforms_golden`` (1e-14 on the map, 1e-12 on its derivatives), relative to
max(1, |reference|) per component.  The statement-by-statement form of the reference fails this sweep from x = +20 in T''/T' (3.6e-8)
and from x = +30 in log|T'| (1e-3; -inf from 37)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hess_host'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))

import constraint_reference as cr  # noqa: E402
import hess_host  # noqa: E402

LO, HI = -1., 2.


def _grid(kind):
    """a few thousand points of [-745, 745], dense where the logistic kind's naive form degrades, with every probe value on it; the
    one-sided kinds stop at +3 (exp(x) rg leaves every range of interest beyond)"""
    top = 745. if kind in (0, 1) else 3.
    g = np.concatenate([np.linspace(-745., top, 1201), np.linspace(10., 40., 601), np.linspace(-40., -10., 601),
                        np.linspace(-3., 3., 241), cr.PROBES_TWO_SIDED if kind == 1 else cr.PROBES_ONE_SIDED, [0., -0.]])
    return np.unique(g[g <= top])


def _err(got, ref):
    return np.abs(got - ref) / np.maximum(1., np.abs(ref))


@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_helper_sweep(kind):
    x = _grid(kind)
    assert x.size > 2000 or kind > 1
    probes = cr.PROBES_TWO_SIDED if kind == 1 else (cr.PROBES_ONE_SIDED if kind else [])
    assert all(v in x for v in probes)
    got = hess_host.constraint(x, kind, LO, HI)
    ref = np.empty_like(got)
    for i, v in enumerate(x):
        T, J, J2 = cr.to_original(v, kind, LO, HI)
        lj, lj1, lj2 = cr.log_jac(v, kind, LO, HI)
        ref[i] = [float(T), float(J), float(lj), float(lj1), float(lj2)]
    assert np.all(np.isfinite(got)), 'non-finite at x = %s' % x[~np.all(np.isfinite(got), axis=1)][:5]
    names = ['xo', 'J', 'log|J|', 'J2/J', 'd2 log|J|/dx2']
    tols = [1e-14, 1e-12, 1e-14, 1e-12, 1e-12]
    for c in range(5):
        e = _err(got[:, c], ref[:, c])
        w = int(np.argmax(e))
        print('kind %d %-14s max err %.3g at x = %g' % (kind, names[c], e[w], x[w]))
        assert e[w] <= tols[c], (names[c], x[w], got[w, c], ref[w, c])
    # J is compared to relative accuracy as well: it spans 600 orders of magnitude, and the chain rule multiplies by it
    ok = ref[:, 1] != 0.
    rel = np.abs(got[ok, 1] - ref[ok, 1]) / np.abs(ref[ok, 1])
    normal = np.abs(ref[ok, 1]) > 1e-300   # (below: denormals, accurate to their own spacing)
    assert np.max(rel[normal]) <= 1e-14, (x[ok][normal][np.argmax(rel[normal])], np.max(rel[normal]))


def test_helper_beyond_the_exponent_range():
    """Where J underflows to zero the helper reports log|J| = -inf with it (never a finite number beside J = 0), and NaN stays NaN."""
    for kind, xs in ((1, [800., -800.]), (2, [-800.]), (3, [-800.])):
        got = hess_host.constraint(np.array(xs), kind, LO, HI)
        assert np.all(got[:, 1] == 0.) and np.all(np.isneginf(got[:, 2])), (kind, got)
    for kind in (2, 3):
        got = hess_host.constraint(np.array([800.]), kind, LO, HI)
        assert not np.isfinite(got[0, 0]) and not np.isfinite(got[0, 1])
    for kind in (0, 1, 2, 3):
        got = hess_host.constraint(np.array([np.nan]), kind, LO, HI)[0]
        assert np.all(np.isnan(got[:3] if kind else got[:1]))   # (the affine kind's J does not depend on x)


@pytest.mark.parametrize('input_scales', [None, 'folded', 'kept'])
def test_hess_host_at_the_probe_points(input_scales):
    """``bf_hess_eval`` / ``bf_hess_entry`` (the Laplace and Newton code's arithmetic) at d = 8 on the probe points: value, gradient
    and Hessian against the reference, all at the stand-alone entry points' 1e-11 (``test_gpu_laplace.py`` holds the Hessian to a
    finite-difference tolerance measured per point, 1e-11 and more)."""
    spec = cr.narrow_bounded_spec(8, input_scales=input_scales)
    x = cr.probe_points(spec, 32, mix_lanes=True)
    assert cr.probes_covered(spec, x)
    logp, grad, hess = hess_host.logp_grad_hess(spec, x)
    rl, rg, rh = cr.logp_grad_hess(spec, x)
    el, eg, eh = _err(logp, rl).max(), _err(grad, rg).max(), _err(hess, rh).max()
    print('input_scales %s: logp %.3g grad %.3g hess %.3g' % (input_scales, el, eg, eh))
    assert np.all(np.isfinite(logp))
    assert el <= 1e-11 and eg <= 1e-11 and eh <= 1e-11
