"""The iteration end's one helper (``csrc/bfhip_adapt.h``), compiled for the host, against a plain Python restatement of the reference.

Every sampler kernel ends an iteration through this helper, and the adapted step size and metric are compared bit for bit across
kernels, so the sweep is exact: ``FUSED = false`` must give the bits of statement-by-statement double arithmetic, ``FUSED = true`` the
bits of the same statements with the fused operations rounded once (``helpers/adapt_reference.py``).  No tolerance anywhere."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hess_host'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))

import adapt_reference as ar  # noqa: E402
import hess_host  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# target_accept, gamma, k, t_0: the defaults of the sampler's configuration, and one other set
STEP_PARAMS = [(0.8, 0.05, 0.75, 10.), (0.65, 0.1, 0.6, 25.)]


@pytest.mark.parametrize('one_call', [True, False])   # step(), or consts() and update()
@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('params', STEP_PARAMS)
def test_dual_averaging_is_the_restatement_bit_for_bit(fused, params, one_call):
    target, gamma, k, t_0 = params
    rng = np.random.default_rng(20)
    accept = rng.uniform(0., 1., size=300)
    accept[[0, 7, 150]] = 0.
    accept[[1, 8, 299]] = 1.
    log_step0 = math.log(0.25)
    mu = math.log(10. * 0.25)
    got = hess_host.step_adapt(fused, accept, mu, (0., log_step0, log_step0, 1.), target, gamma, k, t_0, one_call=one_call)
    ref = ar.DualAveraging(log_step0, mu, target, gamma, k, t_0, fused=fused)
    want = np.empty_like(got)
    for i, acc in enumerate(accept):
        ref.update(float(acc))
        want[i] = ref.state()
    assert want[-1, 3] == 301.
    assert np.all(np.isfinite(got))
    bad = np.nonzero(np.any(_bits(got) != _bits(want), axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:1]], want[bad[:1]])


def test_the_two_rounding_policies_differ():
    """(otherwise the sweep above would not tell them apart)"""
    target, gamma, k, t_0 = STEP_PARAMS[0]
    accept = np.random.default_rng(20).uniform(0., 1., size=300)
    a = hess_host.step_adapt(False, accept, 1., (0., 0., 0., 1.), target, gamma, k, t_0)
    b = hess_host.step_adapt(True, accept, 1., (0., 0., 0., 1.), target, gamma, k, t_0)
    assert np.any(_bits(a) != _bits(b))
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-14)


def _welford_columns():
    rng = np.random.default_rng(21)
    cols = {'normal': rng.normal(size=500) * 3. + 1., 'constant': np.full(500, 0.1), 'tiny': rng.normal(size=500) * 1e-150,
            'huge': rng.normal(size=500) * 1e150}
    mixed = rng.normal(size=500)
    mixed[::50] = 1e150
    mixed[25::50] = 1e-150
    cols['mixed'] = mixed
    return cols


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('name', ['normal', 'constant', 'tiny', 'huge', 'mixed'])
def test_welford_add_is_the_restatement_bit_for_bit(fused, name):
    x = _welford_columns()[name]
    assert x.size == 500
    # a fresh background window (weight 10, zeros) and a foreground window that starts from a given mean and variance
    for n0, mean0, raw0 in ((10., 0., 0.), (10., float(x[0]), 10. * 2.5)):
        got = hess_host.welford(fused, x, n0, mean0, raw0)
        ref = ar.RunningVariance(n0, mean0, raw0, fused=fused)
        want = np.empty_like(got)
        for i, v in enumerate(x):
            ref.add(float(v))
            want[i] = (ref.mean, ref.raw)
        assert np.all(np.isfinite(got)), name
        bad = np.nonzero(np.any(_bits(got) != _bits(want), axis=1))[0]
        assert bad.size == 0, (name, bad[:5], got[bad[:1]], want[bad[:1]])
    if name == 'constant':   # the mean closes in on the constant and the raw sum stays at what the start left it
        assert abs(got[-1, 0] - 0.1) < 1e-3 and got[-1, 1] >= 0.


@pytest.mark.parametrize('doubling', [True, False])
@pytest.mark.parametrize('update_window', [1, 3])
def test_metric_window_is_the_restatement_at_every_iteration(update_window, doubling):
    start = (10., 10., 0., 0., 5.)
    got = hess_host.metric_window(start, 200, update_window, doubling)
    ref = ar.MetricWindow(*start, update_window=update_window, doubling=doubling)
    want = np.empty_like(got)
    for i in range(200):
        refresh, roll = ref.update()
        want[i] = ref.state() + (float(refresh), float(roll))
    assert np.array_equal(got, want), np.nonzero(np.any(got != want, axis=1))[0][:5]
    rolls, refreshes = got[:, 6] == 1., got[:, 5] == 1.
    assert rolls.sum() >= 3                       # (doubling: windows of 5, 10, 20, 40, 80 -> rolls at 5, 16, 37, 78, 159)
    assert np.any(refreshes & ~rolls)
    if update_window > 1:
        assert np.any(~refreshes)
    assert got[-1, 4] == (5. * 2. ** rolls.sum() if doubling else 5.)
