"""The extended-precision reference of the autocorrelation reductions (helpers/acor_reference.py) and the case list of
test_gpu_acor_kernels.py (helpers/acor_cases.py), checked on the CPU before the HIP kernels are held to them:

1. the reference's lag sums agree with the host port's FFT autocovariances (utils.acor._host_lag_sums), NaN in the same places;
2. tau assembled from the reference's lag sums reproduces the values the reference package recorded (golden/evidence.npz);
3. the exact cases cover every axis value and every path of the lag kernel that helpers/acor_cases.py names, and their sums are
   exact in float64 whatever the order."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import acor_cases as ac  # noqa: E402
import acor_reference as ar  # noqa: E402


def _reference_lag_sums(x, t0, n_lag):
    x = np.asarray(x, dtype=np.float64)
    mean, inv = ar.moments(x)
    return ar.lag_sums(x, mean, inv, t0, n_lag)[0].astype(np.float64)


@pytest.mark.parametrize('shape', [(3, 1, 2), (2, 2, 3), (4, 65, 3), (5, 200, 4), (1, 333, 1)])
def test_reference_lag_sums_agree_with_the_fft_port(shape):
    """Every lag, and a block from the middle.  The last column is constant where there is more than one: its sums are 0 / 0 in the
    port and 0 * inf here, NaN in both; n_t = 1 centres every series to 0, which is the same."""
    from bayesfast_amd.utils.acor import _host_lag_sums
    n_w, n_t, n_d = shape
    rng = np.random.default_rng(sum(shape))
    x = np.stack([ac.ar1(rng, p, n_w, n_t, 1)[:, :, 0] for p in np.array([0.5, 0.9, 0., 0.98])[np.arange(n_d) % 4]], axis=-1)
    if n_d > 1:
        x[:, :, -1] = 2.5
    for t0, n_lag in ((0, n_t), (n_t // 3, max(n_t // 2, 1))):
        with np.errstate(invalid='ignore', divide='ignore'):
            want = _host_lag_sums(x, t0, n_lag).numpy()
            got = _reference_lag_sums(x, t0, n_lag)[:want.shape[0]]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(want).all() if n_t == 1 else np.isnan(want[:, :-1 if n_d > 1 else None]).sum() == 0
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=0)


def test_lags_beyond_the_series_are_exactly_zero_and_the_scale_bounds_the_sum():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(3, 20, 2))
    mean, inv = ar.moments(x)
    s, a = ar.lag_sums(x, mean, inv, 15, 10)
    assert s.dtype == ar.LD and s.shape == (10, 2)
    assert np.all(s[5:] == 0) and np.all(a[5:] == 0) and not np.signbit(s[5:]).any()
    assert np.all(np.abs(s) <= a) and np.all(a[:5] > 0)
    # lag 0 of a series normalised by its own a(0): one per walker
    np.testing.assert_allclose(ar.lag_sums(x, mean, inv, 0, 1)[0].astype(np.float64), 3., rtol=1e-15)
    with pytest.raises(ValueError):
        ar.moments(x, ldw=39)
    assert ar.moments(x, ldw=47)[0].tobytes() == mean.tobytes()


def test_tau_from_the_reference_lag_sums_reproduces_the_recorded_values(golden_dir):
    from bayesfast_amd.utils.acor import integrated_time_sharded
    fx = np.load(os.path.join(golden_dir, 'evidence.npz'))
    x = fx['acor.x']
    for xs, key in ((x, 'acor.tau3'), (x[:1], 'acor.tau2'), (x[1:2, :, :1], 'acor.tau1')):
        tau = integrated_time_sharded(xs, xs.shape[0], lag_sums=_reference_lag_sums)
        np.testing.assert_allclose(tau, fx[key], rtol=1e-10)


def test_shape_functions_restate_the_kernel_source():
    """groups and log_td against the constants and the two functions of csrc/bfhip_acor.hip as its text has them."""
    src = open(os.path.join(os.path.dirname(HERE), 'bayesfast_amd', 'csrc', 'bfhip_acor.hip')).read()
    for text in ('#define AC_SLOTS 16', '#define AC_LAGS 64', '#define AC_CT 256', '#define AC_MAXG 256',
                 '*wpg = (n_w + AC_MAXG - 1) / AC_MAXG;', '*n_g = (n_w + *wpg - 1) / *wpg;',
                 'while ((1 << l) < n_d && (1 << l) < AC_SLOTS) ++l;'):
        assert text in src, text
    assert (ar.SLOTS, ar.LAGS, ar.CHUNK, ar.MAX_GROUPS) == (16, 64, 256, 256)
    assert [ar.groups(n) for n in (1, 256, 257, 512, 513, 4096)] == [(1, 1), (1, 256), (2, 129), (2, 256), (3, 171), (16, 256)]
    assert [ar.log_td(n) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17, 33)] == [0, 1, 2, 2, 3, 3, 4, 4, 4, 4]


def test_exact_cases_hit_every_named_path():
    hit = {}
    for c in ac.EXACT:
        for p in ac.paths(c):
            hit.setdefault(p, []).append(ac.case_id(c))
    missing = [p for p in ac.REQUIRED if p not in hit]
    assert not missing, missing
    assert len(set(ac.EXACT)) == len(ac.EXACT)
    # the walker loop of a group runs more than once at both shapes that can make it, and once with a part-filled last pass
    by_shape = {(c.n_w, c.n_d): ac.paths(c) for c in ac.EXACT}
    assert 'wpg>ws_n' in by_shape[(257, 17)] and 'wpg>ws_n' in by_shape[(513, 9)]
    assert 'wpg>ws_n,last_pass_part_filled' in by_shape[(513, 8)]
    # blocks beyond the series both start at n_t and lie further out; padded and tight strides both occur with every td
    assert any(c.t0 == c.n_t for c in ac.EXACT) and any(c.t0 > c.n_t for c in ac.EXACT)
    for td in (1, 2, 4, 8, 16):
        assert {bool(c.pad) for c in ac.EXACT if 'td=%d' % td in ac.paths(c)} == {False, True}, td
    # small shapes: the whole file takes seconds
    for c in ac.EXACT + ac.FLOAT:
        assert c.n_t <= 600 and c.n_w * c.n_t * c.n_d <= 400000, c


def test_exact_cases_are_exact_in_any_order():
    """|x - mean| <= 4, so a product is at most 16 and, times inv <= 4, every partial sum an integer multiple of 1/4 of magnitude
    at most 64 n_w n_t: below 2^53 quarter units (which covers the 9 n_w n_t of values in [-3, 3] alone)."""
    for c in ac.EXACT:
        assert 9 * c.n_w * c.n_t < 2**53 and 4 * 64 * c.n_w * c.n_t < 2**53
        x, mean, inv = ac.exact_inputs(c)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3
        assert set(np.unique(mean)) <= {-1., 0., 1.} and set(np.unique(inv)) <= {0.25, 0.5, 1., 2., 4.}
        if c.diag:
            assert c.n_d == 16 and c.pad == 0 and c.n_w % 2 == 0 and np.all(inv == 1) and not x[:, :, 5:].any()
        elif c.n_w * c.n_d >= 30:      # (fewer series cannot be expected to draw every value)
            assert len(np.unique(mean)) == 3 and len(np.unique(inv)) == 5
        elif c.n_w * c.n_d >= 4:
            assert len(np.unique(mean)) >= 2 and len(np.unique(inv)) >= 2
    c = ac.EXACT[4]
    ref = ac.exact_reference(c)
    assert ref.shape == (c.n_lag, c.n_d) and np.array_equal(ref * 4, np.round(ref * 4))
    assert np.all(ref[c.n_t - c.t0:] == 0) and np.any(ref[:c.n_t - c.t0] != 0)
    # the definition once more, in int64, on this one case
    x, mean, inv = ac.exact_inputs(c)
    y = (x - mean[:, None, :]).astype(np.int64)
    for i in range(c.n_t - c.t0):
        t = c.t0 + i
        want = ((y[:, :c.n_t - t] * y[:, t:]).sum(axis=1) * inv).sum(axis=0)
        assert np.array_equal(ref[i], want)


def test_float_cases_spread_the_variances():
    for c in ac.FLOAT:
        mean, inv, s, a = ac.float_reference(c)
        assert inv.max() / inv.min() > 1e4 and np.isfinite(s).all()
        assert np.all(np.abs(s) <= a)
        assert ac.n_terms(c)[0] == c.n_w * (c.n_t - c.t0)
