"""bfhip_acor_moments and bfhip_acor_lag_sums (csrc/bfhip_acor.hip) called directly and held to the plain extended-precision
reference of helpers/acor_reference.py, at the shapes of helpers/acor_cases.py (tests/test_acor_reference_host.py shows on the host
that they take every path of the lag kernel between them).

Every output is a slice of a larger buffer filled with a NaN of a payload no arithmetic produces; whatever lies outside the
documented size has to keep it.  Every input lies between NaN: a read outside it shows in the result.

Only the float cases and the moments have tolerances, each the worst-case rounding bound of the operation in any order of
summation, in units of U = 2^-53, written out where it is applied.  The exact cases, the block independence, the repeats, the
strided calls and the isolation of a non-finite series compare bytes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import acor_cases as ac  # noqa: E402
import acor_reference as ar  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.**-53                         # the unit roundoff of float64
LD = ar.LD
GUARD = 96                          # doubles kept on either side of every buffer
SENTINEL = 0x7FF8DEADBEEF1234       # a quiet NaN with a payload of its own


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


class _Out:
    """n doubles to be written, inside a sentinel-filled buffer."""

    def __init__(self, ctx, n):
        import torch
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=ctx.device).view(torch.float64)
        self.view = self.buf[GUARD:GUARD + n]

    def bits(self):
        import torch
        return self.buf.view(torch.int64).cpu().numpy()

    def check_outside(self, what):
        b = self.bits()
        assert np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + self.n:] == SENTINEL), '%s: written outside its %d doubles' % (what, self.n)

    def untouched(self):
        return bool(np.all(self.bits() == SENTINEL))

    def numpy(self, shape, what, all_written=True):
        self.check_outside(what)
        b = self.bits()[GUARD:GUARD + self.n]
        if all_written:
            assert not np.any(b == SENTINEL), '%s: not every element was written' % what
        return b.view(np.float64).reshape(shape).copy()


def _between_nan(ctx, a):
    """The float64 array a on the device with NaN on either side -> (buffer, view)."""
    import torch
    flat = np.full(a.size + 2 * GUARD, np.nan)
    flat[GUARD:GUARD + a.size] = np.asarray(a, dtype=np.float64).ravel()
    buf = torch.as_tensor(flat, device=ctx.device)
    return buf, buf[GUARD:GUARD + a.size]


def _place_x(ctx, x, pad):
    """x (n_w, n_t, n_d) at walker stride ldw = n_t n_d + pad, NaN in the gaps and around the whole -> (buffer, view, ldw)."""
    n_w, n_t, n_d = x.shape
    ldw = n_t * n_d + pad
    rows = np.full((n_w, ldw), np.nan)
    rows[:, :n_t * n_d] = x.reshape(n_w, -1)
    return _between_nan(ctx, rows) + (ldw,)


def _device_moments(ctx, xd, shape, ldw):
    """-> (mean, inv) numpy (n_w, n_d), and the _Out pair that holds them on the device."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    n_w, n_t, n_d = shape
    m, v = _Out(ctx, n_w * n_d), _Out(ctx, n_w * n_d)
    _lib.check(ctx._lib.bfhip_acor_moments(ctx.handle, n_w, n_t, n_d, ldw, _ptr(xd), _ptr(m.view), _ptr(v.view)))
    torch.cuda.synchronize(ctx.device)
    return m.numpy((n_w, n_d), 'mean'), v.numpy((n_w, n_d), 'inv'), (m, v)


def _device_lag_sums(ctx, xd, shape, ldw, mean_d, inv_d, t0, n_lag):
    """out (n_lag, n_d) numpy; work is given exactly min(n_w, 256) n_lag n_d doubles."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    n_w, n_t, n_d = shape
    work, out = _Out(ctx, min(n_w, 256) * n_lag * n_d), _Out(ctx, n_lag * n_d)
    _lib.check(ctx._lib.bfhip_acor_lag_sums(ctx.handle, n_w, n_t, n_d, ldw, _ptr(xd), _ptr(mean_d), _ptr(inv_d), t0, n_lag,
                                            _ptr(work.view), _ptr(out.view)))
    torch.cuda.synchronize(ctx.device)
    work.check_outside('work')
    return out.numpy((n_lag, n_d), 'out')


def _lag_sums_of(ctx, x, mean, inv, t0, n_lag, pad):
    """The lag sums of host arrays x, mean and inv."""
    xb, xd, ldw = _place_x(ctx, x, pad)
    mb, md = _between_nan(ctx, mean)
    vb, vd = _between_nan(ctx, inv)
    return _device_lag_sums(ctx, xd, x.shape, ldw, md, vd, t0, n_lag)


def _plus_zero(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.int64) == 0))


# ---- a. exact cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ac.EXACT, ids=ac.case_id)
def test_exact_cases_equal_the_reference_at_every_lag(case):
    """Small integers, integer means and power-of-two inv: no rounding anywhere, so any difference is an indexing, guard or halo
    mistake.  ac.paths(case) names the paths the case takes."""
    ctx = _ctx()
    x, mean, inv = ac.exact_inputs(case)
    want = ac.exact_reference(case)
    got = _lag_sums_of(ctx, x, mean, inv, case.t0, case.n_lag, case.pad)
    assert np.array_equal(got, want), (ac.paths(case), np.argwhere(got != want)[:8])
    beyond = max(case.n_t - case.t0, 0)
    assert _plus_zero(got[beyond:]), 'lags >= n_t are +0'


# ---- b. float cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ac.FLOAT, ids=ac.case_id)
def test_float_cases_within_the_worst_case_bound_of_a_sum(case):
    """|out - S| <= (n_terms + 8) U A.  S is a sum of n_terms = n_w (n_t - t) products of two centred values, each walker's share
    times its inv; A is the same sum of absolute values.  Summed in any order, a term passes at most n_terms - 1 additions that
    round (adding the 0 of an empty slot or of the padding does not), each within a factor 1 +- U; the two centred values carry one
    rounding each, the inv multiply one, the reference's own rounding to float64 is one half, and the products are not rounded
    (fma): (1 + U)^(n_terms + 2.5) - 1 <= (n_terms + 8) U for n_terms U < 1e-9.  A dropped or doubled term is of the order of
    A / n_terms, 1 / (n_terms^2 U) > 1e5 times the bound.  Observed (docs/EXPERIMENTS.md): at most 6.2 U A."""
    ctx = _ctx()
    x = ac.float_inputs(case)
    mean, inv, s, a = ac.float_reference(case)
    got = _lag_sums_of(ctx, x, mean, inv, case.t0, case.n_lag, case.pad)
    n_terms = ac.n_terms(case)[:, None]
    assert n_terms.max() * U < 1e-9
    err = np.abs(got.astype(LD) - s)
    live = a > 0
    print('\nacor float case %s: max |out - S| / (U A) = %.3g (bound %d .. %d)'
          % (ac.case_id(case), float((err[live] / (U * a[live])).max()), n_terms[live.any(axis=1)].min() + 8, n_terms.max() + 8))
    assert np.all(err <= (n_terms + 8) * LD(U) * a)
    assert _plus_zero(got[max(case.n_t - case.t0, 0):])


# ---- c. moments -------------------------------------------------------------------------------------------------------------------

def _check_moments(ctx, x, pad, tag):
    """mean: |mean - mu| <= (n_t + 4) U mean(|x|) =: D.  The sum of n_t values in any order errs by at most (n_t - 1) U sum |x|, the
    division and the reference's rounding add one U |mu| <= U mean(|x|) each.

    inv against the kernel's own mean m: a(0; m) = sum (x - m)^2.  Each difference rounds once and enters squared (2 U), a term
    passes at most n_t - 1 rounding additions, the reciprocal rounds once: the relative error of a sum of positive terms is at
    most r = (n_t + 4) U, and that of its reciprocal r / (1 - r).

    inv against the true a(0) = a(0; mu): sum (x - m)^2 = a(0) + n_t (m - mu)^2 exactly, since sum (x - mu) = 0.  With |m - mu| <= D
    the centring adds at most c a(0), c = n_t D^2 / a(0), so the relative error is r2 = r (1 + c) + c, and r2 / (1 - r2) for
    the reciprocal.  (One ulp of error in the mean gives the n_t (U |mu|)^2 of a typical run; the worst case carries D.)"""
    n_w, n_t, n_d = x.shape
    xb, xd, ldw = _place_x(ctx, x, pad)
    m, inv, _ = _device_moments(ctx, xd, x.shape, ldw)
    xl = x.astype(LD)
    mu = xl.sum(axis=1) / LD(n_t)
    a0 = ((xl - mu[:, None, :])**2).sum(axis=1)
    m_ref, inv_ref = ar.moments(x, ldw)
    assert np.array_equal(m_ref, mu.astype(np.float64))
    absx = np.abs(xl).mean(axis=1)
    d_bound = (n_t + 4) * LD(U) * absx
    m_err = np.abs(m.astype(LD) - m_ref.astype(LD))
    assert np.all(m_err <= d_bound), float((m_err / (LD(U) * absx)).max())
    const = a0 == 0
    a0k = ar.a0_about(x, m)
    assert np.array_equal(a0k == 0, const)
    assert np.all(inv[const] == np.inf) and np.all(inv_ref[const] == np.inf)
    r = (n_t + 4) * LD(U)
    live = ~const
    if live.any():
        rel_own = np.abs(inv.astype(LD)[live] * a0k[live] - 1)
        assert np.all(rel_own <= r / (1 - r)), float((rel_own / LD(U)).max())
        c = n_t * d_bound[live]**2 / a0[live]
        assert np.all(c < 1e-6)          # (the check keeps its meaning: a one-pass variance errs by n_t U mu^2 / a(0))
        r2 = r * (1 + c) + c
        rel = np.abs(inv.astype(LD)[live] / inv_ref.astype(LD)[live] - 1)
        assert np.all(rel <= r2 / (1 - r2) + LD(U)), float((rel / LD(U)).max())   # (+ U: inv_ref is rounded to float64)
        ulp_c = float((n_t * (m.astype(LD) - mu)[live]**2 / a0[live]).max())
        print('\nacor moments %s %s: mean err %.3g U mean|x| (bound %d), inv err about own mean %.3g U (bound %d), about the true '
              'mean %.3g U (bound %.3g U); centring term n_t (m - mu)^2 / a(0) = %.3g'
              % (tag, x.shape, float((m_err / (LD(U) * absx)).max()), n_t + 4, float((rel_own / LD(U)).max()), n_t + 4,
                 float((rel / LD(U)).max()), float((r2 / LD(U)).max()), ulp_c))
    return m, inv


@pytest.mark.parametrize('shape', ac.MOMENT_SHAPES, ids=lambda s: 'w%d-t%d-d%d' % s)
def test_moments_at_the_corners_of_the_grid(shape):
    ctx = _ctx()
    m, inv = _check_moments(ctx, ac.moment_inputs(shape), 0, 'grid')
    if shape[1] == 1:   # one step: the mean is the value, the centred sum of squares 0
        assert np.array_equal(m, ac.moment_inputs(shape)[:, 0]) and np.all(inv == np.inf)


def test_moments_of_a_series_far_from_zero():
    """Offset 1e8, unit spread, 500 steps: a(0) is about 500, and sum x^2 - n_t mean^2 would be a difference of two numbers near
    5e18 whose ulp is 1024.  The two passes keep a(0) to the bounds of _check_moments; there x - mean is exact (Sterbenz) and
    the centring term is n_t (m - mu)^2 <= n_t ((n_t + 4) U 1e8)^2 = 1.6e-8, 3e-11 of a(0)."""
    ctx = _ctx()
    x = ac.offset_inputs()
    assert x.shape[1] == 500 and np.abs(x - ac.OFFSET).max() < 6
    _, inv = _check_moments(ctx, x, 0, 'offset 1e8')
    assert np.all((1 / inv > 400.) & (1 / inv < 600.))   # (500 unit variances: nothing like the 1e3 a lost digit would leave)


def test_moments_constant_column_padded_stride_and_nan_gaps():
    """A constant column (2.5: its sums are exact, so the mean is 2.5 and every centred value 0) has inv = +inf exactly, next to
    live columns; the walker stride is padded and the padding holds NaN."""
    ctx = _ctx()
    for shape, pad in (((5, 70, 3), 7), ((17, 33, 17), 1), ((257, 16, 2), 3)):
        x = ac.moment_inputs(shape).copy()
        x[:, :, 1] = 2.5
        m, inv = _check_moments(ctx, x, pad, 'padded')
        assert np.all(m[:, 1] == 2.5) and np.all(inv[:, 1] == np.inf) and np.isfinite(np.delete(inv, 1, axis=1)).all()
        tight_m, tight_inv = _check_moments(ctx, x, 0, 'tight')
        assert tight_m.tobytes() == m.tobytes() and tight_inv.tobytes() == inv.tobytes()


# ---- d. block independence and repeatability --------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(6, 150, 5), (257, 70, 3)], ids=lambda s: 'w%d-t%d-d%d' % s)
def test_a_lag_does_not_depend_on_its_block_and_calls_repeat(shape):
    """One call over lags 0 .. n_t + 4, then the same lags from every (t0, n_lag) of the exact grid: equal bytes, and +0 past the
    one call's range (all >= n_t).  Column 1 is constant: inv = inf, NaN at every lag < n_t and +0 from n_t on in whichever block.
    The same call again, and the padded stride against the contiguous copy, give equal bytes."""
    ctx = _ctx()
    n_w, n_t, n_d = shape
    x = ac.float_inputs(ac.Case(n_w, n_t, n_d, 0, n_t + 5, 0)).copy()
    x[:, :, 1] = 2.5
    xb, xd, ldw = _place_x(ctx, x, 0)
    pb, pd, pldw = _place_x(ctx, x, 11)
    _, _, (m, v) = _device_moments(ctx, xd, shape, ldw)
    _, _, (pm, pv) = _device_moments(ctx, pd, shape, pldw)
    assert np.array_equal(m.bits(), pm.bits()) and np.array_equal(v.bits(), pv.bits())
    full = _device_lag_sums(ctx, xd, shape, ldw, m.view, v.view, 0, n_t + 5)
    assert np.isnan(full[:n_t, 1]).all() and np.isfinite(np.delete(full[:n_t], 1, axis=1)).all() and _plus_zero(full[n_t:])
    assert _device_lag_sums(ctx, xd, shape, ldw, m.view, v.view, 0, n_t + 5).tobytes() == full.tobytes()
    assert _device_lag_sums(ctx, pd, shape, pldw, pm.view, pv.view, 0, n_t + 5).tobytes() == full.tobytes()
    whole = np.concatenate([full, np.zeros((ac.T0[-1] + ac.N_LAG[-1], n_d))])
    for t0 in ac.T0:
        for n_lag in ac.N_LAG:
            piece = _device_lag_sums(ctx, xd, shape, ldw, m.view, v.view, t0, n_lag)
            assert piece.tobytes() == whole[t0:t0 + n_lag].tobytes(), (t0, n_lag)
            if (t0 + n_lag) % 3 == 0:
                assert _device_lag_sums(ctx, pd, shape, pldw, pm.view, pv.view, t0, n_lag).tobytes() == piece.tobytes(), (t0, n_lag)


# ---- e. a non-finite sample stays in its column -----------------------------------------------------------------------------------

@pytest.mark.parametrize('bad', [np.nan, np.inf], ids=['nan', 'inf'])
@pytest.mark.parametrize('shape,at', [((5, 100, 3), (2, 50, 1)),      # td = 4: the neighbours are k = 0 and 2 of the same walker
                                      ((257, 40, 3), (100, 39, 1)),   # wpg = 2, ws_n = 4: walker 101 shares the tile, same k
                                      ((3, 70, 16), (1, 0, 7)),       # td = 16
                                      ((2, 300, 8), (0, 299, 7))],    # the last step of the second chunk, the tile's last dimension
                         ids=['td4', 'shared-tile', 'td16', 'last-step'])
def test_a_non_finite_sample_makes_its_column_nan_and_no_other(shape, at, bad):
    """Moments from the device, as the public path has them: the series' mean is NaN, or +inf with centred values -inf and NaN, and
    its 1 / a(0) is NaN either way, so its column is NaN at every lag < n_t; every other column keeps the bytes of the clean run; lags >= n_t are +0 in every column.  (With a finite mean
    supplied instead, which lags of the column turn NaN is not part of the contract: include/bfhip.h.)"""
    ctx = _ctx()
    n_w, n_t, n_d = shape
    clean = ac.float_inputs(ac.Case(n_w, n_t, n_d, 0, n_t + 5, 0))
    dirty = clean.copy()
    dirty[at] = bad
    outs = []
    for x in (clean, dirty):
        xb, xd, ldw = _place_x(ctx, x, 0)
        mean, inv, (m, v) = _device_moments(ctx, xd, shape, ldw)
        outs.append((mean, inv, _device_lag_sums(ctx, xd, shape, ldw, m.view, v.view, 0, n_t + 5),
                     _device_lag_sums(ctx, xd, shape, ldw, m.view, v.view, 17, 63)))
    k = at[2]
    assert np.isnan(outs[1][1][at[0], k])           # inv; the mean is NaN, or +inf for +inf
    for a, b in zip(outs[0][:2], outs[1][:2]):      # the moments: one (w, k) is not finite, the others keep their bytes
        assert not np.isfinite(b[at[0], k]) and np.isfinite(a).all()
        b = b.copy()
        b[at[0], k] = a[at[0], k]
        assert a.tobytes() == b.tobytes()
    for a, b, t0 in ((outs[0][2], outs[1][2], 0), (outs[0][3], outs[1][3], 17)):
        live = max(min(n_t - t0, a.shape[0]), 0)
        assert np.isfinite(a).all() and np.isnan(b[:live, k]).all()
        assert _plus_zero(b[live:]) and _plus_zero(a[live:])
        assert np.delete(a, k, axis=1).tobytes() == np.delete(b, k, axis=1).tobytes()


# ---- f. arguments -----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_by_name_before_anything_is_launched():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    xin = torch.zeros(64, dtype=torch.float64, device=ctx.device)
    ones = torch.ones(8, dtype=torch.float64, device=ctx.device)
    outs = [_Out(ctx, 64) for _ in range(4)]
    X, M, V, N = _ptr(xin), _ptr(ones), _ptr(ones), None
    OM, OV, W, O = (_ptr(o.view) for o in outs)
    good_m = (2, 10, 3, 30, X, OM, OV)
    good_l = (2, 10, 3, 30, X, M, V, 0, 1, W, O)

    def swap(args, i, v):
        return tuple(v if j == i else a for j, a in enumerate(args))

    bad = {
        # (n_w, n_t, n_d, ldw, x, mean, inv): sizes below 1, a stride below n_t n_d, each null pointer
        'bfhip_acor_moments': [swap(good_m, 0, 0), swap(good_m, 0, -1), swap(good_m, 1, 0), swap(good_m, 1, -5), swap(good_m, 2, 0),
                               swap(good_m, 2, -1), swap(good_m, 3, 29), swap(good_m, 3, 0)] + [swap(good_m, i, N) for i in (4, 5, 6)],
        # (n_w, n_t, n_d, ldw, x, mean, inv, t0, n_lag, work, out): the same, t0 < 0, n_lag < 1, more than 65535 tiles of 64 lags
        'bfhip_acor_lag_sums': [swap(good_l, 0, 0), swap(good_l, 0, -1), swap(good_l, 1, 0), swap(good_l, 1, -5), swap(good_l, 2, 0),
                                swap(good_l, 2, -1), swap(good_l, 3, 29), swap(good_l, 3, 0), swap(good_l, 7, -1), swap(good_l, 8, 0),
                                swap(good_l, 8, -64), swap(good_l, 8, 65535 * 64 + 1)] + [swap(good_l, i, N) for i in (4, 5, 6, 9, 10)],
    }
    for name, arg_sets in bad.items():
        f = getattr(ctx._lib, name)
        for args in arg_sets:
            with pytest.raises(ValueError, match=name):
                _lib.check(f(None, *args))
            with pytest.raises(ValueError, match=name):
                _lib.check(f(ctx.handle, *args))
    torch.cuda.synchronize(ctx.device)
    assert all(o.untouched() for o in outs)
    # the valid calls the rows were made from do run, and write their documented sizes
    _lib.check(ctx._lib.bfhip_acor_moments(ctx.handle, *good_m))
    _lib.check(ctx._lib.bfhip_acor_lag_sums(ctx.handle, *good_l))
    torch.cuda.synchronize(ctx.device)
    assert not any(o.untouched() for o in outs)
    for o, n in zip(outs, (6, 6, 6, 3)):   # mean, inv (n_w n_d), work (min(n_w, 256) n_lag n_d), out (n_lag n_d)
        b = o.bits()
        assert np.all(b[GUARD + n:] == SENTINEL) and np.all(b[:GUARD] == SENTINEL) and not np.any(b[GUARD:GUARD + n] == SENTINEL)
