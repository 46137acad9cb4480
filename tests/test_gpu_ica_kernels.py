"""The kernels of the device-resident FastICA iteration (bayesfast_amd/csrc/bfhip_sit.hip: ``bfhip_ica_tanh``,
``bfhip_ica_assemble``, ``bfhip_ica_post``, ``bfhip_polar_ns``) and the host's chunk logic around them
(``transforms/ica.py``, ``_ica_par_device``) against the restatements of tests/helpers/ica_reference.py: extended-precision
sums, mpmath's tanh, extended-precision Newton-Schulz steps and a plain sequential float64 fixed-point loop.

The shapes take every index branch of the glue kernels (the column loop past 256, row groups with idle threads, more than 256
partial rows, waves past the last row, the 64-column stride), the multi-launch form of the polar iteration and every way the
chunk loop can end.  Every tolerance is a rounding bound in units of EPS = 2^-52 worked out next to it."""
import warnings

import numpy as np
import pytest

from helpers import ica_reference as ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# The device's double-precision tanh: the installed ROCm documents no error bound for it, so the largest distance over the inputs of
# test_ica_tanh_* was measured on the MI355X (see the docstring there).  The distance is taken to the C library's extended-precision
# tanh on every element; mpmath's tanh is run on a sample of 300 elements per case, where it confirms that reference to 1/256 ulp.
# The tests assert at the measured figure plus one ulp, and at 4 ulp at the most: a distance above that would be a finding about
# the function, not a tolerance to follow it.
TANH_ULP_MEASURED = 0.861
TANH_ULP = min(TANH_ULP_MEASURED + 1., 4.)
SENTINEL = -12345.678


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _call(ctx, name, *args):
    import torch
    from bayesfast_amd import _lib
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *args))
    torch.cuda.synchronize(ctx.device)


def _full(ctx, shape, value):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device=ctx.device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- bfhip_ica_tanh -----------------------------------------------------------------------------------------------------

_TANH_D = (1, 3, 48, 100, 256, 257, 300)
_TANH_ROWS = ((1, 1), (31, 32), (33, 40), (400, 400), (1190, 1200))
# (n, n_pad) with whole blocks inside the padding, as the iteration has them (n_pad is a multiple of 400 there): two of four blocks,
# and twelve blocks after a ragged one
_TANH_PADDED = ((33, 100), (1190, 1600))
_TANH_CASES = sorted(set([(d, 33, 40) for d in _TANH_D] + [(d, 1190, 1200) for d in _TANH_D]
                         + [(d, n, n_pad) for d in (100, 300) for n, n_pad in _TANH_ROWS]
                         + [(d, n, n_pad) for d in (48, 100, 257, 300) for n, n_pad in _TANH_PADDED]))


def _run_tanh(ctx, y, n):
    from bayesfast_amd.device import _ptr
    n_pad, d = y.shape
    yd = ctx.tensor(y)
    partial = _full(ctx, (-(-n_pad // ref.ROW_BLOCK), d), SENTINEL)
    _call(ctx, 'bfhip_ica_tanh', n, n_pad, d, _ptr(yd), _ptr(partial))
    return yd.cpu().numpy(), partial.cpu().numpy()


def _check_tanh(y, n, g, partial):
    """The assertions of the tanh kernel on finite-or-not inputs y (n_pad, d); returns the number of counted rows per block."""
    t, part, rows = ref.tanh_partials(y, n)
    dist = ref.ulp_distance(g, t)
    worst = float(dist.max())
    print('largest distance of the device tanh to the reference: %.3f ulp' % worst)
    assert worst <= TANH_ULP                                  # every element, the padding rows included
    assert not np.any(partial == SENTINEL)                    # every partial row was written
    fin = np.isfinite(part.astype(np.float64))
    assert np.array_equal(np.isnan(partial), ~fin)            # (a NaN input reaches its own block and column only)
    # 1 - g^2: |d(1 - g^2)| <= 2 |g| dg + EPS with dg <= U EPS, then a sequential sum of `rows` terms <= 1: rows (2 U + 3) EPS
    atol = (rows * (2 * TANH_ULP + 3) * EPS)[:, None] * np.ones_like(partial)
    err = np.abs(partial.astype(ref.LD) - part).astype(np.float64)
    assert np.all(err[fin] <= atol[fin]), (err[fin] / np.maximum(atol[fin], 1e-300)).max()
    assert (rows == 0).sum() == -(-y.shape[0] // ref.ROW_BLOCK) - -(-n // ref.ROW_BLOCK)
    assert np.all(partial[rows == 0] == 0.)                   # blocks inside the padding: exactly zero
    return rows


@pytest.mark.parametrize('d,n,n_pad', _TANH_CASES)
def test_ica_tanh_is_tanh_and_the_block_sums_of_its_derivative(d, n, n_pad):
    """``bfhip_ica_tanh`` on (n_pad, d): every element, padding included, becomes its tanh; partial[b, c] is the sum of
    1 - tanh^2 over the rows < n of block b; padding rows are deliberately non-zero (they must not be counted), blocks inside the
    padding give exactly 0 and no partial row keeps its sentinel.

    Measured on the MI355X (gfx950): over all these cases the device tanh lies within 0.861 ulp of the reference (0.54 to 0.86 per
    case, the largest at d = 300, 1190 rows), so the tests assert 1.861 ulp.  The extended-precision reference is itself checked
    against mpmath on a sample of every case (within 1/256 ulp).  (33, 100) and (1190, 1600) have two and twelve blocks of
    non-zero padding rows alone."""
    ctx = _ctx()
    rng = np.random.default_rng([17, d, n, n_pad])
    y = rng.normal(0., 1.5, size=(n_pad, d))
    y[n:] = rng.uniform(0.5, 2., size=(n_pad - n, d)) * rng.choice([-1., 1.], size=(n_pad - n, d))
    g, partial = _run_tanh(ctx, y, n)
    rows = _check_tanh(y, n, g, partial)
    if (n, n_pad) in _TANH_PADDED:
        assert (rows == 0).sum() == {(33, 100): 2, (1190, 1600): 12}[n, n_pad]      # (the blocks that must give exactly 0)
    pick = rng.choice(y.size, size=min(y.size, 300), replace=False)
    t_ld, t_mp = ref.tanh_ld(y.ravel()[pick]), ref.tanh_mp(y.ravel()[pick])
    assert np.all(np.abs(t_ld - t_mp) <= 2.**-8 * EPS * np.abs(t_mp))      # (the reference's own error: 1/256 ulp at most)


def test_ica_tanh_passes_special_values_through():
    """0, -0., +-1e-310, +-20, +-750, +-inf and NaN in counted rows of separate columns: tanh(+-inf) is exactly +-1, the sign of
    zero is kept, a subnormal comes back as itself, NaN stays NaN and reaches the partial sum of its own block and column only."""
    ctx = _ctx()
    rng = np.random.default_rng(18)
    n, n_pad, d = 33, 40, 16
    y = rng.normal(0., 1.5, size=(n_pad, d))
    y[n:] = 1.25
    edge = [0., -0., 1e-310, -1e-310, 20., -20., 750., -750., np.inf, -np.inf, np.nan]
    for c, v in enumerate(edge):
        y[5 + c % 3, c] = v
    g, partial = _run_tanh(ctx, y, n)
    _check_tanh(y, n, g, partial)
    got = [g[5 + c % 3, c] for c in range(len(edge))]
    assert got[0] == 0. and not np.signbit(got[0]) and got[1] == 0. and np.signbit(got[1])
    assert got[2] == 1e-310 and got[3] == -1e-310
    assert got[6:10] == [1., -1., 1., -1.]
    assert np.isnan(got[10]) and np.isnan(g).sum() == 1
    assert np.isnan(partial[0, 10]) and np.isnan(partial).sum() == 1


# ---- bfhip_ica_assemble -------------------------------------------------------------------------------------------------

# (d, nb, n_pad, n): d in {1, 3, 48, 257, 300}, nb in {1, 3, 21}, ceil(n_pad / 32) in {1, 13, 256, 257, 600}
_ASSEMBLE_CASES = [(1, 1, 32, 32), (3, 3, 416, 400), (48, 21, 8192, 8000), (48, 3, 8193, 8100), (257, 1, 8224, 8200),
                   (300, 3, 19200, 19000), (257, 21, 19200, 19100), (300, 21, 416, 401), (3, 21, 19200, 1), (1, 3, 8192, 8000),
                   (48, 1, 20, 7)]


@pytest.mark.parametrize('d,nb,n_pad,n', _ASSEMBLE_CASES)
@pytest.mark.parametrize('with_meas', [True, False])
def test_ica_assemble_is_the_mean_product_minus_the_mean_derivative_times_w(d, nb, n_pad, n, with_meas):
    """``bfhip_ica_assemble``: A = (sum_b P[b]) / n - gmean[:, None] W, gmean = colsum(partial) / n, against extended-precision
    sums within the worst-case bound of any summation order (helpers.ica_reference.assemble); n < n_pad shows a division by
    n_pad.  The meas slot (7.0 before) is exactly 0 afterwards, its neighbours and the guard bands around A keep their values;
    without a slot the call writes A alone."""
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    rng = np.random.default_rng([19, d, nb, n_pad, n])
    n_blk = -(-n_pad // ref.ROW_BLOCK)
    p = rng.normal(size=(nb, d, d)) * rng.uniform(0.1, 50., size=(nb, 1, 1))
    partial = rng.normal(size=(n_blk, d)) * 8.
    w = rng.normal(size=(d, d))
    pd, gd, wd = ctx.tensor(p), ctx.tensor(partial), ctx.tensor(w)
    buf = _full(ctx, (d * d + 16,), SENTINEL)
    meas = _full(ctx, (5,), 7.)
    _call(ctx, 'bfhip_ica_assemble', d, nb, _ptr(pd), n, n_pad, _ptr(gd), _ptr(wd), _ptr(buf[8:]), _ptr(meas[2:]) if with_meas else None)
    out = buf.cpu().numpy()
    assert np.all(out[:8] == SENTINEL) and np.all(out[-8:] == SENTINEL)
    a, tol = ref.assemble(p, partial, w, n)
    err = np.abs(out[8:-8].reshape(d, d).astype(ref.LD) - a).astype(np.float64)
    assert np.all(err <= tol), (err / tol).max()
    assert meas.cpu().numpy().tolist() == ([7., 7., 0., 7., 7.] if with_meas else [7.] * 5)
    assert np.array_equal(pd.cpu().numpy(), p) and np.array_equal(gd.cpu().numpy(), partial) and np.array_equal(wd.cpu().numpy(), w)


# ---- bfhip_ica_post -----------------------------------------------------------------------------------------------------

N_MEAS = 10


def _run_post(ctx, w1, w_old, k, resid, slot=0.):
    """Wbuf and meas full of sentinels, meas[k] = slot (0: what the assemble kernel leaves): (W1, W, Wbuf, meas) afterwards."""
    from bayesfast_amd.device import _ptr
    d = w1.shape[0]
    w1d, wd = ctx.tensor(w1), ctx.tensor(w_old)
    wbuf = _full(ctx, (N_MEAS, d, d), SENTINEL)
    meas = _full(ctx, (2, N_MEAS), -3.)
    meas[0, k] = slot
    rd = ctx.tensor(np.array([resid]))
    _call(ctx, 'bfhip_ica_post', d, _ptr(w1d), _ptr(wd), _ptr(rd), k, N_MEAS, _ptr(wbuf), _ptr(meas))
    return w1d.cpu().numpy(), wd.cpu().numpy(), wbuf.cpu().numpy(), meas.cpu().numpy()


def _check_post(w1, w_old, k, resid, out):
    w1_after, w_after, wbuf, meas = out
    assert np.array_equal(_bits(w1_after), _bits(w1))
    assert np.array_equal(_bits(w_after), _bits(w1)) and np.array_equal(_bits(wbuf[k]), _bits(w1))
    others = np.delete(wbuf, k, axis=0)
    assert np.all(others == SENTINEL)
    keep = np.ones((2, N_MEAS), dtype=bool)
    keep[0, k] = keep[1, k] = False
    assert np.all(meas[keep] == -3.)
    assert _bits(meas[1, k]) == _bits(resid)
    return meas[0, k]


_POST_CASES = [(1, 0, 1e-3), (3, 4, 1e-3), (5, 0, 1e-3), (5, 4, 1e-3), (5, 9, 1e-3), (63, 0, 1e-3), (64, 4, 1e-3), (65, 9, 1e-3),
               (65, 4, 1e-9), (130, 0, 1e-3), (300, 4, 1e-3), (300, 9, 1e-9)]


@pytest.mark.parametrize('d,k,size', _POST_CASES)
def test_ica_post_hands_the_iterate_over_and_takes_the_convergence_measure(d, k, size):
    """``bfhip_ica_post``: W1 goes to Wbuf[k] and to W bit for bit, no other slice of Wbuf and no other entry of meas is touched,
    meas[n_meas + k] is resid[0] bit for bit, and meas[k] is max_i | |sum_j W1[i, j] W_old[i, j]| - 1 | within the bound of a
    float64 dot product in any order, (d + 2) EPS max_i sum_j |W1 W_old| (at a perturbation of 1e-9 the measure itself is at
    cancellation level)."""
    ctx = _ctx()
    rng = np.random.default_rng([20, d, k])
    w1 = ref.random_orthogonal(rng, d)
    w_old = w1 + size * rng.normal(size=(d, d))
    resid = float(rng.uniform(1e-14, 1e-12))
    got = _check_post(w1, w_old, k, resid, _run_post(ctx, w1, w_old, k, resid))
    lim, atol = ref.lim_measure(w1, w_old)
    print('lim %.3e (device %.3e), atol %.1e' % (float(lim), got, atol))
    assert abs(ref.LD(got) - lim) <= atol


@pytest.mark.parametrize('d,row', [(1, 0), (5, 4), (130, 0), (130, 129), (300, 257)])
def test_ica_post_reports_a_nan_row_as_an_infinite_measure(d, row):
    """A NaN in one row of W1 gives meas[k] = inf (the atomic maximum works on bit patterns of non-negative doubles: NaN is mapped to
    inf), which the host's finiteness test turns into the fallback."""
    ctx = _ctx()
    rng = np.random.default_rng([21, d, row])
    w1 = ref.random_orthogonal(rng, d)
    w_old = w1 + 1e-3 * rng.normal(size=(d, d))
    w1[row, rng.integers(d)] = np.nan
    got = _check_post(w1, w_old, 3, 2e-13, _run_post(ctx, w1, w_old, 3, 2e-13))
    assert got == np.inf


@pytest.mark.parametrize('d', [5, 130])
def test_ica_assemble_clears_the_slot_ica_post_takes_its_maximum_in(d):
    """The contract between the two kernels: the slot holds 7.0 from an earlier chunk; ``bfhip_ica_assemble`` with meas_k pointing
    at it and then ``bfhip_ica_post`` leave the fresh measure there (an atomic maximum needs the slot cleared first)."""
    from bayesfast_amd.device import _ptr
    ctx = _ctx()
    rng = np.random.default_rng([22, d])
    k, n, n_pad, nb = 4, 390, 400, 1
    w1 = ref.random_orthogonal(rng, d)
    w_old = w1 + 1e-3 * rng.normal(size=(d, d))
    w1d, wd = ctx.tensor(w1), ctx.tensor(w_old)
    pd, gd = ctx.tensor(rng.normal(size=(nb, d, d))), ctx.tensor(rng.normal(size=(-(-n_pad // ref.ROW_BLOCK), d)))
    a = ctx.empty((d, d))
    wbuf = _full(ctx, (N_MEAS, d, d), SENTINEL)
    meas = _full(ctx, (2, N_MEAS), -3.)
    meas[0, k] = 7.
    rd = ctx.tensor(np.array([3e-13]))
    _call(ctx, 'bfhip_ica_assemble', d, nb, _ptr(pd), n, n_pad, _ptr(gd), _ptr(wd), _ptr(a), _ptr(meas[0, k:]))
    _call(ctx, 'bfhip_ica_post', d, _ptr(w1d), _ptr(wd), _ptr(rd), k, N_MEAS, _ptr(wbuf), _ptr(meas))
    lim, atol = ref.lim_measure(w1, w_old)
    m = meas.cpu().numpy()
    assert m[0, k] < 1. and abs(ref.LD(m[0, k]) - lim) <= atol
    assert m[1, k] == 3e-13 and np.all(np.delete(m, k, axis=1) == -3.)


# ---- bfhip_polar_ns: the non-finite contract and the multi-launch form's step parity ----------------------------------------

def _polar_matrix(d):
    rng = np.random.default_rng(d)
    return rng.normal(size=(d, d)) * 0.03 + np.diag(rng.uniform(0.05, 2., size=d))


def _run_polar(ctx, A, n_iter, tiles=0):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd._lib import debug_set
    from bayesfast_amd.device import _ptr
    d = A.shape[0]
    a = ctx.tensor(A)
    work = _full(ctx, (2 * d * d + 80,), np.nan)
    x = _full(ctx, (d, d), np.nan)
    debug_set('polar_tiles', tiles)
    try:
        _lib.check(ctx._lib.bfhip_polar_ns(ctx.handle, d, _ptr(a), _ptr(x), n_iter, _ptr(work), _ptr(work[-1:])))
        torch.cuda.synchronize(ctx.device)
    finally:
        debug_set('polar_tiles', 0)
    return x.cpu().numpy(), float(work[-1])


# (d, polar_tiles): X in LDS (16, 128), row blocks (200), a tile per wave with grid barriers (300), multi-launch (513), and the
# forced forms at d = 128 (1: a tile per wave, 2: row blocks with operands from L2)
@pytest.mark.parametrize('d,tiles', [(16, 0), (128, 0), (200, 0), (300, 0), (513, 0), (128, 1), (128, 2)])
def test_polar_ns_reports_a_non_finite_residual_for_input_it_cannot_factor(d, tiles):
    """A NaN entry, an infinite entry and the all-zero matrix (X_0 = 0 / 0): every form of ``bfhip_polar_ns`` reports a residual that
    is not finite -- the trigger of ``_ica_par_device``'s redo with the host's eigen-decomposition.  (A fixed number of steps: a
    residual that never falls below the threshold ends the launch after n_iter of them.)"""
    ctx = _ctx()
    rng = np.random.default_rng([23, d])
    for kind in ('nan', 'inf', 'zero'):
        A = _polar_matrix(d)
        if kind == 'zero':
            A[:] = 0.
        else:
            A[rng.integers(d), rng.integers(d)] = np.nan if kind == 'nan' else np.inf
        _, res = _run_polar(ctx, A, 4, tiles)
        assert not np.isfinite(res), (kind, res)
    _, res = _run_polar(ctx, _polar_matrix(d), 4, tiles)     # (and the same call on the matrix itself: a finite one)
    assert np.isfinite(res)


def test_polar_ns_multi_launch_form_ends_in_x_after_odd_and_even_step_counts():
    """d = 513 (33 tiles a side, the last one a single row and column wide; 129 k-steps: one ragged step in the last batch of
    eight): three and four Newton-Schulz steps both leave their result in x (the form alternates between x and its workspace and
    picks the start by the parity), equal to the same steps taken in extended precision from the same X_0.  The entries of the
    iterates are below 1 and each is a sum of 513 products of such: 513 EPS times the sums' sizes stays far below 1e-13."""
    ctx = _ctx()
    A = _polar_matrix(513)
    steps = ref.newton_schulz(A, 4)
    for n_iter in (3, 4):
        x, res = _run_polar(ctx, A, n_iter)
        want = steps[n_iter - 1].astype(np.float64)
        np.testing.assert_allclose(x, want, rtol=0, atol=1e-13)
        np.testing.assert_allclose(res, np.abs(want @ want.T - np.eye(513)).max(), rtol=1e-9)


# ---- _ica_par_device: the chunk logic ---------------------------------------------------------------------------------------

_SEEDS = {(1300, 5): 2, (1300, 17): 9, (4000, 48): 6, (3000, 130): 1, (3000, 260): 1}     # (data seeds; FastICA's random_state is 3)
_EXPECTED_ITERATIONS = {(1300, 5): 5, (1300, 17): 10, (4000, 48): 13}
_N_REF = 16
_cache = {}


def _case(n, d):
    """Data, white data, start matrix and the host's sequential iteration (computed once per shape, never modified)."""
    if (n, d) not in _cache:
        x = ref.sources(np.random.default_rng([_SEEDS[n, d], n, d]), n, d)
        x1, w0 = ref.whiten(x), ref.start_matrix(d, 3)
        n_ref = _N_REF if (n, d) in _EXPECTED_ITERATIONS else 1
        iterates, lims, mats = ref.fixed_point_sequence(x1, w0, n_ref)
        if (n, d) in _EXPECTED_ITERATIONS:
            hit = np.flatnonzero(lims < 1e-4)
            if not hit.size or hit[0] + 1 != _EXPECTED_ITERATIONS[n, d]:
                pytest.fail('the data of (%d, %d) no longer converge in %d iterations at tol 1e-4: lim = %r'
                            % (n, d, _EXPECTED_ITERATIONS[n, d], lims))
        cond = np.array([np.linalg.cond(m) for m in mats])        # (of every iteration's assembled matrix)
        growth = ref.growth_ratios(x1, w0, n_ref, iterates, np.random.default_rng(5)) if n_ref > 1 else np.ones(1)
        for v in (lims, growth, *iterates):
            v.setflags(write=False)
        _cache[n, d] = dict(x=x, x1=x1, w0=w0, iterates=iterates, lims=lims, cond=cond, growth=growth)
        print('(%d, %d): cond(A) %r, growth of a 1e-12 perturbation %r' % (n, d, np.round(cond).tolist(), np.round(growth, 2).tolist()))
    c = _cache[n, d]
    assert c['cond'].max() < 1e4
    return c


def _w_atol(c, index):
    """Bound of the device's iterate ``index`` (1-based) against the host's: 5e-13 cond(A) for a single polar factor (the bound of
    test_polar_ns_is_the_orthogonal_polar_factor), A the matrix the host sequence assembled in that iteration.  Later iterates
    inherit the earlier ones' errors through a map that is not contractive before convergence: that bound times twice the ratio
    by which a start perturbed by 1e-12 has moved the host sequence's own iterate of that index (``_case`` prints the ratios
    and the condition numbers)."""
    base = 5e-13 * float(c['cond'][index - 1])
    return base if index == 1 else base * 2. * float(c['growth'][index - 1])


def _assert_iterate(c, W, index):
    atol = _w_atol(c, index)
    print('iterate %d: largest difference to the host sequence %.2e, bound %.2e' % (index, np.abs(W - c['iterates'][index - 1]).max(), atol))
    np.testing.assert_allclose(W, c['iterates'][index - 1], rtol=0, atol=atol)


def _run_device(c, max_iter, tol, clear=True):
    from bayesfast_amd.transforms import ica
    ctx = _ctx()
    if clear:
        ica._DEVICE_STATE.clear()
    return ica._ica_par_device(ctx, ctx.tensor(c['x1'].copy()), c['w0'].copy(), max_iter, tol)


@pytest.fixture
def clean_state():
    from bayesfast_amd.transforms import ica
    ica._DEVICE_STATE.clear()
    yield ica
    ica._DEVICE_STATE.clear()


def _steep_48():
    c = _case(4000, 48)
    lims = c['lims']
    if not np.all(lims[7:12] / lims[8:13] >= 1.8):
        pytest.fail('the 48-d lim sequence no longer falls by 1.8 per iteration from iteration 9 on: %r' % lims)
    return c


@pytest.mark.parametrize('stop_at', [10, 11, 13])
def test_device_fastica_stops_at_the_first_iterate_below_tol(clean_state, stop_at):
    """tol between two adjacent values of the host sequence's lim (their geometric mean; 1e-4 for iteration 13): the device
    iteration stops at the last slot of its first chunk, the first slot of its second, and in the middle of it, with the host
    sequence's iterate of that index."""
    c = _steep_48()
    lims = c['lims']
    tol = 1e-4 if stop_at == 13 else float(np.sqrt(lims[stop_at - 2] * lims[stop_at - 1]))
    assert np.flatnonzero(lims < tol)[0] == stop_at - 1
    W, n_iter, converged = _run_device(c, 200, tol)
    assert converged and n_iter == stop_at
    _assert_iterate(c, W, stop_at)


@pytest.mark.parametrize('max_iter', [1, 3, 10, 13])
def test_device_fastica_ends_on_the_iterate_of_max_iter(clean_state, max_iter):
    """max_iter below a chunk, inside the first and the second chunk and on the chunk boundary, tol = 0 (never met): not converged,
    max_iter iterations, the host sequence's iterate of that index."""
    c = _steep_48()
    W, n_iter, converged = _run_device(c, max_iter, 0.)
    assert not converged and n_iter == max_iter
    _assert_iterate(c, W, max_iter)


@pytest.mark.parametrize('n,d', [(3000, 130), (3000, 260)])
def test_device_fastica_first_iterate_at_large_d(clean_state, n, d):
    """One iteration at d > 64 and d > 256 (the glue kernels' strides and column loop, the row-block and tile-per-wave polar forms
    inside the real pipeline) against the host's first iterate within 5e-13 cond(A)."""
    c = _case(n, d)
    W, n_iter, converged = _run_device(c, 1, 0.)
    assert not converged and n_iter == 1
    _assert_iterate(c, W, 1)


@pytest.mark.parametrize('n,d', [(1300, 5), (1300, 17), (4000, 48)])
def test_device_fastica_converges_with_scikit_learn(clean_state, n, d):
    """tol = 1e-4: the iteration count of the host sequence (5, 10 and 13: inside the eager first chunk, on its last slot, inside the
    replayed second chunk) with its iterate, and ``fastica_device`` end to end gives scikit-learn's components and count."""
    from sklearn.decomposition import FastICA
    ica = clean_state
    c = _case(n, d)
    want = _EXPECTED_ITERATIONS[n, d]
    W, n_iter, converged = _run_device(c, 200, 1e-4)
    assert converged and n_iter == want
    _assert_iterate(c, W, want)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        comp, _, n_dev = ica.fastica_device(c['x'].copy(), random_state=3, ctx=_ctx())
        sk = FastICA(random_state=3, whiten='unit-variance').fit(c['x'].copy())
    assert not [w for w in caught if 'converge' in str(w.message)]      # (neither side gave up on these data)
    assert n_dev == sk.n_iter_ == want
    np.testing.assert_allclose(comp, sk.components_, rtol=1e-6, atol=1e-8)


def test_device_fastica_replayed_graph_repeats_the_eager_run(clean_state):
    """The 13-iteration run twice: the first takes its first chunk eagerly and captures the second; the second run replays the graph
    for both chunks and returns the same bits."""
    ica = clean_state
    c = _steep_48()
    first = _run_device(c, 200, 1e-4)
    mid = dict(ica.GRAPH_STATS)
    second = _run_device(c, 200, 1e-4, clear=False)
    assert mid['failed'] == ica.GRAPH_STATS['failed'] and mid['captured'] == ica.GRAPH_STATS['captured']
    assert ica.GRAPH_STATS['replayed'] == mid['replayed'] + 2
    assert first[1:] == second[1:] == (13, True)
    assert np.array_equal(_bits(first[0]), _bits(second[0]))


def test_device_fastica_falls_back_to_the_host_decorrelation(clean_state, monkeypatch):
    """Two Newton-Schulz steps leave the polar residuals far above the acceptance threshold (asserted on the residuals of the last
    chunk, the ones still on the device): the chunks are redone by ``_ica_step_host``, and the result and count are those of a
    loop of ``_ica_step_host`` alone (the same host function on the same device products: 1e-12)."""
    ica = clean_state
    ctx = _ctx()
    c = _steep_48()
    monkeypatch.setattr(ica, '_NS_ITERS', 2)
    W, n_iter, converged = _run_device(c, 200, 1e-4)
    st = next(iter(ica._DEVICE_STATE.values()))
    assert not np.any(st.meas[1].cpu().numpy() < ica._NS_RESID)      # (the trigger: no slot of the last chunk was accepted)
    x1 = ctx.tensor(c['x1'].copy())
    Wh, lim, count = c['w0'].copy(), np.inf, 0
    while count < 200 and not lim < 1e-4:
        Wh, lim = ica._ica_step_host(ctx, x1, Wh)
        count += 1
    assert converged and n_iter == count
    np.testing.assert_allclose(W, Wh, rtol=0, atol=1e-12)
