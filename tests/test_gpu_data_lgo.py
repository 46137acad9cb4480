"""Leave-group-out cross-validation on the device (csrc/bfhip_igamc.h, csrc/bfhip_lgo.h: ``bfhip_igamc``, ``bfhip_lgo_accum``,
``bfhip_lgo_finish``) through ctypes and through ``bayesfast_amd.utils.grouped_loo`` / ``data_lgo``, against the mpmath fixture
tests/golden/igamc.npz, the NumPy loop of helpers/lgo_reference.py and its loop-written reference.

Sizes.  The stages: 24 | 25 the smallest fitted tail, 225 the crossing of the two tail-size rules, 257 a workgroup's 256 threads and
16-row slices plus one, 4097, and 262145, the first size at which the 1024 workgroups of the strided reductions stride.  The
accumulation has one row per thread in workgroups of 256: n = 1, 255 | 256 | 257, 4097; both of its paths (two doubles per load where
the strides are even, single doubles at a row stride of 19).

Tolerances.  ``bfhip_igamc``: relative error at most 16 times the largest relative error of scipy's own ``gammaincc`` on the same
grid, which the fixture holds (device lgamma / exp / log are a few ulp where the host's libm is below one, and the prefactor's
exponent of size ~a amplifies them); below Q = 1e-290 the same bound, absolute.  The accumulation is exact.  The stages' floating
figures are held to 1e-9 relative, the project's figure for a device route against a loop reference; ``ROUNDING`` has ten times the
largest relative difference between the float64 and the numpy.longdouble reference per figure on these very inputs, measured on the
CPU (docs/EXPERIMENTS.md has the table): every entry is below 1e-9, so RTOL holds.  n_tail, flags and NaN patterns are exact.  Each
test prints every figure before it asserts."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import lgo_reference as lr  # noqa: E402
from lgo_cases import RTOL, FIGURES, chi2_case, compare  # noqa: E402
from psis_reference import tail_size  # noqa: E402

STAGE_SIZES = (24, 25, 225, 257, 4097, 262145)
# ten times the largest relative float64-against-longdouble difference of the reference over chi2_case(n, weighting), n in STAGE_SIZES,
# 'plain' and 'weights', the four columns (p_lgo of max(|lpd|, |elpd_lgo|)): every one is below 1e-9, so RTOL holds
ROUNDING = dict(lpd=2.7e-13, p_waic=3.3e-13, elpd_waic=2.1e-13, elpd_lgo=3e-11, p_lgo=3e-11, khat=6.7e-13, sigma=8.1e-13, ess_lgo=2.2e-12,
                chi2_base=1e-13, chi2_lgo=2.5e-13, ppp_base=1.9e-13, ppp_lgo=4.8e-11)


def _ctx():
    from bayesfast_amd.device import get_context
    return get_context()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- 1: Q(a, x) ------------------------------------------------------------------------------------------------------------------------
def igamc(a, x):
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    ad, xd = ctx.tensor(np.asarray(a, dtype=np.float64)), ctx.tensor(np.asarray(x, dtype=np.float64))
    out = torch.full_like(ad, -7.)
    _lib.check(ctx._lib.bfhip_igamc(ctx.handle, ad.numel(), _ptr(ad), _ptr(xd), _ptr(out)))
    return _np(out)


def test_igamc_against_the_fixture():
    fx = np.load(os.path.join(HERE, 'golden', 'igamc.npz'))
    a, x, q, serr = fx['a'], fx['x'], fx['q'], fx['scipy_err']
    big = q >= 1e-290
    bound = 16. * serr[big].max()
    got = igamc(a, x)
    rel = np.abs(got[big] - q[big]) / q[big]
    i = int(np.argmax(rel))
    print('bfhip_igamc: %d points; largest relative error %.3g at a = %g, x = %g (bound %.3g = 16 x scipy\'s %.3g); largest absolute error '
          'below 1e-290: %.3g' % (a.size, rel[i], a[big][i], x[big][i], bound, serr[big].max(), np.abs(got[~big] - q[~big]).max()))
    assert np.all(rel <= bound)
    assert np.all(np.abs(got[~big] - q[~big]) <= bound)
    assert np.all(got[x == 0.] == 1.) and np.all((got >= 0.) & (got <= 1.))
    inf, nan = np.inf, np.nan
    sp = igamc([0.5, 3., 1024., 2., nan, 2., nan, 0., -1., 2.], [0., 0., inf, inf, 1., nan, nan, 1., 1., -1.])
    assert sp[:2].tolist() == [1., 1.] and sp[2:4].tolist() == [0., 0.] and np.isnan(sp[4:]).all()


# ---- 2: the accumulation ---------------------------------------------------------------------------------------------------------------
def accum(zd, ldz, nb, slots, c, start, acc, n=None, lda=16):
    from bayesfast_amd import _lib
    ctx = _ctx()
    n = acc.shape[0] if n is None else n
    cc = None if c is None else (C.c_double * 16)(*[float(v) for v in c])
    sl = None if slots is None else (C.c_int * max(len(slots), 1))(*[int(s) for s in slots])
    return ctx._lib.bfhip_lgo_accum(ctx.handle, n, _ptr(zd), ldz, nb, sl, cc, start, _ptr(acc), lda)


@pytest.mark.parametrize('ldz', [16, 19])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 4097])
def test_accum_is_the_numpy_loop(n, ldz):
    """A plan of calls on one (n, 16) buffer of slots, every call checked bit for bit against the NumPy loop: a group of 1; a group of
    17 split 16 + 1 into slot 0 and 2 + 15 into slot 15 (the same bits in both); a group of 33 over three calls; a group that begins in
    one call and ends in the next beside two others; two groups interleaved in one call; nb = 1 and 15; untouched slots keep what they
    held."""
    import torch
    ctx = _ctx()
    rng = np.random.default_rng(n + ldz)
    c = rng.normal(size=16) * 3.
    z17, z33 = rng.standard_normal((n, 17)) * 1.3, rng.standard_normal((n, 33))
    zs = rng.standard_normal((n, 32))
    acc = torch.full((n, 16), -7., dtype=torch.float64, device=ctx.device)
    want = np.full((n, 16), -7.)

    def call(z, slots, start):
        nonlocal want
        buf = np.full((n, ldz), np.nan)
        buf[:, :z.shape[1]] = z
        mask = sum(1 << s for s in start)
        assert accum(ctx.tensor(buf), ldz, z.shape[1], slots, c, mask, acc) == 0
        want = lr.accum_reference(z, slots, c, want, start)
        assert _np(acc).tobytes() == want.tobytes(), (n, ldz, slots)

    call(zs[:, :1], [3], [3])                                       # a group of 1 (nb = 1)
    call(z17[:, :16], [0] * 16, [0])                                # 17 = 16 + 1 into slot 0
    call(z17[:, 16:], [0], [])
    call(z17[:, :2], [15, 15], [15])                                # 17 = 2 + 15 into slot 15 (nb = 15)
    call(z17[:, 2:], [15] * 15, [])
    loop = np.full(n, c[0])
    for j in range(17):
        loop = loop - 0.5 * (z17[:, j] * z17[:, j])
    assert want[:, 0].tobytes() == loop.tobytes()
    for k0 in (0, 16, 32):                                          # 33 over three calls into slot 7
        call(z33[:, k0:k0 + 16], [7] * min(16, 33 - k0), [7] if k0 == 0 else [])
    call(zs[:, :16], [4] * 10 + [5] * 6, [4, 5])                    # group 5 begins here ...
    call(zs[:, 16:32], [5] * 9 + [6] * 7, [6])                      # ... and ends here, beside group 6 that begins
    call(zs[:, :12], [8, 9] * 6, [8, 9])                            # two groups interleaved
    call(zs[:, :5], [-1, 2, -1, 2, -1], [2])                        # columns that go nowhere
    assert np.all(want[:, [1, 10, 11, 12, 13, 14]] == -7.)
    # the same group in slot 0 and slot 15: restart slot 15 from slot 0's constant
    c2 = c.copy()
    c2[15] = c[0]
    acc2 = torch.full((n, 16), -7., dtype=torch.float64, device=ctx.device)
    for part, st in ((z17[:, :2], 1 << 15), (z17[:, 2:], 0)):
        buf = np.zeros((n, ldz))
        buf[:, :part.shape[1]] = part
        assert accum(ctx.tensor(buf), ldz, part.shape[1], [15] * part.shape[1], c2, st, acc2) == 0
    assert _np(acc2)[:, 15].tobytes() == _np(acc)[:, 0].tobytes()


# ---- 3: the stages against the loop reference ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(n, weighted, col):
    """chi2_case's column ``col`` (all four up to n = 4097: col is None) with its reference"""
    q, dof, const, lw = chi2_case(n, 'weights' if weighted else 'plain')
    cols = list(range(q.shape[1])) if col is None else [col]
    return q[:, cols], dof[cols], const[cols], lw, [lr.group_reference(q[:, j], dof[j], const[j], lw) for j in cols]


STAGE_CASES = [(n, None) for n in STAGE_SIZES if n <= 4097] + [(n, j) for n in STAGE_SIZES if n > 4097 for j in range(4)]


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n,col', STAGE_CASES)
def test_stages_match_the_reference(n, col, weighted):
    """dof 1, 2, 17 and 457 at every size (beyond n = 4097 one column per case: the loop reference takes seconds per column)."""
    from bayesfast_amd.utils import grouped_loo
    ctx = _ctx()
    q, dof, const, lw, refs = stage_case(n, weighted, col)
    qd = ctx.tensor(q)
    got = grouped_loo(qd, dof, const, log_weights=lw)
    for j, r in enumerate(refs):
        for f in FIGURES:
            with np.errstate(all='ignore'):
                print('n=%d w=%d dof=%g' % (n, weighted, dof[j]), f, getattr(got, f)[j], float(r[f]), abs(getattr(got, f)[j] / np.float64(r[f]) - 1))
    compare(got, refs, 'n=%d w=%d' % (n, weighted), ROUNDING)
    assert got.n == n and np.all(np.isinf(got.khat) == (n < 25))
    again = grouped_loo(qd, dof, const, log_weights=lw)
    for f in FIGURES + ('n_tail',):
        assert getattr(got, f).tobytes() == getattr(again, f).tobytes(), f
    if col is None:   # a column's bits do not depend on its slot or its neighbours
        alone = grouped_loo(qd[:, 3:4], dof[3:], const[3:], log_weights=lw)
        for f in FIGURES:
            assert getattr(alone, f)[0].tobytes() == getattr(got, f)[3].tobytes(), f


def test_degenerate_columns_on_the_device():
    """test_data_lgo_host.py's special columns: the device route gives the host port's NaN pattern and flags and the reference's figures."""
    from bayesfast_amd.utils import grouped_loo
    ctx = _ctx()
    n = 1000
    rng = np.random.default_rng(5)
    lw = rng.standard_normal(n)
    lw[rng.random(n) < 0.5] = -np.inf
    lw[7], lw[11] = 0.1, -np.inf
    base = rng.chisquare(3, size=n)
    cols = [base.copy() for _ in range(6)]
    cols[0][7] = np.nan
    cols[1][7] = np.inf
    cols[2][11] = np.nan
    cols[3] *= 2.
    cols[4] = np.round(base / 0.1) * 0.1
    cols[5][:] = 4.
    q = np.stack(cols, axis=1)
    dof, const = np.full(6, 3.), np.full(6, -1.5)
    got = grouped_loo(ctx.tensor(q), dof, const, log_weights=lw)
    host = grouped_loo(q, dof, const, log_weights=lw)
    compare(got, [lr.group_reference(c, 3., -1.5, lw) for c in cols], 'special', waic_abs=(n * 2.3e-16 * 3.5)**2)
    for f in FIGURES:
        assert np.array_equal(np.isnan(getattr(got, f)), np.isnan(getattr(host, f))), f
    assert np.isnan(got.ppp_lgo[[0, 1]]).all() and np.isfinite(got.ppp_lgo[2:]).all()
    few = np.full(n, -np.inf)
    few[[3, 500, 900]] = [0., -1., 0.5]          # fewer rows of weight than the tail: smoothed weight goes to rows of zero weight
    got = grouped_loo(ctx.tensor(q[:, 3:5]), dof[:2], const[:2], log_weights=few)
    compare(got, [lr.group_reference(cols[3], 3., -1.5, few), lr.group_reference(cols[4], 3., -1.5, few)], 'three rows')
    none = grouped_loo(ctx.tensor(q[:, 3:4]), dof[:1], const[:1], log_weights=np.full(n, -np.inf))
    assert all(np.isnan(getattr(none, f)[0]) for f in FIGURES)


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------------------
GROUPS56 = [list(range(17)), list(range(17, 32)), [32, 40]] + [[i] for i in list(range(33, 40)) + list(range(41, 52))]


def test_data_lgo_of_a_pipeline_density():
    """m = 56, d = 4, a dense precision, 4 x 300 points on both sides of the bound, input scales; 21 groups (17, 15, 2, eighteen
    singletons; four outputs in none): two slot batches, and the groups of 17 and 15 lie across the 16-column calls.  ``data_lgo``
    against the reference fed with the restated z = A (y - f) of test_polymodel_kernels.py's extended precision.  z is held to the
    derived model's own bound, 4 (m + _acc_len) EPS sum_j |A_ij| (|y_j| + sf_j); that carries into a group's ell as sum |z| dz, and
    the figures are held to RTOL plus ten times the largest dell (every figure is 1-Lipschitz in a shift of ell up to the PSIS fit,
    whose sensitivity the same factor of ten covers; q moves by twice dell).  Float64 draws, a strided view of them with weights, and
    float32 draws.  The singleton groups agree with ``data_loo`` on the same density within that bound; ``predictive`` before and
    after is byte-equal: the surrogate's own device model came back."""
    import torch
    from test_polymodel_kernels import restate_poly, random_poly, random_points, _acc_len, EPS, LD
    from test_gpu_predictive import _Fixed
    from bayesfast_amd import Chi2PipelineDensity
    from bayesfast_amd.utils import group_whitening_of, data_lgo
    ctx = _ctx()
    rng = np.random.default_rng(561)
    d, m, n_chain, n_draw = 4, 56, 4, 300
    n = n_chain * n_draw
    poly = random_poly(rng, d, m, 'quad')
    pts = random_points(rng, poly, n, far=False)
    su = _Fixed.model(poly)
    lo, hi = rng.normal(size=d) - 3., rng.normal(size=d) + 3.
    su.input_scales = np.stack([lo, hi], 1)
    x_orig = lo + (hi - lo) * pts
    f0 = restate_poly(poly, (x_orig - lo) / (hi - lo), jac=False)[0]
    y = (f0[rng.integers(n)] + 0.3 * rng.normal(size=m)).astype(np.float64)
    bmat = rng.normal(size=(m, m))
    prec = (bmat @ bmat.T / m + 2. * np.eye(m)) / 400.   # (the points spread widely over the bound: at unit scale exp(-ell) overflows)
    den = Chi2PipelineDensity(su, y, prec=prec)
    a, const, sizes, colg = group_whitening_of(prec=prec, groups=GROUPS56)
    al = np.asarray(a, dtype=LD)
    labels = np.full(m, -1)
    for k, g in enumerate(GROUPS56):
        labels[g] = k

    def restated(x_host):
        f, _, sf, _, info = restate_poly(poly, (x_host - lo) / (hi - lo), jac=False)
        assert info['outside'].any() and (~info['outside']).any()
        z = np.einsum('ij,nj->ni', al, y.astype(LD) - f)
        dz = 4 * (m + _acc_len(poly)) * EPS * np.einsum('ij,nj->ni', np.abs(al), np.abs(y.astype(LD)) + sf)
        q = np.stack([(z[:, colg == k]**2).sum(axis=1) for k in range(len(GROUPS56))], axis=1).astype(np.float64)
        dell = float(np.max(np.stack([(np.abs(z) * dz)[:, colg == k].sum(axis=1) for k in range(len(GROUPS56))])))
        return q, dell

    x = ctx.tensor(x_orig.reshape(n_chain, n_draw, d))
    wide = torch.zeros((n_chain, n_draw + 7, d + 3), dtype=torch.float64, device=ctx.device)
    wide[:, 7:, :d] = x
    x32 = x.to(torch.float32)
    lw = 0.3 * rng.standard_normal((n_chain, n_draw))
    before = den.predictive(x, outputs=[0, 55])
    q64, dell64 = restated(x_orig)
    q32, dell32 = restated(_np(x32).astype(np.float64).reshape(n, d))
    print('largest dell', dell64, dell32)
    for label, draws, weights, q, dell, groups in (('float64', x, None, q64, dell64, GROUPS56), ('strided', wide[:, 7:, :d], lw, q64, dell64, labels),
                                                  ('float32', x32, None, q32, dell32, GROUPS56)):
        got = den.data_lgo(draws, groups, log_weights=weights)
        assert got.n == n and got.size.tolist() == sizes.tolist() and [g.tolist() for g in got.groups] == GROUPS56
        for k in range(len(GROUPS56)):
            ref = lr.group_reference(q[:, k], sizes[k], const[k], weights)
            assert got.n_tail[k] == ref['n_tail']
            for fig in FIGURES:
                g, r = getattr(got, fig)[k], np.float64(ref[fig])
                print(label, k, fig, g, r, abs(g / r - 1))
                scale = 1. if fig in ('lpd', 'p_waic', 'elpd_waic', 'elpd_lgo', 'p_lgo') else abs(r)
                assert np.isfinite(r) and abs(g - r) <= RTOL * abs(r) + 10. * dell * max(scale, 1.), (label, k, fig)
        if label == 'float64':
            single = [k for k in range(len(GROUPS56)) if sizes[k] == 1]
            loo = den.data_loo(x, outputs=[GROUPS56[k][0] for k in single])
            for f, g in (('lpd', 'lpd'), ('p_waic', 'p_waic'), ('elpd_lgo', 'elpd_loo'), ('khat', 'khat'), ('ess_lgo', 'ess_loo')):
                u, v = getattr(got, f)[single], getattr(loo, g)
                assert np.all(np.abs(u - v) <= RTOL * np.abs(v) + 10. * dell * np.maximum(np.abs(v) if f in ('khat', 'ess_lgo') else 1., 1.)), f
            assert data_lgo(den, x, GROUPS56).ppp_lgo.tobytes() == got.ppp_lgo.tobytes()
    after = den.predictive(x, outputs=[0, 55])
    for name in before.table.names:
        assert before.table[name].tobytes() == after.table[name].tobytes(), name
    assert _np(before.chi2).tobytes() == _np(after.chi2).tobytes()
    assert 'elpd_lgo' in str(got)


# ---- 5: seams and refusals -------------------------------------------------------------------------------------------------------------
def test_trace_data_lgo_after_sample(monkeypatch):
    """d = 3, m = 5, 4 chains x 60 iterations with 20 of warm-up: ``tt.data_lgo(density, groups)`` and ``density.data_lgo`` are
    ``data_lgo`` on the view ``_diag_input`` hands out, byte for byte, with ``since_iter`` and ``log_weights``."""
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import data_lgo
    rng = np.random.default_rng(6)
    d, m = 3, 5
    su = bfa.PolyModel('quadratic', input_size=d, output_size=m)
    xf = rng.normal(size=(4 * su.n_param, d))
    qc = rng.normal(size=(m, d, d)) * 0.2
    a_lin = rng.normal(size=(d, m))
    model = lambda v: np.einsum('ni,kij,nj->nk', v, qc, v) + v @ a_lin
    yf = model(xf)
    y = model(np.zeros((1, d)) + 0.1)[0]
    den = bfa.Chi2PipelineDensity(su, y, prec_diag=np.full(m, 4.))
    den.fit(xf, -0.5 * 4. * ((yf - y)**2).sum(axis=1), y=yf)
    tt = bfa.sample(den, bfa.NTrace(n_chain=4, n_iter=60, n_warmup=20, x_0=rng.normal(size=(4, d)) * 0.1, random_generator=7),
                    verbose=False)
    groups = [[0, 3], [1], [2, 4]]
    view = tt._diag_input(None, False, True, 'samples')
    got, want, mine = tt.data_lgo(den, groups), data_lgo(den, view, groups), den.data_lgo(view, groups)
    for f in FIGURES:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes() == getattr(mine, f).tobytes(), f
    assert np.isfinite(got.elpd_lgo).all() and np.all((got.ppp_lgo > 0) & (got.ppp_lgo < 1)) and got.n == 160
    lw = 0.2 * rng.standard_normal((4, 30))
    got = tt.data_lgo(den, groups, since_iter=30, log_weights=lw)
    want = data_lgo(den, tt._diag_input(30, False, True, 'samples'), groups, log_weights=lw)
    assert got.n == 120 and got.ppp_lgo.tobytes() == want.ppp_lgo.tobytes()
    with pytest.raises(NotImplementedError):
        data_lgo(den, view.cpu(), groups)
    with pytest.raises(ValueError):
        data_lgo(den, view, [[0, 5]])
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='gather'):
        tt.data_lgo(den, groups)


def test_refusals_leave_the_context_and_the_model_usable():
    import torch
    from test_polymodel_kernels import random_poly, random_points
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel
    ctx = _ctx()
    lib, h = ctx._lib, ctx.handle
    rng = np.random.default_rng(9)
    poly = random_poly(rng, 5, 4, 'quad')
    pts = ctx.tensor(random_points(rng, poly, 40))
    dm = DevicePolyModel(poly, ctx)
    f0 = dm.fun_and_jac(pts, jac=False)[0].clone()
    n = 100
    q = rng.chisquare(3, size=(n, 16))
    series = ctx.tensor(-1.5 - 0.5 * q)
    z = ctx.tensor(rng.standard_normal((n, 16)))
    acc = torch.full((n, 16), -7., dtype=torch.float64, device=ctx.device)
    out = torch.full((_lib.PLOO_NOUT, 16), -7., dtype=torch.float64, device=ctx.device)
    lgo = torch.full((len(_lib.LGO_ROWS), 16), -7., dtype=torch.float64, device=ctx.device)
    val = torch.full((8,), -7., dtype=torch.float64, device=ctx.device)
    keys = torch.zeros((16, tail_size(n) + 1), dtype=torch.int64, device=ctx.device)
    rows = torch.zeros((16, tail_size(n) + 1), dtype=torch.int32, device=ctx.device)
    nbytes = int(lib.bfhip_ploo_work_bytes(n))
    work = ctx.empty((nbytes,), dtype=torch.uint8)
    c16, d16 = (C.c_double * 16)(*([-1.5] * 16)), (C.c_double * 16)(*([3.] * 16))
    bad_dof = (C.c_double * 16)(*([3.] * 15 + [0.]))

    def finish(n=n, s=series, ld=16, nb=16, c=c16, dof=d16, o=out, lg=lgo, wb=nbytes):
        return lib.bfhip_lgo_finish(h, n, _ptr(s), ld, nb, c, dof, None, _ptr(keys), _ptr(rows), _ptr(o), _ptr(lg), _ptr(work), wb)

    for name, kw in {'n = 0': dict(n=0), 'no series': dict(s=None), 'nb = 0': dict(nb=0), 'nb = 17': dict(nb=17), 'ld < nb': dict(ld=8),
                     'no c': dict(c=None), 'no dof': dict(dof=None), 'dof = 0': dict(dof=bad_dof), 'no out': dict(o=None),
                     'no lgo out': dict(lg=None), 'short work buffer': dict(wb=nbytes - 1)}.items():
        assert finish(**kw) == -1, name
        with pytest.raises(ValueError):
            _lib.check(-1)
    assert finish(n=2**31) == -4
    slots = list(range(16))
    for name, rc in {'n = 0': accum(z, 16, 16, slots, [0.] * 16, 0xffff, acc, n=0), 'no z': accum(None, 16, 16, slots, [0.] * 16, 0xffff, acc),
                     'nb = 0': accum(z, 16, 0, slots, [0.] * 16, 0xffff, acc), 'nb = 17': accum(z, 17, 17, slots + [0], [0.] * 16, 0xffff, acc),
                     'ldz < nb': accum(z, 8, 16, slots, [0.] * 16, 0xffff, acc), 'no map': accum(z, 16, 16, None, [0.] * 16, 0xffff, acc),
                     'slot 16': accum(z, 16, 16, [16] * 16, [0.] * 16, 0, acc), 'slot -2': accum(z, 16, 16, [-2] * 16, [0.] * 16, 0, acc),
                     'start without c': accum(z, 16, 16, slots, None, 1, acc), 'start bit 16': accum(z, 16, 16, slots, [0.] * 16, 1 << 16, acc),
                     'lda < 16': accum(z, 16, 16, slots, [0.] * 16, 0xffff, acc, lda=8)}.items():
        assert rc == -1, name
    assert accum(z, 16, 16, slots, [0.] * 16, 0xffff, acc, n=2**31) == -4
    with pytest.raises(NotImplementedError):
        _lib.check(-4)
    for a, x, o, cnt in ((None, val, val, 8), (val, None, val, 8), (val, val, None, 8), (val, val, val, 0)):
        assert lib.bfhip_igamc(h, cnt, _ptr(a), _ptr(x), _ptr(o)) == -1
    assert lib.bfhip_igamc(None, 8, _ptr(val), _ptr(val), _ptr(val)) == -1
    ctx.synchronize()
    assert bool((out == -7.).all()) and bool((lgo == -7.).all()) and bool((acc == -7.).all()) and bool((val == -7.).all())
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
    # the context still works: the three stages on the batch, against the reference
    head = (h, n, _ptr(series), 16, 16, _lib.PLOO_ELL, None, None)
    assert lib.bfhip_ploo_moments(*head, _ptr(out), _ptr(work), nbytes) == 0
    assert lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(keys), _ptr(rows), _ptr(work), nbytes) == 0
    assert finish() == 0
    ctx.synchronize()
    ref = lr.group_reference(q[:, 3], 3., -1.5)
    got = _np(lgo)
    for i, f in enumerate(_lib.LGO_ROWS):
        assert abs(got[i, 3] - ref[f]) <= RTOL * abs(ref[f]), f
    assert abs(_np(out)[3, 3] - ref['elpd_lgo']) <= RTOL * abs(ref['elpd_lgo'])
    assert torch.equal(dm.fun_and_jac(pts, jac=False)[0], f0)
