"""PolyModel.fit_loo on the device against the loop reference of tests/helpers/loo_reference.py.

Shapes (inputs, order, n, outputs, weighted) are chosen for the block structure of the factor (64 x 64 blocks): P = 15 one partial
block; 78 a full and a ragged one; 64 exactly one, with n one past a multiple of 256; 128 two full ones; 136; 595 the factorisation's
two-panels-per-pass path (taken from 576 columns).  The designs are well conditioned (column-equilibrated condition number at most
23, largest leverage about 0.9, so 1 / (1 - h) amplifies by about ten): Cholesky of the equilibrated Gram matrix and QR differ by a few
1e-15 in h.  Everything is held to the project's 1e-9 for the device against a loop reference, arrays relative to their largest
magnitude.  Each test prints every figure before it asserts."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import loo_reference as lr  # noqa: E402

RTOL = 1e-9
SHAPES = [(4, 'quadratic', 40, 3, False), (4, 'quadratic', 40, 3, True), (11, 'quadratic', 200, 2, False),
          (63, 'linear', 257, 2, False), (127, 'linear', 300, 1, True), (15, 'quadratic', 333, 5, True),
          (33, 'quadratic', 1500, 2, True)]
EXPLICIT = SHAPES[:4]   # the three smallest shapes (the first of them weighted and unweighted)


@functools.lru_cache(maxsize=None)
def case(n_in, order, n, m, weighted):
    x, y, w = lr.make_case(n_in, n, m, weighted, seed=n)
    return x, y, w, lr.reference(x, y, order, w)


def model(order, n_in, m, use_bound=False):
    """(the extrapolation bound is host work on x alone and not what is tested here: off, but for the loo_on_fit test)"""
    from bayesfast_amd import PolyModel
    return PolyModel(order, input_size=n_in, output_size=m, bound_options=dict(use_bound=use_bound))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def coefs(mod):
    return [np.array(c._coef) for c in mod.configs]


@pytest.mark.parametrize('n_in,order,n,m,weighted', SHAPES)
def test_report_against_reference(n_in, order, n, m, weighted):
    x, y, w, ref = case(n_in, order, n, m, weighted)
    mod = model(order, n_in, m)
    rep = mod.fit_loo(x, y, w=w)
    print(rep)
    assert rep.n == n and rep.n_param == (ref['P'],) and rep.group_of_output.tolist() == [0] * m
    assert rep.rank_deficient.tolist() == [False] and rep.n_unit_leverage.tolist() == [0]
    h = rep.leverage[0]
    figures = dict(leverage=rel(h, ref['leverage']), residual=rel(rep.residual, ref['residual']),
                   loo_residual=rel(rep.loo_residual, ref['loo_residual']))
    for k in ('rmse', 'loo_rmse', 'r2', 'q2', 'max_abs_loo'):
        figures[k] = float(np.max(np.abs(getattr(rep, k) / ref[k] - 1)))
    print((n_in, order, n, m, weighted), figures, 'sum h - P', h.sum() - ref['P'], 'max h', h.max())
    for k, v in figures.items():
        assert v <= RTOL, (k, v)
    assert h.min() >= 0. and h.max() <= 1.
    assert abs(h.sum() - ref['P']) <= 1e-9 * ref['P']
    assert np.array_equal(rep.argmax_abs_loo, ref['argmax_abs_loo'])


@pytest.mark.parametrize('n_in,order,n,m,weighted', EXPLICIT)
def test_loo_residuals_against_explicit_refits(n_in, order, n, m, weighted):
    x, y, w, _ = case(n_in, order, n, m, weighted)
    rep = model(order, n_in, m).fit_loo(x, y, w=w)
    explicit = lr.loo_explicit(x, y, order, w)
    err = rel(rep.loo_residual, explicit)
    print((n_in, order, n, m, weighted), 'loo vs explicit refits', err)
    assert err <= RTOL


@pytest.mark.parametrize('n_in,order,n,m,weighted', [SHAPES[1], SHAPES[5], SHAPES[6]])
def test_coefficients_bitwise_and_repeatable(n_in, order, n, m, weighted):
    x, y, w, _ = case(n_in, order, n, m, weighted)
    plain, loo = model(order, n_in, m), model(order, n_in, m)
    plain.fit(x, y, w=w)
    assert plain.fit_report is None
    a = loo.fit_loo(x, y, w=w)
    for c0, c1 in zip(coefs(plain), coefs(loo)):
        assert np.array_equal(c0, c1)
    b = loo.fit_loo(x, y, w=w)
    assert np.array_equal(a.leverage[0], b.leverage[0])
    assert a == b


def test_loo_on_fit_leaves_the_report():
    x, y, w, _ = case(*SHAPES[5])
    mod = model('quadratic', 15, 5, use_bound=True)
    logp = -0.5 * np.sum(x * x, axis=1)
    want = mod.fit_loo(x, y, logp, w)
    assert mod.fit_report is want
    mod.fit(x, y, logp, w)
    assert mod.fit_report is None
    mod.loo_on_fit = True
    assert mod.fit(x, y, logp, w) is None
    assert mod.fit_report is not None and mod.fit_report == want
    mod.loo_on_fit = False
    mod.fit(x, y, logp, w)
    assert mod.fit_report is None


def test_workspace_smaller_than_one_pass(monkeypatch):
    """Six tiles of design rows through a workspace of two slices: three passes, the same bits."""
    from bayesfast_amd.modules import poly
    x, y, w, ref = case(*SHAPES[5])
    whole = model('quadratic', 15, 5).fit_loo(x, y, w=w)
    monkeypatch.setattr(poly, 'LOO_WORKSPACE_DOUBLES', 2 * 3 * 64 * 64)   # P = 136: three blocks, a slice is 3 * 64 * 64 doubles
    passes = model('quadratic', 15, 5).fit_loo(x, y, w=w)
    assert passes == whole
    monkeypatch.setattr(poly, 'LOO_WORKSPACE_DOUBLES', 1)   # (at least one slice is always given)
    one = model('quadratic', 15, 5).fit_loo(x, y, w=w)
    assert one == whole
    print('leverage', rel(one.leverage[0], ref['leverage']))
    assert rel(one.leverage[0], ref['leverage']) <= RTOL


def test_two_design_groups():
    """Output 0 has a linear and a quadratic config, output 1 the linear one alone: two designs, two factorisations."""
    from bayesfast_amd import PolyConfig, PolyModel
    x, y, w = lr.make_case(6, 150, 2, True, seed=150)
    mod = PolyModel([PolyConfig('linear'), PolyConfig('quadratic', output_mask=[0])], input_size=6, output_size=2,
                    bound_options=dict(use_bound=False))
    rep = mod.fit_loo(x, y, w=w)
    print(rep)
    refs = [lr.reference(x, y[:, :1], 'quadratic', w), lr.reference(x, y[:, 1:], 'linear', w)]
    assert rep.n_param == (28, 7) and rep.group_of_output.tolist() == [0, 1] and len(rep.leverage) == 2
    for g, ref in enumerate(refs):
        figures = dict(leverage=rel(rep.leverage[g], ref['leverage']), residual=rel(rep.residual[:, g], ref['residual'][:, 0]),
                       loo_residual=rel(rep.loo_residual[:, g], ref['loo_residual'][:, 0]))
        for k in ('rmse', 'loo_rmse', 'r2', 'q2'):
            figures[k] = abs(getattr(rep, k)[g] / ref[k][0] - 1)
        print(g, figures)
        for k, v in figures.items():
            assert v <= RTOL, (g, k, v)


def test_duplicated_input_is_rank_deficient():
    """5 inputs, the fifth equal to the second, quadratic, n = 120: P = 21, rank 15.  The group goes through the fit's eigenvalue
    fallback and its leverages come from the same kept subspace, against the hat diagonal of the design's truncated SVD.
    The same arithmetic in NumPy (eigh of the Gram matrix with the fit's cut of 1e-11 of the largest eigenvalue) differs from the SVD
    by 2.3e-15 of the largest leverage on this input, measured on the CPU; ten times that is below the project's 1e-9 for the
    device against a loop reference, which is therefore the bound."""
    x, y, _ = lr.make_case(5, 120, 2, False, seed=120)
    x[:, 4] = x[:, 1]
    mod = model('quadratic', 5, 2)
    with pytest.warns(RuntimeWarning, match='rank deficient'):
        rep = mod.fit_loo(x, y)
    print(rep)
    h_ref, rank = lr.leverage_svd(lr.design(x, 'quadratic'))
    h = rep.leverage[0]
    print('rank', rank, 'sum h', h.sum(), 'leverage', rel(h, h_ref))
    assert rank == 15 and rep.n_param == (21,)
    assert rep.rank_deficient.tolist() == [True]
    assert abs(h.sum() - 15.) <= 1e-9 * 15.
    assert rel(h, h_ref) <= 1e-9
    # the residuals of the minimum-norm fit are those of any least-squares solution: the reference's own
    c = np.linalg.lstsq(lr.design(x, 'quadratic'), y, rcond=None)[0]
    st = lr.stats_from(y - lr.design(x, 'quadratic') @ c, h_ref, y, None)
    for k in ('residual', 'loo_residual'):
        print(k, rel(getattr(rep, k), st[k]))
        assert rel(getattr(rep, k), st[k]) <= RTOL
    for k in ('rmse', 'loo_rmse', 'r2', 'q2'):
        print(k, np.max(np.abs(getattr(rep, k) / st[k] - 1)))
        assert np.max(np.abs(getattr(rep, k) / st[k] - 1)) <= RTOL


def _lstsq_loo_raw(A, B, with_outputs, sentinel=-7.):
    """bfhip_lstsq_loo (or bfhip_lstsq for with_outputs None) through ctypes on device copies of A and B."""
    import torch
    from bayesfast_amd.device import get_context, _ptr
    from bayesfast_amd import _lib
    ctx = get_context()
    n, P = A.shape
    m = B.shape[1]
    At, Bt = ctx.tensor(A, torch.float64), ctx.tensor(B, torch.float64)
    G, c = ctx.zeros((P, P)), ctx.zeros((P, m))
    work = ctx.zeros((n * m + P * m,))
    info = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    h = torch.full((n,), sentinel, dtype=torch.float64, device=ctx.device)
    e = torch.full((n, m), sentinel, dtype=torch.float64, device=ctx.device)
    s = torch.full((m, _lib.LOO_NSUM), sentinel, dtype=torch.float64, device=ctx.device)
    n_ws = -(-P // 64) * 64 * 64 * -(-n // 64)
    ws = ctx.zeros((n_ws,))
    head = (ctx.handle, n, P, m, _ptr(At), P, _ptr(Bt), _ptr(G), _ptr(c), 2, _ptr(work), _ptr(info))
    if with_outputs is None:
        _lib.check(ctx._lib.bfhip_lstsq(*head))
    elif with_outputs:
        _lib.check(ctx._lib.bfhip_lstsq_loo(*head, _ptr(h), _ptr(e), _ptr(s), None, _ptr(ws), n_ws))
    else:
        _lib.check(ctx._lib.bfhip_lstsq_loo(*head, None, None, None, None, None, 0))
    ctx.synchronize()
    return dict(G=G.cpu().numpy(), c=c.cpu().numpy(), info=int(info.item()), h=h.cpu().numpy(), e=e.cpu().numpy(), s=s.cpu().numpy())


def test_binding_null_outputs_reproduce_lstsq_and_argument_errors():
    from bayesfast_amd.device import get_context, _ptr
    x, y, w, ref = case(*SHAPES[2])
    A = lr.design(x, 'quadratic')
    plain, null, full = _lstsq_loo_raw(A, y, None), _lstsq_loo_raw(A, y, False), _lstsq_loo_raw(A, y, True)
    for r in (null, full):
        assert r['info'] == 0
        assert np.array_equal(r['c'], plain['c']) and np.array_equal(r['G'], plain['G'], equal_nan=True)
    assert np.all(null['h'] == -7.) and np.all(null['e'] == -7.) and np.all(null['s'] == -7.)
    print('leverage', rel(full['h'], ref['leverage']), 'sums', np.max(np.abs(full['s'][:, :3] / ref['sums'][:, :3] - 1)))
    assert rel(full['h'], ref['leverage']) <= RTOL
    assert rel(full['e'], ref['loo_residual']) <= RTOL
    np.testing.assert_allclose(full['s'][:, [0, 1, 2, 4, 5]], ref['sums'][:, [0, 1, 2, 4, 5]], rtol=RTOL, atol=0)
    assert np.array_equal(full['s'][:, [3, 6, 7]], ref['sums'][:, [3, 6, 7]])
    # outputs that do not come together, or no workspace: refused
    import torch
    ctx = get_context()
    t = ctx.zeros((64 * 64 * 8,))
    info = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    head = (ctx.handle, 8, 2, 1, _ptr(t), 2, _ptr(t), _ptr(t), _ptr(t), 0, _ptr(t), _ptr(info))
    assert ctx._lib.bfhip_lstsq_loo(*head, _ptr(t), None, _ptr(t), None, _ptr(t), 4096) == -1
    assert ctx._lib.bfhip_lstsq_loo(*head, _ptr(t), _ptr(t), _ptr(t), None, None, 0) == -1
    assert ctx._lib.bfhip_lstsq_loo(*head, _ptr(t), _ptr(t), _ptr(t), None, _ptr(t), 4095) == -1


def test_binding_rank_deficient_leaves_outputs_untouched():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((90, 70))
    A[:, 69] = A[:, 3]
    B = rng.standard_normal((90, 2))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        r = _lstsq_loo_raw(A, B, True)
    print('info', r['info'])
    assert r['info'] != 0
    assert np.all(r['h'] == -7.) and np.all(r['e'] == -7.) and np.all(r['s'] == -7.)
