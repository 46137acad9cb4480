"""PolyModel.fit_ridge on the device against the loop reference of tests/helpers/ridge_reference.py, and bfhip_ridge_path on its own.

Shapes (inputs, order, n, outputs, weighted) are chosen for the tile edges of the path kernel (64 rows, 16 outputs, 8 penalties a
sweep, steps of four directions) and for both routes: on the primal side r = 14; 77; 62 with n one past 256; 135 with one output past
a batch of 16; on the dual side r = n - 1 = 19 (without and with weights), 59, 64 (n one past 64) and 128.  The penalties are those
for which the reference's own two routes agree to 1e-10 (tests/test_fit_ridge_host.py has the figures: none is dropped).  Everything is
held to the project's 1e-9 for the device against a loop reference, arrays relative to their largest magnitude: the same arithmetic
in NumPy sits at 1.2e-12 or better on these inputs, so the bound leaves room for the device's eigen-decomposition, not for a wrong
formula.  bfhip_ridge_path against NumPy loops on its own inputs is held to 1e-12.  Each test prints every figure before it asserts."""
import copy
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import loo_reference as lr  # noqa: E402
import ridge_reference as rr  # noqa: E402
from oracle import reference  # noqa: E402

RTOL = 1e-9
EXPLICIT = rr.PRIMAL[:2] + rr.DUAL[:2]


def model(order, n_in, m, use_bound=False):
    from bayesfast_amd import PolyModel
    return PolyModel(order, input_size=n_in, output_size=m, bound_options=dict(use_bound=use_bound))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def path_figures(rep, path, g=0, outs=None):
    """The report's per-point arrays at the chosen penalty and its path tables against the references of a path (one design group)."""
    refs = path['refs']
    ref = refs[path['index']]
    outs = list(range(ref['q2'].size)) if outs is None else outs
    return dict(leverage=rel(rep.leverage[g], ref['leverage']), residual=rel(rep.residual[:, outs], ref['residual']),
                loo_residual=rel(rep.loo_residual[:, outs], ref['loo_residual']),
                dof=rel(rep.dof[g], [r['dof'] for r in refs]),
                press_path=rel(rep.press_path[outs], np.stack([r['press'] for r in refs], axis=1)),
                q2_path=rel(rep.q2_path[outs], np.stack([r['q2'] for r in refs], axis=1)),
                rmse_path=rel(rep.rmse_path[outs], np.stack([r['rmse'] for r in refs], axis=1)),
                score_path=rel(rep.score_path[g], path['score']))


def assert_gap(path):
    """The reference's best and second-best scores differ by more than 1e-6 relative: the choice is not a matter of rounding."""
    sc = np.sort(path['score'])
    print('scores', path['score'], 'best', path['index'])
    assert sc[1] - sc[0] > 1e-6 * sc[0]


@pytest.mark.parametrize('shape', rr.PRIMAL + rr.DUAL)
def test_report_choice_and_predictions_against_reference(shape):
    n_in, order, n, m, weighted = shape
    x, y, w, path = rr.case(shape)
    rhos = rr.rhos_of(shape)
    mod = model(order, n_in, m)
    rep = mod.fit_ridge(x, y, w=w, ridge=rhos)
    print(rep)
    assert mod.fit_report is rep
    ref = path['refs'][path['index']]
    assert rep.n == n and rep.n_param == (ref['P'],) and rep.group_of_output.tolist() == [0] * m
    assert rep.ridge_path.tolist() == list(rhos) and rep.n_unit_leverage.tolist() == [0]
    figures = path_figures(rep, path)
    for k in ('rmse', 'loo_rmse', 'r2', 'q2', 'max_abs_loo'):
        figures[k] = rel(getattr(rep, k), ref[k])
    # predictions: the fitted model at fresh points against the reference's coefficients on the helper's design
    xs = np.random.default_rng(n + 1).standard_normal((32, n_in))
    want = lr.design(xs, order) @ ref['coef']
    got = mod.fun_and_jac_batch(xs, jac=False)[0].cpu().numpy()
    figures['predictions'] = rel(got, want)
    figures['fun'] = rel(np.stack([mod.fun(xi)[0] for xi in xs]), want)
    print(shape, figures, 'dof', rep.dof, 'max h', rep.leverage[0].max())
    assert_gap(path)
    assert rep.ridge_index.tolist() == [path['index']] and rep.ridge.tolist() == [rhos[path['index']]]
    assert rep.at_edge.tolist() == [path['index'] in (0, len(rhos) - 1)]
    for k, v in figures.items():
        assert v <= RTOL, (k, v)
    assert np.array_equal(rep.argmax_abs_loo, ref['argmax_abs_loo'])
    assert rep.leverage[0].min() >= 0. and rep.leverage[0].max() < 1.


@pytest.mark.parametrize('shape', EXPLICIT)
def test_loo_residuals_against_explicit_refits(shape):
    n_in, order, n, m, weighted = shape
    x, y, w, path = rr.case(shape)
    rhos = rr.rhos_of(shape)
    rep = model(order, n_in, m).fit_ridge(x, y, w=w, ridge=rhos)
    explicit = rr.ridge_loo_explicit(x, y, order, float(rep.ridge[0]), w)
    err = rel(rep.loo_residual, explicit)
    print(shape, 'rho', rep.ridge, 'loo vs explicit refits', err)
    assert err <= RTOL


def test_default_grid_and_repeatable():
    from bayesfast_amd.modules.ridge import DEFAULT_RIDGE
    shape = rr.DUAL[2]
    x, y, w, _ = rr.case(shape)
    mod = model(shape[1], shape[0], shape[3])
    a = mod.fit_ridge(x, y)
    coef = [np.array(c._coef) for c in mod.configs]
    print(a)
    assert a.ridge_path.tolist() == list(DEFAULT_RIDGE) and a.dof.shape == (1, 15)
    assert np.all(np.diff(a.dof[0]) < 0.) and a.dof[0, 0] < shape[2] and a.dof[0, -1] > 1.
    assert a.at_edge[0] == (a.ridge_index[0] in (0, 14)) and a.ridge[0] == DEFAULT_RIDGE[a.ridge_index[0]]
    b = mod.fit_ridge(x, y)
    assert a == b
    for c0, c1 in zip(coef, [np.array(c._coef) for c in mod.configs]):
        assert np.array_equal(c0, c1)
    assert copy.deepcopy(a) == a


def _ridge_on_fit_checks(make, shape):
    x, y, w, _ = rr.case(shape)
    rhos = rr.rhos_of(shape)
    mod = make()
    with pytest.raises(ValueError, match='I need at least'):
        mod.fit(x, y, w=w)
    want = make().fit_ridge(x, y, w=w, ridge=rhos)
    mod.ridge_on_fit = rhos
    assert mod.fit(x, y, w=w) is None
    assert mod.fit_report is not None and mod.fit_report == want
    mod.ridge_on_fit = True
    mod.fit(x, y, w=w)
    assert len(mod.fit_report.ridge_path) == 15
    mod.ridge_on_fit = False
    xl, yl, _ = lr.make_case(shape[0], 2 * mod.n_param, shape[3], False, seed=1)
    mod.fit(xl, yl)
    assert mod.fit_report is None
    return mod, want


def test_ridge_on_fit_leaves_the_report():
    shape = rr.DUAL[2]
    _ridge_on_fit_checks(lambda: model(shape[1], shape[0], shape[3]), shape)


@pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')
def test_ridge_on_fit_through_the_reference_subclass():
    from bayesfast_amd import integrate
    bf = reference.load()
    seam = integrate.reference_classes(bf)
    shape = rr.DUAL[2]
    make = lambda: seam.PolyModel(shape[1], input_size=shape[0], output_size=shape[3], bound_options=dict(use_bound=False))  # noqa: E731
    pm = make()
    assert isinstance(pm, bf.modules.PolyModel) and pm.ridge_on_fit is False and pm.fit_report is None
    _, want = _ridge_on_fit_checks(make, shape)
    x, y, w, _ = rr.case(shape)
    ours = model(shape[1], shape[0], shape[3])
    assert ours.fit_ridge(x, y, w=w, ridge=rr.rhos_of(shape)) == want
    pm.fit_ridge(x, y, w=w, ridge=rr.rhos_of(shape))
    for mine, theirs in zip(pm.configs, ours.configs):
        assert np.array_equal(np.asarray(mine._coef), np.asarray(theirs._coef))
    assert pm.ridge_on_fit is False


def test_two_design_groups():
    """Output 0 has a linear and a quadratic config (P = 28, n = 25: the dual side), output 1 the linear one alone (P = 7: the
    primal side): two paths, two chosen penalties, each against its own reference."""
    from bayesfast_amd import PolyConfig, PolyModel
    x, y, w = lr.make_case(6, 25, 2, True, seed=25)
    mod = PolyModel([PolyConfig('linear'), PolyConfig('quadratic', output_mask=[0])], input_size=6, output_size=2,
                    bound_options=dict(use_bound=False))
    rep = mod.fit_ridge(x, y, w=w, ridge=rr.RHO_DUAL)
    print(rep)
    paths = [rr.ridge_path_reference(x, y[:, :1], 'quadratic', rr.RHO_DUAL, w), rr.ridge_path_reference(x, y[:, 1:], 'linear', rr.RHO_DUAL, w)]
    assert rep.n_param == (28, 7) and rep.group_of_output.tolist() == [0, 1] and len(rep.leverage) == 2
    xs = np.random.default_rng(26).standard_normal((32, 6))
    got = mod.fun_and_jac_batch(xs, jac=False)[0].cpu().numpy()
    for g, (path, order) in enumerate(zip(paths, ('quadratic', 'linear'))):
        assert_gap(path)
        figures = path_figures(rep, path, g, [g])
        figures['predictions'] = rel(got[:, g], (lr.design(xs, order) @ path['refs'][path['index']]['coef'])[:, 0])
        print(g, figures)
        assert rep.ridge_index[g] == path['index']
        for k, v in figures.items():
            assert v <= RTOL, (g, k, v)


def test_workspace_smaller_than_one_pass(monkeypatch):
    """Six tiles of rows through a workspace of two tiles, and of one: three and six passes, the same bits."""
    from bayesfast_amd.modules import poly
    shape = rr.PRIMAL[3]
    x, y, w, _ = rr.case(shape)
    rhos = rr.rhos_of(shape)

    def run():
        mod = model(shape[1], shape[0], shape[3])
        return mod.fit_ridge(x, y, w=w, ridge=rhos), [np.array(c._coef) for c in mod.configs]

    whole, coef = run()
    for cap in (2 * 64 * 135, 1):   # r = 135
        monkeypatch.setattr(poly, 'RIDGE_WORKSPACE_DOUBLES', cap)
        passes, coef_p = run()
        assert passes == whole
        assert np.array_equal(passes.sums, whole.sums) and np.array_equal(passes.press_path, whole.press_path)
        for c0, c1 in zip(coef, coef_p):
            assert np.array_equal(c0, c1)


def test_touch_after_fit_ridge():
    """A SurrogateDensity whose device copy exists evaluates the coefficients of a later fit_ridge on its surrogate."""
    from bayesfast_amd import PolyModel, SurrogateDensity
    d = 4
    rng = np.random.default_rng(11)
    den = SurrogateDensity(PolyModel('quadratic', input_size=d, output_size=1, bound_options=dict(use_bound=False)))
    xf = rng.standard_normal((40, d))
    logp = -0.5 * np.sum(xf * xf, axis=1)
    den.fit(xf, logp)
    x = rng.standard_normal((10, d))
    before = np.array(den.logp(x))
    den.surrogate.fit_ridge(xf[:12], (logp + 0.5 * xf[:, 0])[:12, None], logp[:12], ridge=[0.1, 1.])   # (12 points, 15 parameters)
    after = np.array(den.logp(x))
    # the new coefficients by hand: constant and linear part of the linear config, the upper triangle of the quadratic one
    lin, quad = (np.array(c._coef)[0] for c in den.surrogate.configs)
    want = lin[0] + x @ lin[1:] + np.einsum('ij,jk,ik->i', x, quad, x)
    print('moved by', np.max(np.abs(after - before)), 'against the new coefficients', rel(after, want))
    assert not np.allclose(after, before)
    assert rel(after, want) <= 1e-12


# ---- bfhip_ridge_path through ctypes ----
def _loops(Z, Lam, T, lams, Bp, Bw, h0, w, complement):
    n, r = Z.shape
    m, L = T.shape[1], len(lams)
    h, sums = np.zeros((n, L)), np.zeros((L, m, 8))
    resid, e_loo = np.zeros((L, n, m)), np.zeros((L, n, m))
    for l in range(L):
        for i in range(n):
            sh, sf = 0., np.zeros(m)
            for j in range(r):
                g = (lams[l] if complement else 1.) / (Lam[j] + lams[l])
                sh += Z[i, j]**2 * g
                sf += Z[i, j] * T[j] * g
            d = sh if complement else 1. - (h0[i] + sh)
            h[i, l] = 1. - d if complement else h0[i] + sh
            S = sf if complement else Bp[i] - sf
            for o in range(m):
                inf = -np.inf if S[o] < 0. else np.inf
                sl, el = (S[o] / d, S[o] / (d * w[i])) if d > 0. else (inf, inf)
                resid[l, i, o], e_loo[l, i, o] = S[o] / w[i], el
                s = sums[l, o]
                s[0] += S[o]**2
                s[1] += sl**2
                if abs(el) > s[2] or i == 0:
                    s[2], s[3] = abs(el), i
                s[4] += Bw[i, o]
                s[5] += Bw[i, o]**2
                s[6] += 0. if d > 0. else 1.
    return h, sums, resid, e_loo


def _call(ctx, arrays, lams, complement, with_resid, rows=None, row0=0, sums=None, sentinel=-7.):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    Z, Lam, T, Bp, Bw, h0, w = (ctx.tensor(np.ascontiguousarray(a), torch.float64) for a in arrays)
    n, r = Z.shape if rows is None else (rows, Z.shape[1])
    m, L = T.shape[1], len(lams)
    lam_t = ctx.tensor(np.asarray(lams, dtype=np.float64), torch.float64)
    h = torch.full((n, L), sentinel, dtype=torch.float64, device=ctx.device)
    if sums is None:
        sums = torch.full((L, m, 8), sentinel, dtype=torch.float64, device=ctx.device)
    resid = torch.full((n, m), sentinel, dtype=torch.float64, device=ctx.device)
    e_loo = torch.full((n, m), sentinel, dtype=torch.float64, device=ctx.device)
    nw = _lib.ridge_work(n, r, m, L)
    work = ctx.zeros((nw,))
    rc = ctx._lib.bfhip_ridge_path(ctx.handle, n, r, m, L, _ptr(Z[row0:]), Z.shape[1], _ptr(Lam), _ptr(T), _ptr(lam_t), _ptr(Bp[row0:]),
                                   _ptr(Bw[row0:]), _ptr(h0[row0:]), _ptr(w[row0:]), int(complement), row0, _ptr(h), _ptr(sums),
                                   _ptr(resid) if with_resid else None, _ptr(e_loo) if with_resid else None, _ptr(work), nw)
    assert rc == 0
    ctx.synchronize()
    return dict(h=h.cpu().numpy(), sums=sums.cpu().numpy(), resid=resid.cpu().numpy(), e_loo=e_loo.cpu().numpy(), sums_t=sums)


def _kernel_inputs(complement):
    rng = np.random.default_rng(130 + complement)
    n, r, m = 130, 70, 17
    Z = 0.08 * rng.standard_normal((n, r))
    Lam = np.abs(rng.standard_normal(r)) * 3.
    Lam[0] = 1.
    T, Bp, Bw = rng.standard_normal((r, m)), rng.standard_normal((n, m)), rng.standard_normal((n, m))
    h0, w = 0.1 * rng.random(n), np.exp(0.3 * rng.standard_normal(n))
    if not complement:   # the crafted row: z = 2 on the direction with Lam = 1, so h = 2 at lambda = 1
        Z[77] = 0.
        Z[77, 0] = 2.
        h0[77] = 0.
    return Z, Lam, T, Bp, Bw, h0, w


@pytest.mark.parametrize('complement', [0, 1])
@pytest.mark.parametrize('L', [1, 15, 32])
def test_binding_against_loops(L, complement):
    from bayesfast_amd.device import get_context
    ctx = get_context()
    arrays = _kernel_inputs(complement)
    lams = np.concatenate([[1.], np.exp(np.random.default_rng(L).uniform(-3., 3., L - 1))])
    h, sums, resid, e_loo = _loops(arrays[0], arrays[1], arrays[2], lams, *arrays[3:], complement)
    a = _call(ctx, arrays, lams, complement, L == 1)
    b = _call(ctx, arrays, lams, complement, False)
    for k in ('h', 'sums'):
        assert np.array_equal(a[k], b[k])   # two calls: the same bits
    assert np.all(b['resid'] == -7.) and np.all(b['e_loo'] == -7.)   # NULL resid / e_loo: nothing is written
    fin = np.isfinite(sums)
    figures = dict(h=rel(a['h'], h), sums=float(np.max(np.abs(a['sums'][fin] / np.where(sums[fin] == 0., 1., sums[fin]) - (sums[fin] != 0.)))))
    if L == 1:
        ef = np.isfinite(e_loo[0])
        figures.update(resid=rel(a['resid'], resid[0]), e_loo=rel(a['e_loo'][ef], e_loo[0][ef]))
        assert np.array_equal(a['e_loo'][~ef], e_loo[0][~ef])
    print(L, complement, figures)
    for k, v in figures.items():
        assert v <= 1e-12, (k, v)
    assert np.array_equal(a['sums'][~fin], sums[~fin]) and np.array_equal(a['sums'][:, :, [3, 6, 7]], sums[:, :, [3, 6, 7]])
    if not complement:
        # the crafted row at lambda = 1: h = 2, an infinite held-out residual with the sign of S, counted
        assert abs(a['h'][77, 0] - 2.) <= 1e-15
        assert np.all(a['sums'][0, :, 6] == 1.) and np.all(np.isinf(a['sums'][0, :, 1])) and np.all(np.isinf(a['sums'][0, :, 2]))
        assert np.all(a['sums'][0, :, 3] == 77.)
        # (h = 4 / (1 + lambda) there: the other penalties count the row while lambda <= 3, as the loops do -- compared above)
        if L == 1:
            assert np.array_equal(a['e_loo'][77], np.where(resid[0][77] < 0., -np.inf, np.inf))
    # rows in passes: 64 rows, then the other 66 onto the same sums
    first = _call(ctx, arrays, lams, complement, False, rows=64)
    second = _call(ctx, arrays, lams, complement, False, rows=66, row0=64, sums=first['sums_t'])
    assert np.array_equal(second['sums'], a['sums'])
    assert np.array_equal(np.concatenate([first['h'], second['h']]), a['h'])


def test_binding_argument_errors():
    import torch
    from bayesfast_amd.device import get_context, _ptr
    ctx = get_context()
    t = ctx.zeros((4096,))
    p = _ptr(t)

    def call(n=8, r=2, m=1, L=1, row0=0, resid=p, e_loo=p, nw=4096):
        return ctx._lib.bfhip_ridge_path(ctx.handle, n, r, m, L, p, r, p, p, p, p, p, None, None, 0, row0, p, p, resid, e_loo, p, nw)

    assert call(L=0) == -1 and call(L=33) == -1
    assert call(resid=p, e_loo=None) == -1 and call(resid=None, e_loo=p) == -1
    assert call(L=2) == -1                       # resid and e_loo only for L = 1
    assert call(row0=32) == -1 and call(nw=10) == -1
    ctx.synchronize()
    assert torch.all(t == 0.)                    # nothing was launched
