"""The ridge path of the fit, the part that needs no GPU: the loop reference checks itself (augmented least squares with the hat
diagonal against n explicit refits), ``ridge_path_host`` -- the NumPy port of the device route's arithmetic -- against that reference
on every shape of tests/test_gpu_fit_ridge.py, the selection rule, ``RidgeReport``, and the argument errors.

Bounds.  The reference's two routes must agree to 1e-10 of the largest held-out residual for a penalty to be tested at all; measured on
the CPU, all shapes and penalties of tests/helpers/ridge_reference.py: at most 2.1e-13 on the primal shapes (rho 1e-6 .. 10) and
1.2e-12 on the dual ones (rho 1e-2 .. 10; (15, quadratic, 65) at 1e-2), so no penalty is dropped.  The explicit refits of the two
largest shapes take tens of seconds and are not repeated here: the two smallest shapes of each side are.  ``ridge_path_host`` against
the reference was measured at 1.2e-12 or better (the same case); it is held to the project's 1e-9 for the same arithmetic on the device,
arrays relative to their largest magnitude."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import loo_reference as lr  # noqa: E402
import ridge_reference as rr  # noqa: E402

RTOL = 1e-9
EXPLICIT = rr.PRIMAL[:2] + rr.DUAL[:2]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def weighted_design(shape):
    x, y, w, _ = rr.case(shape)
    wv = np.ones(shape[2]) if w is None else w
    return lr.design(x, shape[1]) * wv[:, None], y * wv[:, None]


@pytest.mark.parametrize('shape', EXPLICIT)
def test_reference_identity_against_explicit_refits(shape):
    x, y, w, path = rr.case(shape)
    for rho, ref in zip(rr.rhos_of(shape), path['refs']):
        err = rel(ref['loo_residual'], rr.ridge_loo_explicit(x, y, shape[1], rho, w))
        print(shape, rho, 'identity vs explicit refits', err, 'dof', ref['dof'], 'max h', ref['leverage'].max())
        assert err <= 1e-10
        assert ref['leverage'].min() >= 0. and ref['leverage'].max() < 1.


@pytest.mark.parametrize('shape', rr.PRIMAL + rr.DUAL)
def test_host_port_against_reference(shape):
    from bayesfast_amd.modules.ridge import ridge_path_host
    x, y, w, path = rr.case(shape)
    rhos = rr.rhos_of(shape)
    A, B = weighted_design(shape)
    host = ridge_path_host(A, B, rhos, 0, w)
    assert host['dual'] == (shape in rr.DUAL)
    for l, ref in enumerate(path['refs']):
        figures = dict(leverage=rel(host['h'][:, l], ref['leverage']), residual=rel(host['resid'][l], ref['residual']),
                       loo_residual=rel(host['e_loo'][l], ref['loo_residual']), coef=rel(host['coef'][l], ref['coef']),
                       dof=abs(host['dof'][l] / ref['dof'] - 1), press=float(np.max(np.abs(host['sums'][l][:, 1] / ref['press'] - 1))),
                       sse=float(np.max(np.abs(host['sums'][l][:, 0] / ref['sums'][:, 0] - 1))))
        print(shape, rhos[l], figures)
        for k, v in figures.items():
            assert v <= RTOL, (rhos[l], k, v)
        assert np.array_equal(host['sums'][l][:, 3], ref['sums'][:, 3])
    sc = np.sort(path['score'])
    print('score', path['score'], 'index', path['index'])
    assert sc[1] - sc[0] > 1e-6 * sc[0]
    assert host['index'] == path['index']
    np.testing.assert_allclose(host['score'], path['score'], rtol=RTOL)


def test_host_port_without_a_constant_column():
    """u_col None: every column penalised; against augmented least squares with all P extra rows."""
    from bayesfast_amd.modules.ridge import ridge_path_host
    rng = np.random.default_rng(7)
    for n, P in ((30, 12), (10, 25)):
        A, B = rng.standard_normal((n, P)) * np.arange(1, P + 1), rng.standard_normal((n, 2))
        host = ridge_path_host(A, B, [0.05, 2.], None)
        D = np.sum(A * A, axis=0) / n
        for l, rho in enumerate((0.05, 2.)):
            Aaug = np.vstack([A, np.diag(np.sqrt(n * rho * D))])
            c = np.linalg.lstsq(Aaug, np.vstack([B, np.zeros((P, 2))]), rcond=None)[0]
            Q = np.linalg.qr(Aaug)[0][:n]
            print(n, P, rho, rel(host['coef'][l], c), rel(host['h'][:, l], np.sum(Q * Q, axis=1)))
            assert rel(host['coef'][l], c) <= RTOL and rel(host['h'][:, l], np.sum(Q * Q, axis=1)) <= RTOL
            assert rel(host['resid'][l], B - A @ c) <= RTOL


def test_selection_ties_edges_and_constant_outputs():
    from bayesfast_amd.modules import fit_report as fr
    ridge = np.array([1e-3, 1e-1, 10., 1.])   # (not sorted: a tie goes to the larger VALUE)
    assert fr.ridge_choose([.5, .2, .2, .3], ridge) == (2, False)
    assert fr.ridge_choose([.5, .2, .3, .2], ridge) == (3, True)
    assert fr.ridge_choose([.1, .2, .3, .4], ridge) == (0, True)
    assert fr.ridge_choose([.4, .1, .3, .2], ridge) == (1, False)
    assert fr.ridge_choose([np.inf, .3, np.nan, np.inf], ridge) == (1, False)
    assert fr.ridge_choose([np.nan] * 4, ridge) == (2, False)
    assert fr.ridge_choose([.7], [1.]) == (0, True)
    with pytest.raises(ValueError):
        fr.ridge_choose([.1, .2], [1.])
    # the score: two outputs, n = 4, SS_tot = 30 - 100 / 4 = 5 for the first; the second is constant and left out
    sums = np.zeros((2, 2, 8))
    sums[:, 0, fr.SY], sums[:, 0, fr.SYY], sums[:, 0, fr.PRESS] = 10., 30., (2.5, 10.)
    sums[:, 1, fr.SY], sums[:, 1, fr.SYY], sums[:, 1, fr.PRESS] = 8., 16., (1., 1.)
    assert fr.ridge_score(sums, 4).tolist() == [.5, 2.]
    sums[:, 0] = sums[:, 1]
    assert fr.ridge_score(sums, 4).tolist() == [0., 0.]
    with pytest.raises(ValueError):
        fr.ridge_score(np.zeros((2, 8)), 4)


def _report(shape, rhos=None):
    from bayesfast_amd import RidgeReport
    from bayesfast_amd.modules.ridge import ridge_path_host
    x, y, w, path = rr.case(shape)
    A, B = weighted_design(shape)
    host = ridge_path_host(A, B, rr.rhos_of(shape) if rhos is None else rhos, 0, w)
    i = host['index']
    group = dict(outs=list(range(shape[3])), h=host['h'][:, i], resid=host['resid'][i], e_loo=host['e_loo'][i], path_sums=host['sums'],
                 dof=host['dof'])
    return RidgeReport(shape[2], [A.shape[1]], [0] * shape[3], [group], host['ridge']), host, path


def test_ridge_report_from_host_tables():
    from bayesfast_amd import FitReport, RidgeReport
    from bayesfast_amd.modules import RidgeReport as RR2
    assert RidgeReport is RR2 and issubclass(RidgeReport, FitReport)
    shape = rr.DUAL[2]
    rep, host, path = _report(shape)
    ref = path['refs'][path['index']]
    L = len(rr.RHO_DUAL)
    assert rep.ridge_path.tolist() == list(rr.RHO_DUAL) and rep.ridge_index.tolist() == [path['index']]
    assert rep.ridge.tolist() == [rr.RHO_DUAL[path['index']]] and rep.at_edge.tolist() == [path['index'] in (0, L - 1)]
    assert rep.dof.shape == (1, L) and rep.score_path.shape == (1, L)
    assert rep.press_path.shape == rep.q2_path.shape == rep.rmse_path.shape == (2, L)
    for l, r in enumerate(path['refs']):
        np.testing.assert_allclose(rep.q2_path[:, l], r['q2'], rtol=RTOL)
        np.testing.assert_allclose(rep.rmse_path[:, l], r['rmse'], rtol=RTOL)
        np.testing.assert_allclose(rep.press_path[:, l], r['press'], rtol=RTOL)
        np.testing.assert_allclose(rep.dof[0, l], r['dof'], rtol=RTOL)
    np.testing.assert_allclose(rep.score_path[0], path['score'], rtol=RTOL)
    # the parent's fields are those at the chosen penalty
    for k in ('rmse', 'loo_rmse', 'r2', 'q2', 'max_abs_loo'):
        np.testing.assert_allclose(getattr(rep, k), ref[k], rtol=RTOL)
    assert rel(rep.leverage[0], ref['leverage']) <= RTOL and rel(rep.loo_residual, ref['loo_residual']) <= RTOL
    assert rep.n_param == (78,) and rep.rank_deficient.tolist() == [False] and rep.n_unit_leverage.tolist() == [0]
    text = repr(rep)
    assert text.startswith('RidgeReport') and 'score path' in text and 'loo_rmse' in text


def test_ridge_report_equality_and_pickling():
    from bayesfast_amd import FitReport
    shape = rr.PRIMAL[0]
    a, host, _ = _report(shape)
    b, _, _ = _report(shape)
    assert a == b and not (a != b)
    for clone in (copy.deepcopy(a), pickle.loads(pickle.dumps(a))):
        assert clone == a and np.array_equal(clone.q2_path, a.q2_path) and np.array_equal(clone.ridge, a.ridge)
    c, _, _ = _report(shape, rhos=rr.RHO_PRIMAL[:4])
    assert a != c
    i = host['index']
    plain = FitReport(shape[2], [15], [0] * 3, [dict(outs=[0, 1, 2], h=host['h'][:, i], resid=host['resid'][i], e_loo=host['e_loo'][i],
                                                     sums=host['sums'][i])], [False])
    assert a != plain and plain != a
    with pytest.raises(TypeError):
        hash(a)


def test_argument_errors_before_the_device():
    from bayesfast_amd import PolyModel
    from bayesfast_amd.modules.ridge import DEFAULT_RIDGE, check_ridge, ridge_path_host
    assert len(DEFAULT_RIDGE) == 15 and DEFAULT_RIDGE[0] == 1e-6 and abs(DEFAULT_RIDGE[-1] / 10. - 1) < 1e-15
    assert check_ridge(None).tolist() == list(DEFAULT_RIDGE) and check_ridge(0.5).tolist() == [0.5]
    m = PolyModel('quadratic', input_size=3, output_size=2)
    assert m.ridge_on_fit is False and callable(m.fit_ridge)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((8, 3)), rng.standard_normal((8, 2))
    for bad in ([0.1, 0.], [-1.], [1.] * 33, [], [[1., 2.]], [np.nan], 'abc'):
        with pytest.raises(ValueError, match='ridge'):
            m.fit_ridge(x, y, ridge=bad)
        with pytest.raises(ValueError, match='ridge'):
            ridge_path_host(np.ones((5, 2)), np.ones((5, 1)), bad)
    with pytest.raises(ValueError, match='I need at least 4 points'):   # (the bound is on: more points than inputs)
        m.fit_ridge(x[:3], y[:3])
    m2 = PolyModel('quadratic', input_size=3, output_size=2, bound_options=dict(use_bound=False))
    with pytest.raises(ValueError, match='I need at least 3 points'):
        m2.fit_ridge(x[:2], y[:2])
    with pytest.raises(ValueError, match='I need at least 3 points'):
        ridge_path_host(np.ones((2, 2)), np.ones((2, 1)), [1.])
    with pytest.raises(ValueError, match='x should be a 2-d array'):
        m.fit_ridge(x[:, :2], y)
    with pytest.raises(ValueError, match='invalid shape for w'):
        m.fit_ridge(x, y, w=np.ones(3))
    m.ridge_on_fit = [1., -1.]
    with pytest.raises(ValueError, match='ridge'):
        m.fit(x, y)
    assert m.fit_report is None


def test_binding_rejects_bad_arguments_before_the_device():
    from bayesfast_amd import _lib
    _lib.build()
    lib = _lib.lib()
    assert _lib.ridge_work(130, 70, 17, 15) == 70 * 32 + 3 * 15 * 17 * 7
    assert lib.bfhip_ridge_path(None, 1, 1, 1, 1, None, 1, None, None, None, None, None, None, None, 0, 0, None, None, None, None, None, 0) == -1
    assert b'bfhip_ridge_path' in lib.bfhip_last_error()
    assert lib.bfhip_ridge_rotate(None, 1, 1, 1, None, 1, None, 1, None, 1) == -1
