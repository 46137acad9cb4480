"""Leave-one-out validation of the fit, the part that needs no GPU: the loop reference checks itself (the identity e / (1 - h)
against n explicit refits), FitReport's derived numbers are pure functions of the device sums, and the new API is there and
validates its arguments as ``fit`` does.

Bounds.  The identity against the explicit refits was measured at 2.0e-14 of the largest held-out residual on these three shapes
(designs with a column-equilibrated condition number of at most 23); the test holds it to ten times that.  sum h = P is the trace of
a projector: held to 1e-12 P."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

import loo_reference as lr  # noqa: E402

# (inputs, order, n, outputs, weighted): the three smallest shapes of tests/test_gpu_fit_loo.py
SMALL = [(4, 'quadratic', 40, 3, False), (4, 'quadratic', 40, 3, True), (11, 'quadratic', 200, 2, False), (63, 'linear', 257, 2, False)]


@pytest.mark.parametrize('n_in,order,n,m,weighted', SMALL)
def test_reference_identity_against_explicit_refits(n_in, order, n, m, weighted):
    x, y, w = lr.make_case(n_in, n, m, weighted, seed=n)
    ref = lr.reference(x, y, order, w)
    explicit = lr.loo_explicit(x, y, order, w)
    err = np.max(np.abs(ref['loo_residual'] - explicit)) / np.max(np.abs(explicit))
    print('identity vs explicit', err, 'sum h - P', ref['leverage'].sum() - ref['P'], 'max h', ref['leverage'].max())
    assert err <= 2.0e-13
    assert abs(ref['leverage'].sum() - ref['P']) <= 1e-12 * ref['P']
    assert ref['leverage'].min() >= 0. and ref['leverage'].max() < 1.


def test_report_derived_numbers_from_hand_made_sums():
    from bayesfast_amd.modules import fit_report as fr
    x, y, w = lr.make_case(4, 40, 3, True, seed=40)
    ref = lr.reference(x, y, 'quadratic', w)
    d = fr.derive(ref['sums'], 40)
    for k in ('rmse', 'loo_rmse', 'r2', 'q2'):
        print(k, d[k], ref[k])
        np.testing.assert_allclose(d[k], ref[k], rtol=1e-12, atol=0)
    # by hand: 4 rows, residuals (1, -1, 1, -1), leverages 1/2, targets (1, 2, 3, 4)
    sums = np.array([[4., 16., 2., 0., 10., 30., 0., 0.]])
    d = fr.derive(sums, 4)
    assert d['rmse'][0] == 1. and d['loo_rmse'][0] == 2.
    assert d['r2'][0] == 1. - 4. / 5. and d['q2'][0] == 1. - 16. / 5.
    with pytest.raises(ValueError):
        fr.derive(np.zeros((2, 3)), 4)
    with pytest.raises(ValueError):
        fr.derive(sums, 0)


def test_report_object_from_host_arrays():
    """Two groups, NumPy inputs: the per-output columns land in output order, the per-group ones in group order."""
    from bayesfast_amd import FitReport
    from bayesfast_amd.modules import FitReport as FR2
    assert FitReport is FR2
    n = 5
    g0 = dict(outs=[0, 2], h=np.full(n, .4), resid=np.ones((n, 2)), e_loo=2. * np.ones((n, 2)),
              sums=np.array([[5., 20., 2., 1., 10., 40., 0., 0.], [5., 20., 3., 4., 10., 40., 0., 0.]]))
    g1 = dict(outs=[1], h=np.full(n, .2), resid=-np.ones((n, 1)), e_loo=-3. * np.ones((n, 1)),
              sums=np.array([[5., 45., 3., 0., 0., 20., 2., 0.]]))
    rep = FitReport(n, [2, 1], [0, 1, 0], [g0, g1], [False, True])
    assert rep.n == n and rep.n_param == (2, 1) and rep.group_of_output.tolist() == [0, 1, 0]
    assert rep.rank_deficient.tolist() == [False, True] and rep.n_unit_leverage.tolist() == [0, 2]
    assert len(rep.leverage) == 2 and rep.leverage[1][0] == .2
    assert rep.residual.shape == (n, 3) and rep.residual[0].tolist() == [1., -1., 1.]
    assert rep.loo_residual[0].tolist() == [2., -3., 2.]
    assert rep.max_abs_loo.tolist() == [2., 3., 3.] and rep.argmax_abs_loo.tolist() == [1, 0, 4]
    np.testing.assert_allclose(rep.loo_rmse, [2., 3., 2.])
    np.testing.assert_allclose(rep.r2, [1. - 5. / 20., 1. - 5. / 20., 1. - 5. / 20.])
    text = repr(rep)
    assert 'loo_rmse' in text and 'q2' in text and len(text.splitlines()) == 2 + 3
    import copy
    assert copy.deepcopy(rep) == rep


def test_api_exists_and_validates_before_the_device():
    from bayesfast_amd import PolyModel
    m = PolyModel('quadratic', input_size=3, output_size=2)
    assert m.loo_on_fit is False and m.fit_report is None
    assert callable(m.fit_loo)
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match='x should be a 2-d array'):
        m.fit_loo(rng.standard_normal((20, 2)), rng.standard_normal((20, 2)))
    with pytest.raises(ValueError, match='y should be a 2-d array'):
        m.fit_loo(rng.standard_normal((20, 3)), rng.standard_normal((20, 3)))
    with pytest.raises(ValueError, match='different # of points'):
        m.fit_loo(rng.standard_normal((20, 3)), rng.standard_normal((19, 2)))
    with pytest.raises(ValueError, match='I need at least'):
        m.fit_loo(rng.standard_normal((5, 3)), rng.standard_normal((5, 2)))
    with pytest.raises(ValueError, match='invalid shape for w'):
        m.fit_loo(rng.standard_normal((20, 3)), rng.standard_normal((20, 2)), w=np.ones(3))
    m.loo_on_fit = True
    with pytest.raises(ValueError, match='x should be a 2-d array'):
        m.fit(rng.standard_normal((20, 2)), rng.standard_normal((20, 2)))
    assert m.fit_report is None


def test_binding_rejects_bad_arguments_before_the_device():
    """NULL context, and outputs that do not come together: BFHIP_ERR_ARG without a GPU."""
    from bayesfast_amd import _lib
    _lib.build()
    lib = _lib.lib()
    assert lib.bfhip_version() >= 109
    assert lib.bfhip_lstsq_loo(None, 1, 1, 1, None, 1, None, None, None, 0, None, None, None, None, None, None, None, 0) == -1
    assert b'invalid argument' in lib.bfhip_last_error()
