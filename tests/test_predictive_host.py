"""Posterior predictive summaries, the part that needs no GPU: the C ABI carries ``bfhip_polymodel_columns`` and refuses a NULL
context before anything touches a device, the walk over the selected outputs is a pure plan, and ``Predictive``'s derived numbers
(sigma, pull, the out-of-bound share, ppp) are pure functions of what the device hands back."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_bound_with_the_headers_arguments():
    from bayesfast_amd import _lib
    _lib.build()
    lib = _lib.lib()
    assert lib.bfhip_version() >= 110
    assert 'bfhip_polymodel_columns' in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'bfhip.h')).read()
    decl = re.search(r'int bfhip_polymodel_columns\s*\((.*?)\);', hdr, re.S).group(1)
    assert len(decl.split(',')) == len(_lib.SYMBOLS['bfhip_polymodel_columns'][1]) == 15


def test_null_context_is_refused_before_the_device():
    from bayesfast_amd import _lib
    _lib.build()
    lib = _lib.lib()
    rc = lib.bfhip_polymodel_columns(None, 1, 1, 1, 1, None, 0, 0, None, None, 0, 1, None, 1, None)
    assert rc == -1
    assert b'invalid argument' in lib.bfhip_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_output_plan_and_batch_width():
    from bayesfast_amd.utils.predictive import output_plan, batch_width, chi2_chunk
    idx, batches = output_plan([], 9, 4)
    assert idx.size == 0 and batches == []
    idx, batches = output_plan([6], 9, 4)
    assert idx.tolist() == [6] and batches == [[(6, 1, 0)]]
    idx, batches = output_plan(None, 9, 4)                      # contiguous: all outputs, cut at the width
    assert idx.tolist() == list(range(9)) and batches == [[(0, 4, 0)], [(4, 4, 0)], [(8, 1, 0)]]
    idx, batches = output_plan([3, 4, 5, 20, 36], 37, 16)       # scattered: one batch, three runs side by side
    assert idx.tolist() == [3, 4, 5, 20, 36] and batches == [[(3, 3, 0), (20, 1, 3), (36, 1, 4)]]
    idx, batches = output_plan([3, 4, 5, 20, 36], 37, 2)        # a run cut by the width
    assert batches == [[(3, 2, 0)], [(5, 1, 0), (20, 1, 1)], [(36, 1, 0)]]
    idx, batches = output_plan([7, 2, 2, 8, 3, 7], 9, 16)       # unsorted with duplicates
    assert idx.tolist() == [2, 3, 7, 8] and batches == [[(2, 2, 0), (7, 2, 2)]]
    for calls in batches:                                        # every plan: the columns tile the batch in order
        assert [c for _, _, c in calls] == list(np.cumsum([0] + [nb for _, nb, _ in calls[:-1]]))
    for bad in ([9], [-1], [0, 37]):
        with pytest.raises(ValueError):
            output_plan(bad, 9, 4)
    with pytest.raises(ValueError):
        output_plan([0.5], 9, 4)
    n = 400
    assert batch_width(8 * n, n, 37) == 1 and batch_width(0, n, 37) == 1
    assert batch_width(16 * 8 * n, n, 37) == 16 and batch_width(31 * 8 * n, n, 37) == 16 and batch_width(15 * 8 * n, n, 37) == 15
    assert batch_width(1 << 30, n, 37) == 37 and batch_width(1 << 30, n, 5) == 5
    assert batch_width(1 << 30, 4096 * 1000, 457) == 32          # the flagship shape: two 16-column table batches per buffer
    assert chi2_chunk(1 << 30, 457) == (1 << 30) // (8 * 457) and chi2_chunk(100, 37) == 64


def test_sigma_and_pull():
    from bayesfast_amd.utils.predictive import sigma_of, pull_of
    rng = np.random.default_rng(0)
    b = rng.normal(size=(6, 6))
    cov = b @ b.T + np.eye(6)
    np.testing.assert_allclose(sigma_of(prec=np.linalg.inv(cov)), np.sqrt(np.diag(cov)), rtol=1e-12)
    assert sigma_of(prec_diag=[4., 0.25]).tolist() == [0.5, 2.]
    assert pull_of([3., 1.], [1., 2.], [0.5, 2.]).tolist() == [4., -0.5]
    with pytest.raises(ValueError):
        sigma_of()
    with pytest.raises(ValueError):
        sigma_of(prec=np.eye(2), prec_diag=np.ones(2))


def test_oob_share_from_hand_made_flags_and_weights():
    from bayesfast_amd.utils.predictive import oob_share_of
    flags = np.array([[1, 0, 0, 0], [1, 1, 0, 1], [0, 0, 0, 0]], dtype=bool)
    share, chain = oob_share_of(flags)
    assert share == 4 / 12 and chain.tolist() == [0.25, 0.75, 0.]
    w = np.array([1., 2., 3., 4., 0., 0., 5., 6., 7., 8., 9., 10.])
    share, chain = oob_share_of(flags, w)
    assert share == pytest.approx((1. + 6.) / w.sum(), rel=1e-15) and chain.tolist() == [0.25, 0.75, 0.]   # per chain: unweighted
    assert oob_share_of(np.zeros((2, 3), dtype=bool))[0] == 0.


def test_ppp_from_hand_made_chi_squares():
    import scipy.stats as ss
    from bayesfast_amd.utils.predictive import ppp_of
    rng = np.random.default_rng(1)
    for m in (1, 37, 457):
        c = ss.chi2.rvs(m, size=200, random_state=rng) * rng.uniform(0.5, 1.5)
        np.testing.assert_allclose(ppp_of(c, m), ss.chi2.sf(c, m).mean(), rtol=1e-9)
        w = rng.uniform(size=200)
        w[::7] = 0.
        np.testing.assert_allclose(ppp_of(c, m, w), (w * ss.chi2.sf(c, m)).sum() / w.sum(), rtol=1e-9)
        c2 = c.copy()
        c2[0] = np.nan                                           # weight 0: not part of the sample
        np.testing.assert_allclose(ppp_of(c2, m, w), (w * ss.chi2.sf(c, m)).sum() / w.sum(), rtol=1e-9)
        c2[1] = np.nan                                           # weight > 0: NaN
        assert w[1] > 0 and np.isnan(ppp_of(c2, m, w)) and np.isnan(ppp_of(c2, m))
    assert ppp_of(np.zeros(3), 5) == 1.


def test_integrate_seam_trace_tuple_delegates_predictive():
    """The seam's TraceTuple wraps the device result and hands ``predictive`` to it, as it does ``summary``."""
    from oracle import reference
    if not reference.is_built():
        pytest.skip('needs the reference built into oracle/_ref by build()')
    from bayesfast_amd import integrate
    cls = integrate.reference_classes(reference.load()).TraceTuple

    class _Inner:
        def predictive(self, density, **kw):
            return ('inner', density, kw)

    tt = cls.__new__(cls)
    tt._inner = _Inner()
    assert tt.predictive('den', outputs=[1]) == ('inner', 'den', {'outputs': [1]})


def test_exports_and_entry_points():
    import bayesfast_amd.utils as u
    from bayesfast_amd.utils.predictive import predictive, Predictive
    assert u.predictive is predictive and u.Predictive is Predictive
    assert 'predictive' in u.__all__ and 'Predictive' in u.__all__
    from bayesfast_amd import Chi2PipelineDensity, PolyModel
    from bayesfast_amd.samplers.sample_trace import TraceTuple
    from bayesfast_amd.device import DevicePolyModel
    assert callable(Chi2PipelineDensity.predictive) and callable(TraceTuple.predictive) and callable(DevicePolyModel.fun_columns)
    su = PolyModel('quadratic', input_size=3, output_size=2)
    with pytest.raises(NotImplementedError):                     # no host evaluation of a PolyModel
        predictive(su, np.zeros((2, 8, 3)))
    import torch
    with pytest.raises(NotImplementedError):
        predictive(su, torch.zeros((2, 8, 3), dtype=torch.float64))
