"""The seam's TraceTuple (bayesfast_amd/integrate.py) derives from the REFERENCE's class, which has no convergence diagnostics:
its integrated_time / rhat / ess / summary hand over to the device result it wraps.  Needs the reference that build() compiled into
oracle/_ref (skipped where there is none), no GPU: the wrapped result holds host arrays."""
import os
import sys

import numpy as np
import pytest

from oracle import reference

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))
pytestmark = pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')


def test_seam_tracetuple_hands_the_diagnostics_to_the_device_result():
    import diag_reference as dr
    from bayesfast_amd import _lib, integrate
    from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple
    bf = reference.load()
    c, n, d = 6, 80, 3
    s = dr.ar1((c, n, d), seed=21)
    st = np.zeros((c, n, _lib.STAT_STRIDE))
    st[:, :, 0] = dr.ar1((c, n, 1), seed=22)[:, :, 0]
    inner = TraceTuple(NTrace(n_chain=c, n_iter=n, n_warmup=20), s, st, s * 3 - 1, st[:, :, 0] + 2.)
    tt = integrate.reference_classes(bf).TraceTuple(inner, None)
    assert isinstance(tt, bf.samplers.TraceTuple)
    for kw in (dict(), dict(since_iter=31, original_space=False), dict(return_type='logp', include_warmup=True)):
        ref = dr.reference(tt.get(flatten=False, **kw))
        got = tt.summary(**kw)
        for k in got.names:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-9, err_msg=k)
        np.testing.assert_allclose(tt.rhat(method='split', **kw), ref['rhat_split'], rtol=1e-9)
        np.testing.assert_allclose(tt.ess(method='mean', **kw), ref['ess_mean'], rtol=1e-9)
        assert np.array_equal(tt.integrated_time(quiet=True, **kw), inner.integrated_time(quiet=True, **kw))
    with pytest.raises(ValueError):
        tt.summary(since_iter=79)
