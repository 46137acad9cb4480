"""The front end that the pipeline-data utilities share (bayesfast_amd/utils/_pipeline_data.py): no GPU.

1. Which refusal wins when two things are wrong at once, for ``predictive``, ``data_loo``, ``data_lgo``, ``data_reweight`` and
   ``data_log_ratio``.  The five check one process first; then the first three look at the draws before the density, the two of
   reweight.py at the density before the draws.  The table is what the functions did before they shared their checks.
2. The small helpers against NumPy."""
import numpy as np
import pytest

NI, VE = NotImplementedError, ValueError
FUNCTIONS = ('predictive', 'data_loo', 'data_lgo', 'data_reweight', 'data_log_ratio')
DENSITY_FIRST = ('data_reweight', 'data_log_ratio')
# faults: P two processes, H host draws, D no density, S a CPU tensor of the wrong last dimension
PAIRS = {'PH': (NI, 'one process'), 'PD': (NI, 'one process'), 'PS': (NI, 'one process'), 'HS': (NI, 'GPU tensor'),
         'HD': {False: (NI, 'GPU tensor'), True: (VE, 'Chi2PipelineDensity')},   # the five disagree where the density is wrong too
         'DS': {False: (NI, 'GPU tensor'), True: (VE, 'Chi2PipelineDensity')}}


@pytest.mark.parametrize('pair', sorted(PAIRS))
@pytest.mark.parametrize('name', FUNCTIONS)
def test_which_refusal_wins(name, pair, monkeypatch):
    import torch
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel, utils
    from bayesfast_amd.utils.reweight import data_log_ratio
    fun = data_log_ratio if name == 'data_log_ratio' else getattr(utils, name)
    su = bfa.PolyModel('quadratic', input_size=2, output_size=3)
    model = object() if 'D' in pair else bfa.Chi2PipelineDensity(su, np.zeros(3), prec_diag=np.ones(3))
    x = torch.zeros((10, 5)) if pair == 'DS' else np.zeros((10, 5 if 'S' in pair else 2))
    if 'P' in pair:
        monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    more = {'data_lgo': ([[0]],), 'data_reweight': (np.ones(3),), 'data_log_ratio': (np.ones(3),)}.get(name, ())
    want = PAIRS[pair]
    kind, words = want[name in DENSITY_FIRST] if isinstance(want, dict) else want
    with pytest.raises((NI, VE), match=words) as err:
        fun(model, x, *more)
    assert err.type is kind


def test_small_helpers():
    import torch
    from bayesfast_amd.utils._pipeline_data import host_f64, sum_and_se, dense_precision, logsumexp_host
    for v, want in (([1, 2.5, -3], np.array([1., 2.5, -3.])), (np.arange(6, dtype=np.float32).reshape(2, 3) / 3, None),
                    (torch.arange(4, dtype=torch.float32) / 7, (np.arange(4, dtype=np.float32) / np.float32(7)).astype(np.float64))):
        got = host_f64(v)
        assert got.dtype == np.float64 and np.array_equal(got, np.asarray(v, dtype=np.float64) if want is None else want)
    a = np.array([-1000., -1001., -np.inf])
    assert logsumexp_host(a) == -1000. + np.log(np.exp(a + 1000.).sum())
    total, se = sum_and_se(np.array([2.5]))
    assert total == 2.5 and np.isnan(se)
    v = np.array([1., -2., 4.5])
    total, se = sum_and_se(v)
    assert (total, se) == (float(v.sum()), float(np.sqrt(3 * v.var(ddof=1)))) and isinstance(total, float) and isinstance(se, float)
    p = np.array([[2., 0.5], [0.5, 1.]])
    assert np.array_equal(dense_precision(prec=p), p) and np.array_equal(dense_precision(prec_diag=[2., 3.]), np.diag([2., 3.]))
    for bad in (dict(), dict(prec=p, prec_diag=np.ones(2)), dict(prec=np.ones((2, 3))), dict(prec=np.ones(3)), dict(prec=np.ones((2, 2, 2))),
                dict(prec=np.array([[1., 0.], [0., 0.]])), dict(prec_diag=[1., -1.]), dict(prec_diag=[1., np.nan])):
        with pytest.raises(ValueError):
            dense_precision(**bad)
        from bayesfast_amd.utils.data_loo import whitening_of
        with pytest.raises(ValueError):
            whitening_of(**bad)
