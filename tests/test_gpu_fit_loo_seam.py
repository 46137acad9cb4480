"""GPU: the leave-one-out report through ``integrate``'s PolyModel, the subclass of the reference's own class (oracle/_ref) that an
unmodified Recipe fits: ``loo_on_fit`` on it makes ``fit`` leave the same ``FitReport`` ``bayesfast_amd.PolyModel.fit_loo`` returns."""
import numpy as np
import pytest

from oracle import reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')]


@pytest.fixture(scope='module')
def bf():
    return reference.load()


def test_loo_on_fit_through_the_reference_subclass(bf):
    import copy
    from bayesfast_amd import integrate, PolyModel
    seam = integrate.reference_classes(bf)
    rng = np.random.default_rng(3)
    x = rng.normal(size=(90, 4))
    y = np.stack([np.sin(x[:, 0]) + x[:, 1]**2, x[:, 2] * x[:, 3]], axis=1) + 0.1 * rng.normal(size=(90, 2))
    w = np.exp(0.3 * rng.normal(size=90))
    ours = PolyModel('quadratic', input_size=4, output_size=2, bound_options=dict(use_bound=False))
    want = ours.fit_loo(x, y, w=w)
    pm = seam.PolyModel('quadratic', input_size=4, output_size=2, bound_options=dict(use_bound=False))
    assert isinstance(pm, bf.modules.PolyModel) and pm.loo_on_fit is False and pm.fit_report is None
    pm.fit(x, y, w=w)
    assert pm.fit_report is None
    pm.loo_on_fit = True
    pm.fit(x, y, w=w)
    assert pm.fit_report == want
    for mine, theirs in zip(pm.configs, ours.configs):
        assert np.array_equal(np.asarray(mine._coef), np.asarray(theirs._coef))
    assert copy.deepcopy(pm).fit_report == want   # (core/recipe.py deep-copies its surrogates: the copy holds host arrays)
    pm.loo_on_fit = False
    assert pm.fit_loo(x, y, w=w) == want and pm.loo_on_fit is False
    pm.fit(x, y, w=w)
    assert pm.fit_report is None
