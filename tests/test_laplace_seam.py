"""The Laplace approximation under the reference's Recipe, WITHOUT a GPU: the device entry points are the oracle stand-ins
(helpers/oracle_standin.py, helpers/oracle_standin_laplace.py), so this proves the seam -- the subclass, patch(..., laplace=True),
the hand-over of the density to run() -- not the kernels.  test_gpu_laplace_seam.py runs the same body on the device."""
import os
import sys

import pytest

from oracle import reference

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))
pytestmark = pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')


@pytest.fixture(scope='module')
def bf():
    return reference.load()


@pytest.fixture()
def standins(monkeypatch):
    import oracle_standin
    import oracle_standin_laplace
    oracle_standin.install(monkeypatch)
    oracle_standin_laplace.install(monkeypatch)
    return oracle_standin_laplace.OracleLaplaceDensity


def test_donut_recipe_with_the_laplace_seam(bf, standins):
    import laplace_seam
    from bayesfast_amd import integrate
    laplace_seam.donut_recipe_reaches_the_ring(bf, integrate)
    assert standins.n_maximize >= 1   # the OptimizeStep went through maximize()


def test_concave_recipe_laplace_routes_agree(bf, standins, monkeypatch):
    import laplace_seam
    from bayesfast_amd import integrate
    laplace_seam.concave_recipe_agrees_with_the_reference_route(bf, integrate, monkeypatch)
    assert standins.n_maximize == 3


def test_plain_patch_keeps_the_reference_laplace(bf, standins):
    import laplace_seam
    from bayesfast_amd import integrate
    laplace_seam.plain_patch_keeps_the_reference_laplace(bf, integrate)
