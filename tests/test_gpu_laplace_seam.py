"""GPU: the Laplace approximation under the reference's Recipe (oracle/_ref) with the real device behind
``integrate.patch(bf, laplace=True)`` -- the body of test_laplace_seam.py, kernels instead of stand-ins."""
import os
import sys

import pytest

from oracle import reference

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reference.is_built(), reason='needs the reference built into oracle/_ref by build()')]


@pytest.fixture(scope='module')
def bf():
    return reference.load()


def test_donut_recipe_with_the_laplace_seam(bf):
    import laplace_seam
    from bayesfast_amd import integrate
    laplace_seam.donut_recipe_reaches_the_ring(bf, integrate)


def test_concave_recipe_laplace_routes_agree(bf, monkeypatch):
    import laplace_seam
    from bayesfast_amd import integrate
    laplace_seam.concave_recipe_agrees_with_the_reference_route(bf, integrate, monkeypatch)


def test_plain_patch_keeps_the_reference_laplace(bf):
    import laplace_seam
    from bayesfast_amd import integrate
    laplace_seam.plain_patch_keeps_the_reference_laplace(bf, integrate)
