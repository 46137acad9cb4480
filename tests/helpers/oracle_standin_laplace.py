"""TEST-ONLY: the oracle stand-in of ``DeviceDensity`` (oracle_standin.OracleDensity) with the two entry points of the Laplace
approximation, answered on the CPU by the kernels' own per-point arithmetic compiled for the host (tests/hess_host: bfhip_hess.h with
one thread; test_laplace_host.py checks it against differences of the oracle's gradient and the oracle's own Newton iteration).
Differences of the oracle's gradient cannot stand in inside the recipe: the OptimizeStep's maxima sit on the inside of the decay
term's C^1 surface, where every stencil straddles the kink.  Install after ``oracle_standin.install(monkeypatch)``.  It proves the
seam -- the subclass, ``patch(..., laplace=True)``, the hand-over of the density -- not the kernels."""
import os
import sys

import numpy as np
import torch

from oracle_standin import OracleDensity

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hess_host'))
import hess_host  # noqa: E402


class OracleLaplaceDensity(OracleDensity):
    MAXIMIZE_STATUS = ('converged', 'max_iter reached', 'non-finite logp', 'the last step was short but damped')
    n_maximize = 0   # launches, counted for the tests

    def logp_grad_hess(self, x, original_space=False):
        x = np.asarray(x, dtype=np.float64)
        f, g, H = hess_host.logp_grad_hess(self.spec, x.reshape(-1, self.d), original_space)
        f, g, H = torch.from_numpy(f), torch.from_numpy(g), torch.from_numpy(H)
        return (f[0], g[0], H[0]) if x.ndim == 1 else (f, g, H)

    def maximize(self, x0, max_iter=200, xtol=1e-5):
        type(self).n_maximize += 1
        x, f, H, info = hess_host.maximize(self.spec, np.asarray(x0, dtype=np.float64).reshape(-1, self.d), max_iter, xtol)
        return dict(x=torch.from_numpy(x), logp=torch.from_numpy(f), hess=torch.from_numpy(H), info=torch.from_numpy(info))


def install(monkeypatch):
    from bayesfast_amd.core.density import SurrogateDensity
    OracleLaplaceDensity.n_maximize = 0
    monkeypatch.setattr(SurrogateDensity, 'device', lambda self, ctx=None: OracleLaplaceDensity(self.spec()))
