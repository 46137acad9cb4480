"""TEST-ONLY: the oracle stand-in of ``DeviceDensity`` (oracle_standin.OracleDensity) with the two entry points of the PIPELINE
density's Laplace approximation, answered on the CPU from the oracle alone: the Hessian is the fourth-order central difference of
the oracle's gradient (laplace_cases.hess_fd, symmetrised), the maximum the oracle's own damped Newton iteration
(laplace_cases.oracle_newton).  The oracle has ONE matrix: ``gauss_newton`` is recorded, not computed.  It proves the routing of
``Laplace.run`` -- which entry points it calls with which arguments, and what it builds from their answers -- not the kernels
(tests/test_gpu_pipeline_hess.py holds those to the same oracle)."""
import numpy as np
import torch

import laplace_cases as lc
from oracle_standin import OracleDensity


class OraclePipelineLaplaceDensity(OracleDensity):
    MAXIMIZE_STATUS = ('converged', 'max_iter reached', 'non-finite logp', 'the last step was short but damped')

    def __init__(self, spec, ctx=None, refuse=False):
        super().__init__(spec, ctx)
        self.refuse = refuse       # answer as the library answers a streamed-form pipeline density
        self.calls = []            # (entry point, number of points, gauss_newton)
        self.n_logp_and_grad = 0

    def logp_and_grad(self, x, original_space=False):
        self.n_logp_and_grad += 1
        return super().logp_and_grad(x, original_space)

    def logp_grad_hess(self, x, original_space=False):
        raise NotImplementedError('the scalar call refuses the pipeline density')

    maximize = logp_grad_hess

    def _hess(self, x, original_space):
        H = lc.hess_fd(self.spec, x, original_space)
        return 0.5 * (H + H.T)

    def pipeline_logp_grad_hess(self, x, original_space=False, gauss_newton=False):
        x = np.asarray(x, dtype=np.float64)
        pts = x.reshape(-1, self.d)
        self.calls.append(('pipeline_logp_grad_hess', len(pts), bool(gauss_newton)))
        if self.refuse:
            raise NotImplementedError('stand-in: the streamed form')
        f, g = lc.orc.logp_and_grad(self.spec, pts, original_space=original_space)
        H = np.array([self._hess(p, original_space) for p in pts])
        f, g, H = torch.from_numpy(np.atleast_1d(f)), torch.from_numpy(np.atleast_2d(g)), torch.from_numpy(H)
        return (f[0], g[0], H[0]) if x.ndim == 1 else (f, g, H)

    def pipeline_maximize(self, x0, max_iter=200, xtol=1e-5, gauss_newton=False):
        starts = np.asarray(x0, dtype=np.float64).reshape(-1, self.d)
        self.calls.append(('pipeline_maximize', len(starts), bool(gauss_newton)))
        if self.refuse:
            raise NotImplementedError('stand-in: the streamed form')
        x, f, H, info = [], [], [], []
        for s in starts:
            xs, fs, gs, it = lc.oracle_newton(self.spec, s)
            x.append(xs)
            f.append(fs)
            H.append(self._hess(xs, False))
            info.append([it, 0., 0., 0.])
        return dict(x=torch.from_numpy(np.array(x)), logp=torch.from_numpy(np.array(f)), hess=torch.from_numpy(np.array(H)),
                    info=torch.from_numpy(np.array(info, dtype=np.float64)))
