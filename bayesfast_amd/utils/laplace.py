"""The Laplace approximation of the OptimizeStep (counterpart of ``bayesfast.utils.laplace``, utils/laplace.py:17-205).

Two routes behind one ``Laplace.run``:

* **device** -- ``logp`` is a ``SurrogateDensity`` or a ``Chi2PipelineDensity`` (or its bound ``logp``), the method is the default
  ``'Newton-CG'`` and no ``grad`` / ``hess`` callables are given: every start is maximised inside ONE launch by a damped Newton
  iteration on the analytic Hessian (``DeviceDensity.maximize``, ``bfhip_laplace_opt``; for the pipeline density
  ``DeviceDensity.pipeline_maximize``, ``bfhip_pipeline_laplace_opt``), and the covariance comes from that Hessian -- exact, where
  the reference differences the gradient with ``numdifftools`` at every iteration.  Works in the sampling space
  (``original_space=False``), as the recipe does.  For the pipeline density ``hess_options={'gauss_newton': True}`` steps on, and
  returns, the Gauss-Newton matrix (no term that carries the residual: its likelihood part is negative semi-definite).  A pipeline
  density the device refuses (a surrogate it streams in chunks) takes the host route, silently.
* **host** -- everything else (another ``optimize_method``, user callables):
  ``scipy.optimize.minimize`` as the reference runs it.  Where ``logp`` is one of this package's densities the gradient is the
  device's and a missing Hessian is ONE launch of the gradient on the 4 d points of a fourth-order central difference; plain
  callables are differenced the same way.  Nothing imports ``numdifftools``.
"""
import contextlib
import threading
import warnings
from collections import namedtuple

import numpy as np

from .threads import blas_single_thread

__all__ = ['Laplace', 'LaplaceResult', 'make_positive']

LaplaceResult = namedtuple('LaplaceResult', 'x_max, f_max, samples, cov, beta, opt_result')

DEFAULT_MAX_ITER = 200   # accepted Newton steps per start on the device route (optimize_options['maxiter'] overrides)
FD_STEP = 1e-3           # difference step of the host route, in units of max(1, |x_i|) (grad_options / hess_options['step'] override)


def make_positive(A, max_cond=1e5):
    """``bayesfast.utils.misc.make_positive`` (utils/misc.py:12-18): the symmetric matrix A with every eigenvalue that is not above
    ``max_eigenvalue / max_cond`` raised to the smallest one that is.  ValueError when no eigenvalue is positive."""
    lam, V = np.linalg.eigh(A)
    if lam[-1] <= 0:
        raise ValueError('all the eigenvalues are non-positive.')
    keep = lam > lam[-1] / max_cond
    lam = np.where(keep, lam, lam[keep][0])
    return V @ np.diag(lam) @ V.T


# ---- the seam's hand-over (integrate.patch(..., laplace=True)): the reference's Recipe passes lambdas to run(), so the density they
# close over travels here for the duration of Recipe._opt_surro ----
_CURRENT = threading.local()   # per thread: two recipes optimising in two threads keep their own densities


@contextlib.contextmanager
def current_density(density):
    stack = _CURRENT.__dict__.setdefault('stack', [])
    stack.append(density)
    try:
        yield
    finally:
        stack.pop()


def get_current_density():
    stack = getattr(_CURRENT, 'stack', None)
    return stack[-1] if stack else None


def _our_density(logp):
    """The SurrogateDensity behind ``logp`` (the object, or its bound ``logp`` / ``__call__``), or None."""
    from ..core.density import SurrogateDensity
    if isinstance(logp, SurrogateDensity):
        return logp
    owner = getattr(logp, '__self__', None)
    if isinstance(owner, SurrogateDensity) and getattr(logp, '__name__', '') in ('logp', '__call__'):
        return owner
    return None


def _stencil(x, h):
    """The 4 d points x +- h_j e_j, x +- 2 h_j e_j of the fourth-order central difference, as (4, d, d)."""
    e = np.diag(h)
    return np.stack((x + e, x - e, x + 2. * e, x - 2. * e))


def _fd_steps(x, options):
    return float(options.get('step', FD_STEP)) * np.maximum(1., np.abs(x))


def _fd_gradient(fun, x, options):
    """Fourth-order central difference of a scalar callable: (8 (f(+h) - f(-h)) - (f(+2h) - f(-2h))) / 12 h."""
    x = np.asarray(x, dtype=np.float64)
    h = _fd_steps(x, options)
    f = np.array([[float(fun(p)) for p in row] for row in _stencil(x, h)])
    return (8. * (f[0] - f[1]) - (f[2] - f[3])) / (12. * h)


def _fd_jacobian(grad_batch, x, options):
    """The same difference of a gradient, symmetrised; ``grad_batch`` maps (n, d) points to (n, d) gradients in ONE call."""
    x = np.asarray(x, dtype=np.float64)
    d = x.size
    h = _fd_steps(x, options)
    g = np.asarray(grad_batch(_stencil(x, h).reshape(4 * d, d)), dtype=np.float64).reshape(4, d, d)
    J = ((8. * (g[0] - g[1]) - (g[2] - g[3])) / (12. * h)[:, None]).T   # J[i, j] = d g_i / d x_j
    return 0.5 * (J + J.T)


# ---- settings: written from the specification of bayesfast.utils.Laplace's arguments (utils/laplace.py:23-56) and its messages ----
def _positive(kind, optional):
    """A checker of one setting: a positive ``kind`` (float or int); None passes where the setting is optional."""
    def check(value, message):
        if value is None and optional:
            return None
        try:
            number = kind(value)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(message)
        if not number > 0:   # (NaN included)
            raise ValueError(message)
        return number
    return check


def _mapping(value, message):
    if value is None:
        return {}
    try:
        return dict(value)
    except (TypeError, ValueError):
        raise ValueError(message)


def _method(value, message):
    if callable(value) or isinstance(value, str):
        return value
    try:
        return str(value)
    except Exception:
        raise ValueError(message)


def _generator(value, message):
    if value is None:
        from .sobol import multivariate_normal
        return multivariate_normal
    if not callable(value):
        raise ValueError(message)
    return value


_SETTINGS = (   # argument, checker, message of a refused value; stored as ``_<argument>``
    ('optimize_method', _method, 'invalid value for optimize_method.'),
    ('optimize_tol', _positive(float, optional=True), 'invalid value for optimize_tol.'),
    ('optimize_options', _mapping, 'invalid value for optimize_options.'),
    ('max_cond', _positive(float, optional=False), 'max_cond should be a positive float.'),
    ('n_sample', _positive(int, optional=True), 'invalid value for n_sample.'),
    ('beta', _positive(float, optional=False), 'beta should be a positive float.'),
    ('mvn_generator', _generator, 'invalid value for mvn_generator.'),
    ('grad_options', _mapping, 'invalid value for grad_options.'),
    ('hess_options', _mapping, 'invalid value for hess_options.'),
)


def _negated(fn):
    return lambda x: -np.asarray(fn(x))


class Laplace:
    """Evaluating and sampling the Laplace approximation of a target density, with the arguments, defaults and messages of
    ``bayesfast.utils.Laplace``.  ``grad_options`` / ``hess_options`` went to ``numdifftools`` there; here their ``'step'`` entry
    sets the difference step of the host route, ``hess_options['gauss_newton']`` selects the Gauss-Newton matrix on the device route of
    a pipeline density, and the rest is accepted and unused."""

    def __init__(self, optimize_method='Newton-CG', optimize_tol=1e-5, optimize_options=None, max_cond=1e5, n_sample=2000, beta=1.,
                 mvn_generator=None, grad_options=None, hess_options=None):
        given = locals()
        for name, check, message in _SETTINGS:
            setattr(self, '_' + name, check(given[name], message))

    # ---- run ----
    def run(self, logp, x_0, grad=None, hess=None):
        """Optimise and draw the Laplace samples.  ``x_0``: (d,), the reference's call; on the device route also (n_start, d): all
        starts run in one launch and the one with the largest ``f_max`` is returned (the lowest index on ties), every start's
        result on ``opt_result``: ``all_x``, ``all_fun`` (each start's ``f_max``, i.e. logp, NOT negated as ``fun`` is),
        ``all_status``."""
        den = _our_density(logp)
        if den is None and not callable(logp):
            raise ValueError('logp should be callable.')
        device_route = den is not None and self._optimize_method == 'Newton-CG' and not callable(grad) and not callable(hess)
        try:
            x_0 = np.atleast_1d(np.asarray(x_0, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError('invalid value for x_0.')
        if x_0.ndim != 1 and not (device_route and x_0.ndim == 2):
            raise ValueError('invalid value for x_0.')
        run = self._run_device(den, x_0) if device_route else None
        if run is None:   # (also: a pipeline density in a form the device's maximiser does not cover)
            if x_0.ndim != 1:
                raise ValueError('invalid value for x_0.')
            run = self._run_host(den, logp, x_0, grad, hess)
        opt, H = run
        if not opt.success:
            warnings.warn('the optimization stopped at {}, but maybe it has not converged yet.'.format(opt.x), RuntimeWarning)
        return self._result(opt, H, self._n_sample or min(1000, 10 * x_0.shape[-1]))

    def _result(self, opt, H, n_sample):
        """The Gaussian at the optimiser's point: covariance from the Hessian there, ``n_sample`` draws of it tempered by beta."""
        with blas_single_thread():
            cov = np.linalg.inv(make_positive(-H, self._max_cond))
        return LaplaceResult(x_max=opt.x, f_max=-opt.fun, samples=self._mvn_generator(opt.x, cov / self._beta, n_sample), cov=cov,
                             beta=self._beta, opt_result=opt)

    def _run_device(self, den, x_0):
        """(opt_result, H) of the device's maximiser; None where it refuses a pipeline density (the streamed form, an LDS need above
        the limit): only that call's NotImplementedError is taken as a refusal, every other error is the caller's to see."""
        from scipy.optimize import OptimizeResult
        dev = den.device()
        xtol = 1e-5 if self._optimize_tol is None else self._optimize_tol
        max_iter = int(self._optimize_options.get('maxiter', DEFAULT_MAX_ITER))
        if den.spec().get('chi2') is not None:   # the pipeline density: entry points of its own, and the choice of the matrix
            gn = bool(self._hess_options.get('gauss_newton', False))
            try:
                out = dev.pipeline_maximize(np.atleast_2d(x_0), max_iter=max_iter, xtol=xtol, gauss_newton=gn)
            except NotImplementedError:
                return None
            grad_at = lambda x: dev.logp_and_grad(x, False)[1].reshape(-1)   # (the gradient kernel: no Hessian is needed for it)
        else:
            out = dev.maximize(np.atleast_2d(x_0), max_iter=max_iter, xtol=xtol)
            grad_at = lambda x: dev.logp_grad_hess(x, False)[1]
        fun, info = out['logp'].cpu().numpy(), out['info'].cpu().numpy()
        status = info[:, 1].astype(int)
        finite = np.where(np.isfinite(fun), fun, -np.inf)
        best = int(np.argmax(finite))   # (the first of equal maxima)
        x_best = out['x'][best].cpu().numpy()
        H = out['hess'][best].cpu().numpy()
        g = grad_at(x_best)   # the gradient at the maximum, for opt_result.jac: one launch of one point
        opt = OptimizeResult(x=x_best, fun=-float(fun[best]), jac=-g.cpu().numpy(), nit=int(info[best, 0]), nhev=int(info[best, 0]) + 1,
                             success=bool(status[best] == 0), status=int(status[best]), message=dev.MAXIMIZE_STATUS[status[best]],
                             all_x=out['x'].cpu().numpy(), all_fun=fun, all_status=status, last_step=float(info[best, 2]),
                             damping=float(info[best, 3]))
        return opt, H

    def _run_host(self, den, logp, x_0, grad, hess):
        from scipy.optimize import minimize
        if den is not None:   # one of this package's densities, in the sampling space: value and gradient from the device
            f = lambda x: float(np.asarray(den.logp(x, original_space=False)).reshape(-1)[0])
            grad_batch = lambda pts: den.grad(pts, original_space=False)   # ONE launch for all the rows
            g = grad if callable(grad) else (lambda x: np.asarray(den.grad(x, original_space=False)).reshape(-1))
            if callable(grad):
                grad_batch = lambda pts: np.array([grad(p) for p in pts])
        else:
            f = logp
            g = grad if callable(grad) else (lambda x: _fd_gradient(logp, x, self._grad_options))
            grad_batch = lambda pts: np.array([g(p) for p in pts])
        h = hess if callable(hess) else (lambda x: _fd_jacobian(grad_batch, x, self._hess_options))
        problem = dict(fun=lambda x: -f(x), jac=_negated(g), hess=_negated(h))   # scipy minimises
        with blas_single_thread():
            opt = minimize(x0=x_0, method=self._optimize_method, tol=self._optimize_tol, options=self._optimize_options, **problem)
        return opt, np.asarray(h(opt.x))

    @staticmethod
    def untemper_laplace_samples(laplace_result):
        """The Laplace samples at beta = 1: x_max + sqrt(beta) (samples - x_max)."""
        if not (isinstance(laplace_result, tuple) and getattr(laplace_result, '_fields', None) == LaplaceResult._fields):
            raise ValueError('laplace_result should be a LaplaceResult.')
        return laplace_result.x_max + (laplace_result.samples - laplace_result.x_max) * laplace_result.beta**0.5
