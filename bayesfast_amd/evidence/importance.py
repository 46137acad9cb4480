"""Importance sampling estimate of a normalising constant (reference: bayesfast/evidence/importance.py:10-37).

With x_q ~ q (q normalised) and the log-densities log p(x_q), log q(x_q), log r = log(mean exp(log p - log q)) estimates
log(Z_p / Z_q), and the relative variance of the normalised weights f = exp(log p - log q - log r) gives its error.  Both come
from one device reduction, ``bfhip_logmeanexp_stats``; only its three scalars reach the host."""
import warnings

import numpy as np

__all__ = ['importance']


def _checked_pair(a, b, names, ndim_of):
    """The two inputs as (n,) float64 device tensors of one device, with their common shape.  A device tensor is used where it
    is (cast to float64 there); anything else goes through ``np.asarray``.  ``ndim_of`` (0 or 1) names the input whose
    dimension the message reports, as the reference does."""
    import torch
    from ..device import get_context
    device = next((v.device for v in (a, b) if isinstance(v, torch.Tensor) and v.is_cuda), None)
    try:
        arrs = [v if isinstance(v, torch.Tensor) and v.is_cuda else np.asarray(v, dtype=np.float64) for v in (a, b)]
    except Exception:
        raise ValueError('invalid value for the inputs.')
    shapes = [tuple(v.shape) for v in arrs]
    if len(shapes[ndim_of]) not in (1, 2):
        raise ValueError('dim of {} should be 1 or 2, instead of {}.'.format(names[ndim_of], len(shapes[ndim_of])))
    if shapes[0] != shapes[1]:
        raise ValueError('shape of {}, {}, is different from shape of {}, {}.'.format(names[0], shapes[0], names[1], shapes[1]))
    if int(np.prod(shapes[0])) == 0:
        raise ValueError('{} and {} are empty.'.format(*names))
    ctx = get_context(None if device is None else device.index)
    flat = [ctx.tensor(v, torch.float64).reshape(-1) for v in arrs]
    return ctx, flat, shapes[0]


def _logmeanexp_stats(ctx, x, y, want_terms=False):
    """``bfhip_logmeanexp_stats`` on (n,) device tensors: (L, mean f, var f) on the host, and f as a device tensor when asked."""
    import torch
    from .. import _lib
    from ..device import _ptr
    out = torch.empty(3, dtype=torch.float64, device=ctx.device)
    terms = torch.empty(x.shape[0], dtype=torch.float64, device=ctx.device) if want_terms else None
    _lib.check(ctx._lib.bfhip_logmeanexp_stats(ctx.handle, x.shape[0], _ptr(x), _ptr(y), _ptr(out), _ptr(terms)))
    lme, mean, var = (np.float64(v) for v in out.cpu().numpy())
    return lme, mean, var, terms


def importance(logp_q, logq_q):
    """``(logr, logr_err)`` from log p and log q on draws from q: NumPy arrays or device tensors of shape (n,) or
    (chain, iteration).  Unlike the reference, which returns NaN with NumPy's warnings, empty inputs raise ``ValueError``."""
    ctx, (lpq, lqq), shape = _checked_pair(logp_q, logq_q, ('logp_q', 'logq_q'), 1)
    n_q = lpq.shape[0]
    logr, mean, var, _ = _logmeanexp_stats(ctx, lpq, lqq)
    logr_err = (var / mean**2 / n_q)**0.5
    if logr_err > 0.25:
        warnings.warn('the estimated error for logr may be unreliable, since the result is larger than 0.25.', RuntimeWarning)
    return logr, logr_err
