"""Harmonic mean estimate of a normalising constant (reference: bayesfast/evidence/harmonic.py:10-52).

With x_p ~ p (possibly as (chain, iteration)) and log p(x_p), log q(x_p) for a normalised q, log r = -log(mean exp(log q - log p))
estimates log(Z_p / Z_q).  ``bfhip_logmeanexp_stats`` gives it, the mean and variance of the normalised terms
f = exp(log q - log p + log r) and f itself; f visits the host for the autocorrelation time of the chains, which inflates the
error."""
import warnings

import numpy as np

from ..utils.acor import integrated_time
from .importance import _checked_pair, _logmeanexp_stats

__all__ = ['harmonic']


def harmonic(logp_p, logq_p):
    """``(logr, logr_err)`` from log p and log q on draws from p: NumPy arrays or device tensors of shape (n,) or
    (chain, iteration).  Unlike the reference, which returns NaN with NumPy's warnings, empty inputs raise ``ValueError``."""
    ctx, (lpp, lqp), shape = _checked_pair(logp_p, logq_p, ('logp_p', 'logq_p'), 0)
    n_p = lpp.shape[0]
    lme, mean, var, terms = _logmeanexp_stats(ctx, lqp, lpp, want_terms=True)
    logr = -lme
    foo = terms.cpu().numpy()
    # the autocorrelation time twice, on the chains as given and on the flattened series; the larger error is reported, and a
    # large gap between the two is a warning sign
    tau_uf = integrated_time(foo.reshape(shape)[..., np.newaxis])[0]
    logr_err_uf = (tau_uf * var / mean**2 / n_p)**0.5
    tau_f = integrated_time(foo[..., np.newaxis])[0]
    logr_err_f = (tau_f * var / mean**2 / n_p)**0.5
    with np.errstate(divide='ignore', invalid='ignore'):   # (all terms equal: both errors are 0)
        diff_err = abs(logr_err_f - logr_err_uf) / min(logr_err_f, logr_err_uf)
    logr_err = max(logr_err_f, logr_err_uf)
    if diff_err > 0.25:
        warnings.warn('the estimated error for logr may be unreliable, since flattening before estimating tau makes the '
                      'result differ by more than 25%.', RuntimeWarning)
    if logr_err > 0.25:
        warnings.warn('the estimated error for logr may be unreliable, since the result is larger than 0.25.', RuntimeWarning)
    return logr, logr_err
