"""ctypes front end of ``bayesfast_amd/csrc/bfhip_hess.h`` compiled for the host (TEST INFRASTRUCTURE ONLY): the analytic Hessian
and the damped Newton maximiser of the device kernels, run by one host thread on the tables the upload builds.  Nothing under
``bayesfast_amd/`` imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-C', _HERE, '-s'])
        _lib = C.CDLL(os.path.join(_HERE, '_build', 'libbf_hess_host.so'))
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def logp_grad_hess(spec, x, original_space=False):
    """x (n, d) -> logp (n,), grad (n, d), hess (n, d, d) of the spec's surrogate density, by the header's arithmetic."""
    from bayesfast_amd.device import density_desc_from_spec
    ds, keep = density_desc_from_spec(spec)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    n, d = x.shape
    logp, grad, hess = np.empty(n), np.empty((n, d)), np.empty((n, d, d))
    rc = lib().bfhost_logp_hess(C.byref(ds), C.c_int(n), _p(x), C.c_int(int(bool(original_space))), _p(logp), _p(grad), _p(hess))
    if rc != 0:
        raise RuntimeError('bfhost_logp_hess failed: %d' % rc)
    return logp, grad, hess


def maximize(spec, x0, max_iter=200, xtol=1e-5):
    """x0 (n_start, d) -> x, logp, hess, info as ``bfhip_laplace_opt`` returns them."""
    from bayesfast_amd.device import density_desc_from_spec
    ds, keep = density_desc_from_spec(spec)
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    n, d = x0.shape
    x, logp, hess, info = np.empty((n, d)), np.empty(n), np.empty((n, d, d)), np.empty((n, 4))
    rc = lib().bfhost_laplace_opt(C.byref(ds), C.c_int(int(max_iter)), C.c_double(float(xtol)), C.c_int(n), _p(x0), _p(x), _p(logp),
                                  _p(hess), _p(info))
    if rc != 0:
        raise RuntimeError('bfhost_laplace_opt failed: %d' % rc)
    return x, logp, hess, info


def constraint(x, kind, lo, hi):
    """x (n,) -> (n, 5): T, T', log|T'|, T''/T', d2 log|T'|/dx2 of ``bfhip_constraint.h`` for one kind and range."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.empty((x.size, 5))
    rc = lib().bfhost_constraint(C.c_int(x.size), _p(x), C.c_int(int(kind)), C.c_double(float(lo)), C.c_double(float(hi) - float(lo)), _p(out))
    if rc != 0:
        raise RuntimeError('bfhost_constraint failed: %d' % rc)
    return out


def step_adapt(fused, accept, smu, state, target_accept, gamma, k, t_0, one_call=True):
    """accept (n,) -> (n, 4): hbar, log_step, log_bar, count after each of n successive updates of ``BfStepAdapt<fused>``
    (``bfhip_adapt.h``) from state = (hbar, log_step, log_bar, count); through ``step`` (one_call), or ``consts`` and ``update``."""
    accept = np.ascontiguousarray(accept, dtype=np.float64).ravel()
    state = np.ascontiguousarray(state, dtype=np.float64)
    out = np.empty((accept.size, 4))
    lib().bfhost_step_adapt(C.c_int(int(bool(fused))), C.c_int(int(bool(one_call))), C.c_double(target_accept), C.c_double(gamma), C.c_double(k), C.c_double(t_0),
                            C.c_int(accept.size), _p(accept), C.c_double(smu), _p(state), _p(out))
    return out


def welford(fused, x, n0, mean, raw):
    """x (n,) -> (n, 2): mean, raw after each sample added by ``bf_welford_add<fused>`` to a window that starts at (n0, mean, raw)."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.empty((x.size, 2))
    lib().bfhost_welford(C.c_int(int(bool(fused))), C.c_int(x.size), _p(x), C.c_double(n0), C.c_double(mean), C.c_double(raw), _p(out))
    return out


def metric_window(state, n_iter, update_window, doubling):
    """-> (n_iter, 7): fg_n, bg_n, n_samples, prev_upd, adapt_window after each iteration of ``BfMetricWindow``, then its refresh and
    roll flags."""
    state = np.ascontiguousarray(state, dtype=np.float64)
    out = np.empty((n_iter, 7))
    lib().bfhost_metric_window(C.c_int(int(update_window)), C.c_int(int(bool(doubling))), C.c_int(int(n_iter)), _p(state), _p(out))
    return out
