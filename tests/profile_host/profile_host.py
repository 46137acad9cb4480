"""ctypes front end of ``bayesfast_amd/csrc/bfhip_profile.h`` compiled for the host (TEST INFRASTRUCTURE ONLY): the grid lines of
``bfhip_profile_lines`` -- the masked Newton iteration in continuation -- run by one host thread on the tables the upload builds.
Nothing under ``bayesfast_amd/`` imports this module."""
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
        _lib = C.CDLL(os.path.join(_HERE, '_build', 'libbf_profile_host.so'))
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def line_arrays(d, fixed, walk, x_start, values):
    """The arguments of a profile call as contiguous arrays of the ABI's types: fixed (n_line, d) uint8, walk (n_line,) int32, x_start
    (n_line, d), values (n_line, n_val) or None."""
    x_start = np.ascontiguousarray(np.atleast_2d(x_start), dtype=np.float64)
    n = x_start.shape[0]
    fixed = np.ascontiguousarray(np.broadcast_to(np.asarray(fixed, dtype=bool), (n, d)), dtype=np.uint8)
    walk = np.ascontiguousarray(np.broadcast_to(np.asarray(walk), (n,)), dtype=np.int32)
    if values is not None:
        values = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(n, -1))
    return fixed, walk, x_start, values


def profile_lines(spec, fixed, walk, x_start, values=None, objective=0, max_iter=200, xtol=1e-5):
    """-> dict(x (n_line, n_val, d), logp (n_line, n_val), info (n_line, n_val, 4)) as ``bfhip_profile_lines`` returns them;
    ValueError where that call returns BFHIP_ERR_ARG."""
    from bayesfast_amd.device import density_desc_from_spec
    ds, keep = density_desc_from_spec(spec)
    d = int(spec['d'])
    fixed, walk, x_start, values = line_arrays(d, fixed, walk, x_start, values)
    n = x_start.shape[0]
    n_val = 1 if values is None else values.shape[1]
    x, logp, info = np.empty((n, n_val, d)), np.empty((n, n_val)), np.empty((n, n_val, 4))
    rc = lib().bfhost_profile_lines(C.byref(ds), C.c_int(int(max_iter)), C.c_double(float(xtol)), C.c_int(int(objective)), C.c_int(n),
                                    C.c_int(n_val), _p(fixed), _p(walk), _p(x_start), _p(values), _p(x), _p(logp), _p(info))
    if rc != 0:
        raise ValueError('bfhost_profile_lines refused its arguments: %d' % rc)
    return dict(x=x, logp=logp, info=info)


def objective(spec, x, objective=0):
    """x (n, d) -> value (n,), gradient (n, d) and Hessian diagonal (n, d) of the profile objective at x (sampling coordinates)."""
    from bayesfast_amd.device import density_desc_from_spec
    ds, keep = density_desc_from_spec(spec)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    n, d = x.shape
    f, g, h = np.empty(n), np.empty((n, d)), np.empty((n, d))
    rc = lib().bfhost_profile_objective(C.byref(ds), C.c_int(int(objective)), C.c_int(n), _p(x), _p(f), _p(g), _p(h))
    if rc != 0:
        raise RuntimeError('bfhost_profile_objective failed: %d' % rc)
    return f, g, h
