"""The inputs of tests/test_gpu_data_reweight.py's comparison of ``bfhip_rw_finish`` with the reference, with the reference's results
(computed once per size and shared), and what rounding alone does to the reference on these very inputs:

    python tests/helpers/reweight_cases.py

prints, per figure, the largest difference between the float64 and the numpy.longdouble reference over every case (no GPU; the table
in docs/EXPERIMENTS.md and ``ROUNDING`` in the test come from it)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from reweight_reference import reweight_reference  # noqa: E402

SIZES = (1, 3, 4, 5, 24, 25, 255, 256, 257, 1000, 4097, 12289, 262145)
DIMS = (1, 7, 8, 15, 16, 27)
D_WIDE, N_WIDE = 128, 257          # the widest draw the device path takes, at one size
FIGS = ('log_evidence_ratio', 'khat', 'sigma', 'ess', 'mean', 'sd', 'mcse_mean')


def dims_of(n):
    return DIMS + ((D_WIDE,) if n == N_WIDE else ())


@functools.lru_cache(maxsize=None)
def rw_inputs(n):
    """x (n, 27) -- (n, 128) at n = 257 -- with scales from 1e-2 to 1e2 and offsets up to 1e3; a parameter's sums do not depend on d,
    so the first d columns are the case of d parameters.  Three log ratios up to n = 4097 (a shift of about 0.3, 0.7 and 0.05 sd with a
    little curvature: a light tail, a heavier one, a nearly flat one), one beyond.  Log weights that are -inf in most rows."""
    rng = np.random.default_rng(5000 + n)
    d = max(dims_of(n))
    k = 3 if n <= 4097 else 1
    z = rng.standard_normal((n, d))
    x = z * 10.**rng.uniform(-2., 2., size=d) + rng.uniform(-1., 1., size=d) * 10.**rng.uniform(0., 3., size=d)
    dirs = rng.standard_normal((3, d))
    dirs *= (np.array([0.3, 0.7, 0.05]) / np.sqrt((dirs * dirs).sum(axis=1)))[:, None]
    l = (z @ dirs.T + 0.03 * z[:, :1]**2 * np.array([1., -1., 0.5]) + np.array([0.4, -1.1, 2.]))[:, :k]
    lw = 0.7 * rng.standard_normal(n)
    lw[rng.random(n) < 0.85] = -np.inf
    if n < 25:
        lw[0] = 0.3
    return x, l, lw


@functools.lru_cache(maxsize=None)
def rw_reference(n, weighted, long=False):
    x, l, lw = rw_inputs(n)
    return reweight_reference(x, l, lw if weighted else None, dtype=np.longdouble if long else np.float64)


def rounding_table(sizes=SIZES):
    worst = {f: (0., None) for f in FIGS}
    for n in sizes:
        for weighted in (False, True):
            a, b = rw_reference(n, weighted), rw_reference(n, weighted, True)
            sdb = np.asarray(b['sd_base'], dtype=np.float64)
            for f in FIGS:
                va, vb = np.asarray(a[f], dtype=np.longdouble), np.asarray(b[f], dtype=np.longdouble)
                with np.errstate(all='ignore'):
                    if f == 'mean':
                        err = np.abs(va - vb) / np.where(np.isfinite(sdb) & (sdb > 0), sdb, np.abs(vb))
                    elif f == 'log_evidence_ratio':
                        err = np.abs(va - vb) / np.maximum(1., np.abs(vb))
                    else:
                        err = np.abs(va / vb - 1.)
                err = err[np.isfinite(err)]
                e = float(err.max()) if err.size else 0.
                print('n=%d w=%d %s %.3g' % (n, weighted, f, e), flush=True)
                if e > worst[f][0]:
                    worst[f] = (e, (n, weighted))
    return worst


if __name__ == '__main__':
    for f, (e, at) in rounding_table().items():
        print('%-20s %.3g at %s' % (f, e, at))
