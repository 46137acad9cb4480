"""TEST-ONLY host restatement of a fitted SIT's transforms in fp64 NumPy: the model's own arrays (``_m``, ``_A``, ``_B``,
``_logdetA``) composed with the oracle's ``spline_apply`` on each iteration's splines, step by step as
``SIT._forward_device`` / ``SIT._backward_device`` run them.  ``parts(sit)`` snapshots what a fitted SIT holds now, in the
argument order of ``SIT._from_parts``."""
import numpy as np

from oracle import oracle as orc


def parts(sit):
    """(A, B, m, logdetA, splines) of the SIT as it is now: copies, so that a later refit cannot change them."""
    splines = [[(np.array(s.x), np.array(s.y), np.array(s.c)) for s in t.splines] for t in sit._tables]
    return np.array(sit._A), np.array(sit._B), np.array(sit._m), np.array(sit._logdetA), splines


def _apply(mode, splines, y):
    out = np.empty_like(y)
    for j, (x, v, c) in enumerate(splines):
        out[:, j] = orc.spline_apply(mode, c, x, v, np.ascontiguousarray(y[:, j]))
    return out


def forward(p, x):
    """``forward_transform`` of x (n, d) -> (y, log|J|)."""
    A, _, m, logdetA, splines = p
    y = np.array(x, dtype=np.float64)
    log_j = np.zeros(y.shape[0])
    for i in range(len(splines)):
        y = (y - m[i]) @ A[i].T
        log_j += np.log(_apply('derivative', splines[i], y)).sum(1)
        y = _apply('evaluate', splines[i], y)
    return y, log_j + np.sum(logdetA)


def backward(p, y):
    """``backward_transform`` of y (n, d) -> (x, log|J|)."""
    _, B, m, logdetA, splines = p
    x = np.array(y, dtype=np.float64)
    log_j = np.zeros(x.shape[0])
    for i in reversed(range(len(splines))):
        x = _apply('solve', splines[i], x)
        log_j += np.log(_apply('derivative', splines[i], x)).sum(1)
        x = x @ B[i].T + m[i]
    return x, log_j + np.sum(logdetA)


def logq(p, x):
    y, log_j = forward(p, x)
    return np.sum(-0.5 * y * y - 0.9189385332046727, axis=-1) + log_j
