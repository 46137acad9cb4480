"""The small ``TraceTuple`` that tests/test_trace_readers_host.py and tests/test_gpu_trace_readers.py read, and the byte comparison of
two results of a reader."""
import numpy as np

C, N, D, WARMUP = 6, 40, 3, 12
SELECTIONS = (dict(), dict(since_iter=20), dict(include_warmup=True), dict(original_space=False))


def trace(to=None):
    """(tt, rng): 6 chains x 40 iterations x 3 parameters with 12 of warm-up from ``default_rng(5)``, chains 3..5 shifted by 4,
    samples_original = 10 s + 1, logp_original = stats[..., 0] - 1; ``to`` maps every part (to a device tensor, say); ``rng`` goes
    on to draw the weights."""
    from bayesfast_amd import _lib
    from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple
    rng = np.random.default_rng(5)
    s = rng.normal(size=(C, N, D))
    s[3:] += 4.
    st = np.zeros((C, N, _lib.STAT_STRIDE))
    st[:, :, 0] = rng.normal(size=(C, N))
    parts = (s, st, 10. * s + 1., st[:, :, 0] - 1.)
    if to is not None:
        parts = tuple(to(p) for p in parts)
    return TraceTuple(NTrace(n_chain=C, n_iter=N, n_warmup=WARMUP), *parts), rng


def start_of(sel):
    return sel.get('since_iter', 0 if sel.get('include_warmup') else WARMUP)


def same(a, b):
    """Every array, tensor and field of two results, byte for byte (NaN equals NaN of the same bits)."""
    if hasattr(a, 'detach'):
        return hasattr(b, 'detach') and a.device == b.device and same(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    if isinstance(a, np.ndarray):
        return (isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes())
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if hasattr(a, '__dict__'):
        return type(a) is type(b) and same(vars(a), vars(b))
    return type(a) is type(b) and repr(a) == repr(b)
