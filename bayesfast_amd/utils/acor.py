"""Integrated autocorrelation time with Sokal's automatic window -- the estimator behind the error bar of the bridge
estimate (reference: bayesfast/utils/acor.py:79-145, vendored from emcee; used at evidence/bridge.py:59-64).

All series are transformed at once: one real FFT over the time axis of the (walker, time, dimension) array gives every
autocorrelation function, their walker average rho_k(t), the running sums tau_k(W) = 2 sum_{t <= W} rho_k(t) - 1, and
for each dimension the first window W with W >= c tau_k(W).  Host NumPy.

A GPU tensor takes the device route instead (``integrated_time_sharded``): ``bfhip_acor_moments`` once, then
``bfhip_acor_lag_sums`` over blocks of lags that start at 0 and double in length, until every dimension's window has closed.
Only the (n_lag, n_d) lag sums of each block reach the host; under ``torch.distributed`` they are summed over the ranks first,
so each rank reads only its own chains."""
import logging

import numpy as np

__all__ = ['integrated_time', 'integrated_time_sharded', 'AutocorrError']


class AutocorrError(Exception):
    """The series is too short for the estimate to be trusted; ``tau`` carries the estimate anyway."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super().__init__(*args, **kwargs)


def _as_walkers(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 0:
        x = x.reshape(1)
    shape = {1: (1, x.shape[0], 1), 2: (1,) + x.shape, 3: x.shape}.get(x.ndim)
    if shape is None:
        raise ValueError('invalid dimensions.')
    return x.reshape(shape)


def integrated_time(x, c=5, tol=50, quiet=False):
    """x: (n_t,), (n_t, n_d) or (n_walker, n_t, n_d) -> tau (n_d,).  Raises ``AutocorrError`` (or, with ``quiet``, logs a
    warning) when the series is shorter than ``tol`` autocorrelation times.  A GPU tensor is reduced on its device (other
    dtypes as float64); NumPy arrays and CPU tensors take the host path."""
    if getattr(x, 'is_cuda', False):
        return _device_integrated_time(x, c, tol, quiet)
    x = _as_walkers(x)
    n_t = x.shape[1]
    n_fft = 2 << max(n_t - 1, 0).bit_length()           # twice the next power of two: no wrap-around in the products
    spec = np.fft.fft(x - x.mean(axis=1, keepdims=True), n=n_fft, axis=1)
    acov = np.fft.ifft(spec * np.conjugate(spec), axis=1)[:, :n_t].real
    rho = (acov / acov[:, :1]).mean(axis=0)               # (n_t, n_d): every walker normalised by its own variance
    running = 2.0 * np.cumsum(rho, axis=0) - 1.0
    lags = np.arange(n_t)[:, None]
    beyond = lags >= c * running                           # first lag that is at least c running autocorrelation times
    window = beyond.argmax(axis=0)                         # (0 when the window never closes, as the reference's auto_window)
    tau = running[window, np.arange(running.shape[1])]
    return _checked(tau, n_t, tol, quiet)


def _checked(tau, n_t, tol, quiet):
    too_short = tol * tau > n_t
    if too_short.any():
        text = ('The chain is shorter than {} times the integrated autocorrelation time for {} parameter(s) '
                '(N / {} = {:.0f}, tau = {}): use this estimate with caution and run a longer chain.'
                .format(tol, int(too_short.sum()), tol, n_t / tol, tau))
        if not quiet:
            raise AutocorrError(tau, text)
        logging.warning(text)
    return tau


# ---- the device route ---------------------------------------------------------------------------------------------------------
FIRST_BLOCK = 64   # lags of the first block; every further block doubles


def _device_integrated_time(x, c, tol, quiet):
    import torch
    if x.ndim not in (0, 1, 2, 3):
        raise ValueError('invalid dimensions.')
    if x.dtype != torch.float64:
        x = x.to(torch.float64)
    x = x.reshape({0: (1, 1, 1), 1: (1, -1, 1), 2: (1,) + tuple(x.shape), 3: tuple(x.shape)}[x.ndim])
    with torch.cuda.device(x.device):
        return integrated_time_sharded(x, x.shape[0], c, tol, quiet)


class _DeviceLagSums:
    """``lag_sums`` of the device route: ``bfhip_acor_moments`` on first use, then ``bfhip_acor_lag_sums`` per block.  The
    walkers' (n_t, n_d) blocks must each be contiguous; the walker stride is free, so a ``[:, since:]`` view goes in as it is."""

    def __init__(self):
        self.moments = None

    def __call__(self, x, t0, n_lag):
        from .. import _lib
        from ..device import get_context, _ptr
        import torch
        n_w, n_t, n_d = (int(v) for v in x.shape)
        if x.dtype != torch.float64:
            x = x.to(torch.float64)
        if x.stride(2) != 1 or x.stride(1) != n_d or (n_w > 1 and x.stride(0) < n_t * n_d):
            x = x.contiguous()
        ctx = get_context(x.device.index)
        ldw = int(x.stride(0)) if n_w > 1 else n_t * n_d
        if self.moments is None:
            self.moments = (ctx.empty((n_w, n_d)), ctx.empty((n_w, n_d)))
            _lib.check(ctx._lib.bfhip_acor_moments(ctx.handle, n_w, n_t, n_d, ldw, _ptr(x), *(_ptr(m) for m in self.moments)))
        work = ctx.empty((min(n_w, _lib.ACOR_MAX_GROUPS) * n_lag * n_d,))
        out = ctx.empty((n_lag, n_d))
        _lib.check(ctx._lib.bfhip_acor_lag_sums(ctx.handle, n_w, n_t, n_d, ldw, _ptr(x), *(_ptr(m) for m in self.moments), int(t0),
                                                int(n_lag), _ptr(work), _ptr(out)))
        return out


def _host_lag_sums(x, t0, n_lag):
    """``lag_sums`` on a host shard (CPU tensor or array): the host port's FFT autocovariances, summed over the walkers."""
    y = np.asarray(x, dtype=np.float64)
    n_t = y.shape[1]
    n_fft = 2 << max(n_t - 1, 0).bit_length()
    spec = np.fft.fft(y - y.mean(axis=1, keepdims=True), n=n_fft, axis=1)
    acov = np.fft.ifft(spec * np.conjugate(spec), axis=1)[:, :n_t].real
    import torch
    return torch.as_tensor((acov / acov[:, :1])[:, t0:t0 + n_lag].sum(axis=0))


def integrated_time_sharded(x_local, n_walker, c=5, tol=50, quiet=False, lag_sums=None, stats=None):
    """``integrated_time`` of all ``n_walker`` walkers when this rank holds ``x_local`` (n_loc, n_t, n_d), its own walkers; with
    more than one rank a collective that every rank calls, and every rank returns the same tau (n_d,).

    Lags are summed in blocks: [0, 64), then blocks of twice the previous length, until every dimension's window has closed (or
    its running sum has turned NaN, after which it cannot close) or the lags run out -- at most about twice the lags the windows
    need, in O(log n_t) blocks.  After each block the (n_lag, n_d) walker sums are summed over the ranks
    (``parallel.all_reduce_sum``) and read on the host, where the running sums are carried forward; every rank decides from the
    same reduced numbers, so every rank runs the same blocks.  ``lag_sums(x_local, t0, n_lag)`` -> (n_lag, n_d) tensor of
    sum_w a_wk(t) / a_wk(0) over the local walkers defaults to the device kernels; the CPU tests inject host stand-ins.
    ``stats``, if a dict, receives 'collectives' and 'wire_bytes' (what this rank sent), 'blocks' and 'lags'."""
    import torch
    from .. import parallel
    rank, ws = parallel.world()
    n_t, n_d = int(x_local.shape[1]), int(x_local.shape[2])
    if n_t == 0:
        raise ValueError('attempt to get argmax of an empty sequence')
    if n_d == 0:
        return np.zeros(0)
    on_device = getattr(x_local, 'is_cuda', False)
    if lag_sums is None:
        lag_sums = _DeviceLagSums() if on_device else _host_lag_sums
    dev = x_local.device if on_device else 'cpu'
    rho, t0, n_lag = [], 0, FIRST_BLOCK
    n_coll = wire = n_block = 0
    while True:
        n = min(n_lag, n_t - t0)
        if x_local.shape[0] > 0:
            s = lag_sums(x_local, t0, n)
            if not isinstance(s, torch.Tensor):
                s = torch.as_tensor(np.asarray(s, dtype=np.float64))
        else:   # (a rank without walkers contributes zeros to the collective)
            s = torch.zeros((n, n_d), dtype=torch.float64, device=dev)
        if ws > 1:
            s = parallel.all_reduce_sum(s.contiguous())
            n_coll += 1
            wire += n * n_d * 8
        rho.append(s.cpu().numpy().astype(np.float64, copy=False) / n_walker)
        n_block += 1
        t0 += n
        running = 2.0 * np.cumsum(np.concatenate(rho, axis=0), axis=0) - 1.0
        beyond = np.arange(t0)[:, None] >= c * running
        decided = beyond.any(axis=0) | np.isnan(running[-1])
        if t0 >= n_t or decided.all():
            break
        n_lag *= 2
    if stats is not None:
        stats.update(collectives=n_coll, wire_bytes=wire, blocks=n_block, lags=t0)
    window = beyond.argmax(axis=0)
    tau = running[window, np.arange(n_d)]
    return _checked(tau, n_t, tol, quiet)
