"""The sharded driver of the integrated autocorrelation time (utils/acor.py: integrated_time_sharded) on CPU: the lag-block
search with a NumPy stand-in for the device lag sums against the values recorded from the reference, and the collective on a
spawned gloo world of two ranks with ragged shards -- one all-reduce of the block's lag sums per block, never the samples."""
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def np_lag_sums(x, t0, n_lag):
    """sum_w a_wk(t) / a_wk(0) for t0 <= t < t0 + n_lag by the definition (direct products, no FFT)."""
    y = np.asarray(x, dtype=np.float64)
    y = y - y.mean(axis=1, keepdims=True)
    n_t = y.shape[1]
    a0 = (y * y).sum(axis=1)
    out = np.zeros((n_lag, y.shape[2]))
    for i in range(n_lag):
        t = t0 + i
        if t < n_t:
            out[i] = ((y[:, :n_t - t] * y[:, t:]).sum(axis=1) / a0).sum(axis=0)
    return out


def ar1(rng, phi, n_w, n_t, n_d):
    e = rng.normal(size=(n_w, n_t, n_d))
    for t in range(1, n_t):
        e[:, t] = phi * e[:, t - 1] + np.sqrt(1 - phi * phi) * e[:, t]
    return e


def walkers(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape({1: (1, -1, 1), 2: (1,) + x.shape, 3: x.shape}[x.ndim])


def test_driver_with_a_numpy_stand_in_reproduces_the_reference():
    """tests/golden/evidence.npz acor.tau3 / tau2 / tau1 (recorded from the reference's estimator) to 1e-12, 3-D, 2-D and 1-D."""
    from bayesfast_amd.utils.acor import integrated_time_sharded
    fx = np.load(os.path.join(G, 'evidence.npz'))
    for x, want in ((fx['acor.x'], fx['acor.tau3']), (fx['acor.x'][0], fx['acor.tau2']), (fx['acor.x'][1, :, 0], fx['acor.tau1'])):
        x = walkers(x)
        st = {}
        tau = integrated_time_sharded(x, x.shape[0], lag_sums=np_lag_sums, stats=st)
        np.testing.assert_allclose(tau, want, rtol=1e-12)
        assert st['collectives'] == 0 and st['blocks'] >= 1


def test_long_window_takes_several_doubling_blocks():
    """phi = 0.95 (tau about 39): windows beyond the first block of 64 lags, so blocks of 64, 128, ... until they close -- the
    last block is the first that reaches the windows, within twice the lags they need -- and the same tau and AutocorrError as
    the host port."""
    from bayesfast_amd.utils.acor import integrated_time, integrated_time_sharded, AutocorrError
    x = ar1(np.random.default_rng(3), 0.95, 4, 4000, 2)
    st = {}
    tau = integrated_time_sharded(x, 4, lag_sums=np_lag_sums, stats=st)
    np.testing.assert_allclose(tau, integrated_time(x), rtol=1e-12)
    # lags the windows need: up to the largest first t with t >= 5 tau(t)
    rho = np_lag_sums(x, 0, 4000) / 4
    need = 1 + int(np.max((np.arange(4000)[:, None] >= 5 * (2 * np.cumsum(rho, axis=0) - 1)).argmax(axis=0)))
    assert need > 64 and st['blocks'] >= 2 and st['lags'] == 64 * (2**st['blocks'] - 1)
    assert st['lags'] - 64 * 2**(st['blocks'] - 1) < need <= st['lags'] <= 2 * need + 64
    # a window beyond the last doubling block: every lag is summed; too short -> AutocorrError with the host port's .tau
    xs = ar1(np.random.default_rng(4), 0.999, 2, 300, 1)
    with pytest.raises(AutocorrError) as host:
        integrated_time(xs)
    with pytest.raises(AutocorrError) as drv:
        integrated_time_sharded(xs, 2, lag_sums=np_lag_sums, stats=st)
    np.testing.assert_allclose(drv.value.tau, host.value.tau, rtol=1e-12)
    assert st['lags'] == 300


def test_edge_cases_match_the_host_port():
    """n_t = 1 and 2, a constant dimension (NaN, decided in the first block), c <= 0 (window 0), quiet (a warning)."""
    from bayesfast_amd.utils.acor import integrated_time, integrated_time_sharded, AutocorrError
    rng = np.random.default_rng(5)
    for x in (rng.normal(size=(7, 1, 3)), rng.normal(size=(5, 2, 2))):
        np.testing.assert_allclose(integrated_time_sharded(x, x.shape[0], quiet=True, lag_sums=np_lag_sums),
                                   integrated_time(x, quiet=True), rtol=1e-10, atol=1e-12)
    x = rng.normal(size=(3, 500, 2))
    x[:, :, 1] = 3.
    st = {}
    with np.errstate(invalid='ignore', divide='ignore'):
        tau = integrated_time_sharded(x, 3, lag_sums=np_lag_sums, stats=st)
        np.testing.assert_allclose(tau, integrated_time(x), rtol=1e-12)
    assert np.isnan(tau[1]) and st['blocks'] == 1
    for c in (0, -1.):
        np.testing.assert_array_equal(integrated_time_sharded(x[:, :, :1], 3, c=c, lag_sums=np_lag_sums), [1.])
    with pytest.raises(AutocorrError):
        integrated_time_sharded(x[:, :20, :1], 3, lag_sums=np_lag_sums)
    integrated_time_sharded(x[:, :20, :1], 3, quiet=True, lag_sums=np_lag_sums)   # (logs instead)


def _acor_worker(rank, ws, port, q):
    import torch
    import torch.distributed as dist
    from bayesfast_amd import parallel
    from bayesfast_amd.utils.acor import integrated_time_sharded
    from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    try:
        n_chain, n_t, d = 7, 2000, 3                  # ragged shards: 4 + 3 chains
        x = ar1(np.random.default_rng(8), 0.9, n_chain, n_t, d)
        x[:, :, 2] = ar1(np.random.default_rng(9), 0.97, n_chain, n_t, 1)[:, :, 0]   # a window beyond the first block
        b, e = parallel.shard_range(n_chain, rank, ws)
        st = {}
        tau = integrated_time_sharded(torch.as_tensor(x[b:e]), n_chain, quiet=True, lag_sums=np_lag_sums, stats=st)
        # the TraceTuple method on host shards: the same collective, with the host autocovariances of the shard
        tr = NTrace(n_chain=n_chain, n_iter=n_t, n_warmup=100, random_generator=1)
        lp = np.random.default_rng(10).normal(size=(n_chain, n_t))
        stats = np.zeros((n_chain, n_t, 11))
        stats[:, :, 0] = lp
        tt = TraceTuple(tr, torch.as_tensor(x[b:e]), torch.as_tensor(stats[b:e]), torch.as_tensor(x[b:e]), torch.as_tensor(lp[b:e]))
        tau_tt = tt.integrated_time(quiet=True)
        tau_lp = tt.integrated_time(return_type='logp', original_space=False, since_iter=500)
        q.put((rank, tau.tobytes(), st, tau_tt.tobytes(), tau_lp.tobytes()))
    except Exception as ex:   # (reported, not left for the parent's queue timeout)
        q.put((rank, repr(ex), None, None, None))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_ragged_shards_agree_bitwise_and_move_only_lag_sums():
    """2 ranks, 7 chains (4 + 3): both ranks return the same tau bit for bit, equal to the single-process host port to 1e-12; one
    all-reduce per lag block, and the bytes sent are the blocks' lag sums -- far below the samples'."""
    import torch.multiprocessing as mp
    from bayesfast_amd.utils.acor import integrated_time
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    ps = [ctx.Process(target=_acor_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r[0])
    [p.join(60) for p in ps]
    assert all(r[2] is not None for r in res), res
    assert res[0][1] == res[1][1] and res[0][3] == res[1][3] and res[0][4] == res[1][4]
    x = ar1(np.random.default_rng(8), 0.9, 7, 2000, 3)
    x[:, :, 2] = ar1(np.random.default_rng(9), 0.97, 7, 2000, 1)[:, :, 0]
    np.testing.assert_allclose(np.frombuffer(res[0][1]), integrated_time(x, quiet=True), rtol=1e-12)
    np.testing.assert_allclose(np.frombuffer(res[0][3]), integrated_time(x[:, 100:], quiet=True), rtol=1e-12)
    lp = np.random.default_rng(10).normal(size=(7, 2000))
    np.testing.assert_allclose(np.frombuffer(res[0][4]), integrated_time(lp[:, 500:, None]), rtol=1e-12)
    for _, _, st, _, _ in res:
        assert st['blocks'] >= 2 and st['collectives'] == st['blocks']
        assert st['wire_bytes'] == st['lags'] * 3 * 8
        assert st['wire_bytes'] < x.nbytes / 20
