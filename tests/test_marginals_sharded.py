"""``marginals_sharded`` / ``TraceTuple.marginals`` as a collective, on the CPU: a spawned gloo world of two ranks with ragged shards
(5 and 3 chains) and the NumPy passes standing in for the device's.  Every rank's masses, outside tallies, total and levels equal
the single-process result over the concatenation, ==; the number of collectives is counted and depends on neither d nor n; the
samples never cross."""
import os
import pickle

import numpy as np

FIELDS = ('mass1d', 'mass2d', 'outside', 'levels1d', 'levels2d', 'edges', 'edges2d')
CASES = [dict(n_t=60, d=3, weighted=True, ranges=False), dict(n_t=60, d=3, weighted=False, ranges=False),
         dict(n_t=60, d=3, weighted=True, ranges=True), dict(n_t=60, d=3, weighted=False, ranges=True),
         dict(n_t=211, d=18, weighted=True, ranges=False), dict(n_t=211, d=18, weighted=True, ranges=True)]


def case_data(c):
    rng = np.random.default_rng(c['n_t'] + c['d'])
    x = rng.standard_normal((8, c['n_t'], c['d'])) * (1. + np.arange(c['d']))
    x[6, 3, 0] = 40.                                   # the largest value of column 0 sits in the second shard
    x[1, 2, 1] = np.nan
    lw = 1.5 * rng.standard_normal((8, c['n_t'])) if c['weighted'] else None
    if lw is not None:
        lw[7, 5] = 9.                                  # the largest weight too
        lw[0, :4] = -np.inf
    ranges = np.array([(-2. - i, 3. + i) for i in range(c['d'])]) if c['ranges'] else None
    return x, lw, ranges, dict(bins=20, bins2d=6, pairs=[(0, 1), (c['d'] - 1, 0), (1, 2)], probs=(0.5, 0.9))


def pack(m):
    return {k: getattr(m, k).tobytes() for k in FIELDS} | dict(total=m.total)


def _worker(rank, ws, port, q):
    import torch
    import torch.distributed as dist
    from bayesfast_amd.samplers.sample_trace import NTrace, TraceTuple
    import importlib
    mg = importlib.import_module('bayesfast_amd.utils.marginals')
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    try:
        out = []
        sl = slice(0, 5) if rank == 0 else slice(5, 8)
        for c in CASES:
            x, lw, ranges, opt = case_data(c)
            n_t, d = c['n_t'], c['d']
            st = {}
            chk = mg._check_options(d, opt['bins'], opt['bins2d'], ranges, None, opt['pairs'], opt['probs'])
            passes = mg._HostPasses(x[sl].reshape(-1, d), None if lw is None else lw[sl].reshape(-1), None if lw is None else 'log')
            m = mg.marginals_sharded(passes, *chk, stats=st)
            # the TraceTuple method on host shards: the same collective, over the draws after the warm-up
            tr = NTrace(n_chain=8, n_iter=n_t, n_warmup=10, random_generator=1)
            stats = np.zeros((8, n_t, 11))
            tt = TraceTuple(tr, torch.as_tensor(x[sl]), torch.as_tensor(stats[sl]), torch.as_tensor(x[sl]), torch.as_tensor(stats[sl, :, 0]))
            mt = tt.marginals(None if lw is None else lw[sl, 10:], ranges=ranges, **opt)
            out.append((pack(m), st['collectives'], pack(mt)))
        q.put((rank, pickle.dumps(out)))
    except Exception as ex:   # (reported, not left for the parent's queue timeout)
        import traceback
        q.put((rank, repr(ex) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_ragged_shards_equal_one_process_bin_for_bin():
    import torch.multiprocessing as mp
    from bayesfast_amd.utils import marginals
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r[0])
    [p.join(60) for p in ps]
    assert all(isinstance(r[1], bytes) for r in res), res
    res = [pickle.loads(r[1]) for r in res]
    counts = {}
    for i, c in enumerate(CASES):
        x, lw, ranges, opt = case_data(c)
        for since, pick in ((0, 0), (10, 2)):
            want = pack(marginals(x[:, since:], log_weights=None if lw is None else lw[:, since:], ranges=ranges, **opt))
            assert want['total'] > 0
            for rank in range(2):
                got = res[rank][i][pick]
                for k in want:
                    assert got[k] == want[k], (c, since, rank, k)
        assert res[0][i][1] == res[1][i][1]
        counts.setdefault((c['weighted'], c['ranges']), set()).add(res[0][i][1])
    # the maximum of the weights, the draw count, the extremes, the masses: each one collective, whatever d and n are
    assert counts == {(True, False): {4}, (False, False): {3}, (True, True): {3}, (False, True): {2}}


def test_all_reduce_max_without_a_process_group_is_a_no_op():
    import torch
    from bayesfast_amd import parallel
    t = torch.tensor([1., -2.])
    assert parallel.all_reduce_max(t) is t and t.tolist() == [1., -2.] and 'all_reduce_max' in parallel.__all__
