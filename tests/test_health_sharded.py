"""``sampler_health_sharded`` / ``TraceTuple.health`` as a collective, on the CPU: a spawned gloo world of two ranks with ragged
shards (3 and 2 chains) on host tensors.  Every rank's ``SamplerHealth`` equals the single-process result over all five chains byte
for byte; the number of collectives is 2, whatever n and d are; the draws and the statistics table never cross."""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

CASES = [dict(n=40, d=3, sampler='NUTS'), dict(n=211, d=18, sampler='HMC')]
WARMUP = 10
FIELDS = ('n_divergent', 'n_max_treedepth', 'n_leapfrog', 'max_tree_size', 'n_accepted', 'n_nonfinite', 'n_moved', 'depth_hist_chain',
          'mean_accept', 'logp_mean', 'logp_var', 'energy_mean', 'energy_var', 'bfmi', 'step_size', 'chain_mean', 'chain_var', 'chain_z',
          'var_ratio', 'logp_z', 'depth_hist', 'divergent', 'saturated', 'low_bfmi', 'stuck', 'errored', 'flagged')
SCALARS = ('n_chain', 'n_rows', 'n_transitions', 'n_divergent_total', 'share_divergent', 'n_max_treedepth_total', 'share_max_treedepth',
           'n_leapfrog_total', 'bfmi_min', 'bfmi_median', 'ok', 'sampler', 'max_treedepth')


def case_data(c):
    import health_reference as hr
    rng = np.random.default_rng(c['n'] + c['d'])
    st = hr.random_table(rng, 5, c['n'], c['sampler'])
    x = rng.standard_normal((5, c['n'], c['d'])) * (1. + np.arange(c['d']))
    st[4, 20, 1] = np.nan                              # an errored chain in the second shard
    x[1], st[1, :, 0] = x[1, :1], st[1, 0, 0]          # a frozen one in the first
    return st, x


def pack(h):
    return {k: np.ascontiguousarray(getattr(h, k)).tobytes() for k in FIELDS} | {k: repr(getattr(h, k)) for k in SCALARS} | dict(
        warnings=h.warnings(), text=str(h))


def _worker(rank, ws, port, q):
    import torch
    import torch.distributed as dist
    from bayesfast_amd.samplers.sample_trace import HTrace, NTrace, TraceTuple
    from bayesfast_amd.utils import sampler_health_sharded
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    try:
        out = []
        sl = slice(0, 3) if rank == 0 else slice(3, 5)
        for c in CASES:
            st, x = case_data(c)
            info = {}
            h = sampler_health_sharded(torch.as_tensor(st[sl]), torch.as_tensor(x[sl]), 5, sampler=c['sampler'], max_treedepth=7, stats=info)
            # the TraceTuple method on host shards: the same collective, over the rows after the warm-up
            cls = HTrace if c['sampler'] == 'HMC' else NTrace
            kw = dict() if c['sampler'] == 'HMC' else dict(max_treedepth=7)
            tt = TraceTuple(cls(n_chain=5, n_iter=c['n'], n_warmup=WARMUP, random_generator=1, **kw), torch.as_tensor(x[sl]),
                            torch.as_tensor(st[sl]), torch.as_tensor(x[sl]), torch.as_tensor(st[sl, :, 0]))
            info_t = {}
            ht = tt.health(stats=info_t)
            out.append((pack(h), info, pack(ht), info_t))
        q.put((rank, pickle.dumps(out)))
    except Exception as ex:   # (reported, not left for the parent's queue timeout)
        import traceback
        q.put((rank, repr(ex) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_ragged_shards_equal_one_process_byte_for_byte():
    import torch.multiprocessing as mp
    from bayesfast_amd.utils import sampler_health
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 37500 + os.getpid() % 2000
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r[0])
    [p.join(60) for p in ps]
    assert all(isinstance(r[1], bytes) for r in res), res
    res = [pickle.loads(r[1]) for r in res]
    for i, c in enumerate(CASES):
        st, x = case_data(c)
        for since, pick in ((0, 0), (WARMUP, 2)):
            one = sampler_health(st[:, since:], x[:, since:], sampler=c['sampler'], max_treedepth=7 if (pick == 0 or c['sampler'] == 'NUTS') else 10)
            want = pack(one)
            assert one.errored[4] and one.stuck[1] and not one.ok
            for rank in range(2):
                got = res[rank][i][pick]
                for k in want:
                    assert got[k] == want[k], (c, since, rank, k)
                # two collectives (the float table, the int table), whatever n and d are; a rank sends its own chains' tables
                info = res[rank][i][pick + 1]
                assert info['collectives'] == 2
                assert info['wire_bytes'] == (3, 2)[rank] * 8 * (20 + 7 + 2 * c['d'])
