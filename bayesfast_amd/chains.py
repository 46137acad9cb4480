"""Batched chain state on one GPU and the fused NUTS/HMC launch (bfhip_sampler_run)."""
import ctypes as C
import os

import numpy as np

from . import _lib, layout as _layout
from .device import DeviceDensity, _ptr

__all__ = ['DeviceChains']

# what 'auto' runs while the trees of a group are in step: 'split' (eight waves per 16 chains, two per SIMD with disjoint work:
# integrator and bookkeeper waves; NUTS on the plain surrogate at 33 <= d <= 64 -- the library runs everything else as 'group')
# or 'group'.  Same results either way, bit for bit; 'split' is 3 % (7-leaf trees) to 13 % (15-leaf trees) faster
IN_STEP_LAYOUT = os.environ.get('BFHIP_IN_STEP_LAYOUT', 'split')
if IN_STEP_LAYOUT not in ('group', 'split'):
    raise ValueError("BFHIP_IN_STEP_LAYOUT should be 'group' or 'split', not {!r}.".format(IN_STEP_LAYOUT))


def _torch():
    import torch
    return torch


def _launch_schedule(launch_iters, n_run, n_warmup, i_iter):
    """[(end, step)] of the launches of a ``run`` of ``n_run`` iterations that starts at iteration ``i_iter``: ``end`` counts from
    the start of the run (the last launch may end beyond ``n_run``: it is cut there), ``step`` is the launch's nominal length."""
    # launch lengths: one number, or a sequence whose last entry repeats (sample(): the warm-up in one launch)
    if isinstance(launch_iters, str):
        if launch_iters != 'auto':
            raise ValueError("launch_iters should be a number, a sequence of numbers, None or 'auto'.")
        n_adapting = max(0, min(int(n_warmup) - i_iter, n_run))   # a function of the arguments only
        launch_iters = [100] * (-(-n_adapting // 100)) + [250]
    if isinstance(launch_iters, (list, tuple)):
        lens = [max(1, int(v)) for v in launch_iters]
    else:
        lens = [max(1, int(launch_iters) if launch_iters else n_run)]
    schedule, end = [], 0
    while end < n_run:
        step = lens[min(len(schedule), len(lens) - 1)]
        end += step
        schedule.append((end, step))
    return schedule


def _judging_share(i0, i1, n_warmup):
    """The share of equal trees that counts as "in step" for the launch of iterations [i0, i1).  A launch that ends the warm-up is
    judged more leniently: its last iterations still adapt the step size (a few trees of another size), the launch after it runs
    with the frozen, averaged one.  Launches inside the warm-up: 7-leaf trees with one 15-leaf tree in ten already run faster in
    step -- the late warm-up launches of the default run 5.5 against 6.0 ms, tools/launch_times.py."""
    return 0.85 if i0 < n_warmup <= i1 else (0.8 if i1 < n_warmup else 0.98)


class DeviceChains:
    """All chains of one GPU shard: positions, per-chain step-size and metric adaptation state, RNG streams.

    The per-chain arithmetic is the reference's (``BaseHMC.astep``, samplers/hmc_utils/base_hmc.py:62-85);
    the state that the reference keeps in one ``NTrace``/``HTrace`` object per chain
    (samplers/sample_trace.py:157-455) lives here in three device tensors, so a later ``run`` continues the
    chains exactly where they stopped.

    Parameters
    ----------
    density : DeviceDensity
    x_0 : (n_chain, d) array_like, starting points in the sampler's (transformed) space
    seed, first_stream : the xoshiro256++ stream of chain i is (seed, first_stream + i); with
        first_stream = global index of this shard's first chain, results do not depend on the sharding.
    """

    def __init__(self, density, x_0, seed=0, first_stream=0, step_size=1., metric=None, initial_mean=None,
                 initial_weight=10., adapt_window=60):
        torch = _torch()
        if not isinstance(density, DeviceDensity):
            raise ValueError('density should be a DeviceDensity.')
        self.density = density
        self.ctx = density.ctx
        x_0 = self.ctx.tensor(x_0, torch.float64)
        if x_0.dim() != 2 or x_0.shape[1] != density.d:
            raise ValueError('x_0 should have shape (n_chain, {}).'.format(density.d))
        self.n_chain, self.d = x_0.shape
        self._n_cu = None
        lib, h = self.ctx._lib, self.ctx.handle
        self.rng = torch.empty((self.n_chain, 4), dtype=torch.int64, device=self.ctx.device)
        self.sc = self.ctx.empty((self.n_chain, _lib.SC_N))
        self.vec = self.ctx.empty((self.n_chain, _lib.VEC_N, self.d))
        self.n_leapfrog = torch.zeros((1,), dtype=torch.int64, device=self.ctx.device)
        # metric: None / 1-d variances -> QuadMetricDiag(Adapt); 'full' / 2-d covariance -> QuadMetricFull(Adapt)
        cov0 = None
        self.full_metric = isinstance(metric, str) and metric == 'full'
        if isinstance(metric, str):
            if metric not in ('diag', 'full'):
                raise ValueError('invalid value for metric.')
            metric = None
        elif metric is not None and np.ndim(metric) == 2:
            cov0 = np.asarray(metric, dtype=np.float64)
            if cov0.shape != (self.d, self.d):
                raise ValueError('invalid value for metric.')
            metric, self.full_metric = None, True
        mv = None if metric is None else self.ctx.tensor(np.asarray(metric, dtype=np.float64).reshape(self.d))
        im = None if initial_mean is None else self.ctx.tensor(np.asarray(initial_mean, dtype=np.float64).reshape(self.d))
        _lib.check(lib.bfhip_rng_seed(h, self.n_chain, int(seed) & (2**64 - 1), int(first_stream), _ptr(self.rng)))
        _lib.check(lib.bfhip_chain_init(h, self.n_chain, self.d, _ptr(x_0), float(step_size), _ptr(mv), _ptr(im),
                                        float(initial_weight), int(adapt_window), _ptr(self.sc), _ptr(self.vec)))
        self.mat = None
        if self.full_metric:
            self.mat = torch.zeros((self.n_chain, _lib.MAT_N, self.d, self.d), dtype=torch.float64, device=self.ctx.device)
            c0 = None if cov0 is None else self.ctx.tensor(cov0, torch.float64)
            _lib.check(lib.bfhip_metric_init_full(h, self.n_chain, self.d, _ptr(c0), float(initial_weight), _ptr(self.sc),
                                                  _ptr(self.mat)))
            self.raise_on_error()
        self.i_iter = 0
        self.tu = None            # run_tempered: the tempering coordinate of every chain
        self.last_layout = None   # the layout of the last launch of run()
        self._answers = []        # _note_trees: one entry per launch, oldest first: int, None (no answer: not NUTS) or (event, slot)
        self._step_host = self._step_dev = None   # the answers' pinned ring and the device work buffer, made when first needed
        self._n_flag = 0

    def _sampler_config(self, sampler, n_warmup, max_treedepth, n_int_step, max_change, target_accept, gamma, k, t_0,
                        adapt_step_size, adapt_metric, update_window, doubling):
        """``bfhip_sampler_config`` but for ``chain_layout`` (0; ``run`` sets it per launch)."""
        # (the full-rank metric under TNUTS too, with cubic configs, d = 128, the pipeline density: bfhip_tnuts_gen.hip)
        return _lib.SamplerConfig(
            sampler={'NUTS': 0, 'HMC': 1}[sampler], n_warmup=int(n_warmup), max_treedepth=int(max_treedepth),
            n_int_step=int(n_int_step), max_change=float(max_change), target_accept=float(target_accept), gamma=float(gamma),
            k=float(k), t_0=float(t_0), adapt_step_size=int(bool(adapt_step_size)), adapt_metric=int(bool(adapt_metric)),
            update_window=int(update_window), doubling=int(bool(doubling)), full_metric=int(self.full_metric),
            metric_mat=self.mat.data_ptr() if self.full_metric else None)

    def run(self, n_run, sampler='NUTS', n_warmup=500, max_treedepth=10, n_int_step=32, max_change=1000.,
            target_accept=0.8, gamma=0.05, k=0.75, t_0=10., adapt_step_size=True, adapt_metric=True,
            update_window=1, doubling=True, samples=None, stats=None, check=True, launch_iters='auto', layout='auto'):
        """Advance every chain by ``n_run`` iterations, in kernel launches of at most ``launch_iters`` iterations
        (None: one launch; a sequence: these lengths, the last one repeating; 'auto': launches of 100 while the chains adapt,
        then of 250 -- measured on the default 1500-iteration run of 4096 chains: 64.5 ms in launches of 250, 61.6 ms with the
        warm-up in launches of 100, 72.8 ms with the warm-up in one launch) queued back to back on the context's stream.

        The chains of a workgroup share the gradient tiles of every trip, so they run fastest in step; chains whose
        trees differ drift apart inside a launch and every launch boundary lines them up again (measured on the
        default 1500-iteration run: 83 ms in one launch, 75 ms in launches of 250).  The cut does not change any
        chain's results.

        ``layout`` chooses how a workgroup's 16 chains are laid out (``bfhip_sampler_config.chain_layout``): 'group' (lane
        per chain: fastest while the chains of a workgroup stay in step), 'split' (the same with integrator and bookkeeper
        waves), 'wave' (wave per chain: insensitive to chains out of step) or 'auto', decided per launch by ``layout.choose``
        (layout.py describes the rules) from the shapes and from whether the NUTS trees of an earlier launch's last 32
        iterations had one and the same size.  "Earlier" is the launch just before inside a run, and the one before that for
        the first launch of a run: a pure function of the sequence of launches, never of host timing.  With ``hist_reduce``
        set (``sample()`` does it when the chains are sharded over ranks) the trees of all ranks decide, so the choice does
        not depend on the sharding.
        The layouts follow the same per-chain arithmetic and random streams; their floating-point sums are ordered
        differently, so results are bit-reproducible (and independent of sharding and launch cuts) for a fixed layout,
        and agree to rounding between layouts.

        Returns (samples (n_chain, n_run, d), stats (n_chain, n_run, 11)) device tensors; the stats columns
        follow ``_lib.NSTATS`` / ``_lib.HSTATS`` (samplers/hmc_utils/stats.py:7-14)."""
        torch = _torch()
        self.density.upload_if_needed()
        cfg = self._sampler_config(sampler, n_warmup, max_treedepth, n_int_step, max_change, target_accept, gamma, k, t_0,
                                   adapt_step_size, adapt_metric, update_window, doubling)
        if layout not in ('auto', 'group', 'wave', 'split'):
            raise ValueError("layout should be 'auto', 'group', 'split' or 'wave'.")
        if layout == 'auto':   # (tuning: one layout for every launch the dispatch would have chosen; an explicit layout wins)
            layout = os.environ.get('BFHIP_FORCE_LAYOUT') or layout
            if layout not in ('auto', 'group', 'wave', 'split'):
                raise ValueError("BFHIP_FORCE_LAYOUT should be 'group', 'split' or 'wave'.")
        judged = layout == 'auto'
        if judged:   # the facts of layout.choose, once per run(): a refit or an option change since the last one is seen here
            if self._n_cu is None:
                self._n_cu = int(torch.cuda.get_device_properties(self.ctx.device).multi_processor_count)
            facts = _layout.shape_facts(self.density.spec, self.d, self.n_chain, self._n_cu, self.full_metric, self.n_chain_rule)
        n_run = int(n_run)
        if samples is None:
            samples = self.ctx.empty((self.n_chain, n_run, self.d))
        if stats is None:
            stats = self.ctx.empty((self.n_chain, n_run, _lib.STAT_STRIDE))
        # caller-supplied output buffers: the kernel writes n_chain * n_run rows with these strides, so anything else
        # would be a silent out-of-bounds or garbled write
        for name, t, shape in (('samples', samples, (self.n_chain, n_run, self.d)),
                               ('stats', stats, (self.n_chain, n_run, _lib.STAT_STRIDE))):
            if (tuple(t.shape) != shape or t.dtype != torch.float64 or t.device != self.ctx.device or
                    not t.is_contiguous()):
                raise ValueError('{} should be a contiguous float64 tensor of shape {} on {}.'.format(name, shape, self.ctx.device))
        for i_launch, (done, step) in enumerate(_launch_schedule(launch_iters, n_run, n_warmup, self.i_iter)):
            # output rows are relative to i_iter.  The layout is chosen per launch from the trees of an EARLIER launch, as a pure
            # function of the sequence of launches (never of host timing; layout.py): inside a run, the launch just before (the
            # host waits for its answer: it has nothing else to queue, and the gap is a launch latency); the first launch of a
            # run, the launch before the last one, so that runs issued back to back keep one launch queued behind the running one
            # and still follow the chains' behaviour, one launch late
            lay = layout
            if judged:   # (asked for at every launch: the answers are consumed in order)
                lay = _layout.choose(facts, sampler, self._trees_in_step(lag=1 if i_launch > 0 else 2), IN_STEP_LAYOUT)
            cfg.chain_layout = {'group': 1, 'wave': 2, 'split': 3}[lay]
            self.last_layout = lay
            _lib.check(self.ctx._lib.bfhip_sampler_run(
                self.ctx.handle, C.byref(cfg), self.n_chain, self.i_iter + min(done, n_run), _ptr(self.rng), _ptr(self.sc),
                _ptr(self.vec), self.i_iter, n_run, _ptr(samples), _ptr(stats), _ptr(self.n_leapfrog)))
            if judged:
                self._note_trees(stats, done - step, min(done, n_run), sampler,
                                 share=_judging_share(self.i_iter + done - step, self.i_iter + min(done, n_run), n_warmup))
            else:
                self._answers.append(None)   # (a launch that was not judged: no stale answer later)
                del self._answers[:-4]
        self.i_iter += n_run
        if check:
            self.raise_on_error()
        return samples, stats

    def run_tempered(self, n_run, base_mean, base_cov, logxi=0., u_0=None, n_warmup=500, max_treedepth=10, max_change=1000.,
                     target_accept=0.8, gamma=0.05, k=0.75, t_0=10., adapt_step_size=True, adapt_metric=True,
                     update_window=1, doubling=True, check=True):
        """TNUTS (samplers/tnuts.py; ``bfhip_tnuts_run``) with a Gaussian base density N(base_mean, base_cov) and
        ``logxi`` (``TNTrace(density_base=..., logxi=...)``, samplers/sample_trace.py:540-567).  ``u_0`` (n_chain,): the
        tempering coordinate at the start of a fresh run (default: standard normal draws, as the reference takes them
        from NumPy's global generator, base_hmc.py:241); later calls continue from the chains' own u.

        Returns (samples (n_chain, n_run, d), stats (n_chain, n_run, 11), stats_t (n_chain, n_run, 2) = u and weight)."""
        self.density.upload_if_needed()
        d = self.d
        mean = np.asarray(base_mean, dtype=np.float64).reshape(d)
        cov = np.asarray(base_cov, dtype=np.float64).reshape(d, d)
        prec = np.linalg.inv(cov)
        tp = _lib.Tempering()
        S = self.ctx.tensor(-prec)                     # log N = c0 + lin.x + x.S x / 2
        lin = self.ctx.tensor(prec @ mean)
        tp.base_S, tp.base_lin = S.data_ptr(), lin.data_ptr()
        tp.base_c0 = float(-0.5 * mean @ prec @ mean - 0.5 * (d * np.log(2 * np.pi) + np.linalg.slogdet(cov)[1]))
        tp.logxi = float(logxi)
        if self.tu is None:
            if u_0 is None:
                u_0 = np.random.normal(0, 1, size=self.n_chain)
            self.tu = self.ctx.tensor(np.asarray(u_0, dtype=np.float64).reshape(self.n_chain))
        cfg = self._sampler_config('NUTS', n_warmup, max_treedepth, 1, max_change, target_accept, gamma, k, t_0,
                                   adapt_step_size, adapt_metric, update_window, doubling)
        n_run = int(n_run)
        samples = self.ctx.empty((self.n_chain, n_run, d))
        stats = self.ctx.empty((self.n_chain, n_run, _lib.STAT_STRIDE))
        stats_t = self.ctx.empty((self.n_chain, n_run, 2))
        _lib.check(self.ctx._lib.bfhip_tnuts_run(
            self.ctx.handle, C.byref(cfg), C.byref(tp), self.n_chain, self.i_iter + n_run, _ptr(self.rng), _ptr(self.sc),
            _ptr(self.vec), _ptr(self.tu), self.i_iter, n_run, _ptr(samples), _ptr(stats), _ptr(stats_t), _ptr(self.n_leapfrog)))
        self.i_iter += n_run
        self._answers = []
        if check:
            self.raise_on_error()
        return samples, stats, stats_t

    # ``hist_reduce``: None, or a callable summing an int64 device tensor over the ranks in place (``parallel.all_reduce_sum``;
    # ``sample()`` sets it when the chains are sharded).  With it the 'auto' layout is decided from the tree sizes of ALL
    # ranks' chains -- a collective per launch, the same launches on every rank -- so that every rank picks the same
    # layout and results do not depend on the number of ranks.  Without it each DeviceChains decides from its own chains.
    hist_reduce = None
    n_chain_rule = None   # set by sample() under torch.distributed: chains per rank on average (``layout.shape_facts``)

    def _note_trees(self, stats, row0, row1, sampler, n_last=32, share=0.98):
        """Queue, behind the launch that wrote rows [row0, row1) of ``stats``, the answer to "did the chains run in step?":
        at least ``share`` of the NUTS trees of its last ``n_last`` iterations (all chains) had the most common size
        (``bfhip_tree_size_mode_share``: one small kernel).  The flag travels to a slot of a small pinned ring
        asynchronously; nothing here synchronises (except with ``hist_reduce``, which is a collective)."""
        torch = _torch()
        if sampler != 'NUTS' or row1 <= row0:
            self._answers.append(None)
            return
        r0 = max(row0, row1 - n_last)
        if self.hist_reduce is not None:
            with torch.cuda.stream(self.ctx.stream):
                ts = stats[:, r0:row1, _lib.NSTATS.index('tree_size')].reshape(-1)
                # (binned as bf_tree_mode_kernel bins them: negative and NaN sizes go to bucket 4095)
                ts = torch.where((ts >= 0.) & (ts < 4095.), ts, torch.full_like(ts, 4095.)).to(torch.int64)
                hist = torch.zeros(4096 + 64, dtype=torch.int64, device=self.ctx.device)
                hist.scatter_add_(0, ts, torch.ones_like(ts))
                # (the chains by the size class of their leapfrogs in the window, as bf_tree_mode_kernel counts them)
                edges = torch.tensor(_lib.LAG_EDGES, dtype=torch.int64, device=self.ctx.device)
                cls = (torch.searchsorted(edges, ts.view(self.n_chain, -1).sum(1), right=True) - 1).clamp_(0, 63)
                hist.scatter_add_(0, 4096 + cls, torch.ones_like(cls))
            self.ctx.stream.synchronize()
            self.hist_reduce(hist)
            h = [int(v) for v in hist.cpu()]
            self._answers.append(_layout.answer_from_histograms(h[:4096], h[4096:], share))   # (as bf_tree_mode_kernel decides)
            del self._answers[:-4]
            return
        if self._step_host is None:
            self._step_host = torch.zeros(8, dtype=torch.int32, pin_memory=True)
            self._step_dev = torch.zeros(_lib.TREE_MODE_WORK, dtype=torch.int32, device=self.ctx.device)
        _lib.check(self.ctx._lib.bfhip_tree_size_mode_share(self.ctx.handle, self.n_chain, stats.shape[1], _ptr(stats), r0,
                                                            row1 - r0, float(share), _ptr(self._step_dev)))
        slot = self._n_flag % 8
        self._n_flag += 1
        with torch.cuda.stream(self.ctx.stream):
            self._step_host[slot:slot + 1].copy_(self._step_dev[:1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.ctx.stream)
        self._answers.append((ev, slot))
        del self._answers[:-4]  # (at most the last two are ever read: the ring's 8 slots stay unambiguous)

    def _trees_in_step(self, lag=1):
        """The answer of ``_note_trees`` for the launch ``lag`` launches back (1 = the last one) -- the common tree size when the
        chains ran in step (+ 4096 when some chain builds far larger trees than the rest), else 0 --, waited for if it is still on its way; 0 when there is none (the first launches of a chain set, launches that were not NUTS).  A pure
        function of the launches so far: an answer that happens to have arrived early is not used before its turn."""
        ans = self._answers
        if len(ans) < lag:
            return 0
        a = ans[-lag]
        if isinstance(a, tuple):
            ev, slot = a
            ev.synchronize()
            a = ans[-lag] = int(self._step_host[slot])
        return int(a or 0)

    def raise_on_error(self):
        """Synchronises; raises like the reference does for a chain that hit a fatal condition."""
        err = self.sc[:, _lib.SC_FIELDS.index('error')]
        bad = (err != 0).nonzero()
        if bad.numel():
            i = int(bad[0, 0])
            code = int(err[i])
            if code == 3:  # metrics.py:107-108
                raise ValueError('the input covariance is not positive definite.')
            if code == 1:  # base_hmc.py:72-76
                raise RuntimeError('Bad initial energy for chain #{}, please check the Hamiltonian.'.format(i))
            raise FloatingPointError("logp can't be nan (chain #{}).".format(i))  # nuts.py:201-202

    def covariance(self):
        """Per-chain metric covariance (n_chain, d, d): QuadMetricFull._cov, or diag(var) for the diagonal metric."""
        torch = _torch()
        if self.full_metric:
            return self.mat[:, 0].transpose(1, 2).contiguous()
        return torch.diag_embed(self.field('var'))

    def field(self, name):
        """One per-chain quantity by its reference name (device tensor view)."""
        if name in _lib.SC_FIELDS:
            return self.sc[:, _lib.SC_FIELDS.index(name)]
        return self.vec[:, _lib.VEC_FIELDS.index(name)]

    @property
    def total_leapfrog(self):
        return int(self.n_leapfrog.item())
