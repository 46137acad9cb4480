"""Did the sampler itself work -- the three warnings a NUTS / HMC user expects after a run (divergent transitions, transitions that
hit the maximum tree depth, low E-BFMI), per chain and in total, and which chains are the bad ones.

R-hat says that chains disagree; it cannot say that 3 % of the transitions diverged in a funnel's neck or that one chain of 4096
never moved.  ``sampler_health`` reads the sampler's statistics table (n_chain, n, 11) where ``sample()`` left it: a GPU tensor goes
through ``bfhip_health_chains`` (one workgroup per chain, the rows read in place, a ``[:, since:]`` view included) and, with the
draws, ``bfhip_acor_moments`` for every chain's mean and variance per parameter; a NumPy array or CPU tensor takes the host port
below with the same definitions.  Only the per-chain tables (20 integers and 7 + 2 d doubles per chain) reach the host; the draws
and the statistics are never copied.

Definitions (per chain, over the selected rows):
  n_divergent       rows with ``diverging != 0``
  n_max_treedepth   NUTS rows with ``tree_depth >= max_treedepth``
  n_leapfrog        sum of ``tree_size`` (HMC: of ``n_int_step``); max_tree_size the largest
  n_accepted        HMC rows with ``accepted != 0``
  n_nonfinite       rows whose logp or energy is not finite
  n_moved           rows whose logp differs from the previous row's (0: the chain never moved)
  depth_hist        counts of ``tree_depth`` 0 .. 12 (anything outside in the last bin)
  mean_accept       mean of ``mean_tree_accept`` (HMC: ``accept_stat``)
  logp_mean, logp_var, energy_mean, energy_var   unbiased variances, two passes
  bfmi              sum_{i >= 1} (E_i - E_{i-1})^2 / sum_i (E_i - mean E)^2: Betancourt's E-BFMI in the form Stan uses
  step_size         that of the last selected row
A chain with a non-finite logp or energy has NaN in its moments and bfmi and is ``errored``; a constant energy gives bfmi NaN."""
import warnings as _warnings
from collections import namedtuple

import numpy as np

from .. import _lib
from ._pipeline_data import host_f64

__all__ = ['sampler_health', 'sampler_health_sharded', 'divergent_summary', 'SamplerHealth', 'DivergentSummary']

MIN_CHAINS_FOR_Z = 8   # fewer chains: no robust scores among them
_N_HIST = _lib.MAX_TREEDEPTH + 1
_I0 = len(_lib.HEALTH_I)

DivergentSummary = namedtuple('DivergentSummary', ['summary', 'shift', 'n_divergent'])
DivergentSummary.__doc__ = ('Where the divergences are: ``summary`` the ``weighted_summary`` table of the divergent draws alone, ``shift`` (d,) = '
                            '(mean of the divergent draws - mean of all draws) / sd of all draws, ``n_divergent`` their number.')


def _sampler_id(sampler):
    s = str(sampler).upper()
    if s in ('NUTS', 'TNUTS'):
        return 0
    if s == 'HMC':
        return 1
    raise ValueError('sampler should be NUTS, TNUTS or HMC.')


def _check(stats, samples, max_treedepth):
    if stats.ndim != 3 or stats.shape[2] != _lib.STAT_STRIDE:
        raise ValueError('stats should be (n_chain, n, {}).'.format(_lib.STAT_STRIDE))
    if stats.shape[1] < 2:
        raise ValueError('at least two rows per chain are needed.')
    if samples is not None and (samples.ndim != 3 or tuple(samples.shape[:2]) != tuple(stats.shape[:2]) or samples.shape[2] < 1):
        raise ValueError('samples should be (n_chain, n, d) with the chains and rows of stats.')
    if not 1 <= int(max_treedepth) <= _lib.MAX_TREEDEPTH:
        raise ValueError('max_treedepth should be between 1 and {}.'.format(_lib.MAX_TREEDEPTH))


# ---- the per-chain tables: host port -------------------------------------------------------------------------------------------------
def _host_tables(stats, samples, sid, max_treedepth):
    """(itab (C, HEALTH_I_N) int64, ftab (C, HEALTH_F_N + 2 d) float64: the kernel's table, then chain_mean and chain_var).  Every
    column is made contiguous (C, n) first, so that a chain's sums have an order set by n alone, whichever chains are beside it."""
    st = host_f64(stats)
    n_c, n = st.shape[:2]
    items = _lib.HSTATS if sid else _lib.NSTATS

    def col(name):
        return np.ascontiguousarray(st[:, :, items.index(name)])

    itab = np.zeros((n_c, _lib.HEALTH_I_N), dtype=np.int64)
    ftab = np.empty((n_c, _lib.HEALTH_F_N))
    with np.errstate(all='ignore'):
        lp, en = col('logp'), col('energy')
        size = col('n_int_step' if sid else 'tree_size')
        size = np.where((size > 0) & (size < 2.**52), np.floor(size), 0.)
        itab[:, 0] = (col('diverging') != 0).sum(axis=1)
        itab[:, 2] = size.sum(axis=1).astype(np.int64)
        itab[:, 3] = size.max(axis=1).astype(np.int64) if n_c else 0
        bad = (~(np.isfinite(lp) & np.isfinite(en))).sum(axis=1)
        itab[:, 5] = bad
        itab[:, 6] = (lp[:, 1:] != lp[:, :-1]).sum(axis=1)
        if sid:
            itab[:, 4] = (col('accepted') != 0).sum(axis=1)
        else:
            dp = col('tree_depth')
            itab[:, 1] = (dp >= max_treedepth).sum(axis=1)
            for b in range(_N_HIST - 1):
                itab[:, _I0 + b] = ((dp >= b) & (dp < b + 1)).sum(axis=1)
            itab[:, _I0 + _N_HIST - 1] = n - itab[:, _I0:_I0 + _N_HIST - 1].sum(axis=1)
        ftab[:, 0] = col('accept_stat' if sid else 'mean_tree_accept').sum(axis=1) / n
        for j, v in ((1, lp), (3, en)):
            m = v.sum(axis=1) / n
            ss = ((v - m[:, None])**2).sum(axis=1)
            ftab[:, j], ftab[:, j + 1] = m, ss / (n - 1.)
            if j == 3:
                de = (np.diff(v, axis=1)**2).sum(axis=1)
                ftab[:, 5] = np.where(de == 0, np.nan, de / ss)   # a constant energy: the 0 / 0 it stands for
        ftab[bad > 0, 1:6] = np.nan
        ftab[:, 6] = st[:, -1, items.index('step_size')]
        if samples is not None:
            x = host_f64(samples)
            mean = x.sum(axis=1) / n
            var = ((x - mean[:, None, :])**2).sum(axis=1) / (n - 1.)
            ftab = np.concatenate([ftab, mean, var], axis=1)
    return itab, ftab


# ---- the per-chain tables: device route ----------------------------------------------------------------------------------------------
def _device_chain_moments(ctx, x):
    """(mean, sum (x - mean)^2) per chain and parameter, (n_chain, d) device tensors, of the device draws x (n_chain, n, d) read in
    place: ``bfhip_acor_moments``, two passes."""
    import torch
    from ..device import _ptr
    n_c, n, d = (int(v) for v in x.shape)
    if x.dtype != torch.float64 or x.stride(2) != 1 or x.stride(1) != d or (n_c > 1 and x.stride(0) < n * d):
        x = x.to(torch.float64).contiguous()
    mean, inv = ctx.empty((n_c, d)), ctx.empty((n_c, d))
    _lib.check(ctx._lib.bfhip_acor_moments(ctx.handle, n_c, n, d, int(x.stride(0)) if n_c > 1 else n * d, _ptr(x), _ptr(mean), _ptr(inv)))
    return mean, 1. / inv   # inv = 1 / sum (x - mean)^2; a constant series: 1 / inf = 0


def _device_tables(stats, samples, sid, max_treedepth):
    """As ``_host_tables``, device tensors: ``bfhip_health_chains`` on the table, ``bfhip_acor_moments`` on the draws."""
    import torch
    from ..device import get_context, _ptr
    n_c, n = int(stats.shape[0]), int(stats.shape[1])
    with torch.cuda.device(stats.device):
        ctx = get_context(stats.device.index)
        itab = ctx.empty((n_c, _lib.HEALTH_I_N), dtype=torch.int64)
        ftab = ctx.empty((n_c, _lib.HEALTH_F_N))
        if n_c == 0:
            d = 0 if samples is None else int(samples.shape[2])
            return itab, ctx.empty((0, _lib.HEALTH_F_N + 2 * d))
        width = _lib.STAT_STRIDE
        if stats.dtype != torch.float64 or stats.stride(2) != 1 or stats.stride(1) != width or (n_c > 1 and stats.stride(0) < n * width):
            stats = stats.to(torch.float64).contiguous()
        ldc = int(stats.stride(0)) if n_c > 1 else n * width
        _lib.check(ctx._lib.bfhip_health_chains(ctx.handle, n_c, n, ldc, _ptr(stats), sid, int(max_treedepth), _ptr(itab), _ptr(ftab)))
        if samples is None:
            return itab, ftab
        if samples.device != stats.device:
            raise ValueError('stats and samples should be on one device.')
        mean, ss = _device_chain_moments(ctx, samples)
        return itab, torch.cat([ftab, mean, ss / (n - 1.)], dim=1)


def _local_tables(stats, samples, sid, max_treedepth):
    """This process's chains: (itab, ftab) as torch tensors where the inputs live."""
    import torch
    if getattr(stats, 'is_cuda', False):
        return _device_tables(stats, samples, sid, max_treedepth)
    itab, ftab = _host_tables(stats, samples, sid, max_treedepth)
    return torch.as_tensor(itab), torch.as_tensor(ftab)


# ---- the result ----------------------------------------------------------------------------------------------------------------------
def _robust_z(v):
    """(v - median) / (1.4826 MAD) along the chains (axis 0), NaN entries passed over."""
    with _warnings.catch_warnings(), np.errstate(all='ignore'):
        _warnings.simplefilter('ignore')
        med = np.nanmedian(v, axis=0)
        mad = np.nanmedian(np.abs(v - med), axis=0)
        return (v - med) / (1.4826 * mad)


def _first(mask, k=5):
    idx = np.flatnonzero(mask)
    return ', '.join(str(i) for i in idx[:k]) + (', ...' if idx.size > k else '')


class SamplerHealth:
    """The result of ``sampler_health``.  Per chain (n_chain,): ``n_divergent``, ``n_max_treedepth``, ``n_leapfrog``, ``max_tree_size``,
    ``n_accepted``, ``n_nonfinite``, ``n_moved`` (int64), ``depth_hist_chain`` (n_chain, 13), ``mean_accept``, ``logp_mean``, ``logp_var``,
    ``energy_mean``, ``energy_var``, ``bfmi``, ``step_size``; with draws ``chain_mean``, ``chain_var``, ``chain_z``, ``var_ratio``
    (n_chain, d), else None; ``logp_z`` (n_chain,).  Over all chains: ``n_rows`` (per chain), ``n_transitions``,
    ``n_divergent_total``, ``share_divergent``, ``n_max_treedepth_total``, ``share_max_treedepth``, ``depth_hist`` (13,),
    ``n_leapfrog_total``, ``bfmi_min``, ``bfmi_median``.  Boolean masks (n_chain,): ``divergent``, ``saturated``, ``low_bfmi``,
    ``stuck``, ``errored`` and their union ``flagged``; ``ok`` is True when no chain is flagged.  ``thresholds`` holds the three
    conventions the masks were drawn with."""

    def __init__(self, itab, ftab, n_rows, sampler, max_treedepth, bfmi_min, z_max, var_ratio_min):
        itab, ftab = np.asarray(itab, dtype=np.int64), np.asarray(ftab, dtype=np.float64)
        n_c = itab.shape[0]
        self.n_chain, self.n_rows, self.sampler, self.max_treedepth = n_c, int(n_rows), sampler, int(max_treedepth)
        self.thresholds = dict(bfmi_min=float(bfmi_min), z_max=float(z_max), var_ratio_min=float(var_ratio_min))
        for j, k in enumerate(_lib.HEALTH_I):
            setattr(self, k, itab[:, j].copy())
        self.depth_hist_chain = itab[:, _I0:_I0 + _N_HIST].copy()
        for j, k in enumerate(_lib.HEALTH_F):
            setattr(self, k, ftab[:, j].copy())
        d = (ftab.shape[1] - _lib.HEALTH_F_N) // 2
        self.chain_mean = ftab[:, _lib.HEALTH_F_N:_lib.HEALTH_F_N + d].copy() if d else None
        self.chain_var = ftab[:, _lib.HEALTH_F_N + d:].copy() if d else None
        # totals
        self.n_transitions = n_c * self.n_rows
        self.n_divergent_total = int(self.n_divergent.sum())
        self.n_max_treedepth_total = int(self.n_max_treedepth.sum())
        self.share_divergent = self.n_divergent_total / self.n_transitions if self.n_transitions else float('nan')
        self.share_max_treedepth = self.n_max_treedepth_total / self.n_transitions if self.n_transitions else float('nan')
        self.depth_hist = self.depth_hist_chain.sum(axis=0)
        self.n_leapfrog_total = int(self.n_leapfrog.sum())
        with _warnings.catch_warnings(), np.errstate(all='ignore'):
            _warnings.simplefilter('ignore')
            self.bfmi_min = float(np.nanmin(self.bfmi)) if n_c else float('nan')
            self.bfmi_median = float(np.nanmedian(self.bfmi)) if n_c else float('nan')
            # the scores among the chains
            scored = n_c >= MIN_CHAINS_FOR_Z
            self.logp_z = _robust_z(self.logp_mean) if scored else np.full(n_c, np.nan)
            stuck = self.n_moved == 0   # a constant chain, exactly (a variance of n copies of a value need not come out as 0)
            self.chain_z = self.var_ratio = None
            if d:
                self.chain_z = _robust_z(self.chain_mean) if scored else np.full((n_c, d), np.nan)
                self.var_ratio = self.chain_var / np.nanmedian(self.chain_var, axis=0)
                if scored:
                    stuck |= (np.abs(self.chain_z) > z_max).any(axis=1) | (self.var_ratio < var_ratio_min).any(axis=1)
            if scored:
                stuck |= self.logp_z < -z_max
            self.divergent = self.n_divergent > 0
            self.saturated = self.n_max_treedepth > 0
            self.low_bfmi = self.bfmi < bfmi_min
            self.stuck = stuck
            self.errored = self.n_nonfinite > 0
        self.flagged = self.divergent | self.saturated | self.low_bfmi | self.stuck | self.errored
        self.ok = not bool(self.flagged.any())
        self._stats = self._selection = None

    def warnings(self):
        """Plain sentences, one per kind of trouble found (an empty list when ``ok``), with counts and the first few chains."""
        out, n_c, n_tr = [], self.n_chain, self.n_transitions
        if self.divergent.any():
            out.append('{} of {} ({:.2%}) transitions ended with a divergence, in {} of {} chains (chains {}). Divergences mean the '
                       'sampler could not follow the posterior there and its estimates may be biased: raise target_accept or '
                       'reparametrise.'.format(self.n_divergent_total, n_tr, self.share_divergent, int(self.divergent.sum()), n_c,
                                               _first(self.divergent)))
        if self.saturated.any():
            out.append('{} of {} ({:.2%}) transitions hit the maximum tree depth limit of {}, in {} of {} chains (chains {}). This costs '
                       'efficiency, not validity: raise max_treedepth or improve the metric.'
                       .format(self.n_max_treedepth_total, n_tr, self.share_max_treedepth, self.max_treedepth, int(self.saturated.sum()), n_c,
                               _first(self.saturated)))
        if self.low_bfmi.any():
            out.append('E-BFMI is below {:g} in {} of {} chains (chains {}; lowest {:.3g}): the momentum resampling explores the energy '
                       'levels poorly, as with heavy tails. Reparametrise.'
                       .format(self.thresholds['bfmi_min'], int(self.low_bfmi.sum()), n_c, _first(self.low_bfmi), self.bfmi_min))
        if self.stuck.any():
            out.append('{} of {} chains look stuck or sit far from the others (chains {}): a constant chain, a chain mean more than {:g} '
                       'robust standard deviations from the median chain, or a chain variance below {:g} of the median chain\'s.'
                       .format(int(self.stuck.sum()), n_c, _first(self.stuck), self.thresholds['z_max'], self.thresholds['var_ratio_min']))
        if self.errored.any():
            out.append('{} of {} chains hold a logp or an energy that is not finite (chains {}).'
                       .format(int(self.errored.sum()), n_c, _first(self.errored)))
        return out

    def where(self, tt_or_x, probs=(0.05, 0.5, 0.95)):
        """Where the divergences are (``divergent_summary``): ``tt_or_x`` is the ``TraceTuple`` whose ``health()`` this is (the same
        selection is applied to its draws) or the draws (n_chain, n, d) that go with the statistics this was built from.  None
        when no draw diverged."""
        if self.n_divergent_total == 0:
            return None
        if self._stats is None:
            raise ValueError('this SamplerHealth does not carry its statistics table.')
        x = tt_or_x
        if hasattr(x, '_view') and hasattr(x, '_single_process'):
            x._single_process('the divergent draws are weighted among the draws of ALL chains, and this TraceTuple holds one rank\'s: '
                              'gather the chains and use the host port, utils.divergent_summary.')
            since, original = self._selection if self._selection is not None else (None, True)
            x = x._view(since, False, original)
        return divergent_summary(x, self._stats, self.sampler, probs)

    def __str__(self):
        rows = ['SamplerHealth: {} chains x {} transitions ({})'.format(self.n_chain, self.n_rows, self.sampler),
                '  divergent          {:>12d}  ({:.3%})  in {} chains'.format(self.n_divergent_total, self.share_divergent, int(self.divergent.sum())),
                '  max tree depth {:>2d}  {:>12d}  ({:.3%})  in {} chains'.format(self.max_treedepth, self.n_max_treedepth_total,
                                                                                self.share_max_treedepth, int(self.saturated.sum())),
                '  E-BFMI             min {:.3g}, median {:.3g}; below {:g} in {} chains'.format(self.bfmi_min, self.bfmi_median,
                                                                                                self.thresholds['bfmi_min'], int(self.low_bfmi.sum())),
                '  leapfrog steps     {:>12d}  (largest tree {})'.format(self.n_leapfrog_total, int(self.max_tree_size.max()) if self.n_chain else 0),
                '  stuck {} chains, errored {} chains, flagged {} of {}'.format(int(self.stuck.sum()), int(self.errored.sum()),
                                                                               int(self.flagged.sum()), self.n_chain)]
        return '\n'.join(rows)

    __repr__ = __str__


# ---- the public functions ------------------------------------------------------------------------------------------------------------
def _gather(t, n_chain):
    import torch.distributed as dist
    from .. import parallel
    if dist.get_backend() == 'gloo' and t.is_cuda:   # (plumbing tests: gloo moves host tensors)
        t = t.cpu()
    return parallel.all_gather_chains(t.contiguous(), n_chain)


def sampler_health_sharded(stats_local, samples_local=None, n_chain=None, sampler='NUTS', max_treedepth=10, bfmi_min=0.3, z_max=8.,
                           var_ratio_min=0.1, stats=None):
    """``sampler_health`` of all ``n_chain`` chains when this rank holds ``stats_local`` (n_loc, n, 11) and ``samples_local``
    (n_loc, n, d), its own chains in ``parallel.shard_range`` order; with more than one rank a collective that every rank calls.
    Every rank runs the per-chain pass on its shard; the two per-chain tables (one float64 with ``chain_mean`` and ``chain_var``,
    one int64) cross once each through ``parallel.all_gather_chains``, and every rank returns the ``SamplerHealth`` of all chains,
    bit for bit that of one process (a chain's figures do not depend on the chains beside it).  The draws and the statistics never
    cross.  ``stats``, if a dict, receives 'collectives' (2 with more than one rank, whatever d and n are) and 'wire_bytes'."""
    return _build(stats_local, samples_local, n_chain, sampler, max_treedepth, bfmi_min, z_max, var_ratio_min, stats, True)


def _build(stats_local, samples_local, n_chain, sampler, max_treedepth, bfmi_min, z_max, var_ratio_min, stats, collective):
    from .. import parallel
    sid = _sampler_id(sampler)
    _check(stats_local, samples_local, max_treedepth)
    itab, ftab = _local_tables(stats_local, samples_local, sid, max_treedepth)
    n_coll = wire = 0
    if collective and parallel.world()[1] > 1:
        if n_chain is None:
            raise ValueError('n_chain, the number of chains of all ranks, is needed.')
        wire = itab.numel() * 8 + ftab.numel() * 8
        ftab, itab = _gather(ftab, int(n_chain)), _gather(itab, int(n_chain))
        n_coll = 2
    if stats is not None:
        stats.update(collectives=n_coll, wire_bytes=wire)
    h = SamplerHealth(itab.cpu().numpy(), ftab.cpu().numpy(), stats_local.shape[1], 'HMC' if sid else 'NUTS', max_treedepth, bfmi_min,
                      z_max, var_ratio_min)
    h._stats = stats_local
    return h


def sampler_health(stats, samples=None, sampler='NUTS', max_treedepth=10, bfmi_min=0.3, z_max=8., var_ratio_min=0.1):
    """The health of a sampler run: ``stats`` (n_chain, n, 11), the sampler's statistics table in the layout of ``sampler`` ('NUTS',
    'TNUTS' -- read as NUTS -- or 'HMC'), and optionally the draws ``samples`` (n_chain, n, d) -> a ``SamplerHealth``.  GPU tensors
    take the device route (a ``[:, since:]`` view of either goes in without a copy); NumPy arrays and CPU tensors take the host port
    with the same definitions (see the module's docstring).

    The masks: ``divergent`` n_divergent > 0; ``saturated`` n_max_treedepth > 0; ``low_bfmi`` bfmi < ``bfmi_min``; ``errored``
    n_nonfinite > 0; ``stuck`` a constant chain (n_moved == 0: its logp never changed), or max_j |chain_z| > ``z_max``, or
    min_j var_ratio < ``var_ratio_min``, or logp_z < -``z_max``, where chain_z and logp_z are the robust scores
    (value - median over the chains) / (1.4826 MAD over the chains) of the chain's mean of each parameter and of its mean logp,
    and var_ratio = chain_var / median over the chains of chain_var.  With fewer than 8 chains there is nothing to score a chain
    against: chain_z and logp_z are NaN and ``stuck`` uses the constant-chain test alone.  Without ``samples`` only the logp terms
    are used.

    The three thresholds are conventions, not measurements: 0.3 is the E-BFMI below which Stan warns; 8 robust standard
    deviations is far outside what 4096 x 128 Gaussian chain means reach; 0.1 is a chain whose variance is a tenth of the typical
    chain's.  This call is never a collective: it looks at the chains it is given (``TraceTuple.health`` /
    ``sampler_health_sharded`` are the collective forms)."""
    return _build(stats, samples, None, sampler, max_treedepth, bfmi_min, z_max, var_ratio_min, None, False)


def _pooled_moments(x):
    """(mean (d,), sd (d,)) of all draws of x (n_chain, n, d) from the chains' two-pass moments: the device route through
    ``bfhip_acor_moments``, read in place."""
    n_c, n, d = (int(v) for v in x.shape)
    if getattr(x, 'is_cuda', False):
        import torch
        from ..device import get_context
        with torch.cuda.device(x.device):
            m, ss = (t.cpu().numpy() for t in _device_chain_moments(get_context(x.device.index), x))
    else:
        xh = host_f64(x)
        m = xh.sum(axis=1) / n
        ss = ((xh - m[:, None, :])**2).sum(axis=1)
    with np.errstate(all='ignore'):
        mean_all = m.sum(axis=0) / n_c
        total = ss.sum(axis=0) + n * ((m - mean_all)**2).sum(axis=0)
        return mean_all, np.sqrt(total / (n_c * n - 1.))


def divergent_summary(x, stats, sampler='NUTS', probs=(0.05, 0.5, 0.95)):
    """Where the divergences are: the ``weighted_summary`` of the draws ``x`` (n_chain, n, d) with weight 1 on the rows that
    ``stats`` (n_chain, n, 11) flags ``diverging`` and 0 elsewhere (rows of zero weight are not part of the sample; the draws are
    read in place), and per parameter ``shift`` = (mean of the divergent draws - mean of all draws) / sd of all draws -> a
    ``DivergentSummary``; None when no draw diverged.  Single process."""
    from .psis import weighted_summary
    if x.ndim != 3 or stats.ndim != 3 or tuple(x.shape[:2]) != tuple(stats.shape[:2]):
        raise ValueError('x should be (n_chain, n, d) with the chains and rows of stats.')
    col = (_lib.HSTATS if _sampler_id(sampler) else _lib.NSTATS).index('diverging')
    if getattr(stats, 'is_cuda', False):
        import torch
        w = (stats[:, :, col] != 0).to(torch.float64)
        n_div = int(w.sum().item())
        if not getattr(x, 'is_cuda', False):
            w = w.cpu().numpy()
    else:
        w = (host_f64(stats)[:, :, col] != 0).astype(np.float64)
        n_div = int(w.sum())
    if n_div == 0:
        return None
    table = weighted_summary(x, weights=w, probs=probs)
    mean_all, sd_all = _pooled_moments(x)
    with np.errstate(all='ignore'):
        shift = (table['mean'] - mean_all) / sd_all
    return DivergentSummary(table, shift, n_div)
