"""What the utilities that read a ``Chi2PipelineDensity`` and a GPU tensor of draws share (predictive.py, data_loo.py, reweight.py,
data_lgo.py): the entry checks, one by one, so that every caller keeps its own order; the surrogate's input map on the device; the
base log weights; the driver of the first two PSIS-LOO stages (csrc/bfhip_ploo.h) under the three finishes; and a few host helpers."""
import numpy as np


# ---- the entry checks ------------------------------------------------------------------------------------------------------------------
def check_one_process(who):
    from .. import parallel
    if parallel.world()[1] > 1:
        raise NotImplementedError('%s covers one process: gather() the chains first.' % who)


def check_gpu_draws(who, x):
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise NotImplementedError('%s reads a GPU tensor of draws: the package has no host evaluation of a PolyModel.' % who)


def check_density(density):
    if not (hasattr(density, 'surrogate') and hasattr(density, '_y')):
        raise ValueError('density should be a Chi2PipelineDensity.')


def shaped_draws(x, d):
    """x (n_chain, n_draw, d), or (n, d) taken as one chain -> the (n_chain, n_draw, d) tensor the kernels read in place: x itself
    where it is float64 or float32 with unit stride in its last dimension, else one float64 copy.  Nothing is allocated before the
    shape is known to be right."""
    import torch
    x = x.detach()
    if x.dim() == 2:
        x = x[None]
    d = int(d)
    if x.dim() != 3 or int(x.shape[2]) != d:
        raise ValueError('x should be (n_chain, n_draw, %d) or (n, %d).' % (d, d))
    n = int(x.shape[0]) * int(x.shape[1])
    if n < 1:
        raise ValueError('x is empty.')
    if n > 2**31 - 1:
        raise NotImplementedError('more than 2^31 - 1 draws.')
    if x.dtype not in (torch.float64, torch.float32) or (d > 1 and x.stride(2) != 1):
        x = x.to(torch.float64).contiguous()
    return x


# ---- on the device -------------------------------------------------------------------------------------------------------------------------
def input_map(ctx, su):
    """The surrogate's input map as device tensors (lo, diff); (None, None) without one."""
    import torch
    if su._input_scales is None:
        return None, None
    return (ctx.tensor(np.ascontiguousarray(su._input_scales[:, 0]), torch.float64),
            ctx.tensor(np.ascontiguousarray(su._input_scales_diff), torch.float64))


def base_log_weights(log_weights, like, n, keep_neginf=False):
    """One log weight per draw -> g - logsumexp(g), float64, flat, where ``like`` lives; None without weights.  Where no row has any
    weight the logsumexp is -inf and every row turns NaN; ``keep_neginf`` leaves a row of -inf at -inf (not part of the sample)
    rather than turning it into -inf - -inf."""
    import torch
    if log_weights is None:
        return None
    g = log_weights if isinstance(log_weights, torch.Tensor) else torch.as_tensor(np.asarray(log_weights))
    g = g.detach().to(like.device).reshape(-1).to(torch.float64)
    if g.numel() != n:
        raise ValueError('log_weights should hold one value per draw.')
    b = g - torch.logsumexp(g, 0)
    return (torch.where(torch.isneginf(g), g, b) if keep_neginf else b).contiguous()


class PsisStages:
    """The first two PSIS-LOO stages on one (n, 16) series buffer after another, for n draws under the normalised base log weights
    ``lb`` (None: equal weights).  ``front`` queues them for a batch and hands back what the batch's finish needs; a subclass adds
    the finish and keeps its per-batch blocks; ``collect`` makes the one copy of such a list of blocks to the host."""

    def __init__(self, ctx, n, lb):
        import torch
        from .. import _lib
        from .psis import tail_size
        self.ctx, self.n, self.lb, self._lib = ctx, int(n), lb, _lib
        m1 = tail_size(self.n) + 1
        self.work = ctx.empty((int(ctx._lib.bfhip_ploo_work_bytes(self.n)),), dtype=torch.uint8)
        self.keys = ctx.empty((_lib.DIAG_BATCH, m1), dtype=torch.int64)
        self.idx = ctx.empty((_lib.DIAG_BATCH, m1), dtype=torch.int32)
        self.widths = []

    def front(self, buf, ld, nb, mode, c=None):
        """``bfhip_ploo_moments`` and ``bfhip_ploo_tail`` on the batch's nb columns of ``buf`` -> (out, head, tail): the batch's
        (PLOO_NOUT, 16) block and the leading and trailing arguments that the finish shares with them."""
        from ..device import _ptr
        lib, chk = self.ctx._lib, self._lib.check
        out = self.ctx.empty((self._lib.PLOO_NOUT, self._lib.DIAG_BATCH))
        head = (self.ctx.handle, self.n, _ptr(buf), int(ld), int(nb), int(mode), _ptr(c), _ptr(self.lb))
        tail = (_ptr(self.work), self.work.numel())
        chk(lib.bfhip_ploo_moments(*head, _ptr(out), *tail))
        chk(lib.bfhip_ploo_tail(*head, _ptr(out), _ptr(self.keys), _ptr(self.idx), *tail))
        self.widths.append(int(nb))
        return out, head, tail

    def collect(self, blocks, rows):
        """Per-batch (rows, 16) device blocks -> (rows, sum of the widths) on the host: one copy, after the last launch."""
        import torch
        if not blocks:
            return np.zeros((rows, 0))
        o = torch.stack(blocks).cpu().numpy()
        return np.concatenate([o[i][:, :nb] for i, nb in enumerate(self.widths)], axis=1)


# ---- on the host ---------------------------------------------------------------------------------------------------------------------------
def host_f64(v):
    """An array, a sequence or a CPU tensor as a float64 NumPy array."""
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, dtype=np.float64)


def logsumexp_host(a):
    top = a.max()
    return top + np.log(np.exp(a - top).sum())


def sum_and_se(v):
    """(sum, sqrt(k var(ddof = 1))) of the k values of v; the standard error is NaN for k = 1."""
    k = v.size
    with np.errstate(all='ignore'):
        return float(v.sum()), (float(np.sqrt(k * v.var(ddof=1))) if k > 1 else float('nan'))


def dense_precision(prec=None, prec_diag=None):
    """``prec``, or ``diag(prec_diag)``, as a square float64 matrix with a positive diagonal; anything else: ValueError."""
    if (prec is None) == (prec_diag is None):
        raise ValueError('give me exactly one of prec and prec_diag.')
    p = np.asarray(prec, dtype=np.float64) if prec is not None else np.diag(np.asarray(prec_diag, dtype=np.float64).reshape(-1))
    if p.ndim != 2 or p.shape[0] != p.shape[1] or not np.all(np.diag(p) > 0):
        raise ValueError('the precision should be a square matrix with a positive diagonal.')
    return p
