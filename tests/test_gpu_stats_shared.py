"""What the shared code of the statistics kernels makes checkable: the two sort entry points (``bfhip_sort_keys`` on a flat array,
``bfhip_diag_sort`` on a column of a 16-wide buffer) are one radix sort and must agree with each other and with NumPy's stable
sort; the two column entry points (``bfhip_diag_columns``, ``bfhip_wstat_columns``) are one gather and must agree bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 16


def _call(ctx, name, *args):
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import _ptr
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *(_ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args)))


@pytest.mark.parametrize('n', [1, 2, 257])
@pytest.mark.parametrize('b', [0, 15])
def test_the_sort_entry_points_agree_with_each_other_and_with_numpy(n, b):
    import torch
    from bayesfast_amd.device import get_context
    ctx = get_context()
    rng = np.random.default_rng(n)
    v = np.round(rng.normal(size=n), 1)                       # ties
    special = [np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan, 0.0, -0.0]
    if n > len(special):
        v[rng.choice(n, len(special), replace=False)] = special
    elif n == 2:
        v[:] = [0.0, -0.0]                                    # equal keys: the stable sort keeps their order
    buf = rng.normal(size=(n, W))
    buf[:, b] = v
    flat, buf = torch.as_tensor(v, device='cuda'), torch.as_tensor(buf, device='cuda')
    k1, o1 = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int64)
    k2, o2 = ctx.empty((n,), dtype=torch.int64), ctx.empty((n,), dtype=torch.int32)
    _call(ctx, 'bfhip_sort_keys', n, flat, k1, o1)
    _call(ctx, 'bfhip_diag_sort', n, buf, b, k2, o2)
    k1, o1, k2, o2 = (t.cpu().numpy() for t in (k1, o1, k2, o2))
    assert np.array_equal(k1, k2)
    assert np.array_equal(o1, o2.astype(np.int64))
    assert np.array_equal(o1, np.argsort(v, kind='stable'))   # (NumPy sorts -0 with +0 and every NaN last, as the keys do)


@pytest.mark.parametrize('nb', [1, 16])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_the_column_entry_points_agree_bit_for_bit(nb, dtype):
    import torch
    from bayesfast_amd.device import get_context
    ctx = get_context()
    n_chain, n_draw, since, k0 = 3, 6, 1, 2
    h = n_draw // 2
    rng = np.random.default_rng(nb)
    full = torch.as_tensor(rng.normal(size=(n_chain + 1, 2 * (n_draw + since) + 1, k0 + nb + 3)), device='cuda')
    full = full.to(getattr(torch, dtype))
    x = full[:n_chain, ::2]                                   # strided in chain and row
    f32 = int(dtype == 'float32')
    filled = lambda *shape: torch.full(shape, 7., dtype=torch.float64, device='cuda')
    split, whole, masked = filled(2 * n_chain, h, W), filled(n_chain * n_draw, W), filled(n_chain * n_draw, W)
    _call(ctx, 'bfhip_diag_columns', n_chain, h, x.stride(0), x.stride(1), x, f32, since, k0, nb, 0, None, split)
    _call(ctx, 'bfhip_wstat_columns', n_chain, n_draw, x.stride(0), x.stride(1), x, f32, since, k0, nb, None, whole)
    # split chain 2 c + half, step i  <->  row c n_draw + half h + i: the same memory order
    assert np.array_equal(split.cpu().numpy().reshape(-1, W).view(np.uint64), whole.cpu().numpy().view(np.uint64))
    want = np.zeros((n_chain * n_draw, W))
    want[:, :nb] = x[:, since:since + n_draw, k0:k0 + nb].double().cpu().numpy().reshape(-1, nb)
    assert np.array_equal(whole.cpu().numpy(), want)
    w = rng.random(n_chain * n_draw)
    w[[0, 5, 6, 17]] = 0.
    w_d = torch.as_tensor(w, device='cuda')
    _call(ctx, 'bfhip_wstat_columns', n_chain, n_draw, x.stride(0), x.stride(1), x, f32, since, k0, nb, w_d, masked)
    masked = masked.cpu().numpy()
    want[w == 0., :nb] = np.nan
    assert np.array_equal(np.isnan(masked), np.isnan(want))
    assert np.array_equal(masked[w != 0.], want[w != 0.])
