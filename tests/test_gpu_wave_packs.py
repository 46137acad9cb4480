"""The wave reduction whose results stay in their vector registers, on the device (bfhip_wave_packs_probe: wave_sum_packs, get,
any_le0 of bayesfast_amd/csrc/bfhip_wave.h), on the cases of tests/test_wave_packs_emu.py: for 1 to 7 values reduced together the
values read through get are the BYTES of wave_sum_n on the same lanes (bfhip_wave_sum_probe, the form the library was built
with), and the flag is any(sum <= 0.) of those sums -- with one special sum (zero, the lanes all -0., the smallest negative and a
positive subnormal, -inf, +inf, NaN) in every column of every pack next to positive sums, with a NaN next to a negative sum, and
with no positive sum at all.

Against the emulation every NaN counts as the same NaN (tests/test_gpu_wave_sum.py); between the two probes the bytes are raw."""
import ctypes as C

import numpy as np
import pytest

import test_wave_packs_emu as pe
import test_wave_sum_emu as emu

pytestmark = pytest.mark.gpu


def _packs_probe(x):
    """x (n_batch, n, 64) float64 -> values (n_batch, n), flag (n_batch,) bool from bfhip_wave_packs_probe."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context
    ctx = get_context(0)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)
    out = torch.full(x.shape[:2], -1.25, dtype=torch.float64, device=ctx.device)
    flag = torch.full(x.shape[:1], -7, dtype=torch.int32, device=ctx.device)
    _lib.check(ctx._lib.bfhip_wave_packs_probe(ctx.handle, x.shape[0], x.shape[1], C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(flag.data_ptr())))
    torch.cuda.synchronize()
    f = flag.cpu().numpy()
    assert np.isin(f, (0, 1)).all()
    return out.cpu().numpy(), f == 1


def _sum_probe(x):
    from test_gpu_wave_sum import _probe
    return _probe(x, 'built')


def _one_nan(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


def _check(x):
    v, f = _packs_probe(x)
    assert emu.same_bytes(v, _sum_probe(x))
    ev, ef = pe.values_and_flag(x)
    assert emu.same_bytes(_one_nan(v), _one_nan(ev))
    assert np.array_equal(f, pe.expected_flag(v)) and np.array_equal(f, ef)
    return v, f


@pytest.mark.parametrize('n', pe.N_VALUES)
def test_get_is_wave_sum_n_and_the_flag_is_any_sum_le0_on_random_lanes(n):
    rng = np.random.default_rng(200 + n)
    _check(emu.random_lanes(rng, 200, n))
    _, f = _check(pe.mixed_sign_lanes(rng, 200, n))
    assert f.any()
    _, f = _check(pe.positive_lanes(rng, n)[None])
    assert not f.any()


@pytest.mark.parametrize('n', pe.N_VALUES)
def test_one_special_sum_in_every_column_of_every_pack(n):
    x, owner, flag = pe.special_sum_cases(n)
    v, f = _check(x)
    assert np.array_equal(f, flag)
    own = v[np.arange(len(owner)), owner].reshape(n, len(pe.SPECIAL_SUMS))
    zero = np.zeros(n)
    assert emu.same_bytes(own[:, 0], zero) and emu.same_bytes(own[:, 1], zero)
    assert (own[:, 2] == pe.NEG_SUB).all() and (own[:, 3] == pe.POS_SUB).all()
    assert (own[:, 4] == -np.inf).all() and (own[:, 5] == np.inf).all() and np.isnan(own[:, 6]).all()
    others = np.arange(n)[None, :] != owner[:, None]
    assert (v[others] > 0.).all() and np.isfinite(v[others]).all()


@pytest.mark.parametrize('n', pe.N_VALUES)
def test_flag_is_true_with_a_nan_next_to_a_negative_sum_and_with_no_positive_sum(n):
    v, f = _check(pe.true_flag_cases(n))
    assert f.all()


def test_arguments_are_checked():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context
    ctx = get_context(0)
    buf = torch.zeros(8 * 64, dtype=torch.float64, device=ctx.device)
    ptr = C.c_void_p(buf.data_ptr())
    for args in ((1, 0, ptr, ptr, ptr), (1, _lib.WSUM_MAX + 1, ptr, ptr, ptr), (-1, 2, ptr, ptr, ptr), (1, 2, None, ptr, ptr),
                 (1, 2, ptr, None, ptr), (1, 2, ptr, ptr, None)):
        with pytest.raises(ValueError):
            _lib.check(ctx._lib.bfhip_wave_packs_probe(ctx.handle, *args))
    with pytest.raises(ValueError):
        _lib.check(ctx._lib.bfhip_wave_packs_probe(None, 1, 2, ptr, ptr, ptr))
    _lib.check(ctx._lib.bfhip_wave_packs_probe(ctx.handle, 0, 2, None, None, None))
