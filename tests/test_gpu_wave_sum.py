"""The sampler kernels' 64-lane sum on the device (bfhip_wave_sum_probe, bayesfast_amd/csrc/bfhip_wave.h): the packed form, the
unpacked form and the form the library's kernels were built with give the same BYTES for 1 to 7 values reduced together, and
those are the bytes of the NumPy emulation of the instruction's lane maps (tests/test_wave_sum_emu.py), on that test's cases:
random lanes over 40 decades, and +-0, subnormals, +-inf and NaN confined to one value of a batch.

Which NaN an operation returns (sign, payload) is the processor's choice and differs between the host and the device, so the
comparison with the emulation takes every NaN as the same NaN; between the device's own forms the comparison is on raw bytes."""
import ctypes as C

import numpy as np
import pytest

import test_wave_sum_emu as emu

pytestmark = pytest.mark.gpu


def _probe(x, form):
    """x (n_batch, n, 64) float64 -> (n_batch, n) from bfhip_wave_sum_probe."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context
    ctx = get_context(0)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)
    out = torch.full(x.shape[:2], -1.25, dtype=torch.float64, device=ctx.device)
    _lib.check(ctx._lib.bfhip_wave_sum_probe(ctx.handle, x.shape[0], x.shape[1], _lib.WSUM_FORMS[form], C.c_void_p(xd.data_ptr()),
                                             C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _one_nan(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


def _check(x):
    built, packed, unpacked = (_probe(x, f) for f in ('built', 'packed', 'unpacked'))
    assert emu.same_bytes(packed, unpacked)
    assert emu.same_bytes(built, packed)
    assert emu.same_bytes(_one_nan(packed), _one_nan(emu.wave_sum_packed(x)))
    assert emu.same_bytes(_one_nan(unpacked), _one_nan(emu.wave_sum_unpacked(x)))
    return packed


@pytest.mark.parametrize('n', emu.N_VALUES)
def test_forms_agree_on_random_lanes(n):
    _check(emu.random_lanes(np.random.default_rng(100 + n), 300, n))


@pytest.mark.parametrize('n', emu.N_VALUES)
def test_special_values_stay_in_their_column(n):
    x, owner, clean = emu.special_cases(n)
    p = _check(x)
    others = np.arange(n)[None, :] != owner[:, None]
    assert np.isfinite(p[others]).all()
    assert emu.same_bytes(p[others], _probe(clean, 'packed')[others])


def test_signed_zero_and_subnormal_sums():
    x = np.zeros((1, 4, 64))
    x[0, 1] = -0.
    x[0, 2] = 5e-324
    x[0, 3] = -2.5e-310
    p = _check(x)
    assert emu.same_bytes(p[0, :2], np.zeros(2))
    assert p[0, 2] == 64 * 5e-324 and p[0, 3] == 64 * -2.5e-310


def test_arguments_are_checked():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import get_context
    ctx = get_context(0)
    buf = torch.zeros(8 * 64, dtype=torch.float64, device=ctx.device)
    ptr = C.c_void_p(buf.data_ptr())
    for args in ((1, 0, 0, ptr, ptr), (1, _lib.WSUM_MAX + 1, 0, ptr, ptr), (1, 2, 3, ptr, ptr), (1, 2, -1, ptr, ptr), (-1, 2, 0, ptr, ptr),
                 (1, 2, 0, None, ptr), (1, 2, 0, ptr, None)):
        with pytest.raises(ValueError):
            _lib.check(ctx._lib.bfhip_wave_sum_probe(ctx.handle, *args))
    _lib.check(ctx._lib.bfhip_wave_sum_probe(ctx.handle, 0, 2, 0, None, None))
