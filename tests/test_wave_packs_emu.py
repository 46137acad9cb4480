"""The wave reduction whose results stay in their vector registers (bayesfast_amd/csrc/bfhip_wave.h: wave_sum_packs) emulated in
NumPy with the lane maps of tests/test_wave_sum_emu.py: the packs after the two row rotations, get(i) -- value 4 c + j read from
lane j of pack c -- and any_le0() -- one ordered compare `<= 0.` per pack over all 64 lanes, the lane masks OR-ed.

What is held here, for 1 to 7 values reduced together: get(i) is wave_sum_n's value byte for byte, and the flag is
any(sum <= 0.) of those sums -- false for NaN, true for zero, a negative subnormal and -inf.  The cases put one special sum at a
time into every column of every pack (the last value of a short pack included) next to sums that are all positive, so that a
padding column or a neighbouring column that leaked into the compare would flip the flag.

A sum of exactly -0. cannot be built: the matrix steps accumulate from +0., and +0. + -0. = +0. (test_wave_sum_emu.py:
test_signed_zero_and_subnormal_sums); lanes that are all -0. are the nearest case and give +0., on which the flag is true like on
-0. itself.  The compare's own answer on -0. is held on the emulated register directly (test_compare_on_a_register).

No GPU: tests/test_gpu_wave_packs.py runs the same cases through bfhip_wave_packs_probe."""
import numpy as np
import pytest

import test_wave_sum_emu as emu

N_VALUES = emu.N_VALUES
NEG_SUB, POS_SUB = -5e-324, 5e-324   # the smallest negative subnormal, a positive subnormal
# name -> (lanes of the special value, the others of that value, the sum, the flag it gives on its own)
SPECIAL_SUMS = ('+0', '-0 lanes', 'negative subnormal', 'positive subnormal', '-inf', '+inf', 'nan')


def packs(x):
    """x (..., N, 64) -> list of (..., 64): the packed registers after the two row rotations (one value: the unpacked form's
    register, every lane the sum)."""
    n = x.shape[-2]
    col = np.arange(64) & 3
    with np.errstate(all='ignore'):
        d = emu.mfma_4x4x4(x, 1.)
        if n == 1:
            return [emu.finish(d[..., 0, :])]
        out = []
        for c in range((n + 3) // 4):
            m = min(4, n - 4 * c)
            src = np.asarray(emu.pack_column_source(m))[col] + 4 * c
            out.append(emu.finish(np.take_along_axis(d, np.broadcast_to(src, d.shape[:-2] + (1, 64)), axis=-2)[..., 0, :]))
        return out


def get(pk, n, i):
    return pk[0][..., 0] if n == 1 else pk[i >> 2][..., i & 3]


def any_le0(pk):
    """One compare per pack on the whole register, every lane's answer OR-ed (NaN <= 0. is false)."""
    with np.errstate(invalid='ignore'):
        return np.any([(p <= 0.).any(-1) for p in pk], axis=0)


def values_and_flag(x):
    pk = packs(x)
    n = x.shape[-2]
    return np.stack([get(pk, n, i) for i in range(n)], axis=-1), any_le0(pk)


def positive_lanes(rng, n):
    """(n, 64) lanes in [0.5, 1.5): every sum is positive, about 64."""
    return rng.uniform(0.5, 1.5, size=(n, 64))


def special_lanes(rng, name):
    """64 lanes whose sum is the named special value, and whether that sum is <= 0."""
    v = np.zeros(64)
    k = int(rng.integers(0, 64))
    if name == '+0':
        return v, True
    if name == '-0 lanes':
        return -v, True   # (sums to +0.: see the module's text)
    if name == 'negative subnormal':
        v[k] = NEG_SUB
        return v, True
    if name == 'positive subnormal':
        v[k] = POS_SUB
        return v, False
    v = rng.uniform(0.5, 1.5, size=64)
    v[k] = {'-inf': -np.inf, '+inf': np.inf, 'nan': np.nan}[name]
    return v, name == '-inf'


def special_sum_cases(n, seed=21):
    """(cases, n, 64), owner (cases,), flag (cases,): every special sum in turn in every value of the batch, all other sums positive."""
    rng = np.random.default_rng(seed + n)
    xs, owners, flags = [], [], []
    for owner in range(n):
        for name in SPECIAL_SUMS:
            x = positive_lanes(rng, n)
            x[owner], f = special_lanes(rng, name)
            xs.append(x); owners.append(owner); flags.append(f)
    return np.array(xs), np.array(owners), np.array(flags)


def true_flag_cases(n, seed=33):
    """(cases, n, 64), all with a true flag: a NaN in one value next to a negative sum in another (n >= 2: every ordered pair of
    values), and all sums non-positive (negative, zero, -inf mixed)."""
    rng = np.random.default_rng(seed + n)
    xs = []
    for i in range(n):
        for j in range(n):
            if i != j:
                x = positive_lanes(rng, n)
                x[i, int(rng.integers(0, 64))] = np.nan
                x[j] = -x[j]
                xs.append(x)
    x = -positive_lanes(rng, n)
    xs.append(x.copy())
    x[::2] = 0.
    xs.append(x.copy())
    x[n - 1, 5] = -np.inf
    xs.append(x)
    return np.array(xs)


def mixed_sign_lanes(rng, n_batch, n):
    """Random lanes whose sums take both signs."""
    return rng.normal(size=(n_batch, n, 64)) + rng.normal(size=(n_batch, n, 1)) * 0.2


def expected_flag(sums):
    with np.errstate(invalid='ignore'):
        return (sums <= 0.).any(-1)


@pytest.mark.parametrize('n', N_VALUES)
def test_get_is_wave_sum_n_and_the_flag_is_any_sum_le0_on_random_lanes(n):
    rng = np.random.default_rng(200 + n)
    for x in (emu.random_lanes(rng, 200, n), mixed_sign_lanes(rng, 200, n), positive_lanes(rng, n)[None]):
        v, f = values_and_flag(x)
        ref = emu.wave_sum_packed(x)
        assert emu.same_bytes(v, ref) and emu.same_bytes(v, emu.wave_sum_unpacked(x))
        assert np.array_equal(f, expected_flag(ref))
    assert not f.any()   # (the last set: all sums positive)
    assert expected_flag(emu.wave_sum_packed(mixed_sign_lanes(rng, 200, n))).any()


@pytest.mark.parametrize('n', N_VALUES)
def test_one_special_sum_in_every_column_of_every_pack(n):
    x, owner, flag = special_sum_cases(n)
    v, f = values_and_flag(x)
    ref = emu.wave_sum_packed(x)
    assert emu.same_bytes(v, ref)
    assert np.array_equal(f, expected_flag(ref)) and np.array_equal(f, flag)
    own = ref[np.arange(len(owner)), owner].reshape(n, len(SPECIAL_SUMS))
    zero = np.zeros(n)
    assert emu.same_bytes(own[:, 0], zero) and emu.same_bytes(own[:, 1], zero)
    assert (own[:, 2] == NEG_SUB).all() and (own[:, 3] == POS_SUB).all()
    assert (own[:, 4] == -np.inf).all() and (own[:, 5] == np.inf).all() and np.isnan(own[:, 6]).all()
    others = np.arange(n)[None, :] != owner[:, None]
    assert (ref[others] > 0.).all() and np.isfinite(ref[others]).all()


@pytest.mark.parametrize('n', N_VALUES)
def test_flag_is_true_with_a_nan_next_to_a_negative_sum_and_with_no_positive_sum(n):
    x = true_flag_cases(n)
    v, f = values_and_flag(x)
    ref = emu.wave_sum_packed(x)
    assert emu.same_bytes(v, ref)
    assert f.all() and expected_flag(ref).all()
    n_pairs = n * (n - 1)
    assert np.isnan(ref[:n_pairs]).any(-1).all() and (ref[:n_pairs] < 0.).any(-1).all()
    assert not (ref[n_pairs:] > 0.).any()


@pytest.mark.parametrize('n', N_VALUES)
def test_padding_columns_repeat_a_value_of_their_own_pack(n):
    """What lets the compare run without a lane mask: every lane of every pack holds one of that pack's own sums."""
    x = mixed_sign_lanes(np.random.default_rng(300 + n), 20, n)
    ref = emu.wave_sum_packed(x)
    for c, p in enumerate(packs(x)):
        mine = ref[:, 4 * c:4 * c + 4] if n > 1 else ref
        assert (p.view(np.uint64)[:, :, None] == mine.view(np.uint64)[:, None, :]).any(-1).all()


def test_compare_on_a_register():
    """The ordered compare itself, on a register that holds the value in every lane: true for +-0., the negative subnormal and
    -inf; false for the positive subnormal, +inf and NaN."""
    for val, want in ((0., True), (-0., True), (NEG_SUB, True), (-np.inf, True), (POS_SUB, False), (np.inf, False), (np.nan, False),
                      (-1., True), (1., False)):
        assert bool(any_le0([np.full((1, 64), val)])[0]) is want
