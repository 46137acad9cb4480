"""The sampler kernels' 64-lane sum (bayesfast_amd/csrc/bfhip_wave.h) emulated in NumPy from the lane maps of
v_mfma_f64_4x4x4 -- four 4 x 4 x 4 products, one per block b: A[i][k] from lane 16k + 4b + i, B[k][j] from lane 16k + 4b + j,
D[i][j] = C + sum over k (ascending) of A[i][k] B[k][j] in lane 16i + 4b + j -- and of the row rotations by 8 and 4 lanes.

The packed form gives column j of the second step to value j of a pack of four; the unpacked form repeats one value in all
four columns.  The tests hold the two to the same BYTES for 1 to 7 values reduced together (the kernels reduce 1 to 7), on
random lanes of a wide dynamic range and with +-0, subnormals, +-inf and NaN confined to one value: a non-finite lane of one
value must not reach another value's result.  No GPU: tests/test_gpu_wave_sum.py runs the same cases on the device."""
import numpy as np
import pytest

N_VALUES = (1, 2, 3, 4, 5, 6, 7)
SPECIALS = (0., -0., 5e-324, -2.5e-310, np.inf, -np.inf, np.nan)


def mfma_4x4x4(a, b):
    """D = 0 + A B of the four blocks; a, b (..., 64) lane values (a scalar operand is the same number in every lane)."""
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), np.broadcast(a, b).shape)
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), a.shape)
    d = np.empty(a.shape)
    for i in range(4):
        for blk in range(4):
            for j in range(4):
                acc = np.zeros(a.shape[:-1])
                for k in range(4):   # (one factor is 1: the product is exact, a fused multiply-add rounds as this does)
                    acc = acc + a[..., 16 * k + 4 * blk + i] * b[..., 16 * k + 4 * blk + j]
                d[..., 16 * i + 4 * blk + j] = acc
    return d


def row_ror_add(v, n):
    """v += row_ror:n (v): lane l of a row of 16 receives lane (l - n) mod 16 of its row."""
    lane = np.arange(64)
    src = (lane & ~15) | ((lane - n) & 15)
    return v + v[..., src]


def finish(v):
    return row_ror_add(row_ror_add(mfma_4x4x4(1., v), 8), 4)


def wave_sum_unpacked(x):
    """x (..., N, 64) -> (..., N): wave_sum_n_unpacked, every value on its own; the result is read from lane 0."""
    with np.errstate(all='ignore'):
        return finish(mfma_4x4x4(x, 1.))[..., 0]


def pack_column_source(m):
    """Which value of a pack of m each of the four columns carries (a column without a value of its own repeats another)."""
    return {1: (0, 0, 0, 0), 2: (0, 1, 0, 1), 3: (0, 1, 2, 2), 4: (0, 1, 2, 3)}[m]


def wave_sum_packed(x):
    """wave_sum_n_packed: the first step per value, then per pack of four the operand whose lane l comes from value (l & 3),
    one second step and one pair of rotations; value 4 c + j is read from lane j."""
    n = x.shape[-2]
    if n == 1:
        return wave_sum_unpacked(x)
    out = np.empty(x.shape[:-1])
    col = np.arange(64) & 3
    with np.errstate(all='ignore'):
        d = mfma_4x4x4(x, 1.)
        for c in range((n + 3) // 4):
            m = min(4, n - 4 * c)
            src = np.asarray(pack_column_source(m))[col] + 4 * c
            p = finish(np.take_along_axis(d, np.broadcast_to(src, d.shape[:-2] + (1, 64)), axis=-2)[..., 0, :])
            for j in range(m):
                out[..., 4 * c + j] = p[..., j]
    return out


def random_lanes(rng, n_batch, n):
    """(n_batch, n, 64) lanes: magnitudes over 40 decades and both signs, so that every addition of the tree rounds."""
    return rng.normal(size=(n_batch, n, 64)) * 10. ** rng.uniform(-20., 20., size=(n_batch, n, 64))


def special_cases(n, seed=7):
    """(cases, n, 64), owner (cases,), clean (cases, n, 64): every special value in turn in one lane, in eight lanes and in all
    lanes of ONE value (the owner), random finite lanes elsewhere; clean is the same without the special value."""
    rng = np.random.default_rng(seed + n)
    xs, owners, cleans = [], [], []
    for owner in range(n):
        for s in SPECIALS:
            for lanes in (rng.integers(0, 64, 1), rng.choice(64, 8, replace=False), np.arange(64)):
                clean = random_lanes(rng, 1, n)[0]
                x = clean.copy()
                x[owner, lanes] = s
                xs.append(x); owners.append(owner); cleans.append(clean)
    return np.array(xs), np.array(owners), np.array(cleans)


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_emulation_is_a_sum():
    """The emulated tree adds the 64 lanes: against math.fsum within 64 roundings of the sum of magnitudes."""
    import math
    rng = np.random.default_rng(1)
    x = random_lanes(rng, 50, 3)
    s = wave_sum_unpacked(x)
    for b in range(50):
        for i in range(3):
            assert abs(s[b, i] - math.fsum(x[b, i])) <= 64 * np.finfo(float).eps * math.fsum(np.abs(x[b, i]))


@pytest.mark.parametrize('n', N_VALUES)
def test_packed_equals_unpacked_on_random_lanes(n):
    x = random_lanes(np.random.default_rng(100 + n), 300, n)
    assert same_bytes(wave_sum_packed(x), wave_sum_unpacked(x))


@pytest.mark.parametrize('n', N_VALUES)
def test_special_values_stay_in_their_column(n):
    x, owner, clean = special_cases(n)
    p, u = wave_sum_packed(x), wave_sum_unpacked(x)
    assert same_bytes(p, u)
    others = np.arange(n)[None, :] != owner[:, None]
    # the other values of the batch: finite, and the very bytes they have without the special value next to them
    assert np.isfinite(p[others]).all()
    assert same_bytes(p[others], wave_sum_packed(clean)[others])
    # the owner's result is what its lanes say: NaN lanes give NaN, infinities of one sign that infinity
    own = p[np.arange(len(owner)), owner]
    xo = x[np.arange(len(owner)), owner]
    has_nan = np.isnan(xo).any(1)
    assert np.isnan(own[has_nan]).all()
    pos, neg = (xo == np.inf).any(1), (xo == -np.inf).any(1)
    assert (own[pos & ~neg] == np.inf).all() and (own[neg & ~pos] == -np.inf).all()
    assert np.isfinite(own[~has_nan & ~pos & ~neg]).all()


def test_signed_zero_and_subnormal_sums():
    """All lanes -0 sum to +0 (the accumulator starts at +0) in both forms; 64 lanes of one subnormal ulp sum exactly."""
    x = np.zeros((1, 4, 64))
    x[0, 1] = -0.
    x[0, 2] = 5e-324
    x[0, 3] = -2.5e-310
    p, u = wave_sum_packed(x), wave_sum_unpacked(x)
    assert same_bytes(p, u)
    assert same_bytes(p[0, :2], np.zeros(2))
    assert p[0, 2] == 64 * 5e-324 and p[0, 3] == 64 * -2.5e-310
