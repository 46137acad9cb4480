"""The cases that tests/test_gpu_acor_kernels.py runs on the device and tests/test_acor_reference_host.py checks on the host, with
the path of csrc/bfhip_acor.hip each one takes (``paths``, computed from helpers/acor_reference.py's ``groups`` and ``log_td``) and
their inputs.  NumPy only.

A lag-kernel workgroup takes 16 series slots (td dimensions of ws_n = 16 / td walkers), one tile of 64 lags starting at
tb = t0 + 64 * tile, and a group of wpg = ceil(n_w / 256) walkers, ws_n at a time; it walks n_eff = n_t - tb steps in chunks of
256, a quarter of a chunk per wave, 16 steps at a time."""
import collections
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import acor_reference as ar  # noqa: E402

Case = collections.namedtuple('Case', 'n_w n_t n_d t0 n_lag pad diag', defaults=(False,))

# the axes the exact cases have to cover between them
N_T = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 319, 320, 321, 513)
N_D = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 33)
N_W = (1, 2, 15, 16, 17, 256, 257, 513)
T0 = (0, 1, 15, 16, 17, 63, 64, 65, 100)
N_LAG = (1, 15, 16, 17, 63, 64, 65, 130)

# (n_w, n_t, n_d, t0, n_lag, padding of ldw)                          what the case is there for (``paths`` computes the full list)
EXACT = (
    Case(1, 1, 1, 0, 1, 0),            # the smallest call
    Case(2, 2, 2, 0, 17, 3),           # n_t = 2, lags 2 .. 16 beyond the series inside the one live tile
    Case(3, 15, 3, 1, 15, 0),          # td = 4 with one dimension idle; single tile, tb = 1, odd n_lag, ends at n_t + 1
    Case(2, 16, 4, 0, 16, 5),          # one full group of 16 steps
    Case(2, 17, 5, 15, 17, 0),         # td = 8 ragged; block straddles n_t
    Case(3, 17, 5, 17, 16, 0),         # block starts exactly at n_t: wholly beyond
    Case(3, 63, 8, 0, 63, 0),          # one wave's quarter less one step
    Case(2, 64, 9, 0, 64, 7),          # td = 16 ragged; exactly one tile from lag 0 (B alone in LDS)
    Case(2, 65, 15, 0, 65, 0),         # a second lag tile of one lag; tile 0 aliases A to B with A allocated
    Case(2, 65, 4, 1, 130, 0),         # tiles at 1 (live), 65 (n_eff = 0) and 129 (beyond) in one launch
    Case(2, 63, 16, 100, 130, 0),      # three tiles, all beyond
    Case(2, 255, 16, 17, 63, 0),       # t0 off a 64 boundary, a single tile with tb != 0 and odd n_lag
    Case(1, 256, 17, 63, 130, 1),      # a second dimension tile of one dimension; exactly one chunk at lag 0
    Case(2, 257, 2, 0, 130, 0),        # a second chunk of one step
    Case(1, 319, 33, 64, 65, 0),       # three dimension tiles, the last of one dimension; the driver's second block start
    Case(2, 320, 1, 65, 64, 9),        # chunk plus halo; ws_n = 16 with one walker per group
    Case(1, 321, 3, 100, 130, 0),
    Case(1, 513, 1, 0, 64, 0),         # three chunks, the last of one step
    Case(2, 513, 2, 16, 130, 0),
    Case(1, 513, 2, 448, 70, 0),       # the driver's fourth block start, straddling n_t in its second tile
    Case(15, 70, 1, 0, 75, 0),
    Case(16, 70, 2, 1, 1, 0),          # one lag
    Case(17, 70, 2, 64, 15, 3),        # n_eff = 6: three waves idle
    Case(256, 70, 1, 0, 64, 0),        # the last shape with one walker per group
    Case(257, 70, 17, 17, 65, 0),      # wpg = 2 > ws_n = 1: the walker loop runs twice; the last group holds one walker
    Case(257, 71, 3, 15, 63, 2),       # wpg = 2, ws_n = 4: two walkers share a tile, two slots stay empty
    Case(257, 70, 3, 100, 17, 0),      # the same grid wholly beyond the series
    Case(513, 70, 9, 63, 16, 0),       # wpg = 3 > ws_n = 1: three passes
    Case(513, 70, 8, 0, 75, 5),        # wpg = 3 > ws_n = 2: two passes, the second half filled
    Case(8, 120, 16, 0, 64, 0, True),  # the diagnostics' call: n_d = 16, tight ldw, inv = 1, even n_w, unused columns zero
    Case(8, 120, 16, 64, 56, 0, True),
)

# every path named above: each has to be hit by at least one exact case (tests/test_acor_reference_host.py checks it)
REQUIRED = tuple(['n_t=%d' % v for v in N_T] + ['n_d=%d' % v for v in N_D] + ['n_w=%d' % v for v in N_W] + ['t0=%d' % v for v in T0]
                 + ['n_lag=%d' % v for v in N_LAG] + ['td=%d' % v for v in (1, 2, 4, 8, 16)]
                 + ['ragged_dimension_tile', 'second_tile_of_one_dimension', 'wpg>1', 'wpg>ws_n', 'wpg>ws_n,last_pass_part_filled',
                    'walkers_share_a_tile', 'empty_walker_slots', 'last_group_short', 'one_tile_from_lag_0', 'several_tiles_from_lag_0',
                    'one_tile,tb!=0,odd_n_lag', 't0_off_64', 'part_filled_last_lag_tile', 'straddles_n_t', 'wholly_beyond_n_t',
                    'dead_tile_in_a_live_launch', 'one_chunk', 'several_chunks', 'last_chunk_of_one_step', 'idle_waves',
                    'steps_not_a_multiple_of_16', 'ldw_padded', 'ldw_tight', 'diagnostics_form'])


def paths(c):
    """The names of the lag kernel's paths that case c takes."""
    ltd = ar.log_td(c.n_d)
    td, ws_n = 1 << ltd, ar.SLOTS >> ltd
    wpg, n_g = ar.groups(c.n_w)
    tiles = -(-c.n_lag // ar.LAGS)
    tbs = [c.t0 + ar.LAGS * i for i in range(tiles)]
    live = [c.n_t - tb for tb in tbs if tb < c.n_t]       # n_eff of the tiles that do any work
    p = ['n_t=%d' % c.n_t, 'n_d=%d' % c.n_d, 'n_w=%d' % c.n_w, 't0=%d' % c.t0, 'n_lag=%d' % c.n_lag, 'td=%d' % td,
         'ldw_padded' if c.pad else 'ldw_tight']
    if c.n_d % td:
        p.append('ragged_dimension_tile')
    if c.n_d > td and c.n_d % td == 1:
        p.append('second_tile_of_one_dimension')
    if wpg > 1:
        p.append('wpg>1')
        if ws_n > 1:
            p.append('walkers_share_a_tile')
    if wpg > ws_n:
        p.append('wpg>ws_n')
        if wpg % ws_n:
            p.append('wpg>ws_n,last_pass_part_filled')
    if ws_n > wpg or wpg % ws_n:
        p.append('empty_walker_slots')
    if c.n_w % wpg:
        p.append('last_group_short')
    if c.t0 == 0:
        p.append('one_tile_from_lag_0' if tiles == 1 else 'several_tiles_from_lag_0')
    elif tiles == 1 and c.n_lag % 2:
        p.append('one_tile,tb!=0,odd_n_lag')
    if c.t0 % ar.LAGS:
        p.append('t0_off_64')
    if c.n_lag % ar.LAGS:
        p.append('part_filled_last_lag_tile')
    if c.t0 < c.n_t < c.t0 + c.n_lag:
        p.append('straddles_n_t')
    if c.t0 >= c.n_t:
        p.append('wholly_beyond_n_t')
    elif len(live) < tiles:
        p.append('dead_tile_in_a_live_launch')
    for n_eff in live:
        p.append('one_chunk' if n_eff <= ar.CHUNK else 'several_chunks')
        if n_eff > ar.CHUNK and n_eff % ar.CHUNK == 1:
            p.append('last_chunk_of_one_step')
        if 0 < n_eff % ar.CHUNK <= 3 * ar.CHUNK // 4:
            p.append('idle_waves')
        if n_eff % 16:
            p.append('steps_not_a_multiple_of_16')
    if c.diag:
        p.append('diagnostics_form')
    return sorted(set(p))


def case_id(c):
    return 'w%d-t%d-d%d-from%d-lags%d%s%s' % (c.n_w, c.n_t, c.n_d, c.t0, c.n_lag, '-pad%d' % c.pad if c.pad else '', '-diag' if c.diag else '')


@functools.lru_cache(maxsize=None)
def exact_inputs(c):
    """x: integers in [-3, 3]; mean: integers in {-1, 0, 1}; inv: powers of two in 1/4 .. 4, all varying with (w, k): every centred
    value, product and sum is an integer multiple of 1/4 below 64 n_w n_t / 4 < 2^53, exact in float64 in any order.  The
    diagnostics' form has inv = 1 and only its first five columns in use, the others zero as bfhip_diag_columns leaves them."""
    rng = np.random.default_rng(1000 + EXACT.index(c))
    x = rng.integers(-3, 4, size=(c.n_w, c.n_t, c.n_d)).astype(np.float64)
    mean = rng.integers(-1, 2, size=(c.n_w, c.n_d)).astype(np.float64)
    inv = 2. ** rng.integers(-2, 3, size=(c.n_w, c.n_d))
    if c.diag:
        inv[:] = 1.
        x[:, :, 5:] = 0.
        mean[:, 5:] = 0.
    for a in (x, mean, inv):
        a.setflags(write=False)
    return x, mean, inv


@functools.lru_cache(maxsize=None)
def exact_reference(c):
    """The float64 lag sums of an exact case (the longdouble reference holds the same integers) -- computed once."""
    x, mean, inv = exact_inputs(c)
    s, _ = ar.lag_sums(x, mean, inv, c.t0, c.n_lag)
    out = s.astype(np.float64)
    assert np.array_equal(out.astype(ar.LD), s)
    out.setflags(write=False)
    return out


def ar1(rng, phi, n_w, n_t, n_d):
    e = rng.normal(size=(n_w, n_t, n_d))
    for t in range(1, n_t):
        e[:, t] = phi * e[:, t - 1] + np.sqrt(1 - phi * phi) * e[:, t]
    return e


# the float cases: shapes that take the kernel's distinct paths once more, in one call over every lag and five beyond
FLOAT = (Case(5, 300, 3, 0, 305, 0), Case(17, 257, 17, 0, 262, 3), Case(257, 70, 8, 0, 75, 0), Case(3, 513, 2, 17, 63, 0),
         Case(513, 65, 9, 1, 69, 5))


@functools.lru_cache(maxsize=None)
def float_inputs(c, seed=0):
    """AR(1) series (phi 0, 0.5, 0.9, 0.98 across the dimensions) scaled by 10^u, u uniform in [-1.5, 1.5], and offset by up to ten
    spreads, both per (w, k): the series' variances span 1e-3 to 1e3, so 1 / a_wk(0) differs by up to 1e6 between walkers."""
    rng = np.random.default_rng(2000 + 17 * seed + c.n_w + c.n_t + c.n_d)
    phis = np.array([0., 0.5, 0.9, 0.98])[np.arange(c.n_d) % 4]
    x = np.stack([ar1(rng, p, c.n_w, c.n_t, 1)[:, :, 0] for p in phis], axis=-1)
    scale = 10. ** rng.uniform(-1.5, 1.5, size=(c.n_w, 1, c.n_d))
    x = x * scale + 10. * scale * rng.uniform(-1., 1., size=(c.n_w, 1, c.n_d))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def float_reference(c):
    """(mean, inv, S, A) of a float case: the reference's moments rounded to float64, and its lag sums about them."""
    x = float_inputs(c)
    mean, inv = ar.moments(x)
    s, a = ar.lag_sums(x, mean, inv, c.t0, c.n_lag)
    for v in (mean, inv, s, a):
        v.setflags(write=False)
    return mean, inv, s, a


def n_terms(c):
    """(n_lag,): the number of products in each lag's sum."""
    return c.n_w * np.maximum(c.n_t - (c.t0 + np.arange(c.n_lag)), 0)


# the moments' shapes: the corners of the exact grid's (n_w, n_t, n_d), and shapes whose series count is no multiple of 16
MOMENT_SHAPES = ((1, 1, 1), (1, 513, 1), (1, 513, 33), (513, 1, 33), (513, 70, 1), (513, 70, 33), (257, 2, 17), (16, 257, 16), (17, 65, 15))


@functools.lru_cache(maxsize=None)
def moment_inputs(shape):
    n_w, n_t, n_d = shape
    rng = np.random.default_rng(3000 + n_w + n_t + n_d)
    x = rng.normal(size=shape) * 10. ** rng.uniform(-1.5, 1.5, size=(n_w, 1, n_d)) + rng.normal(size=(n_w, 1, n_d))
    x.setflags(write=False)
    return x


OFFSET = 1e8


@functools.lru_cache(maxsize=None)
def offset_inputs(shape=(4, 500, 3)):
    """Unit spread about 1e8: sum x^2 and n_t mean^2 agree to 16 digits, a(0) is what is left."""
    x = OFFSET + np.random.default_rng(3100).normal(size=shape)
    x.setflags(write=False)
    return x


if __name__ == '__main__':
    for case in EXACT:
        print('%-40s %s' % (case_id(case), ' '.join(q for q in paths(case) if '=' not in q or q.startswith('td'))))
