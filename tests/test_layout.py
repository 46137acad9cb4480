"""The automatic layout policy (bayesfast_amd/layout.py) and the launch schedule of DeviceChains.run, on the CPU: every expected
value below is written out by hand from the rules' thresholds, none is computed by the code under test."""
import numpy as np
import pytest

from bayesfast_amd import layout
from bayesfast_amd.layout import ShapeFacts

N_CU = 256
KINDS = {  # plain, featured, decay, decay_shared
    'plain': (True, False, False, False), 'decay': (False, True, True, False), 'shared': (False, True, True, True),
    'transform': (False, True, False, False), 'other': (False, False, False, False), 'both': (False, False, True, True)}


def F(d, n, kind='plain'):
    return ShapeFacts(d, n, N_CU, *KINDS[kind])


S, G, W = 'split', 'group', 'wave'
LAG = 4096
CELLS = [
    # --- rule 1: in step -> the in-step layout, else the wave layout (64-d x 16 chains per CU: no shape rule applies)
    (F(64, 4096), 'NUTS', 0, S, W), (F(64, 4096), 'NUTS', 7, S, S), (F(64, 4096), 'NUTS', 7, G, G), (F(64, 4096), 'NUTS', 0, G, W),
    (F(64, 4096), 'NUTS', 1, S, S), (F(64, 4096), 'NUTS', 1023, S, S),
    (F(64, 4096), 'HMC', 0, S, S), (F(64, 4096), 'HMC', 0, G, G),
    # --- the laggard flag: the wave layout, in step or not; HMC ignores it
    (F(64, 4096), 'NUTS', LAG + 7, S, W), (F(64, 4096), 'NUTS', LAG, S, W), (F(64, 4096), 'NUTS', LAG + 7, G, W),
    (F(64, 4096), 'HMC', LAG + 7, S, S), (F(64, 4096), 'HMC', LAG, G, G),
    # --- small problem (beats the in-step answer).  Featured: d <= 64 and at most eight chains per CU
    (F(64, 2048, 'decay'), 'NUTS', 7, S, W), (F(64, 2049, 'decay'), 'NUTS', 7, S, S), (F(65, 2048, 'decay'), 'NUTS', 7, S, S),
    (F(32, 2048, 'transform'), 'NUTS', 7, S, W), (F(32, 2049, 'transform'), 'NUTS', 7, S, S),
    (F(64, 2048, 'shared'), 'NUTS', 7, G, W), (F(64, 2049, 'shared'), 'NUTS', 7, G, G),
    # neither plain nor featured: never small
    (F(64, 512, 'other'), 'NUTS', 7, S, S), (F(64, 512, 'other'), 'NUTS', 0, S, W), (F(64, 512, 'both'), 'NUTS', 7, S, S),
    # plain, d <= 16: at most four chains per CU
    (F(16, 1024), 'NUTS', 7, S, W), (F(16, 1025), 'NUTS', 7, S, S), (F(8, 1024), 'NUTS', 7, S, W),
    # plain, 17 <= d <= 32: fewer than six chains per CU
    (F(17, 1535), 'NUTS', 7, S, W), (F(17, 1536), 'NUTS', 7, S, S), (F(32, 1535), 'NUTS', 7, S, W), (F(32, 1536), 'NUTS', 7, S, S),
    (F(16, 1535), 'NUTS', 7, S, S),
    # plain, 33 <= d <= 64: at most four chains per CU
    (F(33, 1024), 'NUTS', 7, S, W), (F(33, 1025), 'NUTS', 7, S, S), (F(33, 1535), 'NUTS', 7, S, S),
    (F(64, 1024), 'NUTS', 7, S, W), (F(64, 1025), 'NUTS', 7, S, S), (F(65, 1024), 'NUTS', 7, S, S), (F(128, 256), 'NUTS', 7, S, S),
    # HMC ignores it
    (F(64, 1024), 'HMC', 0, S, S), (F(64, 2048, 'decay'), 'HMC', 0, S, S),
    # --- lanes whatever the trees: plain, d <= 32, at least sixteen chains per CU (disjoint from the small problems by their chain
    # counts, so the two never meet in one cell); loses to a laggard
    (F(32, 4096), 'NUTS', 0, S, S), (F(32, 4095), 'NUTS', 0, S, W), (F(33, 4096), 'NUTS', 0, S, W), (F(16, 4096), 'NUTS', 0, S, S),
    (F(32, 4096), 'NUTS', 0, G, G), (F(32, 4095), 'NUTS', 0, G, W),
    (F(16, 4096, 'decay'), 'NUTS', 0, S, W), (F(16, 4096, 'transform'), 'NUTS', 0, S, W), (F(16, 4096, 'other'), 'NUTS', 0, S, W),
    (F(32, 4096), 'NUTS', LAG, S, W), (F(32, 4096), 'NUTS', LAG + 7, S, W), (F(16, 4096), 'NUTS', LAG + 7, G, W),
    # --- deep trees.  The decay term sharing the bound's matrix: from 12 leaves at 17 <= d <= 64
    (F(64, 4096, 'shared'), 'NUTS', 11, S, S), (F(64, 4096, 'shared'), 'NUTS', 12, S, W),
    (F(33, 4096, 'shared'), 'NUTS', 11, S, S), (F(33, 4096, 'shared'), 'NUTS', 12, S, W),
    (F(32, 4096, 'shared'), 'NUTS', 11, S, S), (F(32, 4096, 'shared'), 'NUTS', 12, S, W),
    (F(17, 4096, 'shared'), 'NUTS', 11, S, S), (F(17, 4096, 'shared'), 'NUTS', 12, S, W),
    (F(16, 4096, 'shared'), 'NUTS', 1023, S, S), (F(65, 4096, 'shared'), 'NUTS', 1023, S, S),
    (F(64, 4096, 'shared'), 'NUTS', 11, G, G), (F(64, 4096, 'shared'), 'NUTS', 12, G, W),
    # the decay term with a matrix of its own: from 24 leaves at 33 <= d <= 64 only
    (F(64, 4096, 'decay'), 'NUTS', 12, S, S), (F(64, 4096, 'decay'), 'NUTS', 23, S, S), (F(64, 4096, 'decay'), 'NUTS', 24, S, W),
    (F(33, 4096, 'decay'), 'NUTS', 23, S, S), (F(33, 4096, 'decay'), 'NUTS', 24, S, W),
    (F(32, 4096, 'decay'), 'NUTS', 1023, S, S), (F(65, 4096, 'decay'), 'NUTS', 1023, S, S),
    # never behind the constraint transform, with both, or for other densities
    (F(64, 4096, 'transform'), 'NUTS', 1023, S, S), (F(64, 4096, 'both'), 'NUTS', 1023, S, S), (F(64, 4096, 'other'), 'NUTS', 1023, S, S),
    # the plain surrogate at 33 <= d <= 64, more than four and at most eight chains per CU: from 12 leaves
    (F(64, 2048), 'NUTS', 11, S, S), (F(64, 2048), 'NUTS', 12, S, W), (F(64, 2049), 'NUTS', 12, S, S),
    (F(64, 1025), 'NUTS', 11, S, S), (F(64, 1025), 'NUTS', 12, S, W), (F(64, 1024), 'NUTS', 11, S, W),
    (F(33, 2048), 'NUTS', 12, S, W), (F(32, 2048), 'NUTS', 12, S, S), (F(65, 2048), 'NUTS', 12, S, S), (F(64, 2048), 'NUTS', 12, G, W),
    # HMC ignores it
    (F(64, 4096, 'shared'), 'HMC', 1023, S, S), (F(64, 2048), 'HMC', 12, S, S),
    # --- two groups per CU: plain, 17 <= d <= 32, at least 32 chains per CU: 'split' becomes 'group', in step only
    (F(32, 8192), 'NUTS', 7, S, G), (F(32, 8191), 'NUTS', 7, S, S), (F(17, 8192), 'NUTS', 7, S, G), (F(16, 8192), 'NUTS', 7, S, S),
    (F(33, 8192), 'NUTS', 7, S, S), (F(32, 8192, 'decay'), 'NUTS', 7, S, S), (F(32, 8192, 'other'), 'NUTS', 7, S, S),
    (F(32, 8192), 'NUTS', 0, S, S),          # (not in step: the lanes rule's 'split' stays)
    (F(32, 8192), 'NUTS', 7, G, G), (F(32, 8192), 'NUTS', 0, G, G),   # (BFHIP_IN_STEP_LAYOUT=group: nothing to turn)
    (F(32, 8192), 'NUTS', LAG + 7, S, W),
    (F(32, 8192), 'HMC', 0, S, G), (F(32, 8191), 'HMC', 0, S, S), (F(32, 8192), 'HMC', LAG, G, G),
    # --- another number of CUs moves every threshold with it
    (ShapeFacts(64, 1024, 128, True, False, False, False), 'NUTS', 12, S, W),
    (ShapeFacts(64, 512, 128, True, False, False, False), 'NUTS', 7, S, W),
    (ShapeFacts(64, 1025, 128, True, False, False, False), 'NUTS', 12, S, S),
]


@pytest.mark.parametrize('i_cell', range(len(CELLS)))
def test_choose_cell_by_cell(i_cell):
    facts, sampler, answer, in_step_layout, want = CELLS[i_cell]
    assert layout.choose(facts, sampler, answer, in_step_layout) == want, CELLS[i_cell]


def test_the_table_reaches_every_layout_for_both_in_step_layouts():
    assert {(c[3], c[4]) for c in CELLS} == {(S, S), (S, G), (S, W), (G, G), (G, W)}


def _spec(d, configs=('linear', 'quadratic'), use_bound=True, **extra):
    return dict(poly=dict(use_bound=use_bound, configs=[dict(order=o) for o in configs], hess=np.eye(d), mu=np.zeros(d)), **extra)


def test_shape_facts_say_what_the_common_surrogate_is():
    from bayesfast_amd import device
    d = 64
    own = dict(use_decay=True, decay_hess=2. * np.eye(d), decay_mu=np.zeros(d))
    shared = dict(use_decay=True, decay_hess=np.eye(d), decay_mu=np.zeros(d))
    moved = dict(use_decay=True, decay_hess=np.eye(d), decay_mu=np.ones(d))
    tr = dict(ranges=np.zeros((d, 2)))
    flags = lambda sp, full=False: tuple(layout.shape_facts(sp, d, 4096, N_CU, full))[3:]
    assert layout.shape_facts(_spec(d), d, 4096, N_CU, False) == ShapeFacts(64, 4096, 256, True, False, False, False)
    assert flags(_spec(d, **own)) == (False, True, True, False)
    assert flags(_spec(d, **shared)) == (False, True, True, True)
    assert flags(_spec(d, **moved)) == (False, True, True, False)
    assert flags(_spec(d, **tr)) == (False, True, False, False)
    assert flags(_spec(d, **dict(shared, **tr))) == (False, False, True, True)    # no pipelined instantiation with both
    assert flags(_spec(d, link=dict(kind='gaussian'))) == (False, False, False, False)
    assert flags(_spec(d, chi2=dict())) == (False, False, False, False)
    assert flags(_spec(d, ('linear', 'quadratic', 'cubic-2'))) == (False, False, False, False)
    assert flags(_spec(d, ('quadratic',))) == (False, False, False, False)
    assert flags(_spec(d, use_bound=False)) == (False, False, False, False)
    assert flags(_spec(d), full=True) == (False, False, False, False)
    assert flags(_spec(d, **shared), full=True) == (False, False, True, True)
    # input scales: folded into the coefficients at upload when the range lies near the origin (device.folds_input_scales)
    assert flags(_spec(d, su_lo=np.full(d, 1.), su_diff=np.ones(d)))[0] == device.FOLD_INPUT_SCALES
    assert flags(_spec(d, su_lo=np.full(d, 100.), su_diff=np.ones(d))) == (False, False, False, False)
    # sharded chains: chains per rank count, not this rank's chains
    assert layout.shape_facts(_spec(d), d, 16384, N_CU, False, 1024.).n_per_rank == 1024.
    assert layout.choose(layout.shape_facts(_spec(d), d, 16384, N_CU, False, 1024.), 'NUTS', 7, S) == W
    assert layout.choose(layout.shape_facts(_spec(d), d, 16384, N_CU, False), 'NUTS', 7, S) == S
    assert layout.choose(layout.shape_facts(_spec(d), d, 1024, N_CU, False, 8192.), 'NUTS', 7, S) == S
    assert layout.choose(layout.shape_facts(_spec(d), d, 1024, N_CU, False), 'NUTS', 7, S) == W


# lower edges of the size classes, restated: the powers of two and three times them, in order (1, 2, 3, 4, 6, 8, 12, 16, ...)
EDGES = np.array(sorted([1 << k for k in range(33)] + [3 << k for k in range(32)])[:64], dtype=np.int64)


def _numpy_answer(window, share):
    """bf_tree_mode_kernel's decision for a window of tree sizes (n_chain, n_rows), and the two histograms its last block reads."""
    blk = np.where((window >= 0) & (window < 4095), window, 4095).astype(np.int64)
    cnt = np.bincount(blk.ravel(), minlength=4096)
    cls = np.clip(np.searchsorted(EDGES, blk.sum(1), side='right') - 1, 0, 63)
    total = int(blk.sum())
    lag = total > 0 and int(EDGES[cls.max()]) * blk.shape[0] >= 4 * total
    want = (max(1, int(cnt.argmax())) if cnt.max() >= share * blk.size else 0) + (4096 if lag else 0)
    return want, cnt.tolist(), np.bincount(cls, minlength=64).tolist()


def test_answer_from_histograms_matches_a_numpy_restatement():
    from bayesfast_amd import _lib
    assert tuple(int(e) for e in EDGES) == layout.LAG_EDGES and _lib.LAG_EDGES is layout.LAG_EDGES
    w = lambda rows: np.array(rows, dtype=np.int64)
    cases = [
        ('uniform', np.full((8, 4), 7), 0.98, 7),
        ('ties: the smallest of equally common sizes', w([[7, 3]] * 4 + [[3, 7]] * 4), 0.5, 3),
        ('ties, share missed', w([[7, 3]] * 8), 0.51, 0),
        ('all sizes zero: reported as 1, nobody lags', np.zeros((8, 4)), 0.98, 1),
        ('zero the most common size', w([[0, 0, 0, 7]] * 8), 0.75, 1),
        ('bucket 4095: sizes beyond it, negative ones and NaN', np.array([[5000., -1., np.nan, 4095.]] * 8), 0.98, 4095),
        ('share met exactly (24 of 32)', w([[7, 7, 7, 3]] * 8), 0.75, 7),
        ('share missed by one tree (23 of 32)', w([[7, 7, 7, 3]] * 7 + [[7, 7, 3, 3]]), 0.75, 0),
        # four chains of sum 1 and one of sum 16: edge 16 x 5 chains = 80 = 4 x 20
        ('laggard edge met exactly', w([[1, 0]] * 4 + [[8, 8]]), 0.6, 4096),
        ('laggard edge missed by one', w([[1, 0]] * 3 + [[1, 1]] + [[8, 8]]), 0.6, 0),
        # (a sum of 23 lies in the class of edge 16: 16 x 5 = 80 < 4 x 27)
        ('laggard judged by its class edge, not its sum', w([[1, 0]] * 4 + [[8, 15]]), 0.3, 1),
        ('a laggard among trees in step', w([[7, 7]] * 63 + [[1023, 1023]]), 0.98, 4096 + 7),
        ('a laggard among trees that differ', w([[3, 7]] * 63 + [[1023, 1023]]), 0.98, 4096),
    ]
    for name, window, share, want in cases:
        ref, sizes, classes = _numpy_answer(window, share)
        assert ref == want, name
        assert layout.answer_from_histograms(sizes, classes, share) == want, name
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(200):
        n_chain, n_rows = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        window = np.where(rng.uniform(size=(n_chain, n_rows)) < rng.choice([0.5, 0.9, 1.]), 7,
                          rng.choice([0, 1, 3, 15, 31, 5000], size=(n_chain, n_rows)))
        if rng.uniform() < 0.5:
            window[0] = rng.choice([15, 63, 255, 4095])
        share = float(rng.choice([0.5, 0.8, 0.85, 0.98]))
        ref, sizes, classes = _numpy_answer(window, share)
        assert layout.answer_from_histograms(sizes, classes, share) == ref
        seen.add(((ref & 4095) > 0, ref >= 4096))
    assert len(seen) == 4


def test_launch_schedule():
    from bayesfast_amd.chains import _launch_schedule
    assert _launch_schedule(None, 300, 500, 0) == [(300, 300)]
    assert _launch_schedule(0, 300, 500, 0) == [(300, 300)]
    assert _launch_schedule(None, 0, 500, 0) == []
    assert _launch_schedule(100, 300, 500, 0) == [(100, 100), (200, 100), (300, 100)]
    assert _launch_schedule(100, 250, 500, 0) == [(100, 100), (200, 100), (300, 100)]     # the last launch is cut at n_run by the caller
    assert _launch_schedule(250., 100, 500, 0) == [(250, 250)]
    assert _launch_schedule([500, 250], 1100, 500, 0) == [(500, 500), (750, 250), (1000, 250), (1250, 250)]
    assert _launch_schedule((3, 0), 5, 500, 0) == [(3, 3), (4, 1), (5, 1)]
    # 'auto': launches of 100 while the chains adapt, then of 250
    assert _launch_schedule('auto', 1500, 500, 0) == [(100, 100), (200, 100), (300, 100), (400, 100), (500, 100), (750, 250), (1000, 250),
                                                      (1250, 250), (1500, 250)]
    assert _launch_schedule('auto', 150, 500, 0) == [(100, 100), (200, 100)]                          # before the end of the warm-up
    assert _launch_schedule('auto', 400, 500, 350) == [(100, 100), (200, 100), (450, 250)]            # across it
    assert _launch_schedule('auto', 500, 500, 500) == [(250, 250), (500, 250)]                        # after it
    assert _launch_schedule('auto', 300, 500, 900) == [(250, 250), (500, 250)]
    assert _launch_schedule('auto', 300, 0, 0) == [(250, 250), (500, 250)]
    with pytest.raises(ValueError):
        _launch_schedule('automatic', 300, 500, 0)


def test_judging_share_by_where_the_launch_lies():
    from bayesfast_amd.chains import _judging_share
    assert _judging_share(300, 400, 500) == 0.8
    assert _judging_share(400, 499, 500) == 0.8
    assert _judging_share(400, 500, 500) == 0.85      # i0 < n_warmup <= i1: the launch that ends the warm-up
    assert _judging_share(499, 500, 500) == 0.85
    assert _judging_share(0, 1500, 500) == 0.85
    assert _judging_share(499, 501, 500) == 0.85
    assert _judging_share(500, 600, 500) == 0.98
    assert _judging_share(750, 1000, 500) == 0.98
    assert _judging_share(0, 100, 0) == 0.98
