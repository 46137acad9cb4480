"""The pipelined NUTS kernel (bfhip_nuts_pipe.h) against bf_sampler_kernel, bit for bit, at the smallest shapes that reach the
statements its instruction trimming touched: the accumulator that is no longer cleared (waves without a job, trips without an
evaluation, all three tile shapes), the weight rescaling next to the inlined draws, the signed step that is carried from
doubling to doubling instead of being rebuilt every trip (direction changes, the depth limit, the step switching from the
warm-up's to the averaged one inside a launch), the level-0 merge's draw, and a launch cut in the middle.

Every comparison covers the samples, all 11 statistics, the scalar and vector state arrays, the random words and the leapfrog
count.

The reference is bf_sampler_kernel wherever it performs the same arithmetic.  It does not for the headline's instantiation
<4, false, 2, *> (the decay term on the bound's matrix at 33 <= d <= 64): there the pipelined kernel splits every matvec's K sum
in two and bf_sampler_kernel, with its three matrices, does not, so the two agree to rounding only -- with
the parent's library too.  The bit-for-bit reference of that instantiation is bf_lone_kernel, which runs the same two-matrix
form (tests/test_gpu_sampler.py::test_lone_kernel_is_bit_identical_to_pipelined_kernel) and which this change does not touch;
the same cases run without the decay term against bf_sampler_kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ('samples', 'stats', 'sc', 'vec', 'rng')


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _gaussian(d, decay=0, **kw):
    """The correlated Gaussian's surrogate; decay = 1: the decay term about a centre of its own (three matrices), decay = 2: about
    the bound's centre with the bound's matrix (two matrices)."""
    from bayesfast_amd.workloads import correlated_gaussian_spec
    spec, _ = correlated_gaussian_spec(d, **kw)
    if decay:
        po = spec['poly']
        spec = dict(spec, use_decay=True, decay_mu=po['mu'] + (0.05 if decay == 1 else 0.), decay_hess=po['hess'],
                    decay_alpha2=(0.8 * po['alpha'])**2, decay_gamma=0.1)
    return spec


def _run(ctx, spec, x0, runs, pipe, cpg=16, step_size=1., seed=11, **kw):
    """The chains through launches of `runs` iterations on the pipelined kernel (pipe = True), on bf_sampler_kernel (False) or on
    bf_lone_kernel ('lone'); returns the arrays of NAMES (outputs of the launches concatenated), the leapfrog count and the name
    of the last kernel."""
    from bayesfast_amd.device import DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    dens = DeviceDensity(spec, ctx)
    try:
        _lib.debug_set('no_group', 1)
        _lib.debug_set('lone', 2 if pipe == 'lone' else 0)   # (0: few chains would go to the latency kernel by themselves)
        _lib.debug_set('tail_relaunch', 0)   # (one kernel per launch: the one under test)
        _lib.debug_set('wave_cpg', 0 if pipe == 'lone' else cpg)
        _lib.debug_set('no_pipe', 0 if pipe else 1)
        dc = DeviceChains(dens, x0, seed=seed, step_size=step_size)
        outs = [dc.run(n, 'NUTS', layout='wave', launch_iters=None, **kw) for n in runs]
        kernel = _lib.last_kernel()
        s = np.concatenate([o[0].cpu().numpy() for o in outs], axis=1)
        st = np.concatenate([o[1].cpu().numpy() for o in outs], axis=1)
        return [s, st] + [t.cpu().numpy() for t in (dc.sc, dc.vec, dc.rng)], dc.total_leapfrog, kernel
    finally:
        _lib.debug_set('no_pipe', 0)
        _lib.debug_set('wave_cpg', 0)
        _lib.debug_set('tail_relaunch', 1)
        _lib.debug_set('lone', 1)
        _lib.debug_set('no_group', 0)


def _same(got, ref):
    for nm, a, b in zip(NAMES, got[0], ref[0]):
        assert np.array_equal(a, b, equal_nan=True), (nm, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:5])
    assert got[1] == ref[1]


def _col(out, name):
    from bayesfast_amd import _lib
    return out[0][1][:, :, _lib.NSTATS.index(name)]


@pytest.mark.parametrize('decay', [0, 1, 2])
@pytest.mark.parametrize('cpg', [4, 8])
@pytest.mark.parametrize('d', [8, 24])
def test_waves_without_a_job_and_trips_without_an_evaluation(ctx, d, cpg, decay):
    """d = 8: two or three of the sixteen waves own a matvec job, d = 24: eight to twelve; 20 chains leave the last workgroup
    partial; four and eight chains per workgroup run the two 4 x 4 x 4 tile forms.  At max_treedepth = 3 every tree has trips
    in which its chain does not evaluate (the last doubling is not speculated past), and a workgroup's last trips evaluate
    nothing at all."""
    spec = _gaussian(d, decay)
    x0 = np.random.default_rng(2).normal(size=(20, d))
    kw = dict(n_warmup=5, max_treedepth=3)
    pipe = _run(ctx, spec, x0, (8,), True, cpg=cpg, **kw)
    assert pipe[2] == 'bf_nuts_pipe_kernel<%d, false, %d, %d>' % ((d + 15) // 16, decay, 1 if cpg == 4 else 2)
    ref = _run(ctx, spec, x0, (8,), False, cpg=cpg, **kw)
    assert 'bf_sampler_kernel' in ref[2]
    _same(pipe, ref)
    assert _col(pipe, 'tree_depth').max() == 3


def test_weight_rescaling(ctx):
    """Chains that start far out on a wide surrogate with a step of 1: the energy of the first trees falls by more than 600
    along the trajectory, so the running offset of the multinomial weights moves (aw > 600) and the weights collected so far
    are rescaled."""
    spec = _gaussian(16, fit_scale=30.)
    x0 = np.random.default_rng(3).normal(size=(16, 16)) * 30.
    kw = dict(n_warmup=3, max_change=1e6)
    pipe = _run(ctx, spec, x0, (6,), True, **kw)
    assert pipe[2] == 'bf_nuts_pipe_kernel<1, false, 0, 0>'
    assert (_col(pipe, 'max_energy_change') < -600.).any() and (_col(pipe, 'tree_size') > 1).any()
    _same(pipe, _run(ctx, spec, x0, (6,), False, **kw))


@pytest.mark.parametrize('depth,n_warmup', [(1, 30), (2, 30), (3, 30), (3, 5)])
@pytest.mark.parametrize('decay', [2, 0])
def test_direction_changes_and_the_depth_limit(ctx, decay, depth, n_warmup):
    """d = 64: the headline's instantiation (the decay term on the bound's matrix) against bf_lone_kernel, and the same without
    the decay term against bf_sampler_kernel.  At max_treedepth = 1 no doubling follows another; at 2 and 3 the doublings change
    direction about every other time and the last one is never speculated past; n_warmup = 5 switches the step from
    exp(log_step) to exp(log_step_bar) inside the launch."""
    spec = _gaussian(64, decay)
    x0 = np.random.default_rng(2).normal(size=(32, 64))
    kw = dict(n_warmup=n_warmup, max_treedepth=depth)
    pipe = _run(ctx, spec, x0, (10,), True, **kw)
    assert pipe[2] == 'bf_nuts_pipe_kernel<4, false, %d, 0>' % decay
    ref = _run(ctx, spec, x0, (10,), 'lone' if decay else False, **kw)
    assert ('bf_lone_kernel<4, false, 2' if decay else 'bf_sampler_kernel') in ref[2]
    _same(pipe, ref)
    assert _col(pipe, 'tree_depth').max() == depth
    if n_warmup == 5:
        w = _col(pipe, 'warmup')
        assert (w[:, :5] == 1.).all() and (w[:, 5:] == 0.).all()


def test_u_turn_in_a_two_leaf_subtree(ctx):
    """A narrow Gaussian (standard deviations 0.05) under a fixed step of 1.6 standard deviations: many second doublings turn
    in their two-leaf subtree, whose check sums belong to the level-0 merge (and to the full-tree check on the same two
    leaves right after it).  Such a tree has depth 2 and three leaves; a tree cannot end by a U-turn any earlier (the first
    doubling is a single leaf).  Its statistics, mean_tree_accept among them, are the reference kernel's."""
    spec = _gaussian(16, scales=np.full(16, 0.05))
    x0 = np.random.default_rng(4).normal(size=(16, 16)) * 0.05
    kw = dict(n_warmup=0)
    pipe = _run(ctx, spec, x0, (8,), True, step_size=0.08, **kw)
    ref = _run(ctx, spec, x0, (8,), False, step_size=0.08, **kw)
    turned = (_col(pipe, 'tree_depth') == 2) & (_col(pipe, 'tree_size') == 3) & (_col(pipe, 'diverging') == 0)
    assert turned.sum() >= 4
    assert np.array_equal(_col(pipe, 'mean_tree_accept')[turned], _col(ref, 'mean_tree_accept')[turned])
    _same(pipe, ref)


def test_a_launch_cut_in_the_middle(ctx):
    """Two launches of 5 iterations leave what one launch of 10 leaves, and what bf_lone_kernel leaves (the headline's
    instantiation; the warm-up ends inside the second launch)."""
    spec = _gaussian(64, 2)
    x0 = np.random.default_rng(2).normal(size=(32, 64))
    kw = dict(n_warmup=7, max_treedepth=3)
    one = _run(ctx, spec, x0, (10,), True, **kw)
    two = _run(ctx, spec, x0, (5, 5), True, **kw)
    assert one[2] == two[2] == 'bf_nuts_pipe_kernel<4, false, 2, 0>'
    _same(two, one)
    ref = _run(ctx, spec, x0, (5, 5), 'lone', **kw)
    assert 'bf_lone_kernel<4, false, 2' in ref[2]
    _same(two, ref)
