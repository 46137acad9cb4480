"""The NUTS wave kernels after their U-turn tests moved onto the packed sums (bfhip_wave.h: any_le0) and their merge loads were
split by level: the pipelined kernel (bfhip_nuts_pipe.h) and the latency kernel (bfhip_lone.h) against bf_sampler_kernel, which
this change does not touch, bit for bit -- samples, all 11 statistics, the scalar and vector state, the random words and the
leapfrog count (the _run / _same of tests/test_gpu_pipe_trim.py).

Shapes: 16 chains of 8 iterations at max_treedepth = 5 (31 leaves), d = 64, d = 40 (padded lanes) and d = 24 (W = 2), the plain
surrogate and the decay term about a centre of its own (decay = 1).  With decay = 2 at d = 64 (the headline's instantiation)
bf_sampler_kernel agrees to rounding only (tests/test_gpu_pipe_trim.py), so there the pipelined kernel runs against the latency
kernel -- different code calling the same helper -- and the same inputs without the decay term against bf_sampler_kernel.

The target is a Gaussian whose standard deviations spread over a decade, under fixed steps (no warm-up): the fast dimensions turn
inside subtrees while the slow ones go on, so trees end everywhere.  Each case asserts, from the stored statistics, the regimes
it is there for.  With D = tree_depth - 1 the depth at which the last doubling started and k = tree_size - (2^D - 1) its leaves:

  * level 0: k = 2 mod 4 and k < 2^D, not diverging -- the tree ended at a leaf whose only merge is the level-0 one: a U-turn there;
  * level 1: k = 4 mod 8, k < 2^D -- ended at a leaf that closes a four-leaf subtree, by its level-0 merge or by the level-1 merge
    that reads LDS.  The statistics do not say which of the two; but two-leaf merges sit at twice as many leaves with
    k = 2 mod 4 as with k = 4 mod 8, so more trees ending at the latter than at the former (asserted where the counts are
    large) are trees ended by the level-1 merge;
  * level >= 2: k = 0 mod 8, 0 < k < 2^D -- ended at a leaf whose merges go up to a level read from global scratch; and every tree
    of 15 or more leaves has made such a merge and passed it;
  * doubling end: tree_depth = 1 with one leaf, not diverging, under max_treedepth > 1 -- the first doubling has no merge, its
    end turned; and trees of 2^depth - 1 leaves below the depth limit (the end, or the merge of the doubling's two halves);
  * depth limit: tree_depth = max_treedepth with 2^max_treedepth - 1 leaves;
  * a doubling that turned direction: every doubling after the first draws its direction from a fair coin, so trees of
    depth >= 2 each changed direction with probability >= 1/2; at least 20 of them are asserted;
  * outside the bound: samples -- each one a leaf -- with (x - mu)' H (x - mu) > alpha^2 under a bound tightened to 0.4 alpha;
  * a launch's opening evaluation: every launch makes one; one case cuts its launch in two;
  * a trip in which no chain of the workgroup evaluates: at max_treedepth = 1 every tree is one leaf that is never speculated past,
    the sixteen chains stay in step, and every other trip of the workgroup evaluates nothing (where every wave has a matvec job
    the pipelined kernel then multiplies stale operands and must read nothing of it)."""
import numpy as np
import pytest

from test_gpu_pipe_trim import _gaussian, _run, _same, _col

pytestmark = pytest.mark.gpu

MAXD = 5


@pytest.fixture(scope='module')
def ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _spec(d, decay, tight=1.):
    scales = np.logspace(-1., 0., d)
    spec = _gaussian(d, decay, scales=scales)
    if tight != 1.:
        spec = dict(spec)
        spec['poly'] = dict(spec['poly'], alpha=tight * spec['poly']['alpha'])   # (the decay term keeps its radius)
    return spec, np.random.default_rng(2).normal(size=(16, d)) * scales


_REF = {}


def _reference(ctx, key, spec, x0, runs, pipe, **kw):
    """One reference run per set of inputs, shared by the tests that compare against it."""
    if key not in _REF:
        _REF[key] = _run(ctx, spec, x0, runs, pipe, **kw)
    return _REF[key]


def _regimes(outs, maxd=MAXD):
    dp = np.concatenate([_col(o, 'tree_depth').ravel() for o in outs]).astype(int)
    sz = np.concatenate([_col(o, 'tree_size').ravel() for o in outs]).astype(int)
    ok = np.concatenate([_col(o, 'diverging').ravel() for o in outs]) == 0
    D = dp - 1
    k = sz - ((1 << D) - 1)
    mid = ok & (k < (1 << D))
    return dict(level0=int((mid & (k % 4 == 2)).sum()), level1=int((mid & (k % 8 == 4)).sum()),
                level2=int((mid & (k % 8 == 0) & (k > 0)).sum()), scratch_merge=int((sz >= 15).sum()),
                end_first=int((ok & (dp == 1) & (sz == 1)).sum()), end_full=int((ok & (sz == (1 << dp) - 1) & (dp < maxd)).sum()),
                limit=int(((dp == maxd) & (sz == (1 << maxd) - 1)).sum()), deep=int((dp >= 2).sum()), diverging=int((~ok).sum()))


def _outside(out, spec):
    po = spec['poly']
    xm = out[0][0] - np.asarray(po['mu'])
    return int((np.einsum('cni,ij,cnj->cn', xm, np.asarray(po['hess']), xm) > po['alpha']**2).sum())


def _tiles(d):
    return 1 if d <= 16 else (2 if d <= 32 else 4)   # (row tiles of the instantiation: d = 40 runs W = 4 with padded lanes)


def _kernel_name(kind, d, decay):
    w = _tiles(d)
    return ('bf_lone_kernel<%d, false, %d' % (w, decay)) if kind == 'lone' else ('bf_nuts_pipe_kernel<%d, false, %d, 0>' % (w, decay))


# (d, decay, steps, the regimes the case must reach): chosen on the CPU oracle, which builds the same trees; only regimes it reaches
# three times or more are asserted
CASES = [
    (64, 0, (0.8, 1.5), ('level1', 'level2', 'scratch_merge', 'end_full', 'limit', 'diverging')),
    (64, 1, (0.8, 1.9), ('level1', 'scratch_merge', 'end_first', 'end_full', 'limit')),
    (40, 0, (0.8, 1.5), ('level0', 'level1', 'level2', 'scratch_merge', 'end_first', 'end_full', 'limit')),
    (40, 1, (0.8, 1.9), ('level1', 'scratch_merge', 'end_first', 'end_full', 'limit')),
    (24, 0, (0.8, 1.5), ('level0', 'level1', 'level2', 'scratch_merge', 'end_full', 'limit')),
    (24, 1, (0.8, 1.9), ('level0', 'level1', 'scratch_merge', 'end_first', 'end_full', 'limit')),
]


@pytest.mark.parametrize('kind', ['pipe', 'lone'])
@pytest.mark.parametrize('d,decay,steps,want', CASES)
def test_trees_ending_everywhere_against_the_sliced_kernel(ctx, kind, d, decay, steps, want):
    spec, x0 = _spec(d, decay)
    kw = dict(n_warmup=0, max_treedepth=MAXD)
    outs = []
    for step in steps:
        got = _run(ctx, spec, x0, (8,), 'lone' if kind == 'lone' else True, step_size=step, **kw)
        assert _kernel_name(kind, d, decay) in got[2]
        ref = _reference(ctx, ('plain', d, decay, step), spec, x0, (8,), False, step_size=step, **kw)
        assert 'bf_sampler_kernel' in ref[2]
        _same(got, ref)
        outs.append(got)
    r = _regimes(outs)
    print(kind, d, decay, r)
    for name in want:
        assert r[name] > 0, (name, r)
    assert r['deep'] >= 20   # (each a fair coin for a change of direction)
    if decay == 0:
        assert r['level1'] > r['level0']   # (ended by level-1 merges, not only by the level-0 merges of the same leaves: see above)


@pytest.mark.parametrize('kind', ['pipe', 'lone'])
@pytest.mark.parametrize('d,decay,step', [(64, 0, 0.8), (64, 1, 1.5), (40, 1, 1.5), (24, 0, 1.2)])
def test_leaves_outside_the_bound(ctx, kind, d, decay, step):
    """The bound tightened to 0.4 alpha: the chains live outside it, every leaf takes the extrapolation and reads its two sums
    (from the first reduction's packs with the decay term, from a reduction of their own without)."""
    spec, x0 = _spec(d, decay, tight=0.4)
    kw = dict(n_warmup=0, max_treedepth=MAXD)
    got = _run(ctx, spec, x0, (8,), 'lone' if kind == 'lone' else True, step_size=step, **kw)
    assert _kernel_name(kind, d, decay) in got[2]
    ref = _reference(ctx, ('tight', d, decay, step), spec, x0, (8,), False, step_size=step, **kw)
    assert 'bf_sampler_kernel' in ref[2]
    _same(got, ref)
    r = _regimes([got])
    print(kind, d, decay, r, _outside(got, spec))
    assert _outside(got, spec) >= 64 and r['end_full'] > 0 and r['limit'] > 0


@pytest.mark.parametrize('tight,step', [(1., 0.8), (1., 1.0), (0.4, 0.8)])
def test_the_headline_instantiation_against_the_latency_kernel(ctx, tight, step):
    """decay = 2 at d = 64: the decay term on the bound's matrix, bf_nuts_pipe_kernel<4, false, 2, 0> against bf_lone_kernel<4, false,
    2, ..>; the launch of the second case is cut after three iterations in both."""
    spec, x0 = _spec(64, 2, tight)
    kw = dict(n_warmup=0, max_treedepth=MAXD, step_size=step)
    runs = (3, 5) if step == 1.0 else (8,)
    pipe = _run(ctx, spec, x0, runs, True, **kw)
    lone = _run(ctx, spec, x0, runs, 'lone', **kw)
    assert pipe[2] == 'bf_nuts_pipe_kernel<4, false, 2, 0>' and 'bf_lone_kernel<4, false, 2' in lone[2]
    _same(pipe, lone)
    if len(runs) > 1:
        _same(pipe, _run(ctx, spec, x0, (8,), True, **kw))
    r = _regimes([pipe])
    print(tight, step, r, _outside(pipe, spec))
    assert r['scratch_merge'] > 0 and r['deep'] >= 20
    if tight != 1.:
        assert _outside(pipe, spec) >= 64


@pytest.mark.parametrize('cpg', [4, 8, 1])
@pytest.mark.parametrize('d,decay', [(64, 0), (40, 1)])
def test_few_chains_per_workgroup(ctx, d, decay, cpg):
    """The 4 x 4 x 4 tile forms (at most four and at most eight chains of a workgroup): their `job` stays a run-time condition and
    their second operand set alternates like the first."""
    spec, x0 = _spec(d, decay)
    kw = dict(n_warmup=0, max_treedepth=MAXD, step_size=1.5 if decay == 0 else 0.8, cpg=cpg)
    pipe = _run(ctx, spec, x0, (6,), True, **kw)
    assert pipe[2].startswith('bf_nuts_pipe_kernel<%d, false, %d, ' % (_tiles(d), decay)) and not pipe[2].endswith(', 0>')
    if cpg != 1:
        assert pipe[2].endswith(', %d>' % (2 if cpg == 8 else 1))
    ref = _run(ctx, spec, x0, (6,), False, **kw)
    assert 'bf_sampler_kernel' in ref[2]
    _same(pipe, ref)
    r = _regimes([pipe])
    assert r['level1'] > 0 and r['scratch_merge'] > 0 and r['end_full'] > 0


@pytest.mark.parametrize('decay', [0, 2])
def test_trips_in_which_no_chain_evaluates(ctx, decay):
    """max_treedepth = 1 at d = 64, where every wave of the workgroup has a matvec job: sixteen chains in step, every other trip
    without an evaluation.  decay = 2 against the latency kernel, the plain surrogate against bf_sampler_kernel."""
    spec, x0 = _spec(64, decay)
    kw = dict(n_warmup=0, max_treedepth=1, step_size=0.8)
    pipe = _run(ctx, spec, x0, (12,), True, **kw)
    assert pipe[2] == 'bf_nuts_pipe_kernel<4, false, %d, 0>' % decay
    ref = _run(ctx, spec, x0, (12,), 'lone' if decay else False, **kw)
    assert ('bf_lone_kernel<4, false, 2' if decay else 'bf_sampler_kernel') in ref[2]
    _same(pipe, ref)
    assert (_col(pipe, 'tree_size') == 1).all() and (_col(pipe, 'tree_depth') == 1).all()
