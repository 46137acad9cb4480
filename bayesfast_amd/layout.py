"""Which of the three sampler families a launch of ``DeviceChains.run(layout='auto')`` runs: the policy, as pure functions.

The layouts (``bfhip_sampler_config.chain_layout``, include/bfhip.h): 'group' (lane per chain, 16 chains per workgroup: fastest
while the chains of a workgroup stay in step), 'split' (the same with integrator and bookkeeper waves, NUTS on the plain surrogate;
where the library has no such kernel it runs 'group', with the same results bit for bit) and 'wave' (wave per chain: insensitive to
chains out of step, and the only one whose launches have a second part for chains that lag far behind).

``choose`` decides per launch from three things only, never from host timing:

* the shapes and the uploaded arrays (``ShapeFacts``, built once per ``run()`` by ``shape_facts``);
* the answer of an EARLIER launch to "did the chains run in step?" (``DeviceChains._trees_in_step``: the common tree size when at
  least 98 % of the NUTS trees of that launch's last 32 iterations had one and the same size -- 85 % for the launch that ends the
  warm-up, 80 % inside it --, + 4096 when some chain builds trees many times the common size, 0 otherwise and for the first
  launches; ``bf_tree_mode_kernel`` computes it on the device, ``answer_from_histograms`` restates it for chains sharded over ranks);
* what runs while the trees are in step (``BFHIP_IN_STEP_LAYOUT``: 'split', or 'group').

The rules override each other in this order, the later one winning:

1. trees in step (static HMC: always) -> the in-step layout; otherwise 'wave';
2. NUTS, trees in step but deep (``deep_trees_prefer_waves``) -> 'wave';
3. NUTS, a small problem (``small_problem``) -> 'wave', whatever the trees; or else, many chains at a small dimension
   (``lanes_whatever_the_trees``) -> the in-step layout, whatever the trees;
4. NUTS, some chain lags far behind the rest -> 'wave';
5. 'split' with the trees in step where two groups fit a CU (``two_groups_fit_a_cu``) -> 'group'.

An explicit ``layout`` and ``BFHIP_FORCE_LAYOUT`` bypass all of it (``DeviceChains.run``)."""
from collections import namedtuple

from ._lib import LAG_EDGES
from .device import folds_input_scales
from .workloads import decay_shares_bound

__all__ = ['ShapeFacts', 'shape_facts', 'choose', 'answer_from_histograms']

# What the rules read.  plain / featured: the common surrogate (linear + quadratic configs with the bound) with nothing else / with the
# decay term OR the constraint transform (the feature sets the pipelined wave-per-chain kernel has instantiations for); n_per_rank:
# chains per rank (sharded: the ranks' average, equal on all of them); decay_shared: the decay term's matrix and centre are the bound's.
ShapeFacts = namedtuple('ShapeFacts', 'd n_per_rank n_cu plain featured decay decay_shared')


def shape_facts(spec, d, n_chain, n_cu, full_metric, n_chain_rule=None):
    """The facts of a density spec and ``n_chain`` chains on a device of ``n_cu`` CUs; ``n_chain_rule`` (sharded chains: the ranks'
    average) counts in their place where it is set.  The one place that says what "the common surrogate" is.  A function of the
    shapes and the uploaded arrays only."""
    # (input scaling of a linear + quadratic surrogate is folded into its coefficients at upload: device.density_desc_from_spec)
    common = ((spec.get('su_lo') is None or folds_input_scales(spec)) and spec.get('link') is None and spec.get('chi2') is None and
              bool(spec['poly'].get('use_bound')) and
              sorted(c['order'] for c in spec['poly']['configs']) == ['linear', 'quadratic'] and not full_metric)
    dec, tr = bool(spec.get('use_decay')), spec.get('ranges') is not None
    return ShapeFacts(d, n_chain if n_chain_rule is None else n_chain_rule, n_cu, common and not dec and not tr, common and (dec != tr),
                      dec, dec and decay_shares_bound(spec))


def small_problem(f):
    """NUTS where the wave-per-chain kernel beats the lane-per-chain layouts although the trees are in step: the latter have
    d / 16 (group) or 2 d / 16 (split) waves per workgroup of 16 chains, so few chains leave most of a CU idle, while the
    wave-per-chain kernel spreads fewer chains per workgroup over more CUs (bfhip_sampler.hip: wave_layout_cpg).  Measured,
    in-step 7-leaf trees (tools/layout_ab.py, profiles/r03s_layout_ab.log), wave against the best lane-per-chain layout: d = 32
    (split, two + two waves): 1024 chains 3.2 against 3.0 x 10^8, 2048 5.5 against 6.0, 4096 8.2 against 12.1; d = 16 (split,
    one + one wave): 1024 2.75 against 2.80, 4096 7.5 against 11.0; d = 64: the split layout ahead from 2048 chains.  With the
    decay term or behind the constraint transform the lane-per-chain layout is the group kernel (no split instantiation) and the
    pipelined kernel stays ahead up to eight chains per CU (tools/dispatch_sweep.py, profiles/r04e_dispatch_sweep.log: d = 32
    x 1024 chains 3.3 against 2.2 x 10^8 with the decay term, 2.4 against 1.5 bounded; d = 64 x 1024 3.0 against 2.5 and 2.3
    against 1.4; at sixteen chains per CU the group kernel wins everywhere).  A function of the shapes only (never of timing)."""
    if f.featured:
        return f.d <= 64 and f.n_per_rank <= 8 * f.n_cu
    if not f.plain:   # (everything else runs the sliced kernel in the wave layout and the group kernel in step)
        return False
    # (32 < d <= 64: with at most four chains per workgroup -- n <= 4 x CUs, wave_layout_cpg -- the pipelined kernel's jobs run
    # on 4 x 4 x 4 MFMA tiles: 1024 chains 3.7 against the split layout's 2.9 x 10^8, 512 chains 1.9 against 1.5)
    # (round 5: up to four chains per CU at d <= 32 the wave layout is the latency kernel, csrc/bfhip_lone.h -- d = 16 x 1024 chains
    # 4.8 against the split layout's 2.8 x 10^8, profiles/r05_lone_sweep.log -- so four chains per CU are "small" at d <= 16 too)
    return ((f.d <= 16 and f.n_per_rank <= 4 * f.n_cu) or (16 < f.d <= 32 and f.n_per_rank < 6 * f.n_cu) or
            (32 < f.d <= 64 and f.n_per_rank <= 4 * f.n_cu))


def lanes_whatever_the_trees(f):
    """NUTS on the plain surrogate at d <= 32 with at least sixteen chains per CU: the split layout's trip is short there (one or
    two integrator waves per 16 chains), and it stays ahead of the wave layout when the trees of a group differ -- 7- and 15-leaf
    trees side by side: d = 16 x 4096 chains 12.2 against 8.9 x 10^8, d = 32 14.3 against 9.8; trees of 7 to 63 leaves: 10.6 / 10.5
    against 9.8 (tools/dispatch_sweep.py, profiles/r04e_dispatch_sweep.log).  At eight chains per CU it depends on how different
    the trees are, and the judgement of the last launch decides as everywhere else."""
    return f.plain and f.d <= 32 and f.n_per_rank >= 16 * f.n_cu


def deep_trees_prefer_waves(f):
    """The common surrogate WITH the decay term at 33 <= d <= 64: the group kernel's rate falls with the tree size (every trip runs
    the bound's and the decay's tiles, and a chain outside the decay ellipsoid makes its whole group's trips 60 % longer, which the
    launch then waits for), the pipelined wave-per-chain kernel's does not -- 4096 chains x 64-d, trees in step: 7 leaves 9.7 against
    6.2 x 10^8, 15: 7.7 against 6.6, 31: 6.3 against 7.0, 1022 (config 3's second round): 5.8 -- 3.7 with ONE such chain -- against
    7.4 (tools/layout_ab.py, bench.py --workload banana_decay; docs/EXPERIMENTS.md).  From 24 leaves up 'auto' takes the wave
    layout there.  Behind the constraint transform the group kernel stays ahead (31 leaves: 6.6 against 5.0), and the plain
    surrogate's split kernel too (10.6 against 9.2).  Round 6: where the decay term's matrix is the bound's the wave layout runs two
    matrices (bfhip_nuts_pipe.h, DEC = 2) and wins earlier -- 4096 chains, 15-leaf trees: d = 64 8.1 against 7.8 x 10^8, d = 32 9.0
    against 5.7; 7-leaf trees stay with the group kernel (9.8 against 7.8, 8.2 against 7.9): profiles/r06_dispatch_sweep.log.
    Returns the tree size from which 'auto' takes the wave layout (0: never).  A function of the shapes and the uploaded arrays only."""
    if f.plain and 32 < f.d <= 64 and 4 * f.n_cu < f.n_per_rank <= 8 * f.n_cu:
        # (round 6 sweep, the one cell under 0.9: plain surrogate, 64-d x 2048 chains -- eight chains per CU, where the pipelined
        # kernel's jobs run on 4 x 4 x 4 tiles -- 15-leaf trees: wave 6.1 against split 5.3 x 10^8; 7-leaf trees: 5.9 against 6.1)
        return 12
    if not (f.featured and f.decay):
        return 0
    if 32 < f.d <= 64:
        return 12 if f.decay_shared else 24
    if 16 < f.d <= 32 and f.decay_shared:
        return 12
    return 0


def two_groups_fit_a_cu(f):
    """Trees in step at 17 <= d <= 32 with at least two 16-chain groups per CU: the group kernel's two waves and 75 KB of LDS
    let two groups share a CU, a wave per SIMD, where the split kernel's 83 KB admit one -- 8192 chains x 32-d, 7-leaf trees:
    group 1.78 against split 1.27 x 10^9 leapfrog steps/s; at 4096 chains 0.88 against 1.26, and at d <= 16 the split kernel fits
    three groups and stays ahead (2.42 against 1.41; profiles/r05_groups_per_cu.log).  A function of the shapes only."""
    return f.plain and 16 < f.d <= 32 and f.n_per_rank >= 32 * f.n_cu


def choose(facts, sampler, answer, in_step_layout):
    """The layout of one launch: 'split', 'group' or 'wave'.  ``answer``: what ``DeviceChains._trees_in_step`` returns -- the common
    tree size of the launch that is judged, + 4096 when some chain of it lags far behind, 0 for no answer; ``in_step_layout``:
    'split' or 'group' (``BFHIP_IN_STEP_LAYOUT``).  The order of the rules matters (the module docstring lists it)."""
    tree, laggard = answer & 4095, answer >= 4096
    in_step = sampler == 'HMC' or tree > 0
    lay = in_step_layout if in_step else 'wave'
    if sampler == 'NUTS':
        deep = deep_trees_prefer_waves(facts)
        if deep and tree >= deep:
            lay = 'wave'
        if small_problem(facts):
            lay = 'wave'
        elif lanes_whatever_the_trees(facts):
            lay = in_step_layout
        # Some chain builds trees many times the common size (outside the bound, say, where the surrogate is its linear
        # extrapolation; reported from four times the mean over the window, in step or not): a launch lasts as long as its
        # busiest chain, and only the wave layout's launches have a second part for such chains (bfhip_sampler.hip:
        # launch_nuts_pipe).  64-d x 4096 chains, ONE chain of them outside the bound (16 x the others' leapfrogs): split
        # 2.6 x 10^8 (from 11.8), group 1.7, wave 4.9 (tools/leak_probe.py).
        if laggard:
            lay = 'wave'
    if lay == 'split' and in_step and two_groups_fit_a_cu(facts):
        lay = 'group'
    return lay


def answer_from_histograms(sizes, classes, share):
    """The decision of ``bf_tree_mode_kernel``'s last block, from the same two histograms (summed over the ranks: the sharded branch
    of ``DeviceChains._note_trees``): ``sizes[i]`` trees of size i in the window (4096 buckets; negative, NaN and larger sizes in
    bucket 4095), ``classes[j]`` chains whose window sum lies in size class j (64 classes, lower edges ``LAG_EDGES``), both lists of
    ints.  Returns the most common size -- the smallest among equally common ones, size 0 reported as 1 -- when at least ``share``
    of the trees have it, else 0; + 4096 when some chain lags far behind the rest: the busiest chain's class edge is at least four
    times the mean window sum, in integers."""
    best = max(sizes)
    mode = max(1, sizes.index(best))
    n_all, tot = sum(classes), sum(i * v for i, v in enumerate(sizes))
    top = max(j for j in range(64) if classes[j]) if n_all else 0
    lag = 4096 if (tot > 0 and LAG_EDGES[top] * n_all >= 4 * tot) else 0
    return (mode if best >= share * sum(sizes) else 0) + lag
