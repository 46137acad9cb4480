"""Cases, tolerances and the comparison shared by test_eval_reference_host.py and test_gpu_eval_widths.py: the density specs of
the width x feature-set matrix, their evaluation points and leapfrog states, the measured ``ROUNDING`` table and the one function
that decides whether an output agrees with the extended-precision reference (helpers/eval_reference.py).  Nothing here calls the
code under test; the specs come from helpers/laplace_cases.feature_spec (which builds the bound with the oracle's NumPy
restatement of ``_set_bound``)."""
import copy
import functools

import numpy as np

import eval_reference as er
import laplace_cases as lc

EPS = er.EPS

# both sides of every padding edge of the instantiated widths DP = 16, 32, 64, 128
WIDTHS = (2, 16, 17, 32, 33, 64, 65, 127)
DERIVED = ('linear_only', 'no_bound', 'cubic_no_quad', 'decay_no_bound')
EVAL_FEATURES = tuple(lc.FEATURES) + DERIVED
LEAPFROG_FEATURES = ('quadratic', 'everything', 'decay_shared', 'transform', 'cubic', 'linear_only', 'cubic_no_quad', 'decay_no_bound')

N_EVAL = 53        # three full tiles of 16 points and a ragged one
N_CHAINS = 37
GUARD = 16         # rows past n in every output, filled with NAN_BITS
NAN_BITS = np.uint64(0x7ff8c0de5eed1234)   # a quiet NaN with a payload no computation produces

# ROUNDING.  The float64 C oracle against the longdouble reference on the inputs below (eval_points, leapfrog_state), the
# largest |oracle - reference| / (2^-52 scale) over points, feature sets and both spaces, per width
# (test_eval_reference_host.py::test_rounding_table_is_ten_times_the_measurement recomputes it; docs/EXPERIMENTS.md has the table):
#
#     d    logp    grad    q       p       energy
#      2    1.3     1.18    0.511   0.885   1.57
#     16    1.58    2.05    0.812   1.12    1.54
#     17    1.16    1.94    0.788   1.19    1.13
#     32    1.16    2.46    0.835   1.16    1.36
#     33    1.28    2.33    1.18    1.06    1.52
#     64    1.07    3.15    1.05    1.14    2.54
#     65    1.25    3.28    0.697   1.12    1.94
#    127    1.05    3.14    1.04    1.16    3.21
#
# K = ten times the measurement, to two digits: the margin for a device route that sums in another order (MFMA blocks of four,
# then four lanes).  A tolerance is K 2^-52 scale; there is no free-standing absolute term.
ROUNDING = {
    2: dict(logp=13, grad=12, q=5.1, p=8.8, energy=16),
    16: dict(logp=16, grad=20, q=8.1, p=11, energy=15),
    17: dict(logp=12, grad=19, q=7.9, p=12, energy=11),
    32: dict(logp=12, grad=25, q=8.4, p=12, energy=14),
    33: dict(logp=13, grad=23, q=12, p=11, energy=15),
    64: dict(logp=11, grad=31, q=11, p=11, energy=25),
    65: dict(logp=12, grad=33, q=7, p=11, energy=19),
    127: dict(logp=10, grad=31, q=10, p=12, energy=32),
}
FIGURES = ('logp', 'grad', 'q', 'p', 'energy')


def rounding_for(d):
    """The K of dimension d: the table's entry, or for a d the table does not hold the larger of its two neighbours' of the same
    padded width (the same instantiation: the sums have the padded length)."""
    if d in ROUNDING:
        return ROUNDING[d]
    dp = 16 if d <= 16 else (32 if d <= 32 else (64 if d <= 64 else 128))
    same = [ROUNDING[w] for w in WIDTHS if (dp // 2 if dp > 16 else 0) < w <= dp]
    return {f: max(r[f] for r in same) for f in FIGURES}


def two_digits(v):
    return float('%.2g' % v)


# ---- specs ---------------------------------------------------------------------------------------------------------------------
FILL = 1. + float.fromhex('0x1.6a09e667f3bcdp-26')   # 1 + sqrt(2) 2^-26


def q32(a):
    """a rounded to float32, times FILL, in float64: the same 53-bit number on every host.  feature_spec builds its matrices with
    BLAS and LAPACK (G G^T, inv(cov)), whose last bits differ from one CPU to another, and the largest of a few thousand rounding
    errors -- what ROUNDING records -- is a different number on inputs that differ in their last bits: measured on two hosts,
    logp at d = 127 came out 1.09 and 1.42.  Rounded to 24 bits the inputs are the same numbers wherever they are built (a value
    would have to sit within 1e-14 of a rounding boundary not to be).  The one IEEE multiplication by FILL then fills the
    mantissa again, identically everywhere, so that neither a product of two inputs is exact nor a kernel that stages or loads
    at reduced precision goes unnoticed.  Zeros stay zeros."""
    if isinstance(a, float):
        return float(np.float32(a)) * FILL
    return np.asarray(a, dtype=np.float32).astype(np.float64) * FILL


def _rounded(o):
    """every float and float array of a spec through q32; masks, flags and sizes as they are"""
    if isinstance(o, dict):
        return {k: _rounded(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_rounded(v) for v in o)
    if isinstance(o, float) or (isinstance(o, np.ndarray) and o.dtype.kind == 'f') or isinstance(o, np.floating):
        return q32(float(o) if np.ndim(o) == 0 else o)
    return o


@functools.lru_cache(maxsize=None)
def _feature_spec(d, name):
    spec = _rounded(lc.feature_spec(d, name)[0])
    if name == 'decay_shared':
        assert np.array_equal(spec['decay_hess'], spec['poly']['hess']) and np.array_equal(spec['decay_mu'], spec['poly']['mu'])
    return spec


@functools.lru_cache(maxsize=None)
def spec_for(d, name):
    """The density spec of (d, name), every number through q32: laplace_cases.FEATURES, and four derived ones, one per way a matrix
    can be missing from the staged model pd | S | H | Hd:
      'linear_only'     'quadratic' without its quadratic config, the bound's fields kept (an all-linear PolyModel never applies its
                        bound, modules/poly.py:467, 596-597): pd alone;
      'no_bound'        'quadratic' with the bound off: pd S, nothing behind;
      'cubic_no_quad'   'cubic' without its quadratic config, bound on: pd H, H in S's place, and the cubic stage one matrix earlier;
      'decay_no_bound'  'decay_own' with the bound off: pd S Hd, Hd in H's place.
    The bound's mu, hess and alpha stay in the dict either way: the points are laid out with them.  Treat the result as read-only."""
    if name in lc.FEATURES:
        return _feature_spec(d, name)
    base = {'linear_only': 'quadratic', 'no_bound': 'quadratic', 'cubic_no_quad': 'cubic', 'decay_no_bound': 'decay_own'}[name]
    spec = copy.deepcopy(_feature_spec(d, base))
    if name == 'linear_only':
        spec['poly']['configs'] = [cf for cf in spec['poly']['configs'] if cf['order'] == 'linear']
    elif name == 'cubic_no_quad':
        spec['poly']['configs'] = [cf for cf in spec['poly']['configs'] if cf['order'] != 'quadratic']
    else:
        spec['poly']['use_bound'] = False
    return spec


def bound_is_on(spec):
    po = spec['poly']
    return bool(po.get('use_bound')) and not all(cf['order'] == 'linear' for cf in po['configs'])


def has_transform(spec):
    return spec.get('ranges') is not None


# ---- points --------------------------------------------------------------------------------------------------------------------
INSIDE = (0.3, 0.45, 0.6, 0.75, 0.88, 0.95)     # beta / alpha of the bound along random rays from mu
OUTSIDE = (1.15, 1.25, 1.5, 1.7, 2.0, 2.5)


def _su(spec):
    d = int(spec['d'])
    if spec.get('su_lo') is None:
        return np.zeros(d), np.ones(d)
    return np.asarray(spec['su_lo']), np.asarray(spec['su_diff'])


def ray_points(spec, rho, rng):
    """Original-space points at beta / alpha = rho (n,) of the bound along random directions, clipped to |x_s| <= 4.2 in the
    surrogate's input like feature_spec's own points (strictly inside the hard bounds; the clip may lower beta a little)."""
    po = spec['poly']
    mu, H, alpha = np.asarray(po['mu']), np.asarray(po['hess']), float(po['alpha'])
    z = rng.normal(size=(len(rho), mu.size))
    z /= np.sqrt(np.einsum('ni,ij,nj->n', z, H, z))[:, None]
    lo, diff = _su(spec)
    return lo + diff * np.clip(mu + (np.asarray(rho) * alpha)[:, None] * z, -4.2, 4.2)


def _sided(spec, rng, want_out):
    """One point per entry of want_out (bool), inside or outside the bound as asked, the ratios walking through INSIDE / OUTSIDE."""
    pts, k = [], [0, 0]
    for out in want_out:
        for _ in range(20):
            rho = (OUTSIDE if out else INSIDE)[k[int(out)] % 6]
            k[int(out)] += 1
            x = ray_points(spec, [rho], rng)
            rb, _ = lc.bound_ratio(dict(spec, poly=dict(spec['poly'], use_bound=True)), x, True)
            if (rb[0] > 1.02) == bool(out) and abs(rb[0] - 1.) > 0.02:
                break
        else:
            raise AssertionError('no point on the wanted side')
        pts.append(x[0])
    return np.array(pts)


# tile 0 inside the bound, tile 1 with exactly one point outside (lane 5: fifteen bystanders on the extrapolation path), tile 2
# outside, the ragged tile mixed
EVAL_LAYOUT = np.array([0] * 16 + [0] * 5 + [1] + [0] * 10 + [1] * 16 + [0, 1, 0, 1, 0], dtype=bool)
assert EVAL_LAYOUT.size == N_EVAL


@functools.lru_cache(maxsize=None)
def eval_points(d, name):
    """(x_original (53, d), x_sampling (53, d) or None without a transform, outside (53,) bool): the evaluation matrix's inputs,
    made host-independent like the specs (q32; the sampling-space points are then points of their own, a rounding away from the images of
    the original-space ones)."""
    spec = spec_for(d, name)
    rng = np.random.default_rng(77000 + 131 * d + sum(ord(c) for c in name))
    xo = q32(_sided(spec, rng, EVAL_LAYOUT))
    xs = q32(lc.from_original(spec, xo)) if has_transform(spec) else None
    return xo, xs, EVAL_LAYOUT.copy()


def check_eval_inputs(spec, xo, xs, outside):
    """Conditions on the inputs, asserted before anything is evaluated: the tiles' sides, both sides of every surface the spec has,
    no point within 1e-6 of the decay term's surface (the decay term's gradient jumps there), |x| < 12 in the sampling space."""
    full = dict(spec, poly=dict(spec['poly'], use_bound=True))
    rb, rd = lc.bound_ratio(full, xo, True)
    assert np.array_equal(rb > 1., outside), 'the tiles are not laid out as described'
    assert not outside[:16].any() and outside[16:32].sum() == 1 and outside[32:48].all() and 0 < outside[48:].sum() < 5
    if bound_is_on(spec):
        assert lc.covers_both_sides(spec, rb, rd), 'a surface of the spec has points on one side only'
    if spec.get('use_decay'):
        assert np.any(rd > 1.) and np.any(rd < 1.), 'the decay surface has points on one side only'
        assert np.all(np.abs(rd - 1.) > 1e-6)
    if xs is not None:
        assert np.all(np.abs(xs) < 12.)
        rb2, _ = lc.bound_ratio(full, xs, False)
        assert np.array_equal(rb2 > 1., outside)


@functools.lru_cache(maxsize=None)
def leapfrog_state(d, name):
    """n = 37 chains in the sampling space: start points inside and outside the bound, momenta, per-chain and per-dimension variances
    in [0.5, 2], per-chain step sizes of both signs with chain 7's exactly 0, and the gradient at the start (the reference's:
    an input like the others).  All of them go through q32."""
    spec = spec_for(d, name)
    rng = np.random.default_rng(91000 + 131 * d + sum(ord(c) for c in name))
    xo = _sided(spec, rng, np.arange(N_CHAINS) % 3 == 2)
    q = q32(lc.from_original(spec, xo) if has_transform(spec) else xo)
    p = q32(rng.normal(size=(N_CHAINS, d)))
    var = q32(rng.uniform(0.5, 2., size=(N_CHAINS, d)))
    eps = q32(rng.uniform(0.02, 0.12, size=N_CHAINS) * np.where(np.arange(N_CHAINS) % 2, -1., 1.))
    eps[7] = 0.
    g = q32(np.asarray(er.logp_and_grad(spec, q)[1], dtype=np.float64))
    return dict(q=q, p=p, var=var, eps=eps, grad=g)


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def units(got, ref, scale):
    """Largest |got - ref| / (2^-52 scale); scale (n,) serves every component of a row.  Anything not finite counts as infinite."""
    got, ref, scale = np.asarray(got, er.LD), np.asarray(ref, er.LD), np.asarray(scale, er.LD)
    if got.shape != ref.shape:
        return np.inf
    if got.ndim == 2:
        scale = scale[:, None]
    with np.errstate(all='ignore'):
        u = np.abs(got - ref) / (EPS * scale)
    u = np.where(np.isfinite(u), u, np.inf)
    return float(u.max()) if u.size else 0.


def compare(label, parts, K):
    """parts: [(name, figure of K, got, reference, scale)].  Prints every figure's largest error in units of 2^-52 scale next to its
    K, and returns {name: units}, the list of the names beyond K."""
    seen, bad = {}, []
    for name, fig, got, ref, scale in parts:
        u = units(got, ref, scale)
        seen[name] = u
        if not u <= K[fig]:
            bad.append(name)
    print('%-46s %s' % (label, '  '.join('%s %.3g/%.3g' % (n, seen[n], K[f]) for n, f, _, _, _ in parts)))
    return seen, bad


def eval_parts(got_logp, got_grad, ref):
    """ref = eval_reference.logp_and_grad(...)"""
    return [('logp', 'logp', got_logp, ref[0], ref[2]), ('grad', 'grad', got_grad, ref[1], ref[3])]


def leapfrog_parts(got, ref, velocity=True):
    """got: {q, p, grad, logp, energy[, v]} arrays; ref = eval_reference.leapfrog(...).  The velocity var p takes p's K."""
    names = [('q', 'q'), ('p', 'p'), ('grad', 'grad'), ('logp', 'logp'), ('energy', 'energy')] + ([('v', 'p')] if velocity else [])
    return [(n, f, got[n], ref[n][0], ref[n][1]) for n, f in names]
