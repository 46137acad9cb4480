"""Inputs of the pipeline density's Hessian and maximiser tests (test_gpu_pipeline_hess.py, test_laplace_pipeline_host.py).

Specs come from ``workloads.random_pipeline_spec`` with two changes that make every term of the Hessian live: ``f_mu`` is random
(it is zero there, which leaves the compressed outputs' tail scalars dead), and ``alpha`` is scaled down so that the bound's
ellipsoid lies well inside the unit box of the transform (unscaled it contains the whole box at small d: no point would be
outside).  Nothing here calls the code under test; expected values come from the oracle through laplace_cases."""
import numpy as np

import laplace_cases as lc

# (m, d, nq): the smallest shapes at which each code path of the kernels differs
SHAPES = {
    'no_compression': (5, 9, 4),      # m < nf = 20 monomials, one row tile
    'compressed': (40, 9, 4),         # m > nf: the output space is compressed, the tails k_ff / k_fy are live
    'several_tiles': (100, 27, 9),    # several row and column tiles
    'wide': (24, 70, 6),              # d > 64: five column tiles
    'only8': (40, 27, 27),            # 406 monomials: the eight-chain layout of the upload
}
ALPHA_SCALE = 0.12
RATIOS = ((0.3, 0), (0.5, 1), (0.7, 2), (0.85, 2), (1.3, 3), (1.6, 3), (2.0, 4), (2.6, 5))   # (beta / alpha, ray)


def hess_spec(m, d, nq, seed=2, transform=True, decay=False, prior=True, alpha_scale=ALPHA_SCALE):
    """(spec, points in the original space (n, d)): the points lie at the ratios RATIOS of the bound's radius along random rays, two
    pairs on one ray each.  With ``decay`` a decay term of its own (the keys of laplace_cases.feature_spec), its surface between the
    two points of the pair at 0.7 / 0.85: points on both sides of it inside the bound, all points outside the bound outside it."""
    from bayesfast_amd.workloads import random_pipeline_spec
    spec = random_pipeline_spec(m, d, nq, seed=seed, transform=transform)
    rng = np.random.default_rng(100 * seed + d + m)
    poly = dict(spec['poly'])
    poly['f_mu'] = rng.normal(size=m)
    poly['alpha'] = float(poly['alpha']) * alpha_scale
    spec['poly'] = poly
    if not prior:
        spec['prior'] = None
    mu, H, alpha = np.asarray(poly['mu']), np.asarray(poly['hess']), poly['alpha']
    rays = [rng.normal(size=d) for _ in range(6)]
    rays = [z / np.sqrt(z @ H @ z) for z in rays]
    xs = np.array([mu + rho * alpha * rays[k] for rho, k in RATIOS])
    if transform:
        assert np.all(xs > 0.02) and np.all(xs < 0.98), 'a test point left the unit box'
        lo, diff = spec['su_lo'], spec['su_diff']
    else:
        lo, diff = np.zeros(d), np.ones(d)
    pts = lo + diff * xs
    if decay:
        dmu = lo + diff * (mu + 0.01)
        dH = H / np.outer(diff, diff) * (1. + 0.2 * np.eye(d))
        xm = pts[[2, 3]] - dmu
        bd = np.einsum('ni,ij,nj->n', xm, dH, xm)**0.5
        assert bd[1] > 1.15 * bd[0]
        spec.update(use_decay=True, decay_mu=dmu, decay_hess=dH, decay_alpha2=float(bd[0] * bd[1]), decay_gamma=0.4)
    return spec, pts


def cubic_spec(m, d=7, nq=3, seed=2):
    """hess_spec with a cubic-2 config on three inputs (monomials x_j^2 x_k, x_j^3 among them) and a cubic-3 config on four
    (x_j x_k x_l) added to every output: the monomials of degree three, which random_pipeline_spec does not have."""
    spec, pts = hess_spec(m, d, nq, seed=seed)
    rng = np.random.default_rng(31 * seed + m)
    m2, m3 = np.array([0, 2, 5]), np.array([1, 2, 4, 6])
    a3 = np.zeros((m, 4, 4, 4))
    for j in range(4):
        for k in range(j + 1, 4):
            for l in range(k + 1, 4):
                a3[:, j, k, l] = 0.3 * rng.normal(size=m)
    poly = dict(spec['poly'])
    poly['configs'] = list(poly['configs']) + [
        dict(order='cubic-2', input_mask=m2, output_mask=np.arange(m), coef=0.3 * rng.normal(size=(m, 3, 3))),
        dict(order='cubic-3', input_mask=m3, output_mask=np.arange(m), coef=a3)]
    spec['poly'] = poly
    return spec, pts


def points(spec, pts, original_space):
    """The test points in the asked space, those within 5 % of a C^1 surface dropped; asserts the condition on the inputs: at least
    three inside and three outside the bound (and with a decay term, points on both sides of its surface)."""
    x = pts if original_space else lc.from_original(spec, pts)
    ok, rb, rd = lc.keep_off_the_kinks(spec, x, original_space)
    x, rb, rd = x[ok], rb[ok], rd[ok]
    assert (rb < 1.).sum() >= 3 and (rb > 1.).sum() >= 3
    if spec.get('use_decay'):
        assert (rd < 1.).any() and (rd > 1.).any()
    return x, rb


def maximiser_spec(m, d, nq, seed=2):
    """(spec, x0): the maximiser's density -- random_pipeline_spec as it is (the bound contains the box) but for a random f_mu -- and a
    start near the point that generated y (xs = 1/2, i.e. 0 in the sampling space)."""
    from bayesfast_amd.workloads import random_pipeline_spec
    spec = random_pipeline_spec(m, d, nq, seed=seed)
    rng = np.random.default_rng(7 * seed + d)
    spec['poly'] = dict(spec['poly'], f_mu=rng.normal(size=m))
    return spec, 0.15 * rng.normal(size=d)


def residual_curvature(spec, x):
    """-sum_k r_k d2 f_k at x for a spec without transform and input scales, unit precision, inside the bound: from the spec's
    quadratic coefficients in NumPy."""
    poly = spec['poly']
    d, m = spec['d'], poly['output_size']
    lin = [c for c in poly['configs'] if c['order'] == 'linear'][0]
    quad = [c for c in poly['configs'] if c['order'] == 'quadratic'][0]
    mask = np.asarray(quad['input_mask'])
    Q = np.asarray(quad['coef'])                    # (m, nq, nq), upper triangle: f_k += sum_{j <= l} Q[k, j, l] z_j z_l
    z = x[mask]
    f = lin['coef'][:, 0] + lin['coef'][:, 1:] @ x + np.einsum('kjl,j,l->k', Q, z, z)
    r = f - np.asarray(spec['chi2']['y'])
    assert np.array_equal(np.asarray(spec['chi2']['prec_diag']), np.ones(m))
    D2 = np.zeros((d, d))
    D2[np.ix_(mask, mask)] = np.einsum('k,kjl->jl', r, Q + np.swapaxes(Q, 1, 2))
    return -D2


def streamed_spec(d=64, m=6, seed=5):
    """A full quadratic at d = 64: 2145 monomials, the streamed form of the upload (tests/test_gpu_pipeline_stream.py)."""
    from bayesfast_amd.workloads import random_pipeline_spec
    return random_pipeline_spec(m, d, d, seed=seed)
