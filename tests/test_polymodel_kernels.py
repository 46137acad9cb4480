"""The multi-output surrogate kernels of bayesfast_amd/csrc/bfhip_poly.hip -- ``bfhip_polymodel_eval`` (PolyModel.fun / jac /
fun_and_jac of every output in one launch) and ``bfhip_chi2_stage`` (the Gaussian likelihood of those outputs with the
pipeline's chain rule) -- against a plain extended-precision restatement of the reference's formulas:

- modules/poly.py:430-503 (``_fun_and_jac``, the all-linear exemption from the bound, ``_fj_bound``'s extrapolation),
- modules/_poly.pyx (the linear, quadratic, cubic-2 and cubic-3 forms), evaluated per config on ``x[input_mask]`` and added
  into ``output_mask`` as the reference does -- no scatter into dense or compact tables, nothing shared with oracle/ or
  bayesfast_amd/device.py,
- logp = logp0 - (f - y)^T P (f - y) / 2 and grad = -J^T P (f - y) for the chi-square stage.

The restatement accumulates in np.longdouble and returns, next to every value, the sum of the absolute values of the terms
that make it up (propagated through the bound's radius and projection where a point lies outside it).  Every tolerance is
K * EPS * that sum, K counting the roundings along the longest accumulation of the kernel; ``_check`` also asserts that the
tolerance stays below 1e-10 of the term sum, so that one term of relative size 1e-9 added or dropped cannot pass.

Shapes cover each padded tile width T = DP / 16 in {1, 2, 4, 8} at both of its edges, with and without cubic configs, the
output split over blockIdx.y (ny = m, m % ny != 0 with empty workgroups, ny = 1: computed as the launch computes it and
asserted), ragged 16-point tiles and points inside, outside and far outside the bound within one tile."""
import ctypes as C

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
LD = np.longdouble
D_EDGES = (1, 3, 16, 17, 31, 32, 33, 64, 65, 100, 128)   # T = 1, 1, 1, 2, 2, 2, 4, 4, 8, 8, 8
MAX_REL_TOL = 1e-10


def _tiles(d):
    return 1 if d <= 16 else 2 if d <= 32 else 4 if d <= 64 else 8


# ---- the restatement ------------------------------------------------------------------------------------------------

def _config_fj(order, a, xi, jac=True):
    """One PolyConfig at the points xi (n, k) = x[:, input_mask]: f (n, q), J (n, q, k) for its q outputs.  a is the config's
    coef in longdouble (its absolute values for a majorant, with xi >= 0).  modules/poly.py:330-428, modules/_poly.pyx."""
    if order == 'linear':
        f = a[:, 0][None, :] + np.einsum('ok,nk->no', a[:, 1:], xi)
        j = np.broadcast_to(a[:, 1:], (xi.shape[0],) + a[:, 1:].shape) if jac else None
    elif order == 'quadratic':
        # _quadratic_f: sum_j x_j sum_{k >= j} a[j, k] x_k;  _quadratic_j: 2 a[j, j] x_j + sum_{k<j} a[k, j] x_k + sum_{k>j} a[j, k] x_k
        u = a * np.triu(np.ones(a.shape[1:], dtype=bool))
        t = np.einsum('ojk,nk->noj', u, xi)
        f = np.einsum('noj,nj->no', t, xi)
        j = (t + np.einsum('okj,nk->noj', u, xi)) if jac else None
    elif order == 'cubic-2':
        # _cubic_2_f: sum_j x_j^2 sum_k a[j, k] x_k;  _cubic_2_j: 2 x_j sum_k a[j, k] x_k + sum_k a[k, j] x_k^2
        t = np.einsum('ojk,nk->noj', a, xi)
        f = np.einsum('noj,nj->no', t, xi * xi)
        j = (2. * xi[:, None, :] * t + np.einsum('okj,nk->noj', a, xi * xi)) if jac else None
    elif order == 'cubic-3':
        # _cubic_3_f: sum_{j<k<l} a[j, k, l] x_j x_k x_l;  _cubic_3_j: the three places index j takes in j < k < l
        k = a.shape[1]
        r = np.arange(k)
        w = a * ((r[:, None, None] < r[None, :, None]) & (r[None, :, None] < r[None, None, :]))
        f = np.einsum('noj,nj->no', np.einsum('nojk,nk->noj', np.einsum('ojkl,nl->nojk', w, xi), xi), xi)
        j = (np.einsum('ojkl,nk,nl->noj', w, xi, xi) + np.einsum('okjl,nk,nl->noj', w, xi, xi) +
             np.einsum('oklj,nk,nl->noj', w, xi, xi)) if jac else None
    else:
        raise ValueError(order)
    return f, j


def _poly_fj(poly, x, absolute=False, jac=True):
    """Sum over the configs at the points x (n, d), longdouble: f (n, m), J (n, m, d) (None unless jac)."""
    n, d, m = x.shape[0], int(poly['input_size']), int(poly['output_size'])
    f = np.zeros((n, m), dtype=LD)
    jj = np.zeros((n, m, d), dtype=LD) if jac else None
    for cf in poly['configs']:
        im = np.asarray(cf['input_mask'], dtype=np.int64)
        om = np.asarray(cf['output_mask'], dtype=np.int64)
        a = np.asarray(cf['coef'], dtype=LD)
        fo, jo = _config_fj(cf['order'], np.abs(a) if absolute else a, x[:, im], jac)
        f[:, om] += fo
        if jac:
            jj[:, om[:, None], im] += jo
    return f, jj


def restate_poly(poly, x, jac=True):
    """PolyModel._fun_and_jac at the points x (n, d) -> f (n, m), J (n, m, d) and their term sums sf, sj, all longdouble,
    plus a dict of per-point bound data (beta, outside, kappa).  jac=False: f and sf only (J and sj None).

    Inside the bound (or without it) sf and sj are the sums of |terms| of the polynomial at x.  Outside, every value is a
    function of beta = sqrt((x-mu)^T H (x-mu)) and of the projected point x_0 = mu + alpha (x-mu) / beta: their rounding
    errors are relative kappa EPS, kappa = |x-mu|^T |H| |x-mu| / beta^2, and carry into f and J through the same terms.  So
    the majorant is taken at z = |x_0| + |mu| + alpha |x| / beta (covering x_0's own rounding) and multiplied by kappa, with
    the extrapolation's factors (beta / alpha, the f_mu term, the rank-one update of the Jacobian) applied to it."""
    x = np.asarray(x, dtype=LD)
    n, d = x.shape
    m = int(poly['output_size'])
    want_j = jac
    f, jac = _poly_fj(poly, x, jac=want_j)
    sf, sj = _poly_fj(poly, np.abs(x), absolute=True, jac=want_j)
    info = dict(beta=np.zeros(n, dtype=LD), outside=np.zeros(n, dtype=bool), kappa=np.ones(n, dtype=LD))
    all_linear = all(cf['order'] == 'linear' for cf in poly['configs'])
    if not poly.get('use_bound', False) or all_linear:   # modules/poly.py:467: the all-linear model ignores its bound
        return f, jac, sf, sj, info
    mu = np.asarray(poly['mu'], dtype=LD).reshape(d)
    hess = np.asarray(poly['hess'], dtype=LD).reshape(d, d)
    alpha = LD(float(poly['alpha']))
    f_mu = np.asarray(poly['f_mu'], dtype=LD).reshape(m)
    xm = x - mu
    b2 = np.einsum('ni,ij,nj->n', xm, hess, xm)          # np.dot(np.dot(x - mu, hess), x - mu)
    beta = np.sqrt(np.maximum(b2, 0))
    out = beta > alpha
    info['beta'], info['outside'] = beta, out
    if not out.any():
        return f, jac, sf, sj, info
    xo, xmo, bo = x[out], xm[out], beta[out][:, None]
    x0 = (alpha * xo + (bo - alpha) * mu) / bo             # modules/poly.py:482
    f0, j0 = _poly_fj(poly, x0, jac=want_j)
    ff = (bo * f0 - (bo - alpha) * f_mu) / alpha
    f[out] = ff
    axm = np.abs(xmo)
    kappa = np.einsum('ni,ij,nj->n', axm, np.abs(hess), axm) / np.einsum('ni,ij,nj->n', xmo, hess, xmo)
    info['kappa'][out] = kappa
    z = np.abs(x0) + np.abs(mu) + alpha * np.abs(xo) / bo
    af, aj = _poly_fj(poly, z, absolute=True, jac=want_j)
    k1 = kappa[:, None]
    sf[out] = k1 * (bo / alpha) * (af + np.abs(f_mu))
    if not want_j:
        return f, jac, sf, sj, info
    grad_beta = np.einsum('ij,nj->ni', hess, xmo) / bo     # np.dot(self._hess, x - self._mu) / beta: H, not H^T
    coef = (f0 - f_mu) / alpha - np.einsum('noj,nj->no', j0, xmo) / bo
    jac[out] = j0 + coef[:, :, None] * grad_beta[:, None, :]
    ac = (af + np.abs(f_mu)) / alpha + np.einsum('noj,nj->no', aj, axm) / bo
    ahv = np.einsum('ij,nj->ni', np.abs(hess), axm) / bo
    sj[out] = k1[:, :, None] * (aj + ac[:, :, None] * ahv[:, None, :])
    return f, jac, sf, sj, info


def restate_chi2(f, jac, y, prec=None, prec_diag=None, logp0=0.):
    """logp = logp0 - (f-y)^T P (f-y) / 2, grad = -J^T P (f-y) (core/density.py:552-560 with a Gaussian likelihood), longdouble;
    with the term sums slp, sg.  jac may be None (no gradient)."""
    f = np.asarray(f, dtype=LD)
    y = np.asarray(y, dtype=LD)
    r0 = f - y
    a0 = np.abs(f) + np.abs(y)
    if prec is not None:
        p = np.asarray(prec, dtype=LD)
        r, ar = np.einsum('ok,nk->no', p, r0), np.einsum('ok,nk->no', np.abs(p), a0)
    else:
        p = np.asarray(prec_diag, dtype=LD)
        r, ar = p * r0, np.abs(p) * a0
    logp = LD(logp0) - 0.5 * np.sum(r0 * r, axis=1)
    slp = abs(LD(logp0)) + 0.5 * np.sum(a0 * ar, axis=1)
    if jac is None:
        return logp, None, slp, None, ar
    jac = np.asarray(jac, dtype=LD)
    grad = -np.einsum('nod,no->nd', jac, r)
    sg = np.einsum('nod,no->nd', np.abs(jac), ar)
    return logp, grad, slp, sg, ar


def _acc_len(poly):
    """Summands along the longest accumulation of bfhip_polymodel_eval for one value: the d-term matvec and dot products,
    the cubic configs' loops over their masks, the few combining additions and the extrapolation."""
    d = int(poly['input_size'])
    n2 = max([len(cf['input_mask']) for cf in poly['configs'] if cf['order'] == 'cubic-2'] or [0])
    n3 = max([len(cf['input_mask']) for cf in poly['configs'] if cf['order'] == 'cubic-3'] or [0])
    return d + n2 + 2 * n3 + 8


def _check(got, ref, scale, k, what):
    """|got - ref| <= k EPS scale elementwise (k: twice the roundings along the value's accumulation, from _acc_len & co)."""
    got = np.asarray(got, dtype=LD)
    tol = LD(k * EPS) * np.asarray(scale, dtype=LD)
    rel = np.max(tol / np.maximum(np.asarray(scale, dtype=LD), LD(1e-300)))
    assert rel < MAX_REL_TOL, '%s: tolerance %.3g of the term sums is too loose to see a 1e-9 term' % (what, float(rel))
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(tol, LD(1e-300)), 0)), err.shape)
        raise AssertionError('%s: %d of %d entries off; worst at %s: got %r, want %r, |err| %.3g > tol %.3g (scale %.3g)' % (
            what, int(bad.sum()), bad.size, i, float(got[i]), float(ref[i]), float(err[i]), float(tol[i]), float(scale[i])))


# ---- random models and points ---------------------------------------------------------------------------------------

def _mask(rng, d, k, must=()):
    k = min(k, d)
    keep = [v for v in must if 0 <= v < d]
    rest = np.setdiff1d(np.arange(d), keep)
    pick = rng.choice(rest, size=max(0, k - len(keep)), replace=False) if k > len(keep) else []
    return np.unique(np.concatenate([np.array(keep, dtype=np.int64), np.asarray(pick, dtype=np.int64)]))


def random_poly(rng, d, m, kind, use_bound=True):
    """A PolyModel.poly_spec() dict with random coefficients.
    kind 'linear': one linear config on a mask (missing one input), with a bound that the model must ignore;
         'quad'  : linear + two quadratic configs on masks, their lower triangles filled with noise the reference never reads;
         'cubic' : linear + quadratic + cubic-2 + cubic-3 on masks that reach the last input and cross tile edges, the two
                   cubic configs overlapping on some outputs, and outputs that carry a cubic term only.
    The bound's Hessian is SPD plus an antisymmetric part: beta is unchanged, H (x-mu) and H^T (x-mu) differ."""
    outs = np.arange(m)
    edge = (0, 15, 16, 31, 32, 63, 64, d - 1)
    cfgs = []
    if kind == 'cubic' and m >= 3:
        cub_only = outs[m - max(1, m // 5):]                 # no linear or quadratic config on these
    else:
        cub_only = outs[:0]
    lo = np.setdiff1d(outs, cub_only)
    im = _mask(rng, d, max(1, d - 1)) if kind == 'linear' else np.arange(d)
    cfgs.append(dict(order='linear', input_mask=im, output_mask=lo, coef=rng.normal(size=(lo.size, im.size + 1))))
    if kind in ('quad', 'cubic'):
        half = lo[: max(1, lo.size // 2)]
        for om, k in ((half, max(1, d // 2)), (np.setdiff1d(lo, half), d)):
            if om.size == 0:
                continue
            qm = _mask(rng, d, k, must=edge)
            cfgs.append(dict(order='quadratic', input_mask=qm, output_mask=om,
                             coef=rng.normal(size=(om.size, qm.size, qm.size)) * (0.5 / np.sqrt(qm.size))))
    if kind == 'cubic':
        o2 = np.union1d(outs[: max(1, m // 2)], cub_only)
        m2 = _mask(rng, d, 10, must=edge)
        cfgs.append(dict(order='cubic-2', input_mask=m2, output_mask=o2,
                         coef=rng.normal(size=(o2.size, m2.size, m2.size)) * (0.2 / m2.size)))
        if d >= 3:
            o3 = np.union1d(outs[max(0, m // 2 - 1):], cub_only)   # overlaps o2 on output m//2 - 1 and on cub_only
            m3 = _mask(rng, d, 6, must=(0, 16, 64, d - 1))
            cfgs.append(dict(order='cubic-3', input_mask=m3, output_mask=o3,
                             coef=rng.normal(size=(o3.size,) + (m3.size,) * 3) * 0.2))
    poly = dict(input_size=d, output_size=m, use_bound=bool(use_bound), configs=cfgs)
    if use_bound:
        a = rng.normal(size=(d, d))
        spd = a @ a.T / d + np.eye(d)
        k = rng.normal(size=(d, d)) * 0.3
        poly.update(mu=rng.normal(size=d) * 0.5, hess=spd + (k - k.T), alpha=1.5, f_mu=rng.normal(size=m) * 2.)
    return poly


def random_points(rng, poly, n, far=True):
    """n points: two thirds inside the bound (beta <= 0.9 alpha), a third outside (beta in [1.1, 4] alpha), every 16-point tile
    holding both; some far out (beta / alpha ~ 1e3) and one exactly at mu.  Without a bound: normal points of similar size."""
    d = int(poly['input_size'])
    if 'mu' not in poly:
        return rng.normal(size=(n, d))
    mu, hess, alpha = np.asarray(poly['mu']), np.asarray(poly['hess']), float(poly['alpha'])
    u = rng.normal(size=(n, d))
    u /= np.sqrt(np.einsum('ni,ij,nj->n', u, hess, u))[:, None]
    t = rng.uniform(0.05, 0.9, size=n) * alpha
    i = np.arange(n)
    t[i % 3 == 1] = rng.uniform(1.1, 4., size=int(np.sum(i % 3 == 1))) * alpha
    if far:
        t[i % 16 == 7] = rng.uniform(5e2, 2e3, size=int(np.sum(i % 16 == 7))) * alpha
    x = mu + t[:, None] * u
    if n > 5:
        x[5] = mu
    return x


def _n_cu(ctx):
    import torch
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _ny(n, m, n_cu):
    """The output split of launch_polymodel_eval (bfhip_poly.hip): about four workgroups per CU, at most m."""
    grid = (n + 63) // 64
    return max(1, min(m, (4 * n_cu + grid - 1) // grid))


def _rows(rng, n, m, d, budget=2_000_000):
    """Rows whose Jacobians are compared: all of them when n m d is small, else 200 random rows and the whole last tile."""
    if n * m * d <= budget:
        return np.arange(n)
    last = np.arange(16 * ((n - 1) // 16), n)
    return np.union1d(rng.choice(n, size=200, replace=False), last)


def test_parametrisation_reaches_both_edges_of_every_tile_width():
    """D_EDGES holds, for each padded width T in {1, 2, 4, 8}, the smallest and the largest d the launch maps to it."""
    for t in (1, 2, 4, 8):
        lo, hi = 1 if t == 1 else 8 * t + 1, 16 * t
        assert _tiles(lo) == _tiles(hi) == t and (lo == 1 or _tiles(lo - 1) != t) and (hi == 128 or _tiles(hi + 1) != t)   # (128: BFHIP_MAX_DIM)
        assert lo in D_EDGES and hi in D_EDGES


# ---- CPU: the restatement against the oracle's C restatement --------------------------------------------------------

@pytest.mark.parametrize('kind', ['linear', 'quad', 'cubic'])
@pytest.mark.parametrize('d,m', [(1, 2), (3, 4), (7, 5), (12, 3)])
def test_restatement_matches_oracle_poly_fun_and_jac(kind, d, m):
    """The restatement equals oracle.poly_fun_and_jac (modules/poly.py:430-503 in C, double) to about 1e-13 of the term sums,
    inside, outside and far outside the bound; for the all-linear model the bound is ignored (nothing is extrapolated)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(100 * d + m + len(kind))
    poly = random_poly(rng, d, m, kind)
    x = random_points(rng, poly, 40)
    f, j, sf, sj, info = restate_poly(poly, x)
    assert info['outside'].any() == (kind != 'linear')
    f0, j0 = orc.poly_fun_and_jac(poly, x)
    k = 4 * _acc_len(poly)
    _check(f0, f, sf, k, 'f')
    _check(j0, j, sj, k, 'J')
    if kind == 'linear':   # the bound is there but does not apply: f is affine in x everywhere
        lin = poly['configs'][0]
        fx = np.zeros((x.shape[0], m))
        fx[:, lin['output_mask']] = lin['coef'][:, 0] + x[:, lin['input_mask']] @ lin['coef'][:, 1:].T
        np.testing.assert_allclose(f0, fx, rtol=1e-13, atol=1e-13 * np.abs(fx).max())


def test_restatement_reads_upper_triangles_and_the_extrapolation_terms():
    """The restatement's own semantics, independent of any implementation: a quadratic config's lower triangle and a cubic-3
    config's entries outside j < k < l are never read; outside the bound, f at x is the straight line through (mu, f_mu) and
    (x_0, f(x_0)) and J follows the reference's rank-one update with H, not H^T."""
    rng = np.random.default_rng(3)
    d, m = 6, 3
    poly = random_poly(rng, d, m, 'cubic')
    x = random_points(rng, poly, 32)
    f, j, _, _, info = restate_poly(poly, x)
    noisy = dict(poly, configs=[dict(c) for c in poly['configs']])
    for c in noisy['configs']:
        a = np.array(c['coef'], dtype=np.float64)
        n_ = len(c['input_mask'])
        if c['order'] == 'quadratic':
            a[:, np.tril_indices(n_, -1)[0], np.tril_indices(n_, -1)[1]] += 7.
        elif c['order'] == 'cubic-3':
            r = np.arange(n_)
            a[:, ~((r[:, None, None] < r[None, :, None]) & (r[None, :, None] < r[None, None, :]))] += 5.
        c['coef'] = a
    f2, j2, _, _, _ = restate_poly(noisy, x)
    assert np.array_equal(f, f2) and np.array_equal(j, j2)
    out = np.flatnonzero(info['outside'])
    assert out.size and (~info['outside']).any()
    mu, alpha, hess = np.asarray(poly['mu']), float(poly['alpha']), np.asarray(poly['hess'])
    for i in out[:4]:
        b = float(info['beta'][i])
        x0 = mu + alpha * (x[i] - mu) / b
        fa, ja, _, _, ia = restate_poly(dict(poly, use_bound=False), x0[None, :])
        want = np.asarray(poly['f_mu']) + (fa[0].astype(np.float64) - poly['f_mu']) * b / alpha
        np.testing.assert_allclose(f[i].astype(np.float64), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        gb = hess @ (x[i] - mu) / b
        cf = (fa[0].astype(np.float64) - poly['f_mu']) / alpha - ja[0].astype(np.float64) @ (x[i] - mu) / b
        np.testing.assert_allclose(j[i].astype(np.float64), ja[0].astype(np.float64) + np.outer(cf, gb), rtol=1e-11,
                                   atol=1e-11 * np.abs(j[i]).max())
        cf_t = hess.T @ (x[i] - mu) / b
        assert np.max(np.abs(np.outer(cf, gb) - np.outer(cf, cf_t))) > 1e-3 * np.abs(j[i].astype(np.float64)).max()


@pytest.mark.parametrize('dense', [True, False])
def test_chi2_restatement_matches_oracle_pipeline_density(dense):
    """The two restatements composed equal oracle.logp_and_grad on a pipeline spec (a chi-square stage after a multi-output
    surrogate, no transform or prior), inside and outside the bound, dense and diagonal precision."""
    from oracle import oracle as orc
    rng = np.random.default_rng(7 + dense)
    d, m = 5, 9
    poly = random_poly(rng, d, m, 'cubic')
    x = random_points(rng, poly, 33)
    y = rng.normal(size=m)
    b = rng.normal(size=(m, m))
    prec = b @ b.T / m + np.eye(m) if dense else None
    pdiag = None if dense else rng.uniform(0.5, 2., size=m)
    spec = dict(d=d, ranges=None, hard_bounds=None, su_lo=None, su_diff=None, poly=poly, use_decay=False, link=None,
                chi2=dict(y=y, prec=prec, prec_diag=pdiag, logp0=-3.25), prior=None)
    lp0, g0 = orc.logp_and_grad(spec, x)
    f, j, sf, sj, _ = restate_poly(poly, x)
    lp, g, slp, sg, ar = restate_chi2(f, j, y, prec, pdiag, -3.25)
    k = 4 * (_acc_len(poly) + 2 * m + 4)
    # the surrogate's own errors (k EPS sf, k EPS sj) reach logp through r = P (f - y) and grad through r and P J
    pabs = np.abs(np.asarray(prec, dtype=LD)) if dense else np.diag(np.abs(np.asarray(pdiag, dtype=LD)))
    s_lp, s_g = _composed_sums(sf, sj, j, ar, slp, sg, pabs)
    _check(lp0, lp, s_lp, k, 'logp')
    _check(g0, g, s_g, k, 'grad')


def _composed_sums(sf, sj, j, ar, slp, sg, pabs):
    """Term sums of the surrogate followed by the chi-square stage: an error e_f of f moves logp by r . e_f and grad by
    J^T P e_f, an error e_J of J moves grad by e_J^T r (|r| <= ar elementwise)."""
    s_lp = slp + np.sum(ar * sf, axis=1)
    s_g = sg + np.einsum('nod,no->nd', sj, ar) + np.einsum('nod,no->nd', np.abs(j), np.einsum('ok,nk->no', pabs, sf))
    return s_lp, s_g


# ---- GPU: bfhip_polymodel_eval ---------------------------------------------------------------------------------------

def _ctx():
    from bayesfast_amd.device import get_context
    return get_context(0)


def _compare_eval(dm, poly, x, rng, what):
    """Run the device model on x; check f at every row and J at _rows against the restatement.  Returns f, J (device) and
    the restatement's bound data of every row."""
    import torch
    f_d, j_d = dm.fun_and_jac(x)
    n, m, d = x.shape[0], int(poly['output_size']), int(poly['input_size'])
    k = 4 * _acc_len(poly)
    rows = _rows(rng, n, m, d)
    full = rows.size == n
    f, jr, sf, sjr, info = restate_poly(poly, x, jac=full)
    # kappa (the bound's conditioning) multiplies the term sums outside the bound: it must not loosen them past 1e-10
    assert float(np.max(info['kappa'])) * k * EPS < MAX_REL_TOL, what
    _check(f_d.cpu().numpy(), f, sf, k, what + ': f')
    if not full:
        _, jr, _, sjr, _ = restate_poly(poly, x[rows])
    _check(j_d[torch.as_tensor(rows, device=j_d.device)].cpu().numpy(), jr, sjr, k, what + ': J')
    return f_d, j_d, info


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['linear', 'quad', 'cubic'])
@pytest.mark.parametrize('d', D_EDGES)
def test_polymodel_eval_matches_restatement_at_every_tile_width(d, kind):
    """bfhip_polymodel_eval at each T = DP / 16 on both of its edges (T = 8 reads S from global memory, the others stage it in
    LDS; with cubic configs T = 4 and T = 8 use exactly 64 KB of dynamic LDS), for an all-linear model under a bound it must
    ignore, linear + quadratic on masks with lower-triangle noise, and every config order with overlapping cubic configs and
    cubic-only outputs; 67 points: ragged last tile, inside / outside / far outside the bound in each tile, one at mu."""
    from bayesfast_amd.device import DevicePolyModel
    rng = np.random.default_rng(1000 * d + len(kind))
    m = 7
    poly = random_poly(rng, d, m, kind)
    if kind == 'cubic':
        assert any(c['order'] == 'cubic-2' for c in poly['configs'])
    x = random_points(rng, poly, 67)
    dm = DevicePolyModel(poly, _ctx())
    f_d, j_d, info = _compare_eval(dm, poly, x, rng, 'd=%d %s' % (d, kind))
    if kind == 'linear':
        assert not info['outside'].any()
    else:
        out = info['outside']
        assert out.any() and (~out).any()
        assert all(out[t:t + 16].any() and (~out[t:t + 16]).any() for t in range(0, 64, 16))
        assert np.max(info['beta'] / float(poly['alpha'])) > 400.
    # jac=False: the same f, bit for bit; one point alone
    f2, j2 = dm.fun_and_jac(x, jac=False)
    assert j2 is None and np.array_equal(f2.cpu().numpy(), f_d.cpu().numpy())
    f1, j1 = dm.fun_and_jac(x[7])
    fr, jr, sfr, sjr, _ = restate_poly(poly, x[7:8])
    _check(f1.cpu().numpy(), fr[0], sfr[0], 4 * _acc_len(poly), 'one point: f')
    _check(j1.cpu().numpy(), jr[0], sjr[0], 4 * _acc_len(poly), 'one point: J')


def _batching_cases():
    out = []
    for n in (1, 15, 16, 17, 63, 64, 65):
        out.append((n, 'ny=m'))
    out += [(None, 'ragged'), (None, 'ny=1')]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('d', [17, 65])
@pytest.mark.parametrize('n,regime', _batching_cases())
def test_polymodel_eval_output_split_regimes(n, regime, d):
    """The output split over blockIdx.y, computed here as launch_polymodel_eval computes it from the CU count and asserted:
    ny = m with m >= 100 (one output per workgroup row) at every small n around the 16- and 64-point tiles; m % ny != 0 with
    workgroups whose output range is empty (m = 35, a few thousand points); ny = 1 with every output in one workgroup."""
    from bayesfast_amd.device import DevicePolyModel
    ctx = _ctx()
    n_cu = _n_cu(ctx)
    rng = np.random.default_rng(d * 7 + (n or 0) + len(regime))
    if regime == 'ny=m':
        m = 130
        assert _ny(n, m, n_cu) == m
    elif regime == 'ragged':
        m = 35
        n = next(v for v in range(2000, 20000, 37)
                 if m % _ny(v, m, n_cu) and (_ny(v, m, n_cu) - 1) * -(-m // _ny(v, m, n_cu)) >= m)
        ny = _ny(n, m, n_cu)
        assert m % ny != 0 and (ny - 1) * -(-m // ny) >= m   # the last workgroup row has no outputs
    else:
        m = 5
        n = 64 * 4 * n_cu + 17
        assert _ny(n, m, n_cu) == 1
    poly = random_poly(rng, d, m, 'cubic')
    x = random_points(rng, poly, n)
    _compare_eval(DevicePolyModel(poly, ctx), poly, x, rng, '%s n=%d m=%d d=%d' % (regime, n, m, d))


@pytest.mark.gpu
def test_polymodel_reupload_alternating_models_is_bitwise_stable():
    """Two DevicePolyModels of different T (d = 20, cubic; d = 100, quadratic) used alternately on one context: each
    re-upload gives the bits of its first upload."""
    from bayesfast_amd.device import DevicePolyModel
    ctx = _ctx()
    rng = np.random.default_rng(11)
    pa, pb = random_poly(rng, 20, 9, 'cubic'), random_poly(rng, 100, 4, 'quad')
    xa, xb = random_points(rng, pa, 50), random_points(rng, pb, 50)
    a, b = DevicePolyModel(pa, ctx), DevicePolyModel(pb, ctx)
    fa, ja = [t.cpu().numpy() for t in a.fun_and_jac(xa)]
    fb, jb = [t.cpu().numpy() for t in b.fun_and_jac(xb)]
    fr, _, sfr, _, _ = restate_poly(pa, xa, jac=False)
    _check(fa, fr, sfr, 4 * _acc_len(pa), 'a: f')
    fr, _, sfr, _, _ = restate_poly(pb, xb, jac=False)
    _check(fb, fr, sfr, 4 * _acc_len(pb), 'b: f')
    for _ in range(2):
        f, j = a.fun_and_jac(xa)
        assert np.array_equal(f.cpu().numpy(), fa) and np.array_equal(j.cpu().numpy(), ja)
        f, j = b.fun_and_jac(xb)
        assert np.array_equal(f.cpu().numpy(), fb) and np.array_equal(j.cpu().numpy(), jb)


# ---- GPU: bfhip_chi2_stage --------------------------------------------------------------------------------------------

def _chi2_call(ctx, f, j, y, prec, pdiag, logp0, logp, grad, n=None, m=None, d=None):
    from bayesfast_amd.device import _ptr
    n = f.shape[0] if n is None else n
    m = f.shape[1] if m is None else m
    d = (j.shape[2] if j is not None else 1) if d is None else d
    return ctx._lib.bfhip_chi2_stage(ctx.handle, n, m, d, _ptr(f), _ptr(j), _ptr(y), _ptr(prec), _ptr(pdiag), float(logp0),
                                     _ptr(logp), _ptr(grad))


def _spd(rng, m):
    b = rng.normal(size=(m, m))
    return b @ b.T / m + 0.5 * np.eye(m)


@pytest.mark.gpu
@pytest.mark.parametrize('dense', [True, False])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 128, 457])
def test_chi2_stage_alone_matches_restatement(m, dense):
    """bfhip_chi2_stage on random f and J (no poly kernel before it) at m around the 64-lane stride of the output loop and
    at the DES size, d around the stride of the gradient loop, n in {1, 3, 5, 4097} (4097 where n m d stays moderate),
    dense SPD and diagonal precision; grad = NULL leaves logp unchanged bit for bit."""
    import torch
    from bayesfast_amd import _lib
    ctx = _ctx()
    rng = np.random.default_rng(m * 2 + dense)
    y = rng.normal(size=m)
    prec = _spd(rng, m) if dense else None
    pdiag = None if dense else rng.uniform(0.2, 3., size=m)
    yt, pt = ctx.tensor(y), (ctx.tensor(prec) if dense else None)
    pdt = None if dense else ctx.tensor(pdiag)
    k = 4 * (2 * m + 8)
    for d in (1, 64, 65, 128):
        for n in (1, 3, 5, 4097):
            if n * m * d > 2e7:
                continue
            f = rng.normal(size=(n, m)) + y
            j = rng.normal(size=(n, m, d))
            ft, jt = ctx.tensor(f), ctx.tensor(j)
            lp, g = ctx.empty((n,)), ctx.empty((n, d))
            _lib.check(_chi2_call(ctx, ft, jt, yt, pt, pdt, -1.5, lp, g))
            lp2 = torch.full((n,), np.nan, dtype=torch.float64, device=ctx.device)
            _lib.check(_chi2_call(ctx, ft, None, yt, pt, pdt, -1.5, lp2, None, d=d))
            assert torch.equal(lp, lp2), 'grad = NULL changed logp (m=%d d=%d n=%d)' % (m, d, n)
            rows = np.arange(n) if n * m * max(m if dense else 1, d) <= 4e6 else np.union1d(
                rng.choice(n, 100, replace=False), np.arange(n - 5, n))
            lr, gr, slp, sg, _ = restate_chi2(f[rows], j[rows], y, prec, pdiag, -1.5)
            what = 'm=%d d=%d n=%d %s' % (m, d, n, 'dense' if dense else 'diag')
            _check(lp.cpu().numpy()[rows], lr, slp, k, what + ': logp')
            _check(g.cpu().numpy()[rows], gr, sg, k, what + ': grad')


@pytest.mark.gpu
def test_chi2_stage_scratch_follows_batch_size():
    """Small, then larger (the context's scratch grows), then small again on one context: every result right."""
    from bayesfast_amd import _lib
    ctx = _ctx()
    rng = np.random.default_rng(5)
    m, d = 70, 9
    y, prec = rng.normal(size=m), _spd(rng, m)
    yt, pt = ctx.tensor(y), ctx.tensor(prec)
    for n in (3, 5000, 2, 6001, 7):
        f, j = rng.normal(size=(n, m)), rng.normal(size=(n, m, d))
        lp, g = ctx.empty((n,)), ctx.empty((n, d))
        _lib.check(_chi2_call(ctx, ctx.tensor(f), ctx.tensor(j), yt, pt, None, 0.5, lp, g))
        rows = np.union1d(np.arange(min(n, 40)), np.arange(n - 3, n))
        lr, gr, slp, sg, _ = restate_chi2(f[rows], j[rows], y, prec, None, 0.5)
        _check(lp.cpu().numpy()[rows], lr, slp, 4 * (2 * m + 8), 'n=%d: logp' % n)
        _check(g.cpu().numpy()[rows], gr, sg, 4 * (2 * m + 8), 'n=%d: grad' % n)


def _fixed_pipeline(poly, y, prec=None, prec_diag=None, logp0=0.):
    """A Chi2PipelineDensity whose surrogate is a PolyModel carrying the given coefficients."""
    from bayesfast_amd import PolyModel, PolyConfig, Chi2PipelineDensity

    class _Fixed(PolyModel):
        def poly_spec(self, use_bound=None):
            return poly

    cfgs = [PolyConfig(c['order'], input_mask=np.asarray(c['input_mask']), output_mask=np.asarray(c['output_mask']))
            for c in poly['configs']]
    su = _Fixed(cfgs, input_size=int(poly['input_size']), output_size=int(poly['output_size']))
    return Chi2PipelineDensity(su, y, prec=prec, prec_diag=prec_diag, logp0=logp0)


@pytest.mark.gpu
@pytest.mark.parametrize('d,m,kind', [(27, 457, 'quad'), (128, 130, 'cubic')])
def test_two_kernel_pipeline_route_matches_restatement(d, m, kind):
    """Chi2PipelineDensity.logp_and_grad_device (bfhip_polymodel_eval + bfhip_chi2_stage) at the DES shape (d = 27, m = 457,
    dense precision) and at d = 128, m = 130, inside and outside the bound, against the restatement and against
    oracle.logp_and_grad; at d <= 64 also the fused pipeline density (bfhip_pld), which covers d <= 64 only."""
    from oracle import oracle as orc
    rng = np.random.default_rng(d + m)
    poly = random_poly(rng, d, m, kind)
    poly['hess'] = 0.5 * (poly['hess'] + poly['hess'].T)   # a fitted bound's H = inv(cov); the asymmetric case is tested above
    n = 80 if d < 100 else 40
    x = random_points(rng, poly, n, far=False)
    y = rng.normal(size=m)
    prec = _spd(rng, m)
    den = _fixed_pipeline(poly, y, prec=prec, logp0=2.5)
    lpd, gd = den.logp_and_grad_device(x)
    f, j, sf, sj, info = restate_poly(poly, x)
    assert info['outside'].any() and (~info['outside']).any()
    lp, g, slp, sg, ar = restate_chi2(f, j, y, prec, None, 2.5)
    k = 4 * (_acc_len(poly) + 2 * m + 8)
    s_lp, s_g = _composed_sums(sf, sj, j, ar, slp, sg, np.abs(np.asarray(prec, dtype=LD)))
    _check(lpd.cpu().numpy(), lp, s_lp, k, 'two-kernel logp')
    _check(gd.cpu().numpy(), g, s_g, k, 'two-kernel grad')
    lpo, go = orc.logp_and_grad(den.spec(), x)
    _check(lpo, lp, s_lp, k, 'oracle logp')
    _check(go, g, s_g, k, 'oracle grad')
    lpn, gn = den.logp_and_grad_device(x, grad=False)
    assert gn is None and np.array_equal(lpn.cpu().numpy(), lpd.cpu().numpy())
    if d <= 64:
        # the fused route whitens: P = L L^T is folded into the coefficients, so its rounding is that of |L^T| applied to the
        # term sums (and of the factorisation, |L| |L^T| for P)
        lf, gf = den.logp_and_grad(x)
        lch = np.abs(np.linalg.cholesky(prec)).astype(LD)
        w = np.einsum('ko,nk->no', lch, sf + np.abs(y))
        s_lp_w = s_lp + np.sum(w * w, axis=1)
        s_g_w = s_g + np.einsum('nod,no->nd', sj + np.abs(j), np.einsum('ok,nk->no', lch, w))
        kf = 4 * (_acc_len(poly) + 2 * m + 2 * d + 16)
        _check(lf, lp, s_lp_w, kf, 'fused logp')
        _check(gf, g, s_g_w, kf, 'fused grad')


# ---- refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_polymodel_upload_and_eval_refusals_leave_the_model_usable():
    """Refused uploads (d = 0 or 129, m = 0, use_bound without hess or with alpha <= 0, a mask index >= d, cubic coefficients
    without their mask) and a refused evaluation (n < 0) return BFHIP_ERR_ARG and leave the uploaded model answering with
    the same bits; n = 0 succeeds and writes nothing."""
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DevicePolyModel, polymodel_desc_from_poly, _ptr
    ctx = _ctx()
    L = ctx._lib
    rng = np.random.default_rng(21)
    poly = random_poly(rng, 9, 4, 'cubic')
    x = ctx.tensor(random_points(rng, poly, 20))
    dm = DevicePolyModel(poly, ctx)
    f0, j0 = [t.clone() for t in dm.fun_and_jac(x)]

    def still_same():
        f, j = torch.full_like(f0, np.nan), torch.full_like(j0, np.nan)
        _lib.check(L.bfhip_polymodel_eval(ctx.handle, 20, _ptr(x), _ptr(f), _ptr(j)))
        return torch.equal(f, f0) and torch.equal(j, j0)

    def refused(mutate):
        ds, keep = polymodel_desc_from_poly(poly)
        extra = mutate(ds)
        rc = L.bfhip_polymodel_upload(ctx.handle, C.byref(ds))
        del extra, keep
        return rc

    bad_mask = np.array([0, 1, 9], dtype=np.int32)   # 9 >= d
    cases = {
        'd = 0': lambda ds: setattr(ds, 'd', 0),
        'd = 129': lambda ds: setattr(ds, 'd', 129),
        'm = 0': lambda ds: setattr(ds, 'm', 0),
        'no hess': lambda ds: setattr(ds, 'hess', None),
        'alpha = 0': lambda ds: setattr(ds, 'alpha', 0.),
        'alpha < 0': lambda ds: setattr(ds, 'alpha', -1.),
        'mask2 index >= d': lambda ds: (setattr(ds, 'n2', 3), setattr(ds, 'mask2', bad_mask.ctypes.data_as(C.POINTER(C.c_int)))),
        'mask3 index >= d': lambda ds: (setattr(ds, 'n3', 3), setattr(ds, 'mask3', bad_mask.ctypes.data_as(C.POINTER(C.c_int)))),
        'cubic2 without mask': lambda ds: setattr(ds, 'mask2', None),
        'cubic3 without mask': lambda ds: setattr(ds, 'mask3', None),
    }
    for name, mutate in cases.items():
        assert refused(mutate) == -1, name
        assert still_same(), name
    assert L.bfhip_polymodel_eval(ctx.handle, -1, _ptr(x), _ptr(f0), _ptr(j0)) == -1
    assert still_same()
    f, j = torch.full_like(f0, 7.), torch.full_like(j0, 7.)
    assert L.bfhip_polymodel_eval(ctx.handle, 0, None, _ptr(f), _ptr(j)) == 0
    ctx.synchronize()
    assert bool((f == 7.).all()) and bool((j == 7.).all())


@pytest.mark.gpu
def test_chi2_stage_refusals_and_empty_call():
    """m < 1, d < 1, neither prec nor prec_diag, grad without jac: BFHIP_ERR_ARG; n = 0 succeeds and writes nothing."""
    import torch
    ctx = _ctx()
    rng = np.random.default_rng(8)
    n, m, d = 6, 5, 4
    f, j, y = ctx.tensor(rng.normal(size=(n, m))), ctx.tensor(rng.normal(size=(n, m, d))), ctx.tensor(rng.normal(size=m))
    pd = ctx.tensor(np.ones(m))
    lp, g = torch.full((n,), 7., dtype=torch.float64, device=ctx.device), torch.full((n, d), 7., dtype=torch.float64,
                                                                                       device=ctx.device)
    assert _chi2_call(ctx, f, j, y, None, pd, 0., lp, g, m=0) == -1
    assert _chi2_call(ctx, f, j, y, None, pd, 0., lp, g, d=0) == -1
    assert _chi2_call(ctx, f, j, y, None, None, 0., lp, g) == -1
    assert _chi2_call(ctx, f, None, y, None, pd, 0., lp, g, d=d) == -1
    assert _chi2_call(ctx, f, j, y, None, pd, 0., lp, g, n=0) == 0
    ctx.synchronize()
    assert bool((lp == 7.).all()) and bool((g == 7.).all())
    assert _chi2_call(ctx, f, j, y, None, pd, 0., lp, g) == 0
    ctx.synchronize()
    assert bool(torch.isfinite(lp).all()) and not bool((g == 7.).any())
