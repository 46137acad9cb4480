"""Posterior predictive summaries on the device: ``bfhip_polymodel_columns`` (a batch of the polymodel's outputs at draws read in
place from the chain tensor, bayesfast_amd/csrc/bfhip_poly.hip) through ``DevicePolyModel.fun_columns``, and
``bayesfast_amd.utils.predictive`` on top of it.

Every value is held to the extended-precision restatement of tests/test_polymodel_kernels.py with its own tolerance,
``k EPS (sum of |terms|)``, ``k = 4 * _acc_len(poly)``, and ``_check``'s cap at 1e-10 of the term sum.  The bound radius beta is
held to ``k EPS kappa beta`` with kappa = |x - mu|^T |H| |x - mu| / (x - mu)^T H (x - mu), the conditioning of the quadratic form it
is the root of (computed here for every point; the restatement keeps it for the outside points only).  The tables are compared
byte for byte where the same device values go through the same device routes, and to the restatement within the largest
perturbation of the values (mean, sd and quantiles are 1-Lipschitz in it) plus 64 EPS max|f| for their own arithmetic."""
import ctypes as C

import numpy as np
import pytest

from test_polymodel_kernels import restate_poly, random_poly, random_points, _check, _acc_len, _ctx

EPS = np.finfo(np.float64).eps
LD = np.longdouble
PROBS = (0.16, 0.5, 0.84)

pytestmark = pytest.mark.gpu


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _np(t):
    return t.detach().cpu().numpy()


def _raw_call(ctx, x, k0, nb, out, ldo, lo=None, diff=None, beta=None, since=0, ldr=None, n_draw=None):
    """bfhip_polymodel_columns as the header declares it, on x (n_chain, n_draw, >= d)."""
    import torch
    from bayesfast_amd.device import _ptr
    return ctx._lib.bfhip_polymodel_columns(ctx.handle, int(x.shape[0]), int(x.shape[1] if n_draw is None else n_draw), int(x.stride(0)),
                                            int(x.stride(1) if ldr is None else ldr), _ptr(x), int(x.dtype == torch.float32), since,
                                            _ptr(lo), _ptr(diff), k0, nb, _ptr(out), ldo, _ptr(beta))


def _kappa_all(poly, xs):
    """Conditioning of beta^2 = (x - mu)^T H (x - mu) at every point (1 where x = mu)."""
    xm = np.asarray(xs, dtype=LD) - np.asarray(poly['mu'], dtype=LD)
    h = np.asarray(poly['hess'], dtype=LD)
    num = np.einsum('ni,ij,nj->n', np.abs(xm), np.abs(h), np.abs(xm))
    den = np.einsum('ni,ij,nj->n', xm, h, xm)
    return np.where(den > 0, num / np.where(den > 0, den, 1), 1)


class _Fixed:
    """Holder of the models the tests hand to ``predictive``: a PolyModel that carries the given coefficients."""

    @staticmethod
    def model(poly):
        from bayesfast_amd import PolyModel, PolyConfig

        class _FixedPoly(PolyModel):
            def poly_spec(self, use_bound=None):
                return poly

        cfgs = [PolyConfig(c['order'], input_mask=np.asarray(c['input_mask']), output_mask=np.asarray(c['output_mask']))
                for c in poly['configs']]
        return _FixedPoly(cfgs, input_size=int(poly['input_size']), output_size=int(poly['output_size']))


# ---- 1, 2: values at every tile width, and agreement with the existing kernel ------------------------------------------------------
@pytest.mark.parametrize('variant', ['plain', 'map', 'f32'])
@pytest.mark.parametrize('kind', ['linear', 'quad', 'cubic'])
@pytest.mark.parametrize('d', [3, 17, 33, 65])
def test_columns_match_restatement_at_every_tile_width(d, kind, variant):
    """T = 1, 2, 4, 8; m = 21 in the batches (0, 16), (16, 5) and (5, 3); x (3, 25, d) cut from a (3, 27, d + 2) parent with
    since = 2 (neither stride is the tight one; 75 points leave a ragged last tile), inside / outside / far outside the bound in every
    tile and one point at mu; float64, float64 through an input map, and float32.  Also against bfhip_polymodel_eval on the gathered
    points, within the sum of the two tolerances (whether the two are bit-identical is printed, not asserted)."""
    import torch
    from bayesfast_amd.device import DevicePolyModel
    ctx = _ctx()
    rng = np.random.default_rng(1000 * d + 10 * len(kind) + len(variant))
    m = 21
    poly = random_poly(rng, d, m, kind)
    pts = random_points(rng, poly, 75)
    lo = diff = None
    raw = pts
    if variant == 'map':
        lo, diff = rng.normal(size=d), rng.uniform(0.5, 3., size=d)
        raw = lo + diff * pts
    parent = rng.normal(size=(3, 27, d + 2))
    parent[:, 2:, :d] = raw.reshape(3, 25, d)
    if variant == 'f32':
        parent = parent.astype(np.float32)
    pd = torch.as_tensor(parent, device=ctx.device)
    xv = pd[:, 2:, :d]
    assert xv.stride(0) == 27 * (d + 2) and xv.stride(1) == d + 2 and not xv.is_contiguous()
    seen = parent[:, 2:, :d].reshape(75, d).astype(np.float64)
    xs = (seen - lo) / diff if variant == 'map' else seen            # the NumPy expression the kernel's input map restates
    f, _, sf, _, info = restate_poly(poly, xs, jac=False)
    k = 4 * _acc_len(poly)
    alpha = float(poly['alpha'])
    if kind == 'linear':
        assert not info['outside'].any()
    else:
        b = info['beta'].astype(np.float64)
        assert np.all((b <= 0.95 * alpha) | (b >= 1.05 * alpha)), 'the inside / outside flag is ambiguous'
        out = info['outside']
        assert all(out[t:t + 16].any() and (~out[t:t + 16]).any() for t in range(0, 64, 16)) and out[64:].any() and (~out[64:]).any()
        assert np.max(b / alpha) > 400.
        assert float(np.max(info['kappa'])) * k * EPS < 1e-10
    dm = DevicePolyModel(poly, ctx)
    lo_d = None if lo is None else ctx.tensor(lo)
    diff_d = None if diff is None else ctx.tensor(diff)
    f_ev = _np(dm.fun_and_jac(ctx.tensor(xs), jac=False)[0])
    beta_d = None
    for k0, nb in ((0, 16), (16, 5), (5, 3)):
        got, bt = dm.fun_columns(xv, k0, nb, lo_d, diff_d, beta=True)
        assert tuple(got.shape) == (3, 25, nb) and tuple(bt.shape) == (3, 25)
        g = _np(got).reshape(75, nb)
        what = 'd=%d %s %s (%d, %d)' % (d, kind, variant, k0, nb)
        _check(g, f[:, k0:k0 + nb], sf[:, k0:k0 + nb], k, what)
        _check(g, f_ev[:, k0:k0 + nb].astype(LD), 2 * sf[:, k0:k0 + nb], k, what + ' against bfhip_polymodel_eval')
        print(what, 'bit-identical to bfhip_polymodel_eval:', _bytes_equal(g, f_ev[:, k0:k0 + nb]))
        if beta_d is None:
            beta_d = _np(bt).reshape(75)
        else:
            assert _bytes_equal(beta_d, _np(bt).reshape(75))
    if kind == 'linear':      # the bound is there and does not apply
        assert not beta_d.any()
    else:
        kap = _kappa_all(poly, xs)
        tol = LD(k * EPS) * kap * info['beta']
        assert np.all(np.abs(beta_d.astype(LD) - info['beta']) <= tol), np.max(np.abs(beta_d - info['beta'].astype(np.float64)))
        assert np.array_equal(beta_d > alpha, info['outside'])
        if variant == 'plain':
            assert beta_d[5] == 0.   # the point at mu
    if variant == 'plain':   # the header's own addressing: the parent with since = 2 and ldr = d + 2
        out = torch.full((3, 25, 16), -7., dtype=torch.float64, device=ctx.device)
        from bayesfast_amd import _lib
        _lib.check(_raw_call(ctx, pd, 0, 16, out, 16, since=2, n_draw=25))
        assert torch.equal(out, dm.fun_columns(xv, 0, 16))


# ---- 3: independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,kind', [(5, 'cubic'), (17, 'quad'), (40, 'cubic'), (70, 'quad')])
def test_a_value_depends_on_its_point_and_its_output_only(d, kind):
    import torch
    from bayesfast_amd.device import DevicePolyModel
    ctx = _ctx()
    rng = np.random.default_rng(77 + d)
    poly = random_poly(rng, d, 21, kind)
    x = ctx.tensor(random_points(rng, poly, 75).reshape(3, 25, d))
    dm = DevicePolyModel(poly, ctx)
    a, beta = dm.fun_columns(x, 0, 16, beta=True)
    a = a.clone()
    assert torch.equal(a, dm.fun_columns(x, 0, 16)), 'two identical calls'
    assert torch.equal(a[:, :, 7], dm.fun_columns(x, 7, 1)[:, :, 0]), '(7, 1)'
    assert torch.equal(a[:, :, 7], dm.fun_columns(x, 5, 9)[:, :, 2]), '(5, 9)'
    wide = torch.full((3, 25, 40), -7., dtype=torch.float64, device=ctx.device)
    got = dm.fun_columns(x, 0, 16, out=wide)
    assert got.data_ptr() == wide.data_ptr() and torch.equal(got, a), 'ldo = 40'
    assert bool((wide[:, :, 16:] == -7.).all()), 'columns beyond nb were written'
    wide.fill_(-7.)
    dm.fun_columns(x, 5, 3, out=wide[:, :, 9:])
    assert torch.equal(wide[:, :, 9:12], a[:, :, 5:8]) and bool((wide[:, :, :9] == -7.).all()) and bool((wide[:, :, 12:] == -7.).all())
    alone, b1 = dm.fun_columns(x[1:2], 0, 16, beta=True)
    assert torch.equal(alone, a[1:2]) and torch.equal(b1, beta[1:2]), 'chain 1 alone (another place in its tile)'
    # the launch's size: the same 75 draws at both ends of 300000 (many workgroups, every output group in one workgroup row)
    big = torch.zeros((1, 300000, d), dtype=torch.float64, device=ctx.device)
    big[0, :75] = x.reshape(75, d)
    big[0, -75:] = x.reshape(75, d)
    gb, bb = dm.fun_columns(big, 0, 16, beta=True)
    assert torch.equal(gb[0, :75], a.reshape(75, 16)) and torch.equal(gb[0, -75:], a.reshape(75, 16)), 'launch size'
    assert torch.equal(bb[0, :75], beta.reshape(75)) and torch.equal(bb[0, -75:], beta.reshape(75))


# ---- 4: tables -----------------------------------------------------------------------------------------------------------------------
def _assemble(dm, x, m, **kw):
    import torch
    return torch.cat([dm.fun_columns(x, k0, min(16, m - k0), **kw) for k0 in range(0, m, 16)], dim=2).contiguous()


def _same_table(got, want, rows=None):
    assert got.names == want.names
    for name in want.names:
        w = want[name] if rows is None else want[name][rows]
        assert _bytes_equal(got[name], w), name


@pytest.mark.parametrize('n_draw', [100, 101])
def test_tables_are_the_device_tables_of_the_assembled_outputs(n_draw):
    """Quad model, d = 5, m = 37, x (4, n_draw, 5): ``predictive(...).table`` is ``utils.summary`` (``utils.weighted_summary`` with
    weights) of the (4, n_draw, 37) tensor assembled from ``fun_columns``, byte for byte, whatever the batch width (W = 1, 16, 37)
    and for a scattered selection; and within the values' tolerance of the same statistics of the restatement."""
    import torch
    from bayesfast_amd.utils import predictive, summary, weighted_summary
    ctx = _ctx()
    rng = np.random.default_rng(4 + n_draw)
    d, m, n = 5, 37, 4 * n_draw
    poly = random_poly(rng, d, m, 'quad')
    pts = random_points(rng, poly, n)
    x = ctx.tensor(pts.reshape(4, n_draw, d))
    su = _Fixed.model(poly)
    full = _assemble(su.device_model(), x, m)
    assert tuple(full.shape) == (4, n_draw, m)
    want = summary(full, PROBS)
    for bb, w in ((8 * n, 1), (16 * 8 * n, 16), (1 << 30, 37)):
        from bayesfast_amd.utils.predictive import batch_width
        assert batch_width(bb, n, m) == w
        if n_draw == 101 and w == 1:
            continue   # (37 single-column tables: once is enough)
        res = predictive(su, x, probs=PROBS, batch_bytes=bb)
        _same_table(res.table, want)
        assert res.outputs.tolist() == list(range(m)) and res.chi2 is None and res.ppp is None
    sel = [3, 4, 5, 20, 36]
    _same_table(predictive(su, x, outputs=sel, probs=PROBS).table, want, rows=sel)
    _same_table(predictive(su, x, outputs=[36, 20, 3, 4, 5, 5], probs=PROBS, batch_bytes=2 * 8 * n).table, want, rows=sel)
    lw = rng.normal(size=(4, n_draw))
    lw[rng.random(size=(4, n_draw)) < 0.1] = -np.inf
    want_w = weighted_summary(full, log_weights=torch.as_tensor(lw, device=ctx.device), probs=PROBS)
    for bb in (16 * 8 * n, 1 << 30):
        _same_table(predictive(su, x, log_weights=lw, probs=PROBS, batch_bytes=bb).table, want_w)
    _same_table(predictive(su, x, log_weights=torch.as_tensor(lw, device=ctx.device).reshape(-1), outputs=sel, probs=PROBS).table, want_w,
                rows=sel)
    # against the restatement (``summary`` splits every chain in two halves: of an odd number of draws it leaves the first one out)
    f, _, sf, _, _ = restate_poly(poly, pts, jac=False)
    keep = (np.arange(n) % n_draw) >= (n_draw & 1)
    f, sf = f[keep], sf[keep]
    k = 4 * _acc_len(poly)
    tol = (LD(k * EPS) * sf.max(axis=0) + 64 * EPS * np.abs(f).max(axis=0)).astype(np.float64)
    f64 = f.astype(np.float64)
    ref = dict(mean=f.mean(axis=0).astype(np.float64), sd=f64.std(axis=0, ddof=1))
    for p in PROBS:
        ref['q%g' % (100 * p)] = np.quantile(f64, p, axis=0)
    for name, r in ref.items():
        err = np.abs(want[name] - r)
        print(name, 'largest error / tolerance', float(np.max(err / tol)))
        assert np.all(err <= tol), name


# ---- 5: chi-square, ppp and the out-of-bound share ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [True, False])
def test_chi2_ppp_and_out_of_bound_share(dense):
    import scipy.stats as ss
    import torch
    from bayesfast_amd import Chi2PipelineDensity
    from bayesfast_amd.utils import predictive
    ctx = _ctx()
    rng = np.random.default_rng(50 + dense)
    d, m, n_draw = 5, 37, 100
    n = 4 * n_draw
    poly = random_poly(rng, d, m, 'quad')
    pts = random_points(rng, poly, n, far=False)
    f, _, sf, _, info = restate_poly(poly, pts, jac=False)
    y = (f[rng.integers(n)] + rng.normal(size=m)).astype(np.float64)
    bmat = rng.normal(size=(m, m))
    prec = bmat @ bmat.T / m + 0.5 * np.eye(m) if dense else None
    pdiag = None if dense else rng.uniform(0.2, 3., size=m)
    su = _Fixed.model(poly)
    lo, hi = rng.normal(size=d) - 3., rng.normal(size=d) + 3.
    su.input_scales = np.stack([lo, hi], 1)              # the density's input map: x is in the original space
    x_orig = lo + (hi - lo) * pts
    xs = (x_orig - lo) / (hi - lo)
    f, _, sf, _, info = restate_poly(poly, xs, jac=False)
    b = info['beta'].astype(np.float64)
    assert np.all((b <= 0.95 * float(poly['alpha'])) | (b >= 1.05 * float(poly['alpha'])))
    den = Chi2PipelineDensity(su, y, prec=prec, prec_diag=pdiag, logp0=-3.25)
    x = ctx.tensor(x_orig.reshape(4, n_draw, d))
    # the restated chi-square and its term sums: the stage's own sums and the surrogate's errors carried through r = P (f - y)
    pm_ = np.asarray(prec, dtype=LD) if dense else np.diag(np.asarray(pdiag, dtype=LD))
    r0, a0 = f - y.astype(LD), np.abs(f) + np.abs(y.astype(LD))
    chi2_ref = np.einsum('no,ok,nk->n', r0, pm_, r0)
    ar = np.einsum('ok,nk->no', np.abs(pm_), a0)
    scale = np.sum(a0 * ar, axis=1) + 2 * np.sum(ar * sf, axis=1)
    k = 4 * (_acc_len(poly) + 2 * m + 8)
    lw = rng.normal(size=(4, n_draw))
    lw[rng.random(size=(4, n_draw)) < 0.1] = -np.inf
    first = None
    for bb in (8 * n, 1 << 30):                           # chi-square passes of 64 draws, and of all draws at once
        res = den.predictive(x, outputs=[0, 7], probs=PROBS, batch_bytes=bb)
        c = _np(res.chi2)
        assert c.shape == (4, n_draw)
        _check(c.reshape(-1), chi2_ref, scale, k, 'chi2, batch_bytes %d' % bb)
        if first is None:
            first = c
        assert _bytes_equal(first, c), 'the chunk size changed a chi-square'
        i = int(np.argmin(c.reshape(-1)))
        assert res.chi2_min == c.reshape(-1)[i] and res.best == (i // n_draw, i % n_draw) and res.dof == m
        np.testing.assert_allclose(res.ppp, ss.chi2.sf(c, m).mean(), rtol=1e-9)
        flags = info['outside'].reshape(4, n_draw)
        assert np.array_equal(_np(res.beta) > res.alpha, flags) and res.alpha == float(poly['alpha'])
        assert res.oob_share == flags.mean() and np.array_equal(res.oob_share_chain, flags.mean(axis=1))
        assert 0. < res.oob_share < 1.
        sig = np.asarray(pdiag)**-0.5 if not dense else np.sqrt(np.diag(np.linalg.inv(prec)))
        np.testing.assert_allclose(res.sigma, sig, rtol=1e-12)
        assert np.array_equal(res.y, y) and res.outputs.tolist() == [0, 7]
        assert _bytes_equal(res.pull, (res.table['mean'] - y[[0, 7]]) / res.sigma[[0, 7]])
        from bayesfast_amd.utils import summary
        want = summary(res.chi2[:, :, None], PROBS)
        _same_table(res.chi2_table, want)
        assert 'ppp' in str(res) and len(str(res).splitlines()) <= 6
    res = den.predictive(x, log_weights=lw, outputs=[0], probs=PROBS)
    assert _bytes_equal(_np(res.chi2), first)
    w = np.exp(lw - lw.max())
    np.testing.assert_allclose(res.ppp, (w * ss.chi2.sf(first, m)).sum() / w.sum(), rtol=1e-9)
    np.testing.assert_allclose(res.oob_share, (w * flags).sum() / w.sum(), rtol=1e-12)
    assert np.array_equal(res.oob_share_chain, flags.mean(axis=1))
    masked = np.where(w > 0, first, np.inf).reshape(-1)
    assert res.chi2_min == masked.min() and res.best == divmod(int(np.argmin(masked)), n_draw)


# ---- 6: after sample() -----------------------------------------------------------------------------------------------------------------
def test_trace_predictive_after_sample(monkeypatch):
    """d = 3, m = 5, 4 chains x 60 iterations with 20 of warm-up: ``tt.predictive(density)`` is ``predictive`` on the view
    ``_diag_input`` hands out, byte for byte; the integrate seam's TraceTuple has the method."""
    import bayesfast_amd as bfa
    from bayesfast_amd import parallel
    from bayesfast_amd.utils import predictive
    rng = np.random.default_rng(6)
    d, m = 3, 5
    su = bfa.PolyModel('quadratic', input_size=d, output_size=m)
    xf = rng.normal(size=(4 * su.n_param, d))
    q = rng.normal(size=(m, d, d)) * 0.2
    model = lambda v: np.einsum('ni,kij,nj->nk', v, q, v) + v @ a_lin
    a_lin = rng.normal(size=(d, m))
    yf = model(xf)
    y = model(np.zeros((1, d)) + 0.1)[0]
    den = bfa.Chi2PipelineDensity(su, y, prec_diag=np.full(m, 4.))
    den.fit(xf, -0.5 * 4. * ((yf - y)**2).sum(axis=1), y=yf)
    tt = bfa.sample(den, bfa.NTrace(n_chain=4, n_iter=60, n_warmup=20, x_0=rng.normal(size=(4, d)) * 0.1, random_generator=7),
                    verbose=False)
    view = tt._diag_input(None, False, True, 'samples')
    assert tuple(view.shape) == (4, 40, d) and view.is_cuda
    got, want = tt.predictive(den, probs=PROBS), predictive(den, view, probs=PROBS)
    _same_table(got.table, want.table)
    _same_table(got.chi2_table, want.chi2_table)
    assert _bytes_equal(_np(got.chi2), _np(want.chi2)) and _bytes_equal(_np(got.beta), _np(want.beta))
    assert got.ppp == want.ppp and got.best == want.best and got.oob_share == want.oob_share and got.dof == m
    assert np.isfinite(got.pull).all() and np.isfinite(_np(got.chi2)).all()
    got = tt.predictive(den, since_iter=30, outputs=[1, 2], probs=PROBS)
    _same_table(got.table, predictive(den, tt._diag_input(30, False, True, 'samples'), outputs=[1, 2], probs=PROBS).table)
    assert tuple(got.chi2.shape) == (4, 30)
    from oracle import reference
    if reference.is_built():   # the seam's classes exist only next to the reference package that build() compiles
        from bayesfast_amd import integrate
        assert callable(integrate.reference_classes(reference.load()).TraceTuple.predictive)
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        tt.predictive(den)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_usable():
    import torch
    from bayesfast_amd import _lib
    from bayesfast_amd.device import DeviceContext, DevicePolyModel
    from bayesfast_amd.utils import predictive
    ctx = _ctx()
    rng = np.random.default_rng(9)
    d, m = 9, 6
    poly = random_poly(rng, d, m, 'cubic')
    pts = random_points(rng, poly, 40)
    x = ctx.tensor(pts.reshape(2, 20, d))
    dm = DevicePolyModel(poly, ctx)
    f0 = dm.fun_and_jac(ctx.tensor(pts), jac=False)[0].clone()
    out = torch.full((2, 20, 8), -7., dtype=torch.float64, device=ctx.device)
    lo = ctx.tensor(np.zeros(d))
    cases = {
        'k0 + nb > m': dict(k0=4, nb=3, ldo=8),
        'nb = 0': dict(k0=0, nb=0, ldo=8),
        'in_lo alone': dict(k0=0, nb=4, ldo=8, lo=lo),
        'in_diff alone': dict(k0=0, nb=4, ldo=8, diff=lo),
        'ldo < nb': dict(k0=0, nb=4, ldo=3),
        'ldr < d': dict(k0=0, nb=4, ldo=8, ldr=d - 1),
        'k0 < 0': dict(k0=-1, nb=2, ldo=8),
    }
    for name, kw in cases.items():
        rc = _raw_call(ctx, x, out=out, **kw)
        assert rc == -1, name
        with pytest.raises(ValueError):
            _lib.check(rc)
        assert torch.equal(dm.fun_and_jac(ctx.tensor(pts), jac=False)[0], f0), name
    ctx.synchronize()
    assert bool((out == -7.).all())
    assert _raw_call(ctx, x[:0], 0, 4, out, 8) == 0 and _raw_call(ctx, x, 0, 4, out, 8, n_draw=0) == 0   # nothing to do
    ctx.synchronize()
    assert bool((out == -7.).all())
    other = DeviceContext(0)
    try:
        rc = _raw_call(other, x, 0, 4, out, 8)
        assert rc == -2
        with pytest.raises(RuntimeError):
            _lib.check(rc)
    finally:
        other.close()
    su = _Fixed.model(poly)
    with pytest.raises(NotImplementedError):
        predictive(su, pts.reshape(2, 20, d))
    with pytest.raises(NotImplementedError):
        dm.fun_columns(pts.reshape(2, 20, d), 0, 4)
    with pytest.raises(ValueError):
        predictive(su, x, outputs=[m])
    with pytest.raises(ValueError):
        dm.fun_columns(x, 0, 4, in_lo=lo)
    assert torch.equal(dm.fun_columns(x, 0, m).reshape(40, m), dm.fun_columns(x, 0, m).reshape(40, m))
    _check(_np(dm.fun_columns(x, 0, m)).reshape(40, m), *restate_poly(poly, pts, jac=False)[0:3:2], 4 * _acc_len(poly), 'after the refusals')
