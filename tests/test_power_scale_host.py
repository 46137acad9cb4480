"""The host side of power-scaling sensitivity (bayesfast_amd/utils/power_scale.py): no GPU.

1. The host port of ``power_scale`` against the loop-written reference of helpers/power_scale_reference.py at n = 1, 2, 3, 24, 25, 257
   and 4097 (helpers/power_scale_cases.py: a parameter with ties, -inf base weights, a constant component whose u is w): 1e-9 relative,
   the project's figure for a route against a loop reference (ten times what rounding alone does to the reference stays below it:
   ``ROUNDING`` in the cases); the reweighted figures as tests/test_data_reweight_host.py holds them.  The constant component without
   weights gives exact zeros; with weights its u is w up to the rounding of the normalisation, a relative n EPS in every weight, so its
   distances are held to 4 n EPS absolute.
2. The ECDF distance alone at its edges, with weights the test sets.
3. The conjugate normal model: prior N(mu0, s0), likelihood N(ybar | x, sl), 40 000 i.i.d. draws of the exact posterior.  The three
   regimes' diagnoses, and each sensitivity against the quadrature of the exact Gaussian CDFs over the sample's own range.  Over 8 seeds
   (helpers/power_scale_cases.py prints them) the ratio of the host port's sensitivity to the quadrature's was 0.998 to 0.999 in the
   mean, with a standard deviation of 0.008 to 0.038 (``CONJUGATE`` in the cases has every one); the margin is five times the
   regime's and component's own.
4. Exports, errors, the components of a density.
Every test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, 'helpers')):
    if p not in sys.path:
        sys.path.insert(0, p)

import power_scale_cases as pc  # noqa: E402
from power_scale_reference import ecdf_reference  # noqa: E402
from test_data_reweight_host import assert_against  # noqa: E402
from bayesfast_amd.utils.power_scale import power_scale, data_power_scale, PowerScale, ecdf_distance, component_names  # noqa: E402

RTOL = 1e-9
EPS = 2.**-52
RW_FIGS = ('khat', 'ess', 'log_evidence_ratio', 'mean', 'sd', 'mcse_mean')


def flat_reweighted(got):
    """The reweighted figures of a ``PowerScale`` as the (K,) and (K, d) arrays ``assert_against`` reads, K = C A"""
    k, d = got.khat.size, got.mean_base.size
    out = {f: getattr(got, f).reshape(k) for f in ('khat', 'ess', 'log_evidence_ratio', 'flags')}
    out.update({f: getattr(got, f).reshape(k, d) for f in ('mean', 'sd', 'mcse_mean')})
    out.update(mean_base=got.mean_base, sd_base=got.sd_base)
    return out


def assert_power_scale(got, ref, label, n, rtol=RTOL, abs_l=0., abs_cjs=0., floor_last=True):
    """got a ``PowerScale``, ref the reference's dict: NaN patterns and flags exact, the reweighted figures as ``assert_against`` holds
    them, the distances relative (the last component, where ``floor_last``, to 4 n EPS absolute).  A gradient is a difference of two
    means (sds) over sd_base and over dl2 = log2 alpha_hi - log2 alpha_lo: a mean is held to rtol sd_base, an sd to rtol sd, and an sd is
    a few sd_base at the most, so the gradients are held to rtol |.| + 2 (4) rtol / dl2.  ``abs_l`` is what is known of the error of
    the ratios fed to the two, ``abs_cjs`` that over the spread of the ratios: a distance is to first order linear in them."""
    flat = flat_reweighted(got)
    flat['n_tail'] = ref['n_tail']
    assert_against(flat, ref, label, rtol=rtol, abs_l=abs_l, figs=RW_FIGS)
    c, a, d = got.cjs.shape
    l2lo = np.log2(max(v for v in got.alphas if v < 1.))
    l2hi = np.log2(min(v for v in got.alphas if v > 1.))
    for f in ('cjs', 'ks'):
        g, r = getattr(got, f).reshape(c * a, d), np.asarray(ref[f], dtype=np.float64)
        with np.errstate(all='ignore'):
            err = np.abs(g - r)
            print(label, f, 'largest relative error', np.nanmax(err[:-a] / np.abs(r[:-a])) if np.isfinite(r[:-a]).any() else np.nan,
                  'last component: largest |got|', np.nanmax(np.abs(g[-a:])) if np.isfinite(g[-a:]).any() else np.nan)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, f, g, r)
        ok = ~np.isnan(r)
        bound = (rtol + abs_cjs) * np.abs(r)
        if floor_last:
            bound[-a:] = 4 * n * EPS
        assert np.all(err[ok] <= bound[ok]), (label, f, g, r)
    for f in ('sensitivity', 'mean_gradient', 'sd_gradient'):
        g, r = getattr(got, f), np.asarray(ref[f], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, f)
        ok = ~np.isnan(r)
        with np.errstate(all='ignore'):
            err = np.abs(g - r)
        if f == 'sensitivity':
            bound = (rtol + abs_cjs) * np.abs(r)
            if floor_last:
                bound[-1:] = 4 * n * EPS / min(abs(l2lo), l2hi)
        else:
            bound = rtol * np.abs(r) + (2. if f == 'mean_gradient' else 4.) * (rtol + abs_l) / (l2hi - l2lo)
        print(label, f, 'largest error over its bound', np.nanmax(err[ok] / bound[ok]) if ok.any() else np.nan)
        assert np.all(err[ok] <= bound[ok]), (label, f, g, r)


# ---- 1: the host port against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', pc.SIZES)
def test_host_port_matches_the_reference(n):
    x, g, lw = pc.ps_inputs(n)
    for weighted in (False, True):
        ref = pc.ps_reference(n, weighted)
        got = power_scale(x, g, log_weights=lw if weighted else None, alphas=pc.ALPHAS, names=['a', 'b', 'flat'])
        assert isinstance(got, PowerScale) and got.n == n and got.cjs.shape == (3, 4, 3) and got.diagnosis is None
        assert_power_scale(got, ref, 'n=%d w=%d' % (n, weighted), n)
        if not weighted and n > 1:   # every ratio equal, no base weights: u is w bit for bit
            assert np.all(got.cjs[2] == 0.) and np.all(got.ks[2] == 0.) and np.all(got.sensitivity[2] == 0.)
        if n == 1:
            assert np.isnan(got.cjs).all() and np.isnan(got.ks).all()
        # as tensors, in chains
        if n % 3 == 0:
            import torch
            again = power_scale(torch.as_tensor(x.reshape(3, n // 3, 3)), torch.as_tensor(g.reshape(3, n // 3, 3)),
                                log_weights=lw.reshape(3, n // 3) if weighted else None, alphas=pc.ALPHAS)
            assert again.cjs.tobytes() == got.cjs.tobytes() and again.mean.tobytes() == got.mean.tobytes()
    assert ('largest sensitivity' in str(got)) == (n > 1) and 'PowerScale: 3 components x 4 powers' in str(got)


# ---- 2: the distance at its edges ---------------------------------------------------------------------------------------------------------
def test_ecdf_distance_edges():
    """u one-hot on the first and on the last position, u zero on the lowest positions (Q = 0: 0 log 0), u bit-equal to w, ties, one
    and two draws, a constant parameter, a non-finite draw: the host port's distance against the loop reference, NaN patterns exact."""
    rng = np.random.default_rng(3)
    n = 60
    v = np.sort(np.round(rng.standard_normal(n) * 4.) / 4. - 0.3)   # ties, both signs
    w = rng.random(n)
    w /= w.sum()
    first, last, low = np.zeros(n), np.zeros(n), w.copy()
    first[0] = last[-1] = 1.
    low[:20] = 0.
    low /= low.sum()
    tilt = w * np.exp(0.3 * v)
    tilt /= tilt.sum()
    u = np.stack([first, last, low, w, tilt], axis=1)
    j, b, c, k = ecdf_distance(v, w, u)
    for s in range(u.shape[1]):
        ref = ecdf_reference(v, w, u[:, s])
        print('column', s, 'J', j[s], ref['J'], 'bound', b[s], ref['bound'], 'cjs', c[s], ref['cjs'], 'ks', k[s], ref['ks'])
        for got, name in ((j[s], 'J'), (b[s], 'bound'), (c[s], 'cjs'), (k[s], 'ks')):
            assert abs(got - ref[name]) <= RTOL * abs(ref[name]), (s, name)
    assert c[3] == 0. and k[3] == 0. and j[3] == 0.
    assert abs(k[0] - (1. - w[0])) < 1e-15 and abs(k[1] - (1. - w[-1])) < 1e-15 and np.all(c[[0, 1, 2, 4]] > 0.)
    one = ecdf_distance(v[:1], np.ones(1), np.ones((1, 2)))
    assert np.isnan(one[2]).all() and np.isnan(one[3]).all() and np.all(one[1] == 0.)
    two = ecdf_distance(np.array([1., 3.]), np.array([0.5, 0.5]), np.array([[0.25], [0.75]]))
    ref = ecdf_reference(np.array([1., 3.]), np.array([0.5, 0.5]), np.array([0.25, 0.75]))
    assert abs(two[2][0] - ref['cjs']) <= RTOL * ref['cjs'] and two[3][0] == 0.25 and two[1][0] == 2. * 0.75
    const = ecdf_distance(np.full(5, 2.), np.full(5, 0.2), np.full((5, 1), 0.2))
    assert np.isnan(const[2]).all() and np.isnan(const[3]).all()
    bad = ecdf_distance(np.array([0., 1., np.inf]), np.full(3, 1. / 3), np.full((3, 1), 1. / 3))
    assert all(np.isnan(t).all() for t in bad)
    assert all(np.isnan(t) for t in ecdf_reference(np.array([0., 1., np.nan]), np.full(3, 1. / 3), np.full(3, 1. / 3)).values())


def test_degenerate_scenarios_and_draws():
    """A non-finite component value at non-zero weight makes its scenarios NaN (flag 1) and no other; a non-finite draw at non-zero
    weight takes its parameter in every scenario; the same in a row of zero weight is ignored; no row of weight is flag 4."""
    n = 300
    x, g, lw = (np.array(v[:n]) for v in pc.ps_inputs(4097))
    lw[5], lw[9] = -np.inf, 0.1
    g[9, 1] = np.nan
    g[5, 0] = np.inf
    x[5, 0] = np.nan
    x[9, 2] = np.inf
    got = power_scale(x, g, log_weights=lw, alphas=pc.ALPHAS)
    print(got.flags, got.cjs[:, 0])
    assert got.flags[1].tolist() == [1] * 4 and not got.flags[0].any()
    assert np.isnan(got.cjs[1]).all() and np.isnan(got.ks[1]).all() and np.isnan(got.cjs[:, :, 2]).all() and np.isnan(got.mean[:, :, 2]).all()
    assert np.isfinite(got.cjs[0, :, :2]).all() and np.isfinite(got.sensitivity[0, :2]).all()
    none = power_scale(x, g, log_weights=np.full(n, -np.inf), alphas=pc.ALPHAS)
    assert np.all(none.flags >= 4) and np.isnan(none.cjs).all()


# ---- 3: the conjugate normal model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('par', list(pc.CONJUGATE))
def test_conjugate_normal_regimes(par):
    """Measured here (CPU, seed 100): (0, 10, 1, 1) prior 0.00108, likelihood 0.0747, '-'; (0, 1, 3, 1) 0.125 and 0.168, 'prior-data
    conflict'; (0, 1, 0.5, 10) 0.0735 and 0.00125, 'strong prior / weak likelihood'; the ratios to the quadrature 1.016 | 1.001, 1.008 |
    0.999 and 1.002 | 0.997 (prior | likelihood).  Over 8 seeds the ratio's mean is 0.998 to 0.999 and its standard deviation 0.011 |
    0.038, 0.008 | 0.014 and 0.038 | 0.026."""
    want_diag, sd_prior, sd_like = pc.CONJUGATE[par]
    x, g = pc.conjugate_draws(*par, seed=100)
    got = power_scale(x, g, names=['prior', 'likelihood'])
    quad = pc.conjugate_quadrature(*par, lo=x.min(), hi=x.max())
    ratio = got.sensitivity[:, 0] / np.array(quad)
    print(par, 'sensitivity', got.sensitivity[:, 0], 'quadrature', quad, 'ratio', ratio, got.diagnosis, 'khat', got.khat.ravel())
    assert got.diagnosis == [want_diag]
    assert (got.sensitivity[0, 0] > 0.05) == (want_diag != '-') and (got.sensitivity[1, 0] > 0.05) == (want_diag != 'strong prior / weak likelihood')
    assert abs(ratio[0] - 1.) <= 5. * sd_prior and abs(ratio[1] - 1.) <= 5. * sd_like
    assert got.n_khat_bad == 0


# ---- 4: exports, errors, components ---------------------------------------------------------------------------------------------------------
def test_exports_and_errors():
    import bayesfast_amd as bfa
    from bayesfast_amd import utils
    for name in ('power_scale', 'data_power_scale', 'PowerScale'):
        assert name in utils.__all__ and name in bfa.__all__ and getattr(bfa, name) is getattr(utils, name)
    assert hasattr(bfa.Chi2PipelineDensity, 'power_scale') and hasattr(bfa.TraceTuple, 'power_scale')
    x, g, lw = pc.ps_inputs(25)
    for bad in ((1.01, 1.1), (0.9, 0.99), (0.99, 1., 1.01), (1.01,), (-0.5, 1.5), (0.99, np.nan, 1.01)):
        with pytest.raises(ValueError, match='each side of 1'):
            power_scale(x, g, alphas=bad)
    with pytest.raises(ValueError):
        power_scale(x[:, 0], g)
    with pytest.raises(ValueError):
        power_scale(x, g[:-1])
    with pytest.raises(ValueError):
        power_scale(x, g[:, 0])
    with pytest.raises(ValueError):
        power_scale(x[:0], g[:0])
    with pytest.raises(ValueError):
        power_scale(x, g, log_weights=lw[:-1])
    with pytest.raises(ValueError):
        power_scale(x, g, names=['a', 'b'])
    with pytest.raises(ValueError):
        power_scale(x, g, names=['a', 'a', 'b'])
    got = power_scale(x, g[:, :2], names=['likelihood', 'prior'], threshold=0.)
    assert got.names == ['likelihood', 'prior'] and len(got.diagnosis) == 3 and got.threshold == 0.


def test_components_of_a_density():
    """A density without a prior has no 'prior' component; ``prior_each`` names the inputs with a prior; draws on the host are refused."""
    import bayesfast_amd as bfa
    d, m = 4, 3
    su = bfa.PolyModel('quadratic', input_size=d, output_size=m)
    plain = bfa.Chi2PipelineDensity(su, np.zeros(m), prec_diag=np.ones(m))
    assert component_names(plain) == ['likelihood'] and component_names(plain, True) == ['likelihood']
    some = bfa.Chi2PipelineDensity(su, np.zeros(m), prec_diag=np.ones(m), prior_mu=np.zeros(d), prior_prec=np.array([0., 2., 0., 0.5]))
    assert component_names(some) == ['likelihood', 'prior']
    assert component_names(some, True) == ['likelihood', 'prior', 'prior[1]', 'prior[3]']
    none = bfa.Chi2PipelineDensity(su, np.zeros(m), prec_diag=np.ones(m), prior_mu=np.zeros(d), prior_prec=np.zeros(d))
    assert component_names(none, True) == ['likelihood']
    with pytest.raises(NotImplementedError, match='GPU tensor'):
        data_power_scale(some, np.zeros((10, d)))
    with pytest.raises(ValueError):
        data_power_scale(object(), np.zeros((10, d)))
    # without a 'prior' component there is no diagnosis
    x, g, _ = pc.ps_inputs(25)
    assert power_scale(x, g[:, :1], names=['likelihood']).diagnosis is None
