"""The inputs that tests/test_power_scale_host.py and tests/test_gpu_power_scale.py share, with their references (computed once and
shared), the conjugate normal model with its quadrature, and what rounding and sampling do to the figures:

    python tests/helpers/power_scale_cases.py

prints, per figure, the largest difference between the float64 and the numpy.longdouble reference over every case, and per regime of
the conjugate model the ratio of the host port's sensitivity to the quadrature's over 8 seeds (no GPU; the tables in
docs/EXPERIMENTS.md, ``ROUNDING`` and ``CONJUGATE`` below come from it)."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from power_scale_reference import power_scale_reference  # noqa: E402

SIZES = (1, 2, 3, 24, 25, 257, 4097)
ALPHAS = (0.7, 0.9, 1.1, 1.4)      # with components of spread 0.1 to 1 the log ratios spread by 0.01 to 0.4 over the draws
FIGS = ('cjs', 'ks', 'sensitivity', 'mean_gradient', 'sd_gradient')
# ten times the largest float64-against-longdouble difference of the reference over ps_reference(n, weighted), n in SIZES, both
# weightings, relative (the gradients in their own units, differences of means over sd_base; the constant component, whose u is w up
# to rounding, left out): every one is below the 1e-9 of a route against a loop reference, which therefore holds (docs/EXPERIMENTS.md has the table)
ROUNDING = dict(cjs=4.7e-11, ks=8.4e-11, sensitivity=3.2e-11, mean_gradient=8.3e-13, sd_gradient=9.3e-14)
# the conjugate normal model: (mu0, s0, ybar, sl) -> the standard deviation over 8 seeds of the ratio of the host port's sensitivity
# (prior, likelihood) to the quadrature's at 40 000 draws; the tests hold the ratio to 1 within five times that
CONJUGATE = {(0., 10., 1., 1.): ('-', 0.0111, 0.0381), (0., 1., 3., 1.): ('prior-data conflict', 0.0078, 0.0142),
             (0., 1., 0.5, 10.): ('strong prior / weak likelihood', 0.0383, 0.0262)}
N_CONJUGATE = 40000


@functools.lru_cache(maxsize=None)
def ps_inputs(n):
    """x (n, 3): a smooth parameter, one rounded to a grid (ties), one negative and of mixed sign on another scale; g (n, 3): two
    components of spread 1 and 0.1 that lean on the parameters, and a constant one (every ratio equal: u is w); log weights that are
    -inf in a third of the rows."""
    rng = np.random.default_rng(7000 + n)
    z = rng.standard_normal((n, 3))
    x = np.stack([3. + 0.5 * z[:, 0], np.round(z[:, 1] / 0.25) * 0.25, -40. * z[:, 2] - 5.], axis=1)
    g = np.stack([-0.5 * (z[:, 0] + 0.3 * z[:, 1])**2 + 0.2 * z[:, 2], 0.1 * z[:, 1] - 2., np.full(n, 0.75)], axis=1)
    lw = 0.5 * rng.standard_normal(n)
    lw[rng.random(n) < 0.33] = -np.inf
    lw[0] = 0.2
    return x, g, lw


@functools.lru_cache(maxsize=None)
def ps_reference(n, weighted, long=False):
    x, g, lw = ps_inputs(n)
    return power_scale_reference(x, g, lw if weighted else None, ALPHAS, dtype=np.longdouble if long else np.float64)


def ecdf_vector(x, w, u):
    """``ecdf_reference`` for every column of u (n, S) at once by NumPy's running sums, for the sizes at which a loop takes minutes
    (the tests hold it to the loop at the smaller sizes): dict of (S,) arrays."""
    keep = w != 0
    xs, ws, us = x[keep], w[keep], u[keep]
    s = u.shape[1]
    nan = np.full(s, np.nan)
    if not np.isfinite(xs).all():
        return dict(J=nan, bound=nan, cjs=nan, ks=nan)
    order = np.argsort(xs, kind='stable')
    xs, ws, us = xs[order], ws[order], us[order]
    with np.errstate(all='ignore'):
        big_p = np.cumsum(ws)[:-1, None]
        big_d = np.cumsum(us - ws[:, None], axis=0)[:-1]
        h = np.diff(xs)[:, None]
        tot = big_p + (big_p + big_d)
        t = np.clip(big_d / tot, -1., 1.)
        a, b = 1. - t, 1. + t
        f = np.where(a == 0, 0., a * np.log1p(-t)) + np.where(b == 0, 0., b * np.log1p(t))
        bound = (h * tot).sum(axis=0)
        big_j = (h * (tot / 2.) * f).sum(axis=0) / np.log(2.)
        ks = np.where(h > 0, np.abs(big_d), 0.).max(axis=0) if len(xs) > 1 else np.zeros(s)
        ok = bound != 0
        return dict(J=big_j, bound=bound, cjs=np.where(ok, np.sqrt(big_j / np.where(ok, bound, 1.)), np.nan),
                    ks=np.where(ok & ~np.isnan(big_j), ks, np.nan))


# ---- the conjugate normal model --------------------------------------------------------------------------------------------------------
def conjugate_draws(mu0, s0, ybar, sl, seed, n=N_CONJUGATE):
    """n i.i.d. draws of the exact posterior of x under the prior N(mu0, s0) and the likelihood N(ybar | x, sl) -> x (n, 1) and the
    components g (n, 2): log prior and log likelihood up to constants."""
    prec = 1. / s0**2 + 1. / sl**2
    mean = (mu0 / s0**2 + ybar / sl**2) / prec
    x = mean + np.random.default_rng(seed).standard_normal(n) / math.sqrt(prec)
    return x[:, None], np.stack([-0.5 * ((x - mu0) / s0)**2, -0.5 * ((ybar - x) / sl)**2], axis=1)


def _phi(z):
    return 0.5 * (1. + np.vectorize(math.erf)(z / math.sqrt(2.)))


def _trapezoid(y, grid):
    return float((0.5 * (y[1:] + y[:-1]) * np.diff(grid)).sum())


def conjugate_quadrature(mu0, s0, ybar, sl, lo, hi, alphas=(0.99, 1.01), points=20001):
    """(prior, likelihood) sensitivity from the exact Gaussian CDFs of the base and the power-scaled posteriors, the integrals of the
    definitions taken over [lo, hi] by the trapezoidal rule."""
    grid = np.linspace(lo, hi, points)

    def cdf(ap, al):
        prec = ap / s0**2 + al / sl**2
        return _phi((grid - (ap * mu0 / s0**2 + al * ybar / sl**2) / prec) * math.sqrt(prec))

    def cjs(big_p, big_q):
        with np.errstate(all='ignore'):
            m = 0.5 * (big_p + big_q)
            term = np.where(big_p > 0, big_p * np.log2(big_p / m), 0.) + np.where(big_q > 0, big_q * np.log2(big_q / m), 0.)
        return math.sqrt(_trapezoid(term, grid) / _trapezoid(big_p + big_q, grid))

    base = cdf(1., 1.)
    out = []
    for which in (0, 1):
        c = [cjs(base, cdf(a if which == 0 else 1., a if which == 1 else 1.)) for a in alphas]
        out.append(0.5 * (c[0] / abs(math.log2(alphas[0])) + c[1] / math.log2(alphas[1])))
    return out


def conjugate_table(seeds=range(8)):
    root = os.path.dirname(os.path.dirname(HERE))
    if root not in sys.path:
        sys.path.insert(0, root)
    from bayesfast_amd.utils import power_scale
    for par in CONJUGATE:
        ratio = []
        for seed in seeds:
            x, g = conjugate_draws(*par, seed=100 + seed)
            got = power_scale(x, g, names=['prior', 'likelihood'])
            want = conjugate_quadrature(*par, lo=x.min(), hi=x.max())
            ratio.append(got.sensitivity[:, 0] / np.array(want))
            print(par, seed, got.sensitivity[:, 0], want, got.diagnosis, flush=True)
        ratio = np.array(ratio)
        print(par, 'ratio: mean', ratio.mean(axis=0), 'sd', ratio.std(axis=0, ddof=1))


def rounding_table(sizes=SIZES):
    worst = {f: (0., None) for f in FIGS}
    for n in sizes:
        for weighted in (False, True):
            a, b = ps_reference(n, weighted), ps_reference(n, weighted, True)
            for f in FIGS:
                va, vb = np.asarray(a[f], dtype=np.longdouble), np.asarray(b[f], dtype=np.longdouble)
                if not f.endswith('gradient'):   # (the constant component's u is w up to rounding: its distances are no figures)
                    va, vb = va[:-len(ALPHAS) if f != 'sensitivity' else -1], vb[:-len(ALPHAS) if f != 'sensitivity' else -1]
                with np.errstate(all='ignore'):
                    err = np.abs(va - vb) if f.endswith('gradient') else np.abs(va / vb - 1.)
                err = err[np.isfinite(err)]
                e = float(err.max()) if err.size else 0.
                print('n=%d w=%d %s %.3g' % (n, weighted, f, e), flush=True)
                if e > worst[f][0]:
                    worst[f] = (e, (n, weighted))
    return worst


if __name__ == '__main__':
    for f, (e, at) in rounding_table().items():
        print('%-20s %.3g at %s' % (f, e, at))
    conjugate_table()
