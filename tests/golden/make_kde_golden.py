"""Writes tests/golden/kde.npz: what the reference's own ``utils/kde.py`` computes on three small data sets.

    python tests/golden/make_kde_golden.py <root of a checkout of the reference>

The reference's module is loaded by file path (it needs NumPy and scipy only; its package, with the Cython extensions, is not
imported).  Recorded per case: the data, the weights, the queries ((m, d) rows, as the reference's code takes them) and its
``factor``, ``covariance``, ``pdf`` and ``logpdf``.  Its ``cdf`` calls ``np.asscalar``, which NumPy no longer has, and is not
recorded: tests/test_kde_host.py checks ``cdf`` in closed form."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load(root):
    spec = importlib.util.spec_from_file_location('reference_utils_kde', os.path.join(root, 'bayesfast', 'utils', 'kde.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kde


def cases():
    rng = np.random.default_rng(20211)
    mix = rng.standard_normal((4, 4))
    x4 = rng.standard_normal((300, 4)) @ mix + np.array([1., -2., 0.5, 30.])
    w4 = rng.uniform(0.1, 1., size=300)
    q4 = np.vstack([x4[:10] + 0.1, rng.standard_normal((20, 4)) @ mix * 2. + np.array([1., -2., 0.5, 30.])])
    x1 = np.concatenate([rng.standard_normal(120) - 2., 0.5 * rng.standard_normal(80) + 1.5])
    q1 = np.linspace(-6., 4., 41)
    x2 = rng.standard_normal((150, 2)) * np.array([1., 3.])
    q2 = rng.standard_normal((25, 2)) * np.array([2., 5.])
    return dict(a=(x4, w4, q4, dict(bw_method='silverman', bw_factor=0.8)),
                b=(x1, None, q1, dict(bw_method='scott')),
                c=(x2, None, q2, dict(bw_method=0.37)))


def main(root):
    kde = load(root)
    out = {}
    for name, (x, w, q, kw) in cases().items():
        est = kde(x, weights=w, **kw)
        out[name + '_x'], out[name + '_q'] = x, q
        if w is not None:
            out[name + '_w'] = w
        out[name + '_factor'] = np.float64(est.factor)
        out[name + '_covariance'] = np.asarray(est.covariance)
        out[name + '_pdf'] = est.pdf(q)
        out[name + '_logpdf'] = est.logpdf(q)
    path = os.path.join(HERE, 'kde.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
