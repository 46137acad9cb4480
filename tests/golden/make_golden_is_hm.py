#!/usr/bin/env python3
"""Generate tests/golden/evidence_is_hm.npz by calling the reference's own ``importance`` and ``harmonic``
(bayesfast/evidence/importance.py, harmonic.py) on synthetic log-density arrays.

Runs only where a checkout of the reference exists (make_golden.py:prepare_reference builds and imports it).  The file holds data
only: for every case the two input arrays (float32 values, so that their float64 reading is exact), the reference's ``logr`` and
``logr_err``, and which of its two RuntimeWarnings it raised.

Usage:  python tests/golden/make_golden_is_hm.py [--ref /root/reference] [--work /tmp/bfref]
"""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import prepare_reference  # noqa: E402

LOG2PI = np.log(2 * np.pi)


def _norm_logpdf(x, sd):
    return -0.5 * (x / sd)**2 - np.log(sd) - 0.5 * LOG2PI


def _ar1(rng, shape, rho):
    """AR(1) series along the last axis with unit marginal variance."""
    e = rng.normal(size=shape)
    x = np.empty(shape)
    x[..., 0] = e[..., 0]
    for t in range(1, shape[-1]):
        x[..., t] = rho * x[..., t - 1] + np.sqrt(1 - rho**2) * e[..., t]
    return x


def cases(rng):
    """name -> (kind, first input, second input): importance(logp_q, logq_q) or harmonic(logp_p, logq_p)."""
    out = {}
    # importance: draws from q = N(0, 1), p an unnormalised N(0.1, 1.1^2)
    x = rng.normal(size=3000)
    out['is_1d'] = ('is', _norm_logpdf(x - 0.1, 1.1) + 2.3, _norm_logpdf(x, 1.))
    x = rng.normal(size=(4, 800))
    out['is_2d'] = ('is', _norm_logpdf(x + 0.2, 0.9) - 7.1, _norm_logpdf(x, 1.))
    # p much wider than q: the weights have no finite variance, the error exceeds 0.25
    x = rng.normal(size=400)
    out['is_heavy'] = ('is', _norm_logpdf(x - 1.5, 3.) + 0.4, _norm_logpdf(x, 0.5))
    # a few draws outside p's support
    x = rng.normal(size=2000)
    lp = _norm_logpdf(x, 1.2) + 1.1
    lp[rng.choice(x.size, 6, replace=False)] = -np.inf
    out['is_inf'] = ('is', lp, _norm_logpdf(x, 1.))
    # harmonic: samples of p = N(0, 1) (unnormalised), q = N(0, 1.2^2)
    x = rng.normal(size=3000)
    out['hm_1d'] = ('hm', _norm_logpdf(x, 1.) + 1.7, _norm_logpdf(x, 1.2))
    # correlated chains: tau matters
    x = _ar1(rng, (4, 1500), 0.9)
    out['hm_ar1'] = ('hm', _norm_logpdf(x, 1.) - 3.2, _norm_logpdf(x, 1.25))
    # chains at different levels: flattening changes tau by far more than 25 %
    x = _ar1(rng, (4, 1000), 0.5) + np.array([-0.45, -0.15, 0.15, 0.45])[:, None]
    out['hm_offset'] = ('hm', _norm_logpdf(x, 1.) + 0.5, _norm_logpdf(x - 0.3, 1.1))
    # q a narrow bump in p's tail: a few samples carry the whole mean, the error exceeds 0.25
    x = rng.normal(size=300)
    out['hm_heavy'] = ('hm', _norm_logpdf(x, 1.) + 2., _norm_logpdf(x - 3., 0.5))
    return out


def gen_is_hm(bf, out_dir):
    from bayesfast.evidence import importance, harmonic
    rng = np.random.default_rng(1729)
    z = {}
    names = []
    for name, (kind, a, b) in cases(rng).items():
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            logr, err = (importance if kind == 'is' else harmonic)(a32.astype(np.float64), b32.astype(np.float64))
        msgs = [str(m.message) for m in w if m.category is RuntimeWarning]
        z[name + '.a'], z[name + '.b'] = a32, b32
        z[name + '.logr'], z[name + '.err'] = np.float64(logr), np.float64(err)
        z[name + '.w_large'] = np.int8(any('larger than 0.25' in m for m in msgs))
        z[name + '.w_tau'] = np.int8(any('more than 25%' in m for m in msgs))
        names.append(name)
        print('%-10s logr %.6f err %.4g warnings %s' % (name, logr, err, msgs))
    z['cases'] = np.array(names)
    np.savez_compressed(os.path.join(out_dir, 'evidence_is_hm.npz'), **z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--work', default='/tmp/bfref')
    a = ap.parse_args()
    gen_is_hm(prepare_reference(a.ref, a.work), HERE)
    print('wrote evidence_is_hm')


if __name__ == '__main__':
    main()
