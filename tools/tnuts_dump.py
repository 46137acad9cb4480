"""Bit-equality of two builds of the tempered-NUTS kernels: a fixed list of cases through DeviceChains.run_tempered, their samples,
statistics and (u, weight) written to an .npz.  Run it once per library, each in a fresh process (BFHIP_LIBRARY selects the
build), then compare: every array must be EQUAL.
usage: python tools/tnuts_dump.py out.npz            (dump)
       python tools/tnuts_dump.py a.npz b.npz        (compare; exit status 1 when an array differs)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHORT = dict(max_treedepth=3, max_change=50.)   # trees that end at the depth limit and by divergences (tests/test_tempered.py)


def with_bounds(spec, d):
    lo = np.full(d, -9.) + np.arange(d) * 0.01
    spec.update(ranges=np.stack([lo, lo + 18.], 1), hard_bounds=np.array(([[1, 1], [1, 0], [0, 1], [0, 0]] * d)[:d], dtype=np.uint8))


def with_decay(spec):
    po = spec['poly']
    spec.update(use_decay=True, decay_mu=np.asarray(po['mu']) + 0.05, decay_hess=po['hess'], decay_alpha2=(0.8 * float(po['alpha']))**2,
                decay_gamma=0.1)


def with_cubic(spec, d, rng):
    a3 = np.zeros((1, d, d, d))
    for j in range(d):
        for k in range(j + 1, d):
            for l in range(k + 1, d):
                a3[0, j, k, l] = 0.01 * rng.normal()
    spec['poly']['configs'] = list(spec['poly']['configs']) + [
        dict(order='cubic-2', input_mask=np.arange(d), output_mask=np.arange(1), coef=0.01 * rng.normal(size=(1, d, d))),
        dict(order='cubic-3', input_mask=np.arange(d), output_mask=np.arange(1), coef=a3)]


def cases():
    """(name, spec, base covariance scale, chains, iterations, warm-up, DeviceChains keywords, forced generic)"""
    from bayesfast_amd.workloads import correlated_gaussian_spec, random_pipeline_spec
    out = []
    for d in (12, 24, 40):   # the tuned kernel at W = 1, 2, 4 row tiles
        for feat in ('plain', 'bounds', 'decay') + (('bounds_decay',) if d == 40 else ()):
            spec = dict(correlated_gaussian_spec(d, fit_scale=1.5)[0])
            if 'bounds' in feat:
                with_bounds(spec, d)
            if 'decay' in feat:
                with_decay(spec)
            out.append(('tuned_d%d_%s' % (d, feat), spec, 0.3 if 'bounds' in feat else 1.5, 37, 24, 16, {}, 0))
    spec, cov = correlated_gaussian_spec(24, fit_scale=1.5)
    out.append(('generic_d24', dict(spec), 1.5, 37, 24, 16, {}, 1))
    spec = dict(correlated_gaussian_spec(12, fit_scale=1.5)[0])
    spec['poly'] = dict(spec['poly'])
    with_cubic(spec, 12, np.random.default_rng(3))
    out.append(('cubic_d12', spec, 1.2, 21, 20, 12, {}, 0))
    out.append(('d128', dict(correlated_gaussian_spec(128, fit_scale=1.5)[0]), 1.5, 9, 10, 6, {}, 0))
    spec, cov = correlated_gaussian_spec(12, fit_scale=1.5)
    out.append(('full_fixed_d12', dict(spec), 1.5, 19, 16, 0, dict(metric=cov * 0.9), 0))
    out.append(('full_adapt_d12', dict(spec), 1.5, 19, 20, 14, dict(metric=cov * 0.9), 0))
    out.append(('pipeline_40_9_4', random_pipeline_spec(40, 9, 4, seed=2), 0.5, 11, 12, 8, {}, 0))
    return out


def dump(path):
    from bayesfast_amd.device import get_context, DeviceDensity
    from bayesfast_amd.chains import DeviceChains
    from bayesfast_amd import _lib
    ctx = get_context(0)
    res = {}
    for name, spec, bscale, n_chain, n_iter, n_warmup, kw, generic in cases():
        d = int(spec['d'])
        rng = np.random.default_rng(8)
        x0, u0 = rng.normal(size=(n_chain, d)) * 0.3, rng.normal(size=n_chain)
        dens = DeviceDensity(spec, ctx)
        for tag, run_kw in (('', {}), ('.short', SHORT)):
            _lib.debug_set('tnuts_generic', generic)
            try:
                dc = DeviceChains(dens, x0, seed=31, adapt_window=5, **kw)
                arr = dc.run_tempered(n_iter, np.zeros(d), np.eye(d) * bscale, logxi=0.2, u_0=u0, n_warmup=n_warmup, **run_kw)
            finally:
                _lib.debug_set('tnuts_generic', 0)
            for k, t in zip(('samples', 'stats', 'stats_t'), arr):
                res['%s%s.%s' % (name, tag, k)] = t.cpu().numpy()
            ts = res['%s%s.stats' % (name, tag)][:, :, _lib.NSTATS.index('tree_size')]
            print('%-28s %3d chains x %2d iterations, %6d leapfrog steps, %d diverging' % (
                name + tag, n_chain, n_iter, int(ts.sum()), int(res['%s%s.stats' % (name, tag)][:, :, _lib.NSTATS.index('diverging')].sum())), flush=True)
    np.savez(path, **res)
    print('library %s -> %s (%d arrays)' % (_lib.LIB_PATH, path, len(res)))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for case in sorted({k.rsplit('.', 1)[0] for k in a.files}):
        diff = [k for k in ('samples', 'stats', 'stats_t') if not np.array_equal(a[case + '.' + k], b[case + '.' + k], equal_nan=True)]
        print('%-28s %s' % (case, 'EQUAL' if not diff else 'DIFFERENT: ' + ', '.join(diff)))
        bad += diff
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 2:
        dump(sys.argv[1])
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
