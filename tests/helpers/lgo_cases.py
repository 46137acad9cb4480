"""The inputs that tests/test_data_lgo_host.py and tests/test_gpu_data_lgo.py share, and the one comparison of a ``DataLGO`` with
``lgo_reference.group_reference``'s dicts.

``chi2_case(n, weighting)``: four columns of conditional chi-squares with DOF = (1, 2, 17, 457) degrees of freedom, each scaled a
little off its nominal law, their constants, and base log weights: 'plain' (None), 'weights' (a tenth of the rows -inf) or
'mostly zero' (four fifths of the rows -inf)."""
import numpy as np

DOF = (1, 2, 17, 457)
SCALE = (1., 1.3, 0.8, 1.05)
CONST = (-0.3, 0.4, -11.1, -300.5)
RTOL = 1e-9
FIGURES = ('lpd', 'p_waic', 'elpd_waic', 'elpd_lgo', 'p_lgo', 'khat', 'sigma', 'ess_lgo', 'chi2_base', 'chi2_lgo', 'ppp_base', 'ppp_lgo')


def chi2_case(n, weighting):
    rng = np.random.default_rng(7919 * n + len(weighting))
    q = rng.chisquare(DOF, size=(n, len(DOF))) * np.array(SCALE)
    lw = 0.7 * rng.standard_normal(n)
    if weighting == 'plain':
        lw = None
    else:
        lw[rng.random(n) < (0.1 if weighting == 'weights' else 0.8)] = -np.inf
        lw[0] = 0.
    return q, np.array(DOF, dtype=np.float64), np.array(CONST), lw


def compare(got, refs, label, rounding=None, offset=0, waic_abs=0.):
    """Every figure of got's columns offset .. against the reference dicts: RTOL relative, or the figure's entry of ``rounding`` where
    that is larger; p_lgo, a difference, relative to the larger of its two terms; n_tail and non-finite values exactly.  ``waic_abs``:
    what a constant column's p_waic, rounding alone, may be off by."""
    for j, r in enumerate(refs):
        k = offset + j
        assert int(got.n_tail[k]) == r['n_tail'], (label, k)
        for f in FIGURES:
            g, w = getattr(got, f)[k], np.float64(r[f])
            tol = max(RTOL, (rounding or {}).get(f, 0.))
            if not np.isfinite(w):
                assert np.array_equal(g, w, equal_nan=True), (label, k, f, g, w)
            elif f == 'p_lgo':
                assert abs(g - w) <= tol * max(abs(np.float64(r['lpd'])), abs(np.float64(r['elpd_lgo']))), (label, k, f, g, w)
            else:
                assert abs(g - w) <= tol * abs(w) + (waic_abs if 'waic' in f else 0.), (label, k, f, g, w)
