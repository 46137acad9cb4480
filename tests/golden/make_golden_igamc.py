"""Writes tests/golden/igamc.npz: Q(a, x), the regularised upper incomplete gamma function, from mpmath at 40 digits on the grid of
tests/test_gpu_data_lgo.py, with scipy's own error against it (the yardstick of the device function's bound).

  a    (N,)  of {0.5, 1, 1.5, 2, 4, 8.5, 16, 64, 228.5, 512, 1024}
  x    (N,)  a times {1e-3, 0.01, 0.3, 0.7, 0.9, 0.99, 1, 1.01, 1.1, 1.5, 3, 8}, and x = 0
  q    (N,)  Q(a, x) rounded to double (0 where it underflows)
  scipy_err (N,)  |scipy.special.gammaincc - Q|: relative where Q >= 1e-290, absolute below

Run: python tests/golden/make_golden_igamc.py"""
import os

import mpmath
import numpy as np
from scipy.special import gammaincc

A = (0.5, 1., 1.5, 2., 4., 8.5, 16., 64., 228.5, 512., 1024.)
RATIO = (0., 1e-3, 0.01, 0.3, 0.7, 0.9, 0.99, 1., 1.01, 1.1, 1.5, 3., 8.)
TINY = 1e-290


def main():
    mpmath.mp.dps = 40
    a = np.repeat(A, len(RATIO))
    x = a * np.tile(RATIO, len(A))   # the doubles the test hands to the device: mpmath sees exactly these
    exact = [mpmath.gammainc(mpmath.mpf(float(ai)), mpmath.mpf(float(xi)), mpmath.inf, regularized=True) for ai, xi in zip(a, x)]
    q = np.array([float(e) for e in exact])
    got = gammaincc(a, x)
    err = np.array([float(abs(mpmath.mpf(float(g)) - e) / e) if float(e) >= TINY else float(abs(mpmath.mpf(float(g)) - e))
                    for g, e in zip(got, exact)])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'igamc.npz'), a=a, x=x, q=q, scipy_err=err)
    big = q >= TINY
    print('%d points; scipy: largest relative error %.3g (Q >= %g), largest absolute error below %.3g'
          % (a.size, err[big].max(), TINY, err[~big].max() if (~big).any() else 0.))


if __name__ == '__main__':
    main()
