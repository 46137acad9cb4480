"""FitReport: the leave-one-out validation of a ``PolyModel`` fit (``PolyModel.fit_loo``).

For linear least squares the residual of point i under a fit made WITHOUT point i is ``e_i / (1 - h_i)`` exactly, where
``h_i = a_i^T (A^T A)^-1 a_i`` is the leverage of design row ``a_i``: no refit and no call of the true model.  The device
computes the leverages from the Cholesky factor the fit keeps, the held-out residuals and, per output, a handful of sums
(``bfhip_lstsq_loo``, include/bfhip.h); everything else here is a pure function of those sums and needs no GPU.

Units.  Row weights enter as in ``fit``: row i of the design and of ``y`` is multiplied by ``w_i`` and the least-squares
problem is the weighted one.  ``residual`` and ``loo_residual`` are in the units of ``y``; the sums, and with them ``rmse``,
``loo_rmse``, ``r2`` and ``q2``, are in the fit's weighted units (those of ``w y``, the quantity the fit minimises; the
total sum of squares is taken about the plain mean of ``w y``).  Without weights the two are the same.
"""
import numpy as np

__all__ = ['FitReport', 'derive', 'SUM_NAMES']

# the columns of the device sums (BFHIP_LOO_* of include/bfhip.h)
SUM_NAMES = ('sse', 'press', 'max_abs_loo', 'argmax_abs_loo', 'sum_y', 'sum_yy', 'n_unit', 'reserved')
SSE, PRESS, MAX, ARGMAX, SY, SYY, NUNIT = range(7)


def derive(sums, n):
    """rmse, loo_rmse, r2, q2 (each (m,)) from the (m, 8) sums over n rows:
    rmse = sqrt(SSE / n), loo_rmse = sqrt(PRESS / n), SS_tot = sum y^2 - (sum y)^2 / n, r2 = 1 - SSE / SS_tot,
    q2 = 1 - PRESS / SS_tot.  A constant output (SS_tot = 0) has r2 = q2 = nan unless its residuals vanish too."""
    sums = np.asarray(sums, dtype=np.float64)
    if not (sums.ndim == 2 and sums.shape[1] == len(SUM_NAMES)):
        raise ValueError('sums should have shape (# of outputs, {}), instead of {}.'.format(len(SUM_NAMES), sums.shape))
    n = int(n)
    if n < 1:
        raise ValueError('n should be positive.')
    sse, press = sums[:, SSE], sums[:, PRESS]
    ss_tot = sums[:, SYY] - sums[:, SY]**2 / n
    with np.errstate(divide='ignore', invalid='ignore'):
        r2 = 1. - sse / ss_tot
        q2 = 1. - press / ss_tot
    return dict(rmse=np.sqrt(sse / n), loo_rmse=np.sqrt(press / n), r2=r2, q2=q2)


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


class FitReport:
    """What ``PolyModel.fit_loo`` returns.

    n : number of fit points;  n_param : parameters per design group (outputs that share a set of configs share a design);
    group_of_output : (output_size,) index of each output's group;  rank_deficient : (n_group,) bool, the group went through
    the fit's minimum-norm fallback (its leverages then sum to the kept rank);  n_unit_leverage : (n_group,) rows whose
    ``1 - h`` is not positive after rounding (their held-out residual is infinite and so are the output's ``loo_rmse`` and
    ``max_abs_loo``);
    leverage : list of (n,) arrays, one per group;  residual, loo_residual : (n, output_size), in the units of ``y``;
    rmse, loo_rmse, r2, q2, max_abs_loo, argmax_abs_loo : (output_size,).

    The per-point arrays stay on the device until they are asked for."""

    def __init__(self, n, n_param, group_of_output, groups, rank_deficient):
        """groups: per design group a dict with ``outs`` (its output indices), ``h`` (n,), ``resid`` and ``e_loo`` (n, len(outs)) and
        ``sums`` (len(outs), 8): NumPy arrays or device tensors."""
        self.n = int(n)
        self.n_param = tuple(int(p) for p in n_param)
        self.group_of_output = np.asarray(group_of_output, dtype=int)
        self.rank_deficient = np.asarray(rank_deficient, dtype=bool)
        self._groups = groups
        m = self.group_of_output.size
        sums = np.zeros((m, len(SUM_NAMES)))
        for g in groups:
            sums[list(g['outs'])] = _host(g['sums'])
        self.sums = sums
        d = derive(sums, self.n)
        self.rmse, self.loo_rmse, self.r2, self.q2 = d['rmse'], d['loo_rmse'], d['r2'], d['q2']
        self.max_abs_loo = sums[:, MAX].copy()
        self.argmax_abs_loo = sums[:, ARGMAX].astype(int)
        self.n_unit_leverage = np.array([int(_host(g['sums'])[0, NUNIT]) for g in groups], dtype=int)
        self._cache = {}

    @property
    def leverage(self):
        if 'h' not in self._cache:
            self._cache['h'] = [np.array(_host(g['h'])) for g in self._groups]
        return self._cache['h']

    def _scatter(self, key):
        if key not in self._cache:
            out = np.empty((self.n, self.group_of_output.size))
            for g in self._groups:
                out[:, list(g['outs'])] = _host(g[key])
            self._cache[key] = out
        return self._cache[key]

    residual = property(lambda self: self._scatter('resid'))
    loo_residual = property(lambda self: self._scatter('e_loo'))

    def __eq__(self, other):
        if not isinstance(other, FitReport):
            return NotImplemented
        return (self.n == other.n and self.n_param == other.n_param
                and np.array_equal(self.group_of_output, other.group_of_output)
                and np.array_equal(self.rank_deficient, other.rank_deficient) and np.array_equal(self.sums, other.sums)
                and all(np.array_equal(a, b) for a, b in zip(self.leverage, other.leverage))
                and np.array_equal(self.residual, other.residual) and np.array_equal(self.loo_residual, other.loo_residual))

    __hash__ = None

    def __getstate__(self):
        """Copies and pickles hold host arrays (a PolyModel's state is host NumPy: core/recipe.py deep-copies its surrogates)."""
        state = dict(self.__dict__)
        state['_groups'] = [{k: (v if k == 'outs' else np.array(_host(v))) for k, v in g.items()} for g in self._groups]
        return state

    def __repr__(self):
        names = ('group', 'rmse', 'loo_rmse', 'r2', 'q2', 'max_abs_loo', 'argmax')
        rows = ['FitReport: n = %d, n_param = %s, rank_deficient = %s, n_unit_leverage = %s'
                % (self.n, list(self.n_param), self.rank_deficient.tolist(), self.n_unit_leverage.tolist()),
                ''.join(['%5s' % ''] + ['%12s' % k for k in names])]
        for i in range(self.group_of_output.size):
            rows.append('%5d%12d' % (i, self.group_of_output[i])
                        + ''.join('%12.5g' % v for v in (self.rmse[i], self.loo_rmse[i], self.r2[i], self.q2[i], self.max_abs_loo[i]))
                        + '%12d' % self.argmax_abs_loo[i])
        return '\n'.join(rows)
