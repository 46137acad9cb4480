"""FitReport: the leave-one-out validation of a ``PolyModel`` fit (``PolyModel.fit_loo``).

For linear least squares the residual of point i under a fit made WITHOUT point i is ``e_i / (1 - h_i)`` exactly, where
``h_i = a_i^T (A^T A)^-1 a_i`` is the leverage of design row ``a_i``: no refit and no call of the true model.  The device
computes the leverages from the Cholesky factor the fit keeps, the held-out residuals and, per output, a handful of sums
(``bfhip_lstsq_loo``, include/bfhip.h); everything else here is a pure function of those sums and needs no GPU.

Units.  Row weights enter as in ``fit``: row i of the design and of ``y`` is multiplied by ``w_i`` and the least-squares
problem is the weighted one.  ``residual`` and ``loo_residual`` are in the units of ``y``; the sums, and with them ``rmse``,
``loo_rmse``, ``r2`` and ``q2``, are in the fit's weighted units (those of ``w y``, the quantity the fit minimises; the
total sum of squares is taken about the plain mean of ``w y``).  Without weights the two are the same.

``RidgeReport`` (``PolyModel.fit_ridge``) is the same report for a ridge-penalised fit, where the identity holds with the ridge hat
diagonal ``h_i(rho)``, plus the path of penalties the fit's own was chosen from (``ridge_score``, ``ridge_choose``).
"""
import numpy as np

__all__ = ['FitReport', 'RidgeReport', 'derive', 'ridge_score', 'ridge_choose', 'SUM_NAMES']

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


def ridge_score(path_sums, n):
    """The criterion a ridge path is chosen by, (L,) from the (L, m, 8) sums of one design group: the mean over the group's outputs of
    PRESS / SS_tot (1 - q2), outputs with SS_tot = 0 left out (all of them constant: zeros)."""
    path_sums = np.asarray(path_sums, dtype=np.float64)
    if not (path_sums.ndim == 3 and path_sums.shape[2] == len(SUM_NAMES)):
        raise ValueError('path_sums should have shape (# of penalties, # of outputs, {}), instead of {}.'.format(len(SUM_NAMES),
                                                                                                             path_sums.shape))
    ss_tot = path_sums[0, :, SYY] - path_sums[0, :, SY]**2 / int(n)
    ok = ss_tot > 0.
    if not ok.any():
        return np.zeros(path_sums.shape[0])
    return np.mean(path_sums[:, ok, PRESS] / ss_tot[ok], axis=1)


def ridge_choose(score, ridge):
    """(index, at_edge) of the chosen penalty: the smallest score, ties to the larger penalty; at_edge when the choice is the first or
    the last value of the grid.  A score that is not a number never wins (unless all are: the largest penalty then)."""
    score, ridge = np.asarray(score, dtype=np.float64), np.asarray(ridge, dtype=np.float64)
    if not (score.ndim == 1 and score.shape == ridge.shape and score.size >= 1):
        raise ValueError('score and ridge should be 1-d arrays of one size.')
    cand = np.arange(score.size) if np.all(np.isnan(score)) else np.flatnonzero(score == np.nanmin(score))
    index = int(cand[np.argmax(ridge[cand])])
    return index, index in (0, score.size - 1)


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


class RidgeReport(FitReport):
    """What ``PolyModel.fit_ridge`` returns: the ``FitReport`` of the fit at the chosen penalty, and the path it was chosen from.

    The fit minimises ``|B - A c|^2 + n rho sum_j D_j c_j^2`` with ``D_j`` the mean square of (weighted) design column j, the constant
    column unpenalised; one penalty per design group, chosen by exact leave-one-out over the whole path (``ridge_score``,
    ``ridge_choose``).  Beyond the fields of ``FitReport`` (``leverage`` is the ridge hat diagonal, ``n_param`` the number of columns):
    ridge_path : (L,) the grid of rho;  ridge, ridge_index, at_edge : (n_group,) the chosen rho, its index, and whether it is the
    first or last grid value (the optimum may lie outside the grid);  dof, score_path : (n_group, L) the effective number of
    parameters sum_i h_i and the selection criterion;  press_path, q2_path, rmse_path : (output_size, L)."""

    def __init__(self, n, n_param, group_of_output, groups, ridge_path):
        """groups: as for ``FitReport`` without ``sums``, with ``path_sums`` (L, len(outs), 8) and ``dof`` (L,); the per-point arrays
        are those at the penalty ``ridge_choose`` picks from ``path_sums``."""
        self.ridge_path = np.array(ridge_path, dtype=np.float64)
        L = self.ridge_path.size
        index, edge, score = [], [], []
        for g in groups:
            g['path_sums'] = np.asarray(_host(g['path_sums']), dtype=np.float64)
            score.append(ridge_score(g['path_sums'], n))
            i, e = ridge_choose(score[-1], self.ridge_path)
            index.append(i)
            edge.append(e)
            g['sums'] = g['path_sums'][i]
        super().__init__(n, n_param, group_of_output, groups, [False] * len(groups))
        self.ridge_index = np.array(index, dtype=int)
        self.ridge = self.ridge_path[self.ridge_index]
        self.at_edge = np.array(edge, dtype=bool)
        self.score_path = np.array(score).reshape(len(groups), L)
        self.dof = np.array([np.asarray(_host(g['dof']), dtype=np.float64) for g in groups]).reshape(len(groups), L)
        m = self.group_of_output.size
        self.press_path, self.q2_path, self.rmse_path = np.zeros((m, L)), np.zeros((m, L)), np.zeros((m, L))
        for g in groups:
            outs = list(g['outs'])
            for l in range(L):
                d = derive(g['path_sums'][l], self.n)
                self.press_path[outs, l] = g['path_sums'][l][:, PRESS]
                self.q2_path[outs, l] = d['q2']
                self.rmse_path[outs, l] = d['rmse']

    def __eq__(self, other):
        if not isinstance(other, RidgeReport):
            return False if isinstance(other, FitReport) else NotImplemented
        return (np.array_equal(self.ridge_path, other.ridge_path) and np.array_equal(self.ridge_index, other.ridge_index)
                and np.array_equal(self.dof, other.dof) and len(self._groups) == len(other._groups)
                and all(np.array_equal(a['path_sums'], b['path_sums']) for a, b in zip(self._groups, other._groups))
                and FitReport.__eq__(self, other))

    __hash__ = None

    def __repr__(self):
        rows = ['RidgeReport: ridge = %s (index %s of %d, at_edge = %s), dof = %s'
                % (self.ridge.tolist(), self.ridge_index.tolist(), self.ridge_path.size, self.at_edge.tolist(),
                   ['%.4g' % self.dof[g, i] for g, i in enumerate(self.ridge_index)])]
        rows += ['  group %d score path: %s' % (g, ' '.join('%.4g' % v for v in self.score_path[g])) for g in range(len(self._groups))]
        return '\n'.join(rows + [FitReport.__repr__(self)])
