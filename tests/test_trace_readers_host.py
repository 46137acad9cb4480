"""``TraceTuple``'s analysis readers on host parts: each is the ``utils`` function on what ``get(flatten=False)`` selects, byte for
byte; what each refuses, and with which words; and the integration seam forwards every reader that ``TraceTuple.READERS`` names.
No GPU: the parts are NumPy arrays (helpers/trace_cases.py), so every reader takes its host port."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, 'helpers') not in sys.path:
    sys.path.insert(0, os.path.join(HERE, 'helpers'))

from trace_cases import SELECTIONS, same, trace  # noqa: E402

WITH_DENSITY = ('predictive', 'data_loo', 'data_lgo', 'data_reweight', 'profile')
# the words of the single-process readers, as they were before the readers shared one refusal
RANKED = ('rhat, ess and summary rank every value among the draws of ALL chains, and this TraceTuple holds one rank\'s: gather the '
          'chains and use the host port, utils.diagnostics.summary(tt.gather().get(flatten=False)).')
REFUSALS = dict(
    {name: RANKED for name in ('rhat', 'ess', 'summary') + WITH_DENSITY},
    weighted_summary='the weights are normalised over the draws of ALL chains, and this TraceTuple holds one rank\'s: gather the chains '
                     'and use the host port, utils.weighted_summary(tt.gather().get(flatten=False), log_weights).',
    kde='the estimate is built from the draws of ALL chains, and this TraceTuple holds one rank\'s: gather the chains and use the host '
        'port, utils.kde(tt.gather().get(flatten=True)).',
    modes='the modes are those of the draws of ALL chains, and this TraceTuple holds one rank\'s: gather the chains and use the host '
          'port, utils.modes(tt.gather().get(flatten=True)).',
    parameter_shift='the difference sample pairs the draws of ALL chains, and this TraceTuple holds one rank\'s: gather the chains and '
                    'use the host port, utils.parameter_shift(tt.gather().get(flatten=True), other.gather().get(flatten=True)).')


def _call(tt, name, **kw):
    """The reader ``name`` with the least it needs besides the selection (a density it never gets to look at)."""
    first = dict(weighted_summary=(np.zeros(1),), data_lgo=(None, None), data_reweight=(None, None), parameter_shift=(tt,))
    return getattr(tt, name)(*first.get(name, (None,) if name in WITH_DENSITY else ()), **kw)


def _selected(tt, rng, sel):
    """(x (n_chain, n_t, d) as ``get`` selects it, the logp column (n_chain, n_t, 1), log weights (n_chain, n_t))."""
    x = tt.get(flatten=False, **sel)
    return x, tt.get(flatten=False, return_type='logp', **sel)[:, :, None], rng.normal(size=x.shape[:2])


def test_readers_are_the_utilities_on_the_selected_draws():
    """Everything but ``modes`` and ``marginals`` (below): the functions these readers call were public before them."""
    from bayesfast_amd.utils import acor, diagnostics
    from bayesfast_amd.utils.kde import kde
    from bayesfast_amd.utils.psis import weighted_summary
    from bayesfast_amd.utils.shift import parameter_shift
    tt, rng = trace()
    other = rng.normal(size=(50, 3)) * 10.
    for sel in SELECTIONS:
        x, lp, lw = _selected(tt, rng, sel)
        flat = x.reshape(-1, x.shape[-1])
        assert same(tt.integrated_time(quiet=True, **sel), acor.integrated_time(x, 5, 50, True))
        assert same(tt.integrated_time(quiet=True, return_type='logp', c=4, **sel), acor.integrated_time(lp, 4, 50, True))
        assert same(tt.rhat(**sel), diagnostics.rhat(x)) and same(tt.rhat(method='split', return_type='logp', **sel),
                                                                  diagnostics.rhat(lp, 'split'))
        assert same(tt.ess(**sel), diagnostics.ess(x)) and same(tt.ess(method='tail', prob=(0.1, 0.9), **sel),
                                                                diagnostics.ess(x, 'tail', (0.1, 0.9)))
        assert same(tt.summary(**sel), diagnostics.summary(x)) and same(tt.summary(return_type='logp', probs=(0.5,), **sel),
                                                                        diagnostics.summary(lp, (0.5,)))
        assert same(tt.weighted_summary(lw, **sel), weighted_summary(x, log_weights=lw))
        assert same(tt.weighted_summary(lw.reshape(-1), return_type='logp', probs=(0.1,), **sel),
                    weighted_summary(lp, log_weights=lw.reshape(-1), probs=(0.1,)))
        assert same(tt.kde(**sel).logpdf_loo(), kde(flat).logpdf_loo())
        assert same(tt.kde(lw, params=[2, 0], bw_method='silverman', **sel).logpdf_loo(),
                    kde(flat[:, [2, 0]], log_weights=lw.reshape(-1), bw_method='silverman').logpdf_loo())
        assert same(tt.parameter_shift(tt, n_pairs=256, **sel), parameter_shift(x, x, n_pairs=256))
        assert same(tt.parameter_shift(other, lw, n_pairs=256, params=[1], seed=3, **sel),
                    parameter_shift(x, other, log_weights_a=lw, n_pairs=256, params=[1], seed=3))


def test_modes_is_modes_by_chain():
    from bayesfast_amd.utils.kde import kde
    from bayesfast_amd.utils.modes import modes_by_chain, modes_from_seeds
    tt, rng = trace()
    for sel in SELECTIONS:
        x, _, lw = _selected(tt, rng, sel)
        assert same(tt.modes(**sel), modes_by_chain(x))
        assert same(tt.modes(lw, per_chain=3, seed=2, params=[0, 2], bw_factor=1.5, merge_tol=1e-2, **sel),
                    modes_by_chain(x, lw, per_chain=3, seed=2, params=[0, 2], bw_factor=1.5, merge_tol=1e-2))
    # the function itself: evenly spaced seeds of every chain, the majority vote, and a chain without weight
    x = tt.get(flatten=False)
    n_t = x.shape[1]
    out = modes_by_chain(x, per_chain=4)
    rows = (np.arange(6)[:, None] * n_t + ((np.arange(4) + 0.5) * n_t / 4).astype(np.int64)[None, :]).reshape(-1)
    assert np.array_equal(out.seed_index, rows) and same(out.label, modes_from_seeds(kde(x.reshape(-1, 3)), rows).label)
    label = out.label.reshape(6, 4)
    for c in range(6):
        got = label[c][label[c] >= 0]
        assert out.chain_mode[c] == (np.argmax(np.bincount(got)) if got.size else -1)
        assert out.chain_split[c] == (got.size > 0 and len(set(got.tolist())) > 1)
    assert set(out.chain_mode[:3].tolist()).isdisjoint(out.chain_mode[3:].tolist())     # the chains shifted by 4 sit elsewhere
    lw = np.zeros(x.shape[:2])
    lw[1] = -np.inf
    assert np.array_equal(modes_by_chain(x, lw, per_chain=2).seed_index[2:4], [n_t, n_t])


def test_marginals_is_marginals_of_shard():
    from bayesfast_amd.utils.marginals import OPTIONS, marginals, marginals_of_shard
    tt, rng = trace()
    for sel in SELECTIONS:
        x, _, lw = _selected(tt, rng, sel)
        assert same(tt.marginals(lw, bins=8, bins2d=4, **sel), marginals_of_shard(x, log_weights=lw, bins=8, bins2d=4))
        assert same(tt.marginals(**sel), marginals_of_shard(x))
        # without a process group the shard is the sample: ``marginals`` itself, with the same defaults
        assert same(tt.marginals(lw, bins=8, bins2d=4, **sel), marginals(x, log_weights=lw, bins=8, bins2d=4))
        assert same(tt.marginals(**sel), marginals(x, **OPTIONS))
    with pytest.raises(TypeError, match='unexpected options: binz.'):
        marginals_of_shard(tt.get(flatten=False), binz=3)


def test_what_the_readers_refuse(monkeypatch):
    from bayesfast_amd import parallel
    from bayesfast_amd.samplers.sample_trace import TraceTuple
    tt, _ = trace()
    readers = ('integrated_time', 'rhat', 'ess', 'summary', 'weighted_summary') + WITH_DENSITY + ('marginals', 'kde', 'modes',
                                                                                                   'parameter_shift')
    assert set(readers) == set(getattr(TraceTuple, 'READERS', readers)) and len(readers) == 14
    with pytest.raises(ValueError, match='since_iter is too large. Nothing to return.'):
        tt.get(since_iter=39)
    for name in readers:
        with pytest.raises(ValueError, match='since_iter is too large. Nothing to return.'):
            _call(tt, name, since_iter=39)
    for name in ('get', 'integrated_time', 'rhat', 'ess', 'summary', 'weighted_summary'):
        with pytest.raises(ValueError, match='invalid value for return_type.'):
            _call(tt, name, return_type='weights')
        with pytest.raises(ValueError, match='since_iter is too large. Nothing to return.'):     # the selection is looked at first
            _call(tt, name, return_type='weights', since_iter=39)
    with pytest.raises(TypeError, match='unexpected options: return_type.'):
        tt.marginals(return_type='logp')
    with pytest.raises(ValueError, match='per_chain should be at least 1.'):
        tt.modes(per_chain=0)
    monkeypatch.setattr(parallel, 'world', lambda: (0, 2))
    for name, words in REFUSALS.items():
        for kw in (dict(), dict(since_iter=39)):     # the refusal comes before the selection
            with pytest.raises(NotImplementedError) as ex:
                _call(tt, name, **kw)
            assert str(ex.value) == words, name
    assert len(REFUSALS) == 12
    for name in ('marginals', 'integrated_time'):    # the collectives do not refuse: they get as far as the selection
        with pytest.raises(ValueError, match='since_iter is too large. Nothing to return.'):
            _call(tt, name, since_iter=39)


def test_seam_forwards_every_reader():
    """The five that the seam lacked while it listed its forwards by hand -- weighted_summary, marginals, kde, modes and
    parameter_shift -- raised AttributeError there."""
    from oracle import reference
    if not reference.is_built():
        pytest.skip('needs the reference built into oracle/_ref by build()')
    from bayesfast_amd import integrate
    inner, rng = trace()
    tt = integrate.reference_classes(reference.load()).TraceTuple(inner, None)
    for name in inner.READERS:
        assert callable(getattr(tt, name)), name
        if name in WITH_DENSITY:     # (device parts only: as far as the inner reader's selection)
            with pytest.raises(ValueError, match='since_iter is too large. Nothing to return.'):
                _call(tt, name, since_iter=39)
    lw = rng.normal(size=(6, 20))
    sel = dict(since_iter=20)
    assert same(tt.integrated_time(quiet=True, **sel), inner.integrated_time(quiet=True, **sel))
    for name in ('rhat', 'ess', 'summary'):
        assert same(getattr(tt, name)(return_type='logp', **sel), getattr(inner, name)(return_type='logp', **sel))
    assert same(tt.weighted_summary(lw, **sel), inner.weighted_summary(lw, **sel))
    assert same(tt.marginals(lw, bins=8, bins2d=4, **sel), inner.marginals(lw, bins=8, bins2d=4, **sel))
    assert same(tt.kde(lw, **sel).logpdf_loo(), inner.kde(lw, **sel).logpdf_loo())
    assert same(tt.modes(lw, per_chain=3, seed=2, **sel), inner.modes(lw, per_chain=3, seed=2, **sel))
    want = inner.parameter_shift(inner, n_pairs=256, **sel)
    assert same(tt.parameter_shift(tt, n_pairs=256, **sel), want) and same(tt.parameter_shift(other=inner, n_pairs=256, **sel), want)
