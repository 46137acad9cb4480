"""The device integrated autocorrelation time (csrc/bfhip_acor.hip through utils/acor.py): the reference's recorded values, the
host port on a grid of shapes, AR(1) coefficients and odd cases, strided input, repeatability, ``TraceTuple.integrated_time``
after ``sample()``, and the full 4096 x 1000 x 64 size."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _ar1(rng, phi, n_w, n_t, n_d):
    e = rng.normal(size=(n_w, n_t, n_d))
    for t in range(1, n_t):
        e[:, t] = phi * e[:, t - 1] + np.sqrt(1 - phi * phi) * e[:, t]
    return e


def test_golden_fixture_on_the_device():
    from bayesfast_amd.utils import integrated_time
    fx = np.load(os.path.join(G, 'evidence.npz'))
    np.testing.assert_allclose(integrated_time(_dev(fx['acor.x'])), fx['acor.tau3'], rtol=1e-10)
    np.testing.assert_allclose(integrated_time(_dev(fx['acor.x'][0])), fx['acor.tau2'], rtol=1e-10)
    np.testing.assert_allclose(integrated_time(_dev(fx['acor.x'][1, :, 0])), fx['acor.tau1'], rtol=1e-10)


@pytest.mark.parametrize('shape', [(1, 3000, 1), (7, 1, 3), (5, 2, 2), (16, 63, 5), (64, 1000, 3), (9, 777, 130)])
def test_shape_grid_matches_the_host_port(shape):
    """AR(1) at 0, 0.5, 0.9 and 0.98 across the dimensions, a constant dimension (NaN in the same places), float32 input."""
    from bayesfast_amd.utils.acor import integrated_time
    rng = np.random.default_rng(sum(shape))
    n_w, n_t, n_d = shape
    phis = np.array([0., 0.5, 0.9, 0.98])[np.arange(n_d) % 4]
    x = np.stack([_ar1(rng, p, n_w, n_t, 1)[:, :, 0] for p in phis], axis=-1)
    if n_d > 2:
        x[:, :, 1] = 2.5
    with np.errstate(invalid='ignore', divide='ignore'):
        want = integrated_time(x, quiet=True)
    got = integrated_time(_dev(x), quiet=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    x32 = x.astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        np.testing.assert_allclose(integrated_time(_dev(x32), quiet=True), integrated_time(x32, quiet=True), rtol=1e-10, atol=1e-12)


def test_long_windows_errors_and_c():
    """Random walks: windows far beyond the first block (c = 5) and closing only in the block that reaches the end of the series
    (c = 100); AutocorrError with the host port's .tau; c <= 0 closes the window at lag 0 (tau = 1).  (A centred series' running
    sum returns to 0 at the last lag, so Sokal's window closes there at the latest: it stays open only for n_t = 1, whose tau is
    NaN, and for a NaN series -- both in the shape grid.)"""
    from bayesfast_amd.utils.acor import integrated_time, AutocorrError
    rng = np.random.default_rng(2)
    x = np.cumsum(rng.normal(size=(3, 300, 2)), axis=1)
    with pytest.raises(AutocorrError) as host:
        integrated_time(x)
    with pytest.raises(AutocorrError) as dev:
        integrated_time(_dev(x))
    np.testing.assert_allclose(dev.value.tau, host.value.tau, rtol=1e-10)
    assert np.all(dev.value.tau > 20)
    np.testing.assert_allclose(integrated_time(_dev(x), c=100, quiet=True), integrated_time(x, c=100, quiet=True), rtol=1e-10)
    for c in (0, -2.):
        assert np.array_equal(integrated_time(_dev(x), c=c), [1., 1.])


def test_quiet_logs_a_warning(caplog):
    from bayesfast_amd.utils.acor import integrated_time
    x = _ar1(np.random.default_rng(3), 0.9, 4, 200, 2)
    with caplog.at_level(logging.WARNING):
        tau = integrated_time(_dev(x), quiet=True)
    assert 'shorter than 50 times' in caplog.text
    np.testing.assert_allclose(tau, integrated_time(x, quiet=True), rtol=1e-10)


def test_strided_view_is_bitwise_its_contiguous_copy_and_calls_repeat():
    from bayesfast_amd.utils.acor import integrated_time
    x = _dev(_ar1(np.random.default_rng(4), 0.9, 40, 1500, 20))
    v = x[:, 137:]
    assert not v.is_contiguous()
    a, b = integrated_time(v, quiet=True), integrated_time(v.contiguous(), quiet=True)
    assert a.tobytes() == b.tobytes()
    assert integrated_time(v, quiet=True).tobytes() == a.tobytes()


def test_trace_tuple_integrated_time_after_sample():
    """A few hundred chains on the banana of workloads, with input scales (two spaces): tau of both spaces, of logp, with since_iter
    and include_warmup, against the host port on tt.get(flatten=False)."""
    from bayesfast_amd import PolyModel, SurrogateDensity, sample, NTrace
    from bayesfast_amd.utils.acor import integrated_time
    from bayesfast_amd.workloads import banana_logp
    d = 4
    logp = banana_logp(d, q=0.5, seed=1)
    rng = np.random.default_rng(5)
    su = PolyModel('quadratic', input_size=d, output_size=1)
    den = SurrogateDensity(su, input_scales=np.stack([-4. * np.ones(d), 5. * np.ones(d)], 1))
    xf = rng.normal(size=(200, d))
    den.fit(xf, logp(xf))
    tt = sample(den, NTrace(n_chain=300, n_iter=400, n_warmup=100, x_0=rng.normal(size=(300, d)) * 0.3, random_generator=7),
                verbose=False)
    cases = [dict(), dict(original_space=False), dict(since_iter=250), dict(include_warmup=True),
             dict(return_type='logp'), dict(return_type='logp', original_space=False, since_iter=150)]
    for kw in cases:
        want = integrated_time(tt.get(flatten=False, **kw)[..., None] if kw.get('return_type') == 'logp' else
                               tt.get(flatten=False, **kw), quiet=True)
        np.testing.assert_allclose(tt.integrated_time(quiet=True, **kw), want, rtol=1e-10, err_msg=str(kw))
    with pytest.raises(ValueError):
        tt.integrated_time(since_iter=399)
    with pytest.raises(ValueError):
        tt.integrated_time(return_type='all')


def test_full_size_ar1_on_the_device():
    """4096 x 1000 x 64 AR(1) generated on the device (phi = 0.5 for even dimensions, 0.3 for odd): tau within a few percent of
    (1 + phi) / (1 - phi) (the estimator's own bias at 1000 steps, from each walker's mean and the window, is about -2 W tau / n_t:
    -4 % at phi = 0.5), and the host port on two of the dimensions."""
    import torch
    from bayesfast_amd.utils.acor import integrated_time
    n_w, n_t, n_d = 4096, 1000, 64
    g = torch.Generator(device='cuda').manual_seed(11)
    phi = torch.where(torch.arange(n_d, device='cuda') % 2 == 0, 0.5, 0.3).to(torch.float64)
    e = torch.randn((n_w, n_t, n_d), generator=g, device='cuda', dtype=torch.float64)
    x = torch.empty_like(e)
    x[:, 0] = e[:, 0]
    s = torch.sqrt(1 - phi * phi)
    for t in range(1, n_t):
        x[:, t] = phi * x[:, t - 1] + s * e[:, t]
    del e
    tau = integrated_time(x)
    want = ((1 + phi) / (1 - phi)).cpu().numpy()
    assert np.all(np.abs(tau / want - 1) < 0.06), tau
    host = integrated_time(x[:, :, :2].cpu().numpy())
    np.testing.assert_allclose(tau[:2], host, rtol=1e-10)
