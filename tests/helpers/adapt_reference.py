"""The end of a sampler iteration restated in plain Python (TEST INFRASTRUCTURE ONLY): dual averaging of the step size
(``samplers/hmc_utils/step_size.py:31-45``), one element of the metric's running mean and variance (``metrics.py:354-360``) and the
metric's window logic (``metrics.py:181-211``).  ``tests/test_adapt_host.py`` holds ``csrc/bfhip_adapt.h`` to it bit for bit.

Python floats are IEEE doubles and every statement below rounds once per operation, which is what the helper's ``FUSED = false`` policy
does.  With ``fused=True`` the operations that the wave-per-chain kernels fuse are evaluated exactly and rounded once, which is what an
fma is."""
import math
from fractions import Fraction


def fma(a, b, c):
    """a * b + c rounded once (finite arguments)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class DualAveraging:
    """``DualAverageAdaptation`` while warming up.  ``count ** -k`` is taken as exp(-k log(count)), the form of every kernel (a power
    function is one more libm entry on the device); the two agree to an ulp or two and the test wants every bit."""

    def __init__(self, log_step, mu, target, gamma, k, t_0, fused=False):
        self.log_step = self.log_bar = log_step
        self.hbar = 0.
        self.mu, self.target, self.gamma, self.k, self.t_0 = mu, target, gamma, k, t_0
        self.count = 1.
        self.fused = fused

    def update(self, accept_stat):
        count = self.count
        w = 1. / (count + self.t_0)
        miss = self.target - accept_stat
        if self.fused:
            self.hbar = fma(w, miss, (1. - w) * self.hbar)
        else:
            self.hbar = (1. - w) * self.hbar + w * miss
        self.log_step = self.mu - self.hbar * math.sqrt(count) / self.gamma
        mk = math.exp(-self.k * math.log(count))
        if self.fused:
            self.log_bar = fma(mk, self.log_step, (1. - mk) * self.log_bar)
        else:
            self.log_bar = mk * self.log_step + (1. - mk) * self.log_bar
        self.count = count + 1.

    def state(self):
        return (self.hbar, self.log_step, self.log_bar, self.count)


class RunningVariance:
    """one element of ``_WeightedVariance`` fed samples of weight 1"""

    def __init__(self, n=10., mean=0., raw=0., fused=False):
        self.n, self.mean, self.raw, self.fused = n, mean, raw, fused

    def add(self, x):
        self.n += 1.
        old_diff = x - self.mean
        self.mean += old_diff / self.n
        new_diff = x - self.mean
        self.raw = fma(old_diff, new_diff, self.raw) if self.fused else self.raw + old_diff * new_diff


class MetricWindow:
    """the counters of ``QuadMetricDiagAdapt.update`` (``QuadMetricFullAdapt.update`` has the same): the foreground and background
    windows' weights, the samples seen, the sample of the last roll and the length of the adaptation window"""

    def __init__(self, fg_n, bg_n, n_samples, prev_upd, adapt_window, update_window, doubling):
        self.fg_n, self.bg_n, self.n_samples, self.prev_upd, self.adapt_window = fg_n, bg_n, n_samples, prev_upd, adapt_window
        self.update_window, self.doubling = update_window, doubling

    def update(self):
        """one warm-up sample -> (refresh, roll): whether the metric was recomputed from the foreground window, and whether the
        background window became the foreground one"""
        delta = self.n_samples - self.prev_upd
        self.fg_n += 1.
        self.bg_n += 1.
        refresh = (delta + 1) % self.update_window == 0
        roll = delta >= self.adapt_window
        if roll:
            self.fg_n = self.bg_n
            self.bg_n = 10.   # a fresh window's initial weight
            self.prev_upd = self.n_samples
            if self.doubling:
                self.adapt_window *= 2
        self.n_samples += 1
        return refresh, roll

    def state(self):
        return (self.fg_n, self.bg_n, self.n_samples, self.prev_upd, self.adapt_window)
