"""The no-U-turn sampler without a GPU: the host restatement (tests/nuts_ref.py) of DESIGN.md section 22's definition --
its Philox blocks, its checkpoint scheme against a brute-force U-turn check, the distribution it targets, the warm-up
schedule driven through it -- and the argument errors of lotka_volterra.nuts_sample / nuts_warmup.

Bounds.  (a) Distribution: the mean and the variance of every coordinate lie within four batch-means standard errors
of the truth (30 batches; the standard error is the batch means' standard deviation / sqrt(30)).  That is a condition
on the committed seed, checked here, not a measurement.  (b) Warm-up: dual averaging gives, exactly, (m + t0) sbar_m =
sum_i (delta - alpha_i) (sbar_0 = 0, eta_i = 1 / (i + t0)) and sbar_m = gamma (mu - log eps_{m + 1}) / sqrt(m), so over
the m steps since a restart  mean(alpha) - delta = -((m + t0) / m) gamma (mu - log eps_{m + 1}) / sqrt(m).  With m = 50
(the final buffer), gamma = 0.05, t0 = 10 and a step size that has stayed within a factor 10 of mu's 10 eps_0 on
either side -- |mu - log eps| <= log 100 -- this is |mean(alpha) - delta| <= 1.2 * 0.05 * log(100) / sqrt(50) = 0.0391."""
import math

import numpy as np
import pytest

from tests import hmc_adapt_ref as A
from tests import nuts_ref as N

SEED = 20261021


def test_philox_blocks_with_two_counter_words_are_numpys():
    for s, c, t, ell in [(0, 0, 1, 1), (SEED, 3, 7, 2), (2 ** 64 - 1, 2 ** 40 + 5, 12345, 1023), (1, 2, 2 ** 33, 64)]:
        want = np.random.Philox(key=np.array([s, c], dtype=np.uint64),
                                counter=np.array([t - 1, ell, 0, 0], dtype=np.uint64)).random_raw(4)
        assert N.philox4x64_10(t, ell, s, c) == [int(v) for v in want], (s, c, t, ell)
    # word 1 = 0 is the existing streams' block
    want = np.random.Philox(key=[5, 6], counter=[0, 0, 0, 0]).random_raw(8)
    assert N.philox4x64_10(1, 0, 5, 6) + N.philox4x64_10(2, 0, 5, 6) == [int(v) for v in want]
    log_u, v, log_ut = N.tree_draws(SEED, 3, 7)(2)
    r = N.philox4x64_10(7, 2, SEED, 3)
    assert log_u == math.log((r[0] >> 11) * 2.0 ** -53) and log_ut == math.log((r[2] >> 11) * 2.0 ** -53)
    assert v == (1 if r[1] >> 63 == 0 else -1)


def _target(rho=0.8):
    """A correlated 4-D Gaussian: covariance, precision, ev."""
    sd = np.array([1.0, 0.5, 2.0, 1.5])
    corr = np.array([[1.0, rho, 0.3, 0.0], [rho, 1.0, 0.2, -0.4], [0.3, 0.2, 1.0, 0.5], [0.0, -0.4, 0.5, 1.0]])
    cov = corr * np.outer(sd, sd)
    return cov, A.gaussian(np.linalg.inv(cov))


def _chain(n_steps, eps, cap, max_depth, seed, chain=0, brute=False, lam=None):
    cov, ev = _target()
    lam = np.eye(4) if lam is None else lam
    c = np.full(4, float(cap))
    z = np.random.default_rng(seed).standard_normal((n_steps, 4))
    x = np.zeros(4)
    lp, g = (v[0] for v in ev(x[None]))
    stage = N.host_stage(ev, eps, lam, c)
    rows, steps = np.empty((n_steps, 4)), []
    for t in range(1, n_steps + 1):
        s = N.step(x, lp, g, z[t - 1], eps, lam, c, max_depth, N.tree_draws(seed, chain, t), stage, brute=brute)
        x, lp, g = s.x, s.lp, s.g
        rows[t - 1] = x
        steps.append(s)
    return cov, rows, steps


@pytest.mark.parametrize('max_depth', [1, 2, 3, 4, 5, 6])
def test_checkpoints_make_the_brute_force_checks_decisions(max_depth):
    _, _, steps = _chain(300, 0.25, np.inf, max_depth, SEED + max_depth, brute=True)
    checks = [c for s in steps for c in s.checks]
    reasons = {r: sum(s.reason == r for s in steps) for r in ('inner', 'whole', 'max_depth', 'divergent')}
    print('max_depth', max_depth, 'blocks tested', len(checks), 'turned', sum(a for a, _ in checks), 'reasons', reasons,
          'stages', sum(s.n_leapfrog for s in steps))
    assert all(a == b for a, b in checks)
    assert all(s.n_leapfrog <= 2 ** max_depth - 1 and s.tree_depth <= max_depth for s in steps)
    assert reasons['divergent'] == 0
    if max_depth >= 2:
        # a step of depth j has tested 2^j - 1 - j ... blocks: the scheme is exercised, with turns and without
        assert len(checks) > 100 and any(a for a, _ in checks) and not all(a for a, _ in checks)
        assert reasons['inner'] > 0
    if max_depth <= 2:
        assert reasons['max_depth'] > 0
    if max_depth >= 4:
        assert reasons['whole'] > 0
        assert any(s.reason == 'inner' and s.block < s.subtree for s in steps)


def _batch_se(v, batches=30):
    m = v[:v.size // batches * batches].reshape(batches, -1).mean(axis=1)
    return m.std(ddof=1) / math.sqrt(batches)


@pytest.mark.parametrize('cap', [0.25, np.inf])
def test_the_definition_targets_the_distribution(cap):
    """Module docstring (a).  eps 0.3; with cap 0.25 a fair share of the kicks is clipped (asserted)."""
    eps, n = 0.3, 3000
    cov, rows, steps = _chain(n, eps, cap, 5, SEED)
    _, ev = _target()
    force = np.abs(eps * ev(rows)[1])
    clipped = (force > cap).mean()
    dev_mean = [abs(rows[:, j].mean()) / _batch_se(rows[:, j]) for j in range(4)]
    dev_var = [abs((rows[:, j] ** 2).mean() - cov[j, j]) / _batch_se(rows[:, j] ** 2) for j in range(4)]
    print('cap', cap, 'clipped share of eps * g at the rows', clipped, 'deviation / standard error: mean', dev_mean,
          'variance', dev_var, 'mean accept_stat', np.mean([s.accept_stat for s in steps]), 'mean stages',
          np.mean([s.n_leapfrog for s in steps]), 'divergent', sum(s.divergent for s in steps))
    if np.isfinite(cap):
        assert 0.2 < clipped < 0.9
    else:
        assert clipped == 0.0
    assert max(dev_mean) < 4.0 and max(dev_var) < 4.0
    assert {v for s in steps for v in s.directions} == {1, -1}


def test_warmup_schedule_through_the_double_settles_near_delta():
    """Module docstring (b): lotka_volterra.hmc_warmup_schedule -- what nuts_warmup runs -- with a run_segment of NUTS
    steps of the double; the identity is checked to rounding, the bound follows from it."""
    from stein_thinning import lotka_volterra as lv
    delta, chains, n_warmup, eps0, max_depth = 0.8, 2, 150, 0.1, 5
    _, ev = _target()
    z = np.random.default_rng(SEED + 1).standard_normal((chains, n_warmup, 4))
    x = np.zeros((chains, 4))
    lp, g = ev(x)
    c = np.full(4, np.inf)
    alphas, eps_used, segments = np.empty((chains, n_warmup)), np.empty((chains, n_warmup)), []

    def run_segment(start, stop, chol, da):
        da = np.array(da, dtype=np.float64)
        mu = da[:, 4].copy()
        rows = np.empty((chains, stop - start, 4))
        for k in range(start, stop):
            for i in range(chains):
                s = N.step(x[i], lp[i], g[i], z[i, k], da[i, 0], chol[i], c, max_depth,
                           N.tree_draws(SEED + 1, i, k + 1), ev=ev)
                x[i], lp[i], g[i] = s.x, s.lp, s.g
                alphas[i, k], eps_used[i, k] = s.accept_stat, da[i, 0]
            da = A.da_update(da, alphas[:, k], delta)
            rows[:, k - start] = x
        segments.append((start, stop, mu, da[:, 0].copy()))
        return rows, da
    eps, chol, windows = lv.hmc_warmup_schedule(run_segment, n_warmup, eps0, np.tile(np.eye(4), (chains, 1, 1)),
                                                window_metric=A.window_metric)
    assert [(w.start, w.stop) for w in windows] == [(75, 100)] and [s[:2] for s in segments] == [(0, 75), (75, 100),
                                                                                                  (100, 150)]
    start, stop, mu, eps_next = segments[-1]
    m = stop - start
    mean = alphas[:, start:stop].mean(axis=1)
    log_next = A.elementwise(math.log, eps_next)
    identity = -((m + A.T0) / m) * A.GAMMA * (mu - log_next) / math.sqrt(m)
    print('final eps', eps.tolist(), 'mean accept_stat of the last window', mean.tolist(), 'identity', identity.tolist(),
          'eps in it', eps_used[:, start:stop].min(), '..', eps_used[:, start:stop].max(), '10 eps_0', np.exp(mu))
    np.testing.assert_allclose(mean - delta, identity, rtol=0, atol=1e-12)
    assert np.all(np.abs(mu - log_next) <= math.log(100.0))
    assert np.all(np.abs(mean - delta) <= 1.2 * 0.05 * math.log(100.0) / math.sqrt(50.0))
    np.testing.assert_array_equal(eps_used[:, 100], windows[0].step_size)
    assert np.all(np.isfinite(eps)) and np.all(eps > 0)


def test_steps_per_launch():
    from stein_thinning import lotka_volterra as lv
    assert [lv.STEPS_PER_LAUNCH_NUTS(d) for d in range(1, 11)] == [64, 21, 9, 4, 2, 1, 1, 1, 1, 1]


def test_argument_errors():
    from stein_thinning import lotka_volterra as lv
    x0 = np.log(lv.THETA)
    for fn, n in ((lv.nuts_sample, 5), (lv.nuts_warmup, 40)):
        for bad in (0, 11, -1, 2.0, True, None, '3'):
            with pytest.raises(ValueError, match='max_depth'):
                fn(x0, n, 0.01, max_depth=bad, seed=1)
        with pytest.raises(TypeError):
            fn(x0, n, 0.01, seed=1, noise=(np.zeros((1, 4, 4)), np.zeros((1, 4))))
        with pytest.raises(ValueError, match='seed'):
            fn(x0, n, 0.01)
        for bad in (0.0, -0.01, np.inf, np.nan, [0.01, 0.01]):
            with pytest.raises(ValueError, match='step_size'):
                fn(x0, n, bad, seed=1)
        for bad in (0.0, -1.0, np.nan, True):
            with pytest.raises(ValueError, match='kick_cap'):
                fn(x0, n, 0.01, seed=1, kick_cap=bad)
        for bad in (0.0, 1.0, 1.5):
            with pytest.raises(ValueError, match='target_accept'):
                fn(x0, n, 0.01, seed=1, target_accept=bad)
        upper = np.eye(4)
        upper[0, 3] = 0.1
        with pytest.raises(ValueError, match='lower triangular'):
            fn(x0, n, 0.01, metric_chol=upper, seed=1)
        with pytest.raises(ValueError, match='metric_chol'):
            fn(x0, n, 0.01, metric_chol=np.eye(3), seed=1)
    with pytest.raises(ValueError, match='n_warmup'):
        lv.nuts_warmup(x0, 19, 0.01, seed=1)
    with pytest.raises(TypeError):
        lv.nuts_sample(x0, 5, 0.01, np.eye(4), 4, seed=1)        # no positional trajectory length
