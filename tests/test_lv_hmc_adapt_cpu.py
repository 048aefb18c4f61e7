"""The host side of hmc_warmup without a GPU: the window list, the metric from a window, the step-size rescale, the
schedule driver on a NumPy test double (tests/hmc_adapt_ref.py) and that restatement against tests/hmc_ref.py."""
import functools
import math

import numpy as np
import pytest

from stein_thinning import lotka_volterra as lv
from tests import hmc_adapt_ref as A


def test_window_list_is_stans():
    assert lv.hmc_warmup_windows(1000) == [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)]
    assert lv.hmc_warmup_windows(150) == [(75, 100)]              # 75 + 25 + 50 fit exactly: one window
    assert lv.hmc_warmup_windows(100) == [(15, 90)]               # 15 % / 10 % / the rest
    assert lv.hmc_warmup_windows(20) == [(3, 18)]
    assert lv.hmc_warmup_windows(151) == [(75, 101)]              # the next window (50) would not fit: stretched
    assert lv.hmc_warmup_windows(200) == [(75, 100), (100, 150)]
    for bad in (19, 0, -5, 20.5, True):
        with pytest.raises(ValueError, match='n_warmup'):
            lv.hmc_warmup_windows(bad)


def test_metric_from_a_window_is_numpys_regularised_covariance():
    rng = np.random.default_rng(11)
    scale = np.array([1e-2, 3e-2, 1.0, 5.0])
    mix = np.linalg.qr(rng.standard_normal((4, 4)))[0]
    for n in (2, 3, 25, 400):
        rows = (rng.standard_normal((3, n, 4)) * scale) @ mix.T + rng.standard_normal((3, 1, 4))
        lam = lv.hmc_window_metric(rows)
        assert isinstance(lam, np.ndarray) and lam.shape == (3, 4, 4)
        for c in range(3):
            want = A.regularised_cov(rows[c])
            got = lam[c] @ lam[c].T
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (n, c)
            assert np.all(np.triu(lam[c], 1) == 0.0) and np.all(np.diag(lam[c]) > 0.0)
    with pytest.raises(ValueError):
        lv.hmc_window_metric(rows[:, :1])
    with pytest.raises(ValueError):
        lv.hmc_window_metric(rows[0])


def test_step_rescale_is_exact_on_diagonal_metrics():
    old = np.stack([np.eye(4), np.diag([2.0, 2.0, 2.0, 2.0]), np.diag([1.0, 4.0, 1.0, 4.0])])
    new = np.stack([np.diag([2.0, 2.0, 2.0, 2.0]), np.eye(4), np.diag([16.0, 1.0, 1.0, 16.0])])
    eps = np.array([0.5, 0.25, 3.0])
    # (det old / det new) ** (1 / 4): (1 / 16) ** .25 = 0.5, 16 ** .25 = 2, (16 / 256) ** .25 = 0.5
    np.testing.assert_array_equal(lv.hmc_rescale_step(eps, old, new), [0.25, 0.5, 1.5])
    np.testing.assert_array_equal(lv.hmc_rescale_step(eps, old, old), eps)
    # off-diagonal entries do not enter the determinant of a triangular factor
    low = new.copy()
    low[:, 3, 0] = 7.0
    np.testing.assert_array_equal(lv.hmc_rescale_step(eps, old, low), [0.25, 0.5, 1.5])


def test_restart_state():
    da = lv.hmc_adapt_restart([0.1, 0.002])
    np.testing.assert_array_equal(da[:, 0], [0.1, 0.002])
    np.testing.assert_array_equal(da[:, 1:4], 0.0)
    np.testing.assert_array_equal(da[:, 4], [math.log(10.0 * 0.1), math.log(10.0 * 0.002)])


# ---- the driver on the NumPy test double: a Gaussian target with condition number 1e4 ----
SEEDS, N_WARMUP, N_DRAWS, L, DELTA, EPS0 = 20, 500, 1000, 4, 0.8, 0.01
# mean alpha of the 1000 post-warm-up steps of the 20 seeds (chain c: default_rng(1000 + c)), as recorded from
# tests/hmc_adapt_ref.py run through lv.hmc_warmup_schedule (RECORDED below); the band is their [min, max] widened by half
# its width on each side
RECORDED = [0.9687, 0.9626, 0.9651, 0.9569, 0.9675, 0.9737, 0.9737, 0.9704, 0.9583, 0.9701, 0.9772, 0.9389, 0.9683, 0.9712,
            0.9575, 0.901, 0.9472, 0.9642, 0.9518, 0.9554]
_HALF = 0.5 * (max(RECORDED) - min(RECORDED))
BAND = (min(RECORDED) - _HALF, max(RECORDED) + _HALF)            # (0.8629, 1.0153)


EIGENVALUES = (1e-4, 1e-2, 1e-1, 1.0)                 # condition number 1e4
# an orthogonal matrix with exactly representable entries (a Hadamard matrix / 2): nothing is factorised
MIX = 0.5 * np.array([[1.0, 1.0, 1.0, 1.0], [1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0], [1.0, -1.0, -1.0, 1.0]])


def _mix(diagonal):
    """MIX diag(diagonal) MIX^T, every sum in a written order (no BLAS: the same bits on every CPU)."""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + (float(MIX[i, k]) * diagonal[k]) * float(MIX[j, k])
            out[i, j] = acc
    return out


def _sigma():
    return _mix(EIGENVALUES)


@functools.lru_cache(maxsize=None)
def _gaussian_run():
    """Everything below is bit-reproducible across CPUs (tests/hmc_adapt_ref.py's header): the recorded values are
    those of ANY machine, which is what lets a band taken from them hold."""
    sigma, precision = _sigma(), _mix([1.0 / v for v in EIGENVALUES])
    assert np.abs(sigma @ precision - np.eye(4)).max() < 1e-12
    assert np.linalg.cond(sigma) >= 1e4 * (1 - 1e-9)
    total = N_WARMUP + N_DRAWS
    z, log_u = np.empty((SEEDS, total, 4)), np.empty((SEEDS, total))
    x0 = np.empty((SEEDS, 4))
    for c in range(SEEDS):
        rng = np.random.default_rng(1000 + c)
        x0[c] = 0.1 * rng.standard_normal(4)
        z[c] = rng.standard_normal((total, 4))
        log_u[c] = A.elementwise(math.log, rng.random(total))
    chains = A.Chains(x0, A.gaussian(precision), lambda t: (z[:, t - 1], log_u[:, t - 1]), L, delta=DELTA)
    rows = []

    def run_segment(start, stop, lam, da):
        out = chains.run(start, stop, lam, da)
        rows.append(out[0])
        return out
    eps, lam, windows = lv.hmc_warmup_schedule(run_segment, N_WARMUP, EPS0, np.tile(np.eye(4), (SEEDS, 1, 1)),
                                               window_metric=A.window_metric)
    warm = np.concatenate(rows, axis=1)
    n_before = len(chains.alphas)
    for t in range(N_WARMUP + 1, total + 1):
        chains.step(t, eps, lam)
    alpha = np.array(chains.alphas[n_before:]).mean(axis=0)
    return eps, lam, windows, warm, alpha, np.array(chains.eps_used).T


def test_driver_on_a_gaussian_target_reaches_the_target_acceptance():
    """20 seeds, 500 warm-up steps from eps 0.01 and the identity metric, then 1000 steps at the adapted eps and
    metric; the mean alpha of those 1000 steps per seed, recorded from this restatement:
        0.9687 0.9626 0.9651 0.9569 0.9675 0.9737 0.9737 0.9704 0.9583 0.9701
        0.9772 0.9389 0.9683 0.9712 0.9575 0.9010 0.9472 0.9642 0.9518 0.9554
    The band is their [min, max] = [0.9010, 0.9772] widened by half its width on each side: (0.8629, 1.0153).  The
    chains are chaotic, so the band holds only because the run gives the same bits on every CPU (the header of
    tests/hmc_adapt_ref.py says how; with NumPy's exp and BLAS products in it, the same seeds gave 0.884 .. 0.984
    depending on the CPU's SIMD level).
    The band lies ABOVE delta = 0.8: while it adapts, the same restatement holds the mean alpha at 0.800 - 0.802 (3000
    steps on N(0, I), 8 seeds), but the schedule ends with exp(xbar) after a final buffer of only 50 steps from
    mu = log(10 eps), whose early, too-small iterates still weigh on the average (exp(xbar) 0.64 .. 0.87 here against
    ~1.05 after 3000 steps).  A final step size below the target's, so an acceptance above it, is what this schedule
    gives."""
    eps, lam, windows, warm, alpha, eps_used = _gaussian_run()
    print('mean alpha per seed', np.round(alpha, 4).tolist(), 'eps', eps.min(), '..', eps.max())
    lo, hi = BAND
    assert np.all(alpha > lo) and np.all(alpha < hi), (alpha.min(), alpha.max(), BAND)
    assert np.all(alpha > DELTA)


def test_driver_returns_the_last_windows_metric_and_follows_the_schedule():
    eps, lam, windows, warm, _, eps_used = _gaussian_run()
    assert [(w.start, w.stop) for w in windows] == lv.hmc_warmup_windows(N_WARMUP)
    assert warm.shape == (SEEDS, N_WARMUP, 4)
    last = windows[-1]
    for c in range(SEEDS):
        want = A.regularised_cov(warm[c, last.start:last.stop])
        got = lam[c] @ lam[c].T
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), c
    np.testing.assert_array_equal(lam, last.metric_chol)
    # the test double's metric is lv.hmc_window_metric's up to rounding, on every window of the run
    for w in windows:
        prod = lv.hmc_window_metric(warm[:, w.start:w.stop])
        got, want = w.metric_chol @ w.metric_chol.transpose(0, 2, 1), prod @ prod.transpose(0, 2, 1)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (w.start, w.stop)
    # every window: the step the chains went on with is the rescaled exp(xbar), and it is the eps of the next step
    old = np.tile(np.eye(4), (SEEDS, 1, 1))
    for w in windows:
        np.testing.assert_array_equal(w.step_size, lv.hmc_rescale_step(A.elementwise(math.exp, w.xbar), old, w.metric_chol))
        np.testing.assert_array_equal(eps_used[:, w.stop], w.step_size)
        old = w.metric_chol
    np.testing.assert_array_equal(eps_used[:, 0], EPS0)
    np.testing.assert_array_equal(eps_used[:, N_WARMUP:], np.repeat(eps[:, None], N_DRAWS, axis=1))
    # the adapted metric undoes the target's condition number (1e4) up to the regulariser and sampling error
    sigma = _sigma()
    for c in range(SEEDS):
        white = np.linalg.solve(lam[c], np.linalg.solve(lam[c], sigma).T)
        assert np.linalg.cond(white) < 1e2, (c, np.linalg.cond(white))


def test_metric_restatement_with_identity_is_hmc_refs_trajectory():
    """Lam = I, one eps: tests/hmc_ref.trajectory bit for bit on the first two steps of chain 0 of its fixed input
    (7 scipy integrations, shared between the two restatements)."""
    from tests import hmc_ref as R
    data = R.reference_data()
    x0, z, log_u = R.fixed_input()
    cache = {}

    def ev1(x):
        key = np.asarray(x, dtype=np.float64).tobytes()
        if key not in cache:
            cache[key] = R.evaluate(np.array(x), data)
        return cache[key]

    def ev(q):
        lp, g, _ = ev1(q[0])
        return np.array([lp]), np.array(g)[None]
    eps4, c = R.constants(R.FIXED_EPS, R.FIXED_CAP)
    x = x0[0].copy()
    lp, g, _ = ev1(x)
    eye, eps1 = np.eye(4)[None], np.array([R.FIXED_EPS])
    for k in range(2):
        q_r, lp_r, g_r, r_r, *_ = R.trajectory(x, g, z[0, k], eps4, c, R.FIXED_L, ev1)
        q_a, lp_a, g_a, r_a = A.trajectory(x[None], np.array(g)[None], z[0, k][None], eps1, eye, c, R.FIXED_L, ev)
        np.testing.assert_array_equal(q_a[0], q_r)
        np.testing.assert_array_equal(r_a[0], r_r)
        np.testing.assert_array_equal(g_a[0], g_r)
        assert lp_a[0] == lp_r
        k0, k1 = R.kinetic(z[0, k]), R.kinetic(r_r)
        assert A.kinetic(z[0, k][None])[0] == k0 and A.kinetic(r_a)[0] == k1
        ok, _ = R.decide(lp, lp_r, k0, k1, log_u[0, k])
        a = (lp_r - lp) + (k0 - k1)
        assert A.accept_stat(np.array([a]))[0] == min(1.0, math.exp(a))
        if ok:
            x, lp, g = q_r, lp_r, g_r
    assert len(cache) == 1 + 2 * R.FIXED_L


def test_accept_stat_and_dual_averaging_restatement():
    np.testing.assert_array_equal(A.accept_stat(np.array([np.nan, 0.0, 3.0, 800.0, -np.inf, np.log(0.25)])),
                                  [0.0, 1.0, 1.0, 1.0, 0.0, 0.25])
    # the first update from a restart, by hand: m = 1, eta = 1 / 11, sbar = (delta - alpha) / 11
    da = A.da_update(lv.hmc_adapt_restart([0.1]), np.array([0.3]), 0.8)
    sbar = (1.0 - 1.0 / 11.0) * 0.0 + (1.0 / 11.0) * (0.8 - 0.3)
    ell = math.log(10.0 * 0.1) - (sbar * 1.0) / 0.05
    np.testing.assert_array_equal(da[0], [math.exp(ell), 1.0, sbar, ell, math.log(10.0 * 0.1)])
