"""HMC with a per-chain step size, a dense metric and step-size adaptation on the GPU (csrc/lv_mcmc.hip:
lv_hmc_metric_wave_kernel; lotka_volterra.hmc_metric_sample, hmc_warmup) against hmc_sample, against NumPy in the stated
order of operations (tests/hmc_adapt_ref.py) and against itself.

Error bounds, u = 2^-52 being one ulp relative: the device's exp, pow and sqrt are documented to
1 ulp (HIP math API), the host's exp and pow (the C library's, tests/hmc_adapt_ref.py) are within 1 ulp and sqrt is
correctly rounded.
  accept_stat: a is formed from the same values by the same operations, so alpha differs by the two exps only: 2 u alpha.
  dual averaging, one transition from the device's state and alpha: m and sbar exact (basic operations only);
    t = (sbar sqrt(m)) / gamma, ell = mu - t:      E_ell = 3 u |t| + u |ell|
    w = pow(m, -0.75):                              2 u w
    xbar' = (1 - w) xbar + w ell:                   E_x = (2 u w + 2 u) |xbar| + 3 u |w ell| + w E_ell + u |xbar'|
    eps' = exp(ell):                                eps' (3 u + E_ell)"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import convergence  # noqa: E402
from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import hmc_adapt_ref as A  # noqa: E402
from tests import hmc_ref as R  # noqa: E402

U = 2.0 ** -52
SEED = 20261021
T_NS = [1, 2, 63, 65, 130]
NAMES = ('samples', 'log_p', 'grad', 'accepted', 'n_failed')
ALL = NAMES + ('accept_stat', 'step_size')
CAP = 0.2
DELTA = 0.8
# every off-diagonal entry non-zero; with the first 130 observations the posterior is ~0.02 wide (test_gpu_lv_hmc.py)
LAM = np.array([[1.0, 0.0, 0.0, 0.0],
                [0.3, 0.9, 0.0, 0.0],
                [-0.2, 0.25, 1.1, 0.0],
                [0.15, -0.35, 0.2, 0.8]])


def _eps(n):
    return 0.012 + 0.002 * np.arange(n)              # differs between chains


@pytest.fixture(scope='module')
def data():
    return lv.reference_data()


def _cut(data, n):
    return lv.LvData(t=data.t[:n], y=data.y[:n], cov=data.cov, t_span=data.t_span, u_init=data.u_init)


def _starts(n):
    rng = np.random.default_rng(42)
    return np.log(lv.THETA) + 0.02 * rng.normal(size=(n, 4))


def _same(a, b, names=ALL, rows=slice(None)):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name)[rows], err_msg=name)


@pytest.mark.parametrize('which', ['fixed', 'failing'])
def test_identity_metric_is_hmc_sample_bit_for_bit(data, which):
    if which == 'fixed':
        (x0, z, log_u), kw = R.fixed_input(), dict(kick_cap=R.FIXED_CAP, data=data)
        n, eps, L = R.FIXED_ROWS, R.FIXED_EPS, R.FIXED_L
    else:
        (x0, z, log_u), kw = R.failing_input(), dict(kick_cap=R.FAIL_CAP, data=data, max_steps=R.failing_max_steps())
        n, eps, L = R.FAIL_ROWS, R.FAIL_EPS, R.FAIL_L
    want = lv.hmc_sample(x0, n, eps, L, noise=(z, log_u), **kw)
    got = lv.hmc_metric_sample(x0, n, eps, np.eye(4), L, noise=(z, log_u), **kw)
    _same(got, want, NAMES)
    print(which, 'accepted', got.accepted.tolist(), 'n_failed', got.n_failed.tolist())
    assert got.accept_stat.shape == got.step_size.shape == (x0.shape[0], n - 1)
    np.testing.assert_array_equal(got.step_size, eps)
    assert np.all((got.accept_stat >= 0) & (got.accept_stat <= 1))
    if which == 'failing':
        assert want.n_failed.sum() > 0
        failed = np.all(got.samples[:, 1:] == got.samples[:, :-1], axis=2)
        assert np.all(got.accept_stat[failed] == 0.0)          # a is NaN
    assert got.adapt_state is None and got.adapt_trace is None


@pytest.mark.parametrize('cap', [CAP, np.inf])
def test_dense_metric_one_stage_is_numpys_bit_for_bit(data, cap):
    sub = _cut(data, 130)
    x0 = R.fixed_input()[0]
    eps = _eps(5)
    run = lv.hmc_metric_sample(x0, 13, eps, LAM, 1, seed=SEED, kick_cap=cap, data=sub, return_noise=True)
    C, S = 5, 12
    e, lam = np.repeat(eps, S), np.tile(LAM, (C * S, 1, 1))
    g = run.grad[:, :-1].reshape(C * S, 4)
    f = np.stack([A.half_kick(g, np.ones(C * S), lam, np.full(4, np.inf))[:, j] * 2.0 for j in range(4)], axis=1)
    clipped = np.abs(e[:, None] * f) > cap
    rp = run.z.reshape(C * S, 4) + A.half_kick(g, e, lam, np.full(4, cap))
    prop = (run.samples[:, :-1].reshape(C * S, 4) + e[:, None] * A.velocity(rp, lam)).reshape(C, S, 4)
    moved = np.any(run.samples[:, 1:] != run.samples[:, :-1], axis=2)
    print('cap', cap, 'accepted', run.accepted.tolist(), 'clipped', int(clipped.sum()), 'of', clipped.size)
    if np.isfinite(cap):
        assert clipped.any() and not clipped.all()
    else:
        assert not clipped.any()
    assert moved.any() and run.n_failed.sum() == 0
    np.testing.assert_array_equal(run.accepted, moved.sum(axis=1))
    np.testing.assert_array_equal(run.samples[:, 1:][moved], prop[moved])
    for name in ('samples', 'log_p', 'grad'):                 # a rejected step repeats the row
        a = getattr(run, name)
        np.testing.assert_array_equal(a[:, 1:][~moved], a[:, :-1][~moved], err_msg=name)
    np.testing.assert_array_equal(run.step_size, np.repeat(eps[:, None], S, axis=1))


def _one_stage(q, r, eps, lam, cap, data):
    n = q.shape[0]
    return lv.hmc_metric_sample(q, 2, eps, lam, 1, noise=(r[:, None, :], np.full((n, 1), -np.inf)), kick_cap=cap,
                                data=data)


@pytest.mark.parametrize('n_leapfrog', [2, 3, 5])
def test_l_stages_are_l_chained_one_stage_steps_and_alpha_is_numpys(data, n_leapfrog):
    """tests/test_gpu_lv_hmc.py's scheme with the dense metric and per-chain eps: every step of a 5-chain, 13-row run
    is rebuilt from one-stage device calls; end point, log_p and grad are the trajectory's bits, the decision
    recomputed in NumPy is the device's, and accept_stat is NumPy's min(1, exp(a)) within 2 ulp (module docstring)."""
    sub = _cut(data, 130)
    eps5 = _eps(5)
    run = lv.hmc_metric_sample(R.fixed_input()[0], 13, eps5, LAM, n_leapfrog, seed=SEED, kick_cap=CAP, data=sub,
                               return_noise=True)
    assert run.n_failed.sum() == 0
    eps, lam, c = np.repeat(eps5, 12), np.tile(LAM, (60, 1, 1)), np.full(4, CAP)
    x, g, lp = (getattr(run, name)[:, :-1].reshape(60, -1) for name in ('samples', 'grad', 'log_p'))
    z, log_u = run.z.reshape(60, 4), run.log_u.reshape(60)
    q, r = x, z
    for stage in range(n_leapfrog):
        one = _one_stage(q, r, eps, lam, CAP, sub)
        assert one.accepted.tolist() == [1] * 60 and one.n_failed.sum() == 0
        np.testing.assert_array_equal(one.samples[:, 0], q)
        if stage == 0:
            np.testing.assert_array_equal(one.grad[:, 0], g)
            np.testing.assert_array_equal(one.log_p[:, 0], lp[:, 0])
        r = (r + A.half_kick(one.grad[:, 0], eps, lam, c)) + A.half_kick(one.grad[:, 1], eps, lam, c)
        q = one.samples[:, 1]
    a = (one.log_p[:, 1] - lp[:, 0]) + (A.kinetic(z) - A.kinetic(r))
    accept = log_u < a
    moved = np.any(run.samples[:, 1:] != run.samples[:, :-1], axis=2).reshape(60)
    alpha = A.accept_stat(a)
    got = run.accept_stat.reshape(60)
    ratio = np.abs(got - alpha) / (2 * U * alpha)
    print('L', n_leapfrog, 'accepted', run.accepted.tolist(), 'smallest |a - log_u|', np.abs(a - log_u).min(),
          'accept_stat: worst error / bound (2 ulp)', ratio.max(), 'alpha', alpha.min(), '..', alpha.max())
    np.testing.assert_array_equal(moved, accept)             # EVERY step
    assert moved.any()
    for name, end in (('samples', q), ('log_p', one.log_p[:, 1:2]), ('grad', one.grad[:, 1])):
        nxt = getattr(run, name)[:, 1:].reshape(60, -1)
        prev = getattr(run, name)[:, :-1].reshape(60, -1)
        np.testing.assert_array_equal(nxt[moved], end[moved], err_msg=name)
        np.testing.assert_array_equal(nxt[~moved], prev[~moved], err_msg=name)
    assert ratio.max() <= 1.0
    assert (alpha < 1).any()


def test_dual_averaging_transitions_are_numpys_within_the_bound(data):
    """steps_per_launch = 1: the state record after every step.  Each transition from the device's state with the
    device's alpha against tests/hmc_adapt_ref.da_update, within the module docstring's bounds; m and sbar exact; the
    recorded step_size[t] is the state's eps before step t."""
    sub = _cut(data, 130)
    x0 = _starts(5)
    eps = _eps(5)
    run = lv.hmc_metric_sample(x0, 13, eps, LAM, 2, seed=SEED, kick_cap=CAP, data=sub, target_accept=DELTA,
                               steps_per_launch=1, return_adapt_trace=True)
    assert run.adapt_trace.shape == (12, 5, 5)
    states = np.concatenate([lv.hmc_adapt_restart(eps)[None], run.adapt_trace])
    np.testing.assert_array_equal(run.adapt_state, states[-1])
    worst = np.zeros(3)
    for t in range(12):
        prev, nxt, alpha = states[t], states[t + 1], run.accept_stat[:, t]
        np.testing.assert_array_equal(run.step_size[:, t], prev[:, 0])
        want = A.da_update(prev, alpha, DELTA)
        m, sbar, mu = want[:, 1], want[:, 2], want[:, 4]
        np.testing.assert_array_equal(nxt[:, 1], m)
        np.testing.assert_array_equal(nxt[:, 1], t + 1.0)
        np.testing.assert_array_equal(nxt[:, 2], sbar)
        np.testing.assert_array_equal(nxt[:, 4], mu)
        tt = (sbar * np.sqrt(m)) / A.GAMMA
        ell = mu - tt
        e_ell = 3 * U * np.abs(tt) + U * np.abs(ell)
        w = A.elementwise(math.pow, m, -A.KAPPA)
        e_x = (2 * U * w + 2 * U) * np.abs(prev[:, 3]) + 3 * U * np.abs(w * ell) + w * e_ell + U * np.abs(want[:, 3])
        e_eps = want[:, 0] * (3 * U + e_ell)
        # ell itself is not stored; log(eps') recovers it to ~2 ulp and is not held to a bound
        worst = np.maximum(worst, [(np.abs(nxt[:, 3] - want[:, 3]) / e_x).max(),
                                   (np.abs(nxt[:, 0] - want[:, 0]) / e_eps).max(), 0.0])
    print('dual averaging: worst error / bound: xbar', worst[0], 'eps', worst[1], 'eps range',
          states[:, :, 0].min(), '..', states[:, :, 0].max(), 'accepted', run.accepted.tolist())
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert np.unique(states[1:, :, 0]).size > 12             # eps moves


@pytest.mark.parametrize('t_n', T_NS)
def test_launch_geometry_does_not_matter_while_adapting(data, t_n):
    sub = _cut(data, t_n)
    x0 = _starts(9)                                  # 9 chains: two full blocks of 4 waves and one wave
    eps = _eps(9)
    names = ALL + ('z', 'log_u', 'adapt_state')
    kw = dict(seed=SEED, kick_cap=CAP, data=sub, target_accept=DELTA)
    r = lv.hmc_metric_sample(x0, 13, eps, LAM, 3, return_noise=True, **kw)
    assert np.all(np.isfinite(r.log_p)) and np.all(np.isfinite(r.grad)) and r.n_failed.sum() == 0
    assert r.accepted.sum() > 0 and np.all(r.adapt_state[:, 1] == 12.0)
    for spl in (1, 5):                               # 12 steps: 12 launches; 5 + 5 + 2
        _same(lv.hmc_metric_sample(x0, 13, eps, LAM, 3, return_noise=True, steps_per_launch=spl, **kw), r, names)
    _same(lv.hmc_metric_sample(x0[4:], 13, eps[4:], LAM, 3, return_noise=True, first_chain=4, **kw), r, names,
          slice(4, None))
    _same(lv.hmc_metric_sample(x0, 13, eps, LAM, 3, **kw), r, ALL + ('adapt_state',))      # records nothing
    _same(lv.hmc_metric_sample(x0, 13, eps, LAM, 3, noise=(r.z, r.log_u), kick_cap=CAP, data=sub, target_accept=DELTA),
          r, ALL + ('adapt_state',))
    for n in (1, 4, 5):                              # one wave of four, a full block, a full block and one wave
        _same(lv.hmc_metric_sample(x0[:n], 13, eps[:n], LAM, 3, return_noise=True, **kw), r, names, slice(0, n))


def _ref_starts():
    return np.log(lv.THETA) + 0.02 * np.random.default_rng(7).standard_normal((5, 4))


def test_warmup_follows_the_schedule_on_the_reference_data(data):
    ad = lv.hmc_warmup(_ref_starts(), 150, 0.001, 4, seed=SEED, kick_cap=0.5, data=data)
    assert [(w.start, w.stop) for w in ad.windows] == [(75, 100)]
    assert ad.samples.shape == (5, 151, 4) and ad.step_sizes.shape == ad.accept_stat.shape == (5, 150)
    w = ad.windows[0]
    for c in range(5):
        want = A.regularised_cov(ad.samples[c, w.start + 1:w.stop + 1])
        got = ad.metric_chol[c] @ ad.metric_chol[c].T
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), c
    np.testing.assert_array_equal(ad.metric_chol, w.metric_chol)
    np.testing.assert_array_equal(w.step_size, lv.hmc_rescale_step(A.elementwise(math.exp, w.xbar), np.tile(np.eye(4), (5, 1, 1)),
                                                                   w.metric_chol))
    np.testing.assert_array_equal(ad.step_sizes[:, w.stop], w.step_size)
    np.testing.assert_array_equal(ad.step_sizes[:, 0], 0.001)
    np.testing.assert_array_equal(ad.last_row, ad.samples[:, -1])
    assert np.all(np.isfinite(ad.step_size)) and np.all(ad.step_size > 0) and ad.n_failed.sum() == 0
    print('eps after the window', w.step_size.tolist(), 'final', ad.step_size.tolist(), 'mean accept_stat',
          ad.accept_stat.mean(axis=1).tolist(), 'diag Lam', np.diagonal(ad.metric_chol, axis1=1, axis2=2)[0].tolist())
    run = lv.hmc_metric_sample(ad.last_row, 21, ad.step_size, ad.metric_chol, 4, seed=SEED + 1, kick_cap=0.5, data=data)
    sizes = np.concatenate([ad.step_sizes, run.step_size], axis=1)
    np.testing.assert_array_equal(sizes[:, 150:], np.repeat(ad.step_size[:, None], 20, axis=1))
    np.testing.assert_array_equal(run.samples[:, 0], ad.last_row)
    np.testing.assert_array_equal(run.log_p[:, 0], ad.log_p[:, -1])
    # the schedule does not depend on the launch split
    again = lv.hmc_warmup(_ref_starts(), 150, 0.001, 4, seed=SEED, kick_cap=0.5, data=data, steps_per_launch=7)
    for name in ('step_size', 'metric_chol', 'samples', 'log_p', 'grad', 'accept_stat', 'step_sizes'):
        np.testing.assert_array_equal(getattr(again, name), getattr(ad, name), err_msg=name)


def test_adapted_chains_have_a_larger_ess_than_the_fixed_step_sampler(data):
    """Same starts and seed, full data, L = 4, kick_cap 0.5: hmc_warmup of 300 steps then 500 draws, against hmc_sample
    at eps = 0.001 for 800 rows of which the last 500 are used (the same gradient evaluations).  The smallest bulk ESS
    over the four parameters of the adapted draws is strictly greater.  Recorded on MI355X: see DESIGN.md section 21."""
    x0 = _ref_starts()
    ad = lv.hmc_warmup(x0, 300, 0.001, 4, seed=SEED, kick_cap=0.5, data=data)
    draws = lv.hmc_metric_sample(ad.last_row, 501, ad.step_size, ad.metric_chol, 4, seed=SEED + 1, kick_cap=0.5,
                                 data=data)
    fixed = lv.hmc_sample(x0, 800, 0.001, 4, seed=SEED, kick_cap=0.5, data=data)
    ess_adapted = convergence.ess(draws.samples[:, 1:], 'bulk')
    ess_fixed = convergence.ess(fixed.samples[:, 300:], 'bulk')
    print('bulk ESS: adapted', ess_adapted.tolist(), 'fixed', ess_fixed.tolist(), 'eps', ad.step_size.tolist(),
          'acceptance adapted', (draws.accepted / 500).tolist(), 'fixed', (fixed.accepted / 799).tolist(),
          'n_failed', ad.n_failed.tolist(), draws.n_failed.tolist(), fixed.n_failed.tolist())
    assert draws.n_failed.sum() == 0 and fixed.n_failed.sum() == 0
    assert ess_adapted.min() > ess_fixed.min(), (ess_adapted, ess_fixed)


def test_bad_input(data):
    sub = _cut(data, 63)
    with pytest.raises(ValueError, match='starting point'):
        lv.hmc_metric_sample(np.array([800.0, 0.0, 0.0, 0.0]), 3, 0.003, np.eye(4), 2, seed=1, data=sub)
    with pytest.raises(ValueError, match='starting point'):
        lv.hmc_warmup(np.array([800.0, 0.0, 0.0, 0.0]), 20, 0.003, 2, seed=1, data=sub)
    bad = np.eye(4)
    bad[2, 2] = 0.0
    with pytest.raises(ValueError, match='positive diagonal'):
        lv.hmc_metric_sample(np.log(lv.THETA), 3, 0.003, bad, 2, seed=1, data=sub)
    upper = np.eye(4)
    upper[0, 3] = 0.1
    with pytest.raises(ValueError, match='lower triangular'):
        lv.hmc_metric_sample(np.log(lv.THETA), 3, 0.003, upper, 2, seed=1, data=sub)
    for wrong in (np.eye(3), np.ones((2, 4, 4)), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError, match='metric_chol'):
            lv.hmc_metric_sample(np.log(lv.THETA), 3, 0.003, wrong, 2, seed=1, data=sub)
    with pytest.raises(ValueError, match='step_size'):
        lv.hmc_metric_sample(_starts(3), 3, [0.003, 0.003], np.eye(4), 2, seed=1, data=sub)
    with pytest.raises(ValueError, match='target_accept'):
        lv.hmc_metric_sample(np.log(lv.THETA), 3, 0.003, np.eye(4), 2, seed=1, data=sub, target_accept=1.0)
    with pytest.raises(ValueError, match='n_warmup'):
        lv.hmc_warmup(np.log(lv.THETA), 19, 0.003, 2, seed=1, data=sub)
    one = lv.hmc_metric_sample(np.log(lv.THETA), 1, 0.003, np.eye(4), 2, seed=1, data=sub, target_accept=DELTA,
                               return_adapt_trace=True)
    assert one.samples.shape == (1, 1, 4) and one.accept_stat.shape == (1, 0) and one.step_size.shape == (1, 0)
    np.testing.assert_array_equal(one.adapt_state, lv.hmc_adapt_restart([0.003]))
    assert one.adapt_trace.shape == (0, 1, 5)
