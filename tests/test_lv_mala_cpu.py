"""MALA sampler, CPU tier: the host restatement (tests/mala_ref.py) against finite differences of its own density,
the conditions on the fixed and the failing input that tests/test_gpu_lv_mala.py relies on, and mala_sample's
argument checks (all before the device is asked for)."""
import numpy as np
import pytest

from tests import mala_ref as R


@pytest.fixture(scope='module')
def data():
    return R.reference_data()


def test_gradient_matches_finite_differences_of_the_restated_density(data):
    """g = theta * grad_from_solution against central differences (half-width 1e-4 in log theta) of the density of
    the SAME 10-state solutions.  Tolerance, derived: the solver holds the local error of every accepted step to
    rtol |y| + atol, so after n accepted steps u and J = du/dtheta carry a relative error of up to about n * rtol
    (errors adding linearly), and g is linear in J and in y - u; the central difference differentiates the
    discretised density, whose error is of that order too.  So |g - fd| <= n * rtol * max|g| per point, n the
    accepted steps of that point's integration (32 at THETA: 3.2e-2).  Truncation (a near-Gaussian posterior has a
    small third derivative) and rounding (2e-16 * 1e3 / 1e-4 = 2e-9) are far below that."""
    x0, _, _ = R.fixed_input()
    delta = 1e-4
    for x in (np.log(R.THETA), x0[0], x0[3]):
        lp, g, n = R.evaluate(x, data)
        fd = np.empty(4)
        for j in range(4):
            e = np.zeros(4)
            e[j] = delta
            fd[j] = (R.evaluate(x + e, data)[0] - R.evaluate(x - e, data)[0]) / (2 * delta)
        err = np.abs(g - fd).max() / np.abs(g).max()
        print('steps', n, 'g', g, 'fd', fd, 'rel err', err)
        assert np.isfinite(lp) and n >= 20
        assert err <= n * 1e-3, (err, n)


def test_restated_gradient_is_theta_times_the_reference_gradient(data):
    """g_j = theta_j acc_j - x_j is exp(x) * grad_log_posterior(exp(x)) (theta * (-log theta / theta) = -x)."""
    from oracle import lv_numpy as ol
    x = R.fixed_input()[0][1]
    theta = np.exp(x)
    _, g, _ = R.evaluate(x, data)
    want = theta * ol.grad_log_posterior(theta, data.t, data.y, data.cov)
    np.testing.assert_allclose(g, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_fixed_input_holds_the_conditions_the_gpu_test_relies_on():
    """Conditions, not measurements: acceptance strictly between 0 and 1 in every chain, a clipped and an
    unclipped drift component both occur, and the smallest margin exceeds 1e-6 (the GPU test replays every step
    whose margin exceeds 1e-7 and may leave none out).  Recorded: accepted 4 .. 8 of 40, smallest margin 7.9e-5."""
    ref = R.fixed_reference()
    steps = R.FIXED_ROWS - 1
    print('accepted', ref['accepted'].tolist(), 'min margin', ref['margins'].min(), 'clipped',
          int(ref['clipped'].sum()), 'of', ref['clipped'].size)
    assert ref['samples'].shape == (R.FIXED_CHAINS, R.FIXED_ROWS, 4) and ref['grad'].shape == ref['samples'].shape
    assert np.all(np.isfinite(ref['log_p'])) and np.all(np.isfinite(ref['grad']))
    assert np.all(ref['accepted'] > 0) and np.all(ref['accepted'] < steps)
    assert np.all(ref['n_failed'] == 0)
    assert ref['clipped'].any() and not ref['clipped'].all()
    assert ref['margins'].min() > 1e-6, ref['margins'].min()


def test_failing_input_fails_some_proposals_and_not_all(data):
    """tests/mcmc_ref.failing_input()'s scheme for the 10-state system, from scipy alone: the start passes, some
    proposals and not all take more accepted steps than max_steps, theta stays finite and positive, and no
    attempted step of any proposal has an error norm within lv_ref.MARGIN_MIN of the accept threshold (so the
    kernel's step counts are scipy's).  Recorded: start 32 steps, proposals 22 .. 67, 47 of 80 fail, smallest
    margin 8.8e-4."""
    from oracle import lv_numpy as ol
    from tests import lv_ref as LR
    x0, z, log_u = R.failing_input()
    max_steps = R.failing_max_steps()
    assert max_steps == ol.n_steps(R.THETA, sensitivity=True) + R.FAIL_K
    eps, h, w, c = R.constants(R.FAIL_EPS, R.FAIL_CAP)
    failed, margin, counts = 0, np.inf, []
    for ch in range(4):
        x = x0[ch]
        lp, g, _ = R.evaluate(x, data, max_steps=max_steps)
        assert np.isfinite(lp)
        for k in range(20):
            p = (x + R.drift(g, h, c)) + eps * z[ch, k]
            with np.errstate(over='raise', under='raise'):
                theta = np.exp(p)
            assert np.all(np.isfinite(theta)) and np.all(theta > 0)
            sol = LR.solution(theta, sensitivity=True)
            margin = min(margin, sol.margin)
            counts.append(sol.accepted)
            lp_new, g_new, n = R.evaluate(p, data, max_steps=max_steps)
            assert n == sol.accepted
            if sol.accepted > max_steps:
                failed += 1
                assert np.isnan(lp_new)
            else:
                assert np.all(np.isfinite(g_new))       # log_u = -inf then accepts
                x, lp, g = p, lp_new, g_new
    print('failed', failed, 'of 80; accepted steps', min(counts), '..', max(counts), 'smallest margin', margin)
    assert 0 < failed < 80
    assert 20 <= failed <= 60, failed
    assert margin > LR.MARGIN_MIN, margin
    # the chain restatement counts the same failures
    got = sum(R.chain(x0[ch], z[ch], log_u[ch], R.FAIL_EPS, R.FAIL_CAP,
                      lambda x: R.evaluate(x, data, max_steps=max_steps))[4] for ch in range(4))
    assert got == failed


def test_mala_sample_argument_checks_precede_the_device(monkeypatch):
    from stein_thinning import _native
    from stein_thinning import lotka_volterra as lv

    class DeviceAsked(Exception):
        pass

    def asked():
        raise DeviceAsked

    monkeypatch.setattr(_native, 'require_device', asked)
    x0 = np.log(lv.THETA_INITS)
    z, log_u = np.zeros((5, 9, 4)), np.zeros((5, 9))
    small = lv.LvData(t=np.linspace(0.0, 25.0, 8), y=np.ones((8, 2)))
    with pytest.raises(TypeError):
        lv.mala_sample(x0, 10, seed=1)                                           # step_size has no default
    bad = [
        dict(log_theta_init=np.zeros((5, 3)), n_samples=10, seed=1),
        dict(log_theta_init=np.zeros((2, 5, 4)), n_samples=10, seed=1),
        dict(log_theta_init=np.zeros((0, 4)), n_samples=10, seed=1),
        dict(log_theta_init=np.full((5, 4), np.nan), n_samples=10, seed=1),
        dict(log_theta_init=x0, n_samples=0, seed=1),
        dict(log_theta_init=x0, n_samples=-4, seed=1),
        dict(log_theta_init=x0, n_samples=2.5, seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=0.0, seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=-0.1, seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=float('nan'), seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=float('inf'), seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=1e-200, seed=1),         # 0.5 / eps^2 overflows
        dict(log_theta_init=x0, n_samples=10, step_size=[0.1, 0.1, 0.1], seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=[0.1, 0.1, 0.0, 0.1], seed=1),
        dict(log_theta_init=x0, n_samples=10, seed=1, drift_cap=0.0),
        dict(log_theta_init=x0, n_samples=10, seed=1, drift_cap=-1.0),
        dict(log_theta_init=x0, n_samples=10, seed=1, drift_cap=float('nan')),
        dict(log_theta_init=x0, n_samples=10, seed=1, drift_cap=None),
        dict(log_theta_init=x0, n_samples=10),                                   # neither seed nor noise
        dict(log_theta_init=x0, n_samples=10, seed=1, noise=(z, log_u)),         # both
        dict(log_theta_init=x0, n_samples=10, seed=-1),
        dict(log_theta_init=x0, n_samples=10, seed=2 ** 64),
        dict(log_theta_init=x0, n_samples=10, seed=1.5),
        dict(log_theta_init=x0, n_samples=11, noise=(z, log_u)),                 # 9 noise rows for 10 steps
        dict(log_theta_init=x0[:4], n_samples=10, noise=(z, log_u)),
        dict(log_theta_init=x0, n_samples=10, noise=(z[:, :, :3], log_u)),
        dict(log_theta_init=x0, n_samples=10, noise=(z, log_u[:, :8])),
        dict(log_theta_init=x0, n_samples=10, noise=(z,)),
        dict(log_theta_init=x0, n_samples=10, seed=1, first_chain=-1),
        dict(log_theta_init=x0, n_samples=10, seed=1, steps_per_launch=0),
        dict(log_theta_init=x0, n_samples=10, seed=1, max_steps=0),
    ]
    for kw in bad:
        kw = dict(kw)
        kw.setdefault('step_size', 0.01)
        with pytest.raises(ValueError):
            lv.mala_sample(kw.pop('log_theta_init'), kw.pop('n_samples'), kw.pop('step_size'), data=small, **kw)
    # valid arguments get through every check: the next thing mala_sample does is ask for the device
    for kw in (dict(seed=1), dict(seed=1, drift_cap=float('inf')), dict(seed=1, drift_cap=0.5),
               dict(noise=(z, log_u)), dict(seed=0, step_size=[0.01, 0.02, 0.03, 0.04])):
        kw = dict(kw)
        with pytest.raises(DeviceAsked):
            lv.mala_sample(x0, 10, kw.pop('step_size', 0.01), data=small, **kw)
    assert isinstance(lv.STEPS_PER_LAUNCH_MALA, int) and lv.STEPS_PER_LAUNCH_MALA >= 1
    assert [f for f in lv.MalaSample.__dataclass_fields__] == ['samples', 'log_p', 'grad', 'accepted', 'n_failed',
                                                              'z', 'log_u']
