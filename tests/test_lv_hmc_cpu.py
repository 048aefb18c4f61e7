"""HMC sampler, CPU tier: the host restatement (tests/hmc_ref.py) is reversible and second order, the conditions on
the fixed and the failing input that tests/test_gpu_lv_hmc.py relies on, and hmc_sample's argument checks (all
before the device is asked for)."""
import numpy as np
import pytest

from tests import hmc_ref as R

TIGHT = dict(rtol=1e-11, atol=1e-13)      # the integrator's error far below the leapfrog's (see the order test)


@pytest.fixture(scope='module')
def data():
    return R.reference_data()


@pytest.fixture(scope='module')
def near_mode(data):
    """A point 0.0002 off log(THETA) (the posterior's width there is ~0.0005) with its tight-tolerance gradient."""
    q0 = np.log(R.THETA) + 0.0002 * np.random.default_rng(5).standard_normal(4)
    ev = lambda x: R.evaluate(x, data, **TIGHT)             # noqa: E731
    lp0, g0, _ = ev(q0)
    return q0, lp0, g0, ev


def test_restated_leapfrog_is_reversible(near_mode):
    """Forward L stages, negate r, forward L stages: back at (q0, -r0).  In exact arithmetic exactly, g being a
    deterministic function of q.  Bound, derived: over the 2L stages every component of q takes 2L rounded
    additions q + eps r' (each within u S_q, u = 2^-53, S_q the largest |q_j| + |eps_j r'_j| met: the rounded
    product is far below the sum's own rounding) and every component of r takes 4L additions of a half kick (each
    within u S_r, S_r the largest |r_j| + |hk_j| met).  An error d in q changes every later kick by at most
    eps G d, G = the largest absolute row sum of dg/dq (measured by forward differences at q0), which the next
    position update carries back into q times eps: per stage an error grows by at most (1 + kappa), kappa =
    eps^2 G.  So |q - q0| <= 2L u S_q (1 + kappa)^(2L), and |r + r0| <= 4L u S_r (1 + kappa)^(2L) + 2L eps G times
    the bound on q.  Both are checked with a factor 2 for the rounding of hk itself (0.5 * clip(eps * g)).
    Recorded (L = 4, eps 0.0002): G 2.9e6, kappa 0.11; |q - q0| 8.1e-20 against 1.7e-15, |r + r0| 0 against 7.8e-12."""
    q0, _, g0, ev = near_mode
    L, eps, c = 4, np.full(4, 0.0002), np.full(4, np.inf)
    r0 = np.random.default_rng(11).standard_normal(4)
    d = 1e-7
    jac = np.stack([(ev(q0 + d * np.eye(4)[j])[1] - g0) / d for j in range(4)], axis=1)
    G = np.abs(jac).sum(axis=1).max()
    q1, _, g1, r1, pts, _, _ = R.trajectory(q0, g0, r0, eps, c, L, ev)
    q2, _, g2, r2, pts2, _, _ = R.trajectory(q1, g1, -r1, eps, c, L, ev)
    u = 2.0 ** -53
    kappa = float(eps[0] ** 2 * G)
    r_max = max(np.abs(r0).max(), np.abs(r1).max()) + 0.5 * eps[0] * max(np.abs(g0).max(), np.abs(g1).max())
    s_q = max(np.abs(pts).max(), np.abs(pts2).max(), np.abs(q0).max()) + eps[0] * r_max
    bound_q = 2 * (2 * L) * u * s_q * (1 + kappa) ** (2 * L)
    bound_r = 2 * (4 * L) * u * r_max * (1 + kappa) ** (2 * L) + 2 * L * eps[0] * G * bound_q
    err_q, err_r = np.abs(q2 - q0).max(), np.abs(r2 + r0).max()
    print('G', G, 'kappa', kappa, 'err q', err_q, 'bound', bound_q, 'err r', err_r, 'bound', bound_r)
    assert np.abs(q1 - q0).max() > 1e-4                     # the trajectory went somewhere
    assert err_q <= bound_q and err_r <= bound_r


def test_restated_leapfrog_is_second_order(near_mode):
    """With L eps = 0.0004 fixed, halving eps divides |dH| by ~4: inside (4 / sqrt 2, 4 sqrt 2), the geometric
    midpoints to orders 1 and 3.  The evaluations use rtol 1e-11, so the integrator's error in lp (~1e-9) is far
    below the smallest |dH| (2.5e-4).  Recorded: dH -1.60e-2, -4.05e-3, -1.01e-3 for L = 1, 2, 4; ratios 3.95, 3.99."""
    q0, lp0, g0, ev = near_mode
    r0 = R.fixed_input()[1][0, 0]
    dh = []
    for L in (1, 2, 4):
        eps = np.full(4, 0.0004 / L)
        _, lp, _, r, _, _, _ = R.trajectory(q0, g0, r0, eps, np.full(4, np.inf), L, ev)
        dh.append((lp0 - R.kinetic(r0)) - (lp - R.kinetic(r)))
    ratios = [dh[i] / dh[i + 1] for i in range(2)]
    print('dH', dh, 'ratios', ratios)
    assert min(abs(v) for v in dh) > 1e-6
    for ratio in ratios:
        assert 4 / np.sqrt(2) < ratio < 4 * np.sqrt(2), ratios


def test_one_stage_trajectories_chain_to_an_l_stage_one(near_mode):
    """The property the GPU test uses, on the host: L stages = L one-stage trajectories through (q, r), bit for bit."""
    q0, _, g0, ev = near_mode
    eps, c = np.array([0.0003, 0.0002, 0.0003, 0.0004]), np.full(4, 0.05)
    r0 = R.fixed_input()[1][1, 0]
    want = R.trajectory(q0, g0, r0, eps, c, 3, ev)
    q, g, r = q0, g0, r0
    for _ in range(3):
        q, lp, g, r, _, _, _ = R.trajectory(q, g, r, eps, c, 1, ev)
    for a, b in zip((q, lp, g, r), want[:4]):
        np.testing.assert_array_equal(a, b)
    assert want[6].any() and not want[6].all()              # the cap bites on some components


def test_fixed_input_holds_the_conditions_the_gpu_test_relies_on():
    """Conditions, not measurements: acceptance strictly between 0 and all in every chain, no failed trajectory, a
    clipped and an unclipped kick component both occur, and the smallest margin exceeds 1e-6.  Recorded: accepted
    7, 6, 2, 8, 8 of 12, smallest margin 1.0e-4, 635 of 720 kick components clipped."""
    ref = R.fixed_reference()
    steps = R.FIXED_ROWS - 1
    print('accepted', ref['accepted'].tolist(), 'min margin', ref['margins'].min(), 'clipped',
          int(ref['clipped'].sum()), 'of', ref['clipped'].size)
    assert (R.FIXED_CHAINS, steps, R.FIXED_L) == (5, 12, 3)
    assert ref['samples'].shape == (R.FIXED_CHAINS, R.FIXED_ROWS, 4) and ref['grad'].shape == ref['samples'].shape
    assert np.all(np.isfinite(ref['log_p'])) and np.all(np.isfinite(ref['grad']))
    assert np.all(ref['accepted'] > 0) and np.all(ref['accepted'] < steps)
    assert np.all(ref['n_failed'] == 0)
    assert np.isfinite(R.FIXED_CAP)
    assert ref['clipped'].any() and not ref['clipped'].all()
    assert ref['margins'].min() > 1e-6, ref['margins'].min()


def test_failing_input_fails_some_trajectories_and_not_all(data):
    """tests/mala_ref.failing_input()'s scheme with L = 2, from scipy alone: the start passes, some trajectories and
    not all have a stage that takes more accepted RK45 steps than max_steps, theta stays finite and positive at
    every evaluated stage, and no attempted RK45 step of any stage has an error norm within lv_ref.MARGIN_MIN of the
    accept threshold (so the kernel's step counts are scipy's).  A stage after a failed one is not evaluated (its q
    is NaN).  Recorded: 4, 7, 3 and 6 of the chains' 12 trajectories fail, 10 of them at stage 1; 21 .. 38 accepted
    steps against max_steps 33; smallest margin 6.7e-5."""
    from tests import lv_ref as LR
    x0, z, log_u = R.failing_input()
    max_steps = R.failing_max_steps()
    margin, counts = np.inf, []

    def ev(x):
        nonlocal margin
        if not np.all(np.isfinite(x)):
            return R.evaluate(x, data, max_steps=max_steps)
        with np.errstate(over='raise', under='raise'):
            theta = np.exp(x)
        assert np.all(np.isfinite(theta)) and np.all(theta > 0)
        sol = LR.solution(theta, sensitivity=True)
        margin = min(margin, sol.margin)
        counts.append(sol.accepted)
        out = R.evaluate(x, data, max_steps=max_steps)
        assert out[2] == sol.accepted and np.isnan(out[0]) == (sol.accepted > max_steps)
        return out

    out = [R.chain(x0[ch], z[ch], log_u[ch], R.FAIL_EPS, R.FAIL_CAP, R.FAIL_L, ev) for ch in range(R.FAIL_CHAINS)]
    res = R._stack(out)
    steps = R.FAIL_ROWS - 1
    bad = (res['counts'] > max_steps).any(axis=2)
    first_only = (res['counts'][:, :, 0] > max_steps)
    print('failed trajectories', bad.sum(axis=1).tolist(), 'of', steps, '(at stage 1:', int(first_only.sum()),
          '); accepted RK45 steps', min(counts), '..', max(counts), 'max_steps', max_steps, 'smallest margin', margin)
    assert np.all(np.isfinite(res['log_p'][:, 0]))
    assert 0 < bad.sum() < bad.size
    assert first_only.any() and (bad & ~first_only).any()    # a failure at the first and at the second stage
    np.testing.assert_array_equal(res['counts'][:, :, 1][first_only], 0)     # no integration after a failed stage
    np.testing.assert_array_equal(res['n_failed'], bad.sum(axis=1))         # once per trajectory
    np.testing.assert_array_equal(res['accepted'], (~bad).sum(axis=1))      # log_u = -inf accepts the rest
    assert margin > LR.MARGIN_MIN, margin


def test_hmc_sample_argument_checks_precede_the_device(monkeypatch):
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
        lv.hmc_sample(x0, 10, 0.01, seed=1)                                      # n_leapfrog has no default
    with pytest.raises(TypeError):
        lv.hmc_sample(x0, 10, seed=1)                                            # nor has step_size
    bad = [
        dict(n_leapfrog=0, seed=1),
        dict(n_leapfrog=-2, seed=1),
        dict(n_leapfrog=1.5, seed=1),
        dict(n_leapfrog=2.0, seed=1),
        dict(n_leapfrog=True, seed=1),
        dict(n_leapfrog=None, seed=1),
        dict(n_leapfrog=2 ** 31, seed=1),
        dict(seed=1, kick_cap=0.0),
        dict(seed=1, kick_cap=-1.0),
        dict(seed=1, kick_cap=float('nan')),
        dict(seed=1, kick_cap=None),
        dict(seed=1, kick_cap=True),
        # the shared checks
        dict(log_theta_init=np.zeros((5, 3)), seed=1),
        dict(log_theta_init=np.zeros((2, 5, 4)), seed=1),
        dict(log_theta_init=np.zeros((0, 4)), seed=1),
        dict(log_theta_init=np.full((5, 4), np.nan), seed=1),
        dict(n_samples=0, seed=1),
        dict(n_samples=-4, seed=1),
        dict(n_samples=2.5, seed=1),
        dict(step_size=0.0, seed=1),
        dict(step_size=-0.1, seed=1),
        dict(step_size=float('nan'), seed=1),
        dict(step_size=float('inf'), seed=1),
        dict(step_size=[0.1, 0.1, 0.1], seed=1),
        dict(step_size=[0.1, 0.1, 0.0, 0.1], seed=1),
        dict(),                                                                  # neither seed nor noise
        dict(seed=1, noise=(z, log_u)),                                          # both
        dict(seed=-1),
        dict(seed=2 ** 64),
        dict(seed=1.5),
        dict(n_samples=11, noise=(z, log_u)),                                    # 9 noise rows for 10 steps
        dict(log_theta_init=x0[:4], noise=(z, log_u)),
        dict(noise=(z[:, :, :3], log_u)),
        dict(noise=(z, log_u[:, :8])),
        dict(noise=(z,)),
        dict(seed=1, first_chain=-1),
        dict(seed=1, steps_per_launch=0),
        dict(seed=1, max_steps=0),
    ]
    for kw in bad:
        kw = dict(kw)
        args = [kw.pop('log_theta_init', x0), kw.pop('n_samples', 10), kw.pop('step_size', 0.01),
                kw.pop('n_leapfrog', 3)]
        with pytest.raises(ValueError):
            lv.hmc_sample(*args, data=small, **kw)
    # valid arguments get through every check: the next thing hmc_sample does is ask for the device
    for kw in (dict(seed=1), dict(seed=1, kick_cap=float('inf')), dict(seed=1, kick_cap=0.5), dict(seed=1, n_leapfrog=1),
               dict(seed=1, n_leapfrog=np.int64(7)), dict(noise=(z, log_u)),
               dict(seed=0, step_size=[0.01, 0.02, 0.03, 0.04])):
        kw = dict(kw)
        with pytest.raises(DeviceAsked):
            lv.hmc_sample(x0, 10, kw.pop('step_size', 0.01), kw.pop('n_leapfrog', 3), data=small, **kw)
    assert [lv.STEPS_PER_LAUNCH_HMC(L) for L in (1, 3, 64, 65)] == [64, 21, 1, 1]
    assert [f for f in lv.HmcSample.__dataclass_fields__] == ['samples', 'log_p', 'grad', 'accepted', 'n_failed',
                                                             'z', 'log_u']
