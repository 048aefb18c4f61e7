"""Random-walk Metropolis sampler, CPU tier: the host restatement of the generator (tests/mcmc_ref.py)
against np.random.Philox, the margins of the fixed input the GPU parity test compares row for row, the
st_lv_rwmh validation rules (all before any HIP call) and rw_sample's argument checks (all before the device
is asked for)."""
import ctypes

import numpy as np
import pytest

from tests import mcmc_ref as M

MOMENT_SEED = 7             # tests/test_gpu_lv_mcmc.py: the seed of the noise-moment test


def test_philox_restatement_matches_numpy():
    for seed, chain in [(0, 0), (1, 0), (12345, 7), (2 ** 64 - 1, 129), (987654321987654321, 2 ** 40 + 3)]:
        key = np.array([seed, chain], dtype=np.uint64)     # (a list with 2**64 - 1 would pass through float)
        want = np.random.Philox(key=key, counter=[0, 0, 0, 0]).random_raw(8 * 5)
        got = np.array([v for t in range(1, 6) for v in M.raw(seed, chain, t)], dtype=np.uint64)
        np.testing.assert_array_equal(got, want)


def test_noise_mapping():
    r = [0, (1 << 64) - 1, 1 << 63, 12345 << 11, 0, 0, 0, 0]
    z, log_u = M.noise_from_raw(r)
    assert log_u == -np.inf                       # a zero uniform always accepts
    assert np.all(np.isfinite(z))                 # u_k >= 2^-53: the radius is at most sqrt(2 * 53 ln 2) = 8.6
    assert abs(z[0]) <= 8.6 and abs(z[1]) <= 8.6
    z, log_u = M.noise_from_raw([(1 << 64) - 1] * 8)
    assert log_u < 0 and np.all(np.abs(z) < 1e-7)   # u = 1: radius 0


def test_fixed_input_keeps_its_margins():
    """The main GPU parity test compares chains row for row, which only holds while no accept / reject
    decision is closer than the error of the densities.  Every margin must exceed 1e-7, 10 times the 1e-8
    the project holds its LV values to against scipy; under that condition no decision is left out.
    Recorded here: acceptance counts 6 .. 24 of 40, smallest margin 2.1e-6."""
    samples, log_p, accepted, margins = M.fixed_reference()
    print('accepted', accepted.tolist(), 'min margin', margins.min())
    assert samples.shape == (10, 41, 4) and log_p.shape == (10, 41) and margins.shape == (10, 40)
    assert np.all(np.isfinite(log_p))
    assert margins.min() > 1e-7, margins.min()
    assert accepted.min() >= 1 and accepted.max() < 40      # both outcomes occur in every chain


def test_moment_seed_passes_on_the_host_by_a_wide_margin():
    """The seed of the GPU noise-moment test (4096 chains, 3 rows: 2 steps), chosen so that the host
    restatement is within 1 standard error where the GPU test allows 5 (seeds 1 .. 8 were tried on the host;
    7 gives 0.10, -0.08 and -0.80 standard errors)."""
    z, log_u = M.device_noise(MOMENT_SEED, 4096, 2)
    n = z.size
    u = np.exp(log_u)
    assert abs(z.mean()) < 1.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 1.0 * np.sqrt(2.0 / n)
    assert abs(u.mean() - 0.5) < 1.0 * np.sqrt(1.0 / 12.0 / u.size)


def test_failing_input_fails_between_a_quarter_and_three_quarters():
    """The conditions on the input of tests/test_gpu_lv_mcmc.py::
    test_failed_proposals_are_those_log_target_density_fails, from scipy alone: the start passes, between 20
    and 60 of the 80 proposals take more accepted steps than max_steps, theta stays finite and positive,
    and no attempted step of any proposal has an error norm within 1e-5 of the accept threshold (so the
    kernels' step counts are scipy's).  Recorded: start 23 steps, proposals 12 .. 45, 25 failures, smallest
    margin 2.9e-3."""
    from tests import lv_ref as R
    x0, z, _ = M.failing_input()
    max_steps = R.solution(M.THETA, sensitivity=False).accepted + M.FAIL_K
    assert max_steps == 23 + M.FAIL_K
    failed, margin, counts = 0, np.inf, []
    for c in range(4):
        x = x0[c]
        for k in range(20):
            p = x + M.FAIL_STEP * z[c, k]
            with np.errstate(over='raise', under='raise'):
                theta = np.exp(p)
            assert np.all(np.isfinite(theta)) and np.all(theta > 0)
            sol = R.solution(theta, sensitivity=False)
            margin = min(margin, sol.margin)
            counts.append(sol.accepted)
            if sol.accepted > max_steps:
                failed += 1
            else:
                x = p
    print('failed', failed, 'of 80; accepted steps', min(counts), '..', max(counts), 'smallest margin', margin)
    assert 20 <= failed <= 60, failed
    assert margin > R.MARGIN_MIN, margin


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_workspace_bytes(lib):
    assert lib.st_lv_rwmh_workspace_bytes(1) == 64
    assert lib.st_lv_rwmh_workspace_bytes(130) == 130 * 64
    assert lib.st_lv_rwmh_workspace_bytes(0) == -1 and lib.st_lv_rwmh_workspace_bytes(-3) == -1


def test_validation_happens_before_any_hip_call(lib):
    from stein_thinning import _native
    inv = _native.ST_ERR_INVALID
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    half = ctypes.c_void_p(p.value + 8)            # 8-byte aligned only
    step = (ctypes.c_double * 4)(0.0025, 0.0025, 0.0025, 0.0025)
    settings = (ctypes.c_double * 6)(0.0, 25.0, 1.0, 1.0, 1e-3, 1e-6)
    whiten = (ctypes.c_double * 4)(5.0, 0.0, 0.0, 5.0)
    names = ['state', 'chains', 'first_chain', 'first_step', 'steps', 'init', 'step_size', 'noise_mode', 'seed', 'z',
             'log_u', 'noise_ld', 'noise_row0', 't_eval', 't_n', 'y_obs', 'span_u0_tol', 'whiten', 'c_log',
             'norm_logc', 'max_steps', 'samples', 'log_p', 'out_ld', 'out_row0', 'stream']
    base = [p, 4, 0, 1, 8, 1, ctypes.cast(step, ctypes.c_void_p), 0, 0, p, p, 8, 0, p, 16, p,
            ctypes.cast(settings, ctypes.c_void_p), ctypes.cast(whiten, ctypes.c_void_p), 0.0, 0.9, 1000, p, p, 9, 1,
            None]
    assert len(names) == len(base)

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_lv_rwmh(*a)

    for name in ('state', 'samples', 'log_p', 't_eval', 'y_obs', 'step_size', 'span_u0_tol', 'whiten'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('state', 'samples', 'log_p', 't_eval', 'y_obs', 'z', 'log_u'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('state', 'samples', 'z'):           # the arrays written / read as 16-byte pairs
        assert call(**{name: half}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('chains', 'steps', 't_n'):
        for v in (0, -1):
            assert call(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
    assert call(first_step=0) == inv and b'first_step' in lib.st_last_error()
    assert call(first_step=-5) == inv
    assert call(first_chain=-1) == inv
    assert call(first_step=2) == inv and b'init' in lib.st_last_error()     # init continues nothing
    assert call(max_steps=0) == inv
    for bad in (0.0, -0.0025, float('inf'), float('nan')):
        for j in range(4):
            s = (ctypes.c_double * 4)(0.0025, 0.0025, 0.0025, 0.0025)
            s[j] = bad
            assert call(step_size=ctypes.cast(s, ctypes.c_void_p)) == inv, (bad, j)
            assert b'step size' in lib.st_last_error()
    # supplied noise (0) and recorded noise (2) need the arrays; device noise (1) does not ask for them
    for mode in (0, 2):
        assert call(noise_mode=mode, z=None) == inv and b'noise' in lib.st_last_error()
        assert call(noise_mode=mode, log_u=None) == inv and b'noise' in lib.st_last_error()
        assert call(noise_mode=mode, noise_ld=7) == inv and b'noise rows' in lib.st_last_error()
        assert call(noise_mode=mode, noise_row0=1) == inv
        assert call(noise_mode=mode, noise_row0=-1) == inv
    assert call(noise_mode=3) == inv and call(noise_mode=-1) == inv
    # output rows: init writes row out_row0 - 1, the steps rows out_row0 .. out_row0 + steps - 1
    assert call(out_row0=0) == inv and b'output rows' in lib.st_last_error()
    assert call(out_ld=8) == inv and b'output rows' in lib.st_last_error()
    assert call(out_row0=2) == inv
    bad_span = (ctypes.c_double * 6)(25.0, 0.0, 1.0, 1.0, 1e-3, 1e-6)
    assert call(span_u0_tol=ctypes.cast(bad_span, ctypes.c_void_p)) == inv
    bad_tol = (ctypes.c_double * 6)(0.0, 25.0, 1.0, 1.0, 0.0, 1e-6)
    assert call(span_u0_tol=ctypes.cast(bad_tol, ctypes.c_void_p)) == inv


def test_rw_sample_argument_checks_precede_the_device():
    from stein_thinning import lotka_volterra as lv
    x0 = np.log(lv.THETA_INITS)
    np.testing.assert_array_equal(lv.THETA_INITS, M.THETA_INITS)
    z, log_u = np.zeros((5, 9, 4)), np.zeros((5, 9))
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
        dict(log_theta_init=x0, n_samples=10, step_size=[0.1, 0.1, 0.1], seed=1),
        dict(log_theta_init=x0, n_samples=10, step_size=[0.1, 0.1, 0.0, 0.1], seed=1),
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
        with pytest.raises(ValueError):
            lv.rw_sample(kw.pop('log_theta_init'), kw.pop('n_samples'), **kw)
