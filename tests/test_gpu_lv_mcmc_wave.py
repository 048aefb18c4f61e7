"""Wave-per-chain layout of the random-walk Metropolis sampler (csrc/lv_mcmc.hip: lv_rwmh_wave_kernel,
lotka_volterra.rw_sample(..., layout='wave')) against the host chain of tests/mcmc_ref.py and against the thread
layout.

Between the two layouts the proposals, the device noise and every per-point term of log_p are bit-identical; only
the order of the sum over the observation times differs (wave: lane l adds the points k = l mod 64 in increasing
k, then an xor butterfly over the 64 partial sums).  So log_p agrees within LP_RTOL, bit for bit where t_n <= 2,
and rows are compared exactly only where no decision can hang on that difference: on the fixed input (margins
above 1e-7, tests/test_lv_mcmc_cpu.py) or with log_u = -inf."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import mcmc_ref as M  # noqa: E402

RTOL = 1e-8          # the project's LV tolerance against scipy
LP_RTOL = 1e-8       # |log_p_wave - log_p_thread| <= LP_RTOL * max(|log_p_thread|, 1)
SEED = 20261020
NAMES = ('samples', 'log_p', 'accepted', 'n_failed')


@pytest.fixture(scope='module')
def data():
    return lv.reference_data()


@pytest.fixture(scope='module')
def fixed(data):
    """rw_sample on the fixed input (supplied noise) in the wave and in the thread layout, computed once."""
    x0, z, log_u = M.fixed_input()
    return (lv.rw_sample(x0, 41, M.STEP, noise=(z, log_u), data=data, layout='wave'),
            lv.rw_sample(x0, 41, M.STEP, noise=(z, log_u), data=data))


@pytest.fixture(scope='module')
def dev130(data):
    """130 chains of 13 rows with device noise, noise returned: 32 full blocks of 4 waves and one with 2."""
    x0 = _starts(130)
    return x0, lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, return_noise=True, layout='wave')


def _starts(n):
    rng = np.random.default_rng(42)
    return np.log(lv.THETA) + 0.02 * rng.normal(size=(n, 4))


def _same(a, b, names=NAMES):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def _lp_close(wave, thread):
    diff = np.abs(wave - thread)
    print('max |log_p wave - thread|', diff.max(), 'at |log_p| up to', np.abs(thread).max())
    assert np.all(diff <= LP_RTOL * np.maximum(np.abs(thread), 1.0)), diff.max()


def test_fixed_input_matches_the_host_chain(fixed):
    wave, _ = fixed
    samples, log_p, accepted, margins = M.fixed_reference()
    assert margins.min() > 1e-7
    err = np.abs(wave.log_p - log_p) / np.abs(log_p)
    print('max rel err of log_p', err.max(), 'accepted', wave.accepted.tolist())
    np.testing.assert_array_equal(wave.accepted, accepted)
    np.testing.assert_array_equal(wave.samples, samples)
    assert err.max() < RTOL, err.max()
    assert wave.n_failed.tolist() == [0] * 10
    assert wave.z is None and wave.log_u is None


def test_fixed_input_matches_the_thread_layout(fixed):
    wave, thread = fixed
    _same(wave, thread, ('samples', 'accepted', 'n_failed'))
    _lp_close(wave.log_p, thread.log_p)


@pytest.mark.parametrize('pick', [1, 2, 63, 64, 65, 130, 'every7th'])
def test_lanes_without_points_and_the_tail(data, pick):
    """Fewer points than lanes, exactly one round, one more, two rounds and two points, and 343 points spread
    over the whole span (5 rounds and 23 points, steps that hold fewer points than the wave has lanes).
    log_u = -inf accepts every proposal that has a density, so no decision depends on a margin."""
    sel = slice(0, pick) if pick != 'every7th' else slice(0, None, 7)
    sub = lv.LvData(t=data.t[sel], y=data.y[sel], cov=data.cov, t_span=data.t_span, u_init=data.u_init)
    t_n = sub.t.size
    assert t_n == (343 if pick == 'every7th' else pick)
    rng = np.random.default_rng(11)
    x0 = _starts(3)
    z = rng.standard_normal((3, 8, 4))
    log_u = np.full((3, 8), -np.inf)
    wave = lv.rw_sample(x0, 9, M.STEP, noise=(z, log_u), data=sub, layout='wave')
    thread = lv.rw_sample(x0, 9, M.STEP, noise=(z, log_u), data=sub)
    assert thread.accepted.tolist() == [8, 8, 8] and thread.n_failed.tolist() == [0, 0, 0]
    _same(wave, thread, ('samples', 'accepted', 'n_failed'))
    _lp_close(wave.log_p, thread.log_p)
    if t_n <= 2:                                   # the two summation orders coincide
        np.testing.assert_array_equal(wave.log_p, thread.log_p)


def test_launch_geometry_does_not_matter(dev130, data):
    x0, r = dev130
    names = NAMES + ('z', 'log_u')
    assert 0 < r.accepted.sum() < 130 * 12 and r.n_failed.sum() == 0
    split = lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, steps_per_launch=5, return_noise=True, layout='wave')
    _same(split, r, names)
    tail = lv.rw_sample(x0[64:], 13, M.STEP, seed=SEED, data=data, first_chain=64, return_noise=True, layout='wave')
    for name in names:
        np.testing.assert_array_equal(getattr(tail, name), getattr(r, name)[64:], err_msg=name)
    # without return_noise the kernel that records nothing draws the same noise
    _same(lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, layout='wave'), r)
    # the same chains from the recorded noise
    _same(lv.rw_sample(x0, 13, M.STEP, noise=(r.z, r.log_u), data=data, layout='wave'), r)
    # blocks that are mostly empty: 1 chain (one wave of four), 5 chains (a full block and one wave)
    for n in (1, 5):
        few = lv.rw_sample(x0[:n], 13, M.STEP, seed=SEED, data=data, return_noise=True, layout='wave')
        for name in names:
            np.testing.assert_array_equal(getattr(few, name), getattr(r, name)[:n], err_msg=(n, name))


def test_device_noise_equals_the_thread_layouts(dev130, data):
    x0, r = dev130
    thread = lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, return_noise=True)
    np.testing.assert_array_equal(r.z, thread.z)
    np.testing.assert_array_equal(r.log_u, thread.log_u)
    _lp_close(r.log_p[:, 0], thread.log_p[:, 0])                  # the start rows are the same points


def test_failed_proposals_are_those_log_target_density_fails(data):
    """tests/test_gpu_lv_mcmc.py's test of the same name, in the wave layout."""
    import warnings
    x0, z, log_u = M.failing_input()
    max_steps = 23 + M.FAIL_K                          # 23: the start row's accepted steps
    r = lv.rw_sample(x0, 21, M.FAIL_STEP, noise=(z, log_u), data=data, max_steps=max_steps, layout='wave')
    proposals = r.samples[:, :-1] + M.FAIL_STEP * z    # x + step * z: one multiply, one add, as the kernel
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        want = lv.log_target_density(proposals.reshape(-1, 4), data, max_steps=max_steps).reshape(4, 20)
    bad = np.isnan(want)
    print('failed proposals', bad.sum(axis=1).tolist())
    assert 20 <= bad.sum() <= 60
    repeats = np.all(r.samples[:, 1:] == r.samples[:, :-1], axis=2)
    np.testing.assert_array_equal(repeats, bad)
    np.testing.assert_array_equal(r.n_failed, bad.sum(axis=1))
    np.testing.assert_array_equal(r.samples[:, 1:][~bad], proposals[~bad])
    err = np.abs(r.log_p[:, 1:][~bad] - want[~bad]) / np.abs(want[~bad])
    print('max rel diff to log_target_density', err.max())
    assert err.max() < RTOL, err.max()
    np.testing.assert_array_equal(r.log_p[:, 1:][bad], r.log_p[:, :-1][bad])


def test_out_of_range_proposals_are_rejected_without_integrating(data):
    x0 = np.log(lv.THETA)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((1, 10, 4))
    log_u = np.log(rng.random((1, 10)))
    ref = lv.rw_sample(x0, 11, M.STEP, noise=(z, log_u), data=data, layout='wave')
    # two extra steps whose proposals land at log theta = +800 (exp: inf) and -800 (exp: 0); their log_u = -inf
    # would accept any proposal that had a density
    bad_hi = np.array([(800.0 - x0[0]) / M.STEP, 0.0, 0.0, 0.0])
    bad_lo = np.array([0.0, 0.0, (-800.0 - x0[2]) / M.STEP, 0.0])
    z2 = np.insert(z, [3, 6], [bad_hi, bad_lo], axis=1)
    log_u2 = np.insert(log_u, [3, 6], -np.inf, axis=1)
    got = lv.rw_sample(x0, 13, M.STEP, noise=(z2, log_u2), data=data, layout='wave')
    assert got.n_failed.tolist() == [2] and ref.n_failed.tolist() == [0]
    np.testing.assert_array_equal(got.accepted, ref.accepted)
    bad_rows = [4, 8]                                  # rows written by the inserted steps (noise rows 3 and 7)
    for row in bad_rows:
        np.testing.assert_array_equal(got.samples[0, row], got.samples[0, row - 1])
        assert got.log_p[0, row] == got.log_p[0, row - 1]
    # the chain goes on as if the two steps had not been there
    np.testing.assert_array_equal(np.delete(got.samples, bad_rows, axis=1), ref.samples)
    np.testing.assert_array_equal(np.delete(got.log_p, bad_rows, axis=1), ref.log_p)


def test_a_start_without_a_density_raises(data):
    with pytest.raises(ValueError, match='starting point'):
        lv.rw_sample(np.array([800.0, 0.0, 0.0, 0.0]), 3, seed=1, data=data, layout='wave')
    with pytest.raises(ValueError, match='starting point'):          # the integration runs out of steps
        lv.rw_sample(np.log(lv.THETA), 3, seed=1, data=data, max_steps=3, layout='wave')
    one = lv.rw_sample(np.log(lv.THETA), 1, seed=1, data=data, return_noise=True, layout='wave')
    assert one.samples.shape == (1, 1, 4) and one.log_p.shape == (1, 1) and one.z.shape == (1, 0, 4)
    assert one.accepted.tolist() == [0] and one.n_failed.tolist() == [0]


def test_auto_layout(dev130, data, monkeypatch):
    """'auto' is 'wave' up to WAVE_MAX_CHAINS chains and 'thread' beyond.  The threshold is set for the test so
    that both sides are exercised whatever value the measurement gave the constant (0 keeps 'auto' on the
    thread layout); the module's own value is then used as it is."""
    x0, r = dev130
    few = {name: getattr(r, name)[:5] for name in NAMES}
    monkeypatch.setattr(lv, 'WAVE_MAX_CHAINS', 5)
    auto = lv.rw_sample(x0[:5], 13, M.STEP, seed=SEED, data=data, layout='auto')
    for name in NAMES:
        np.testing.assert_array_equal(getattr(auto, name), few[name], err_msg=name)
    _same(lv.rw_sample(x0[:6], 2, M.STEP, seed=SEED, data=data, layout='auto'),
          lv.rw_sample(x0[:6], 2, M.STEP, seed=SEED, data=data, layout='thread'))
    monkeypatch.undo()
    n = lv.WAVE_MAX_CHAINS + 1
    xs = _starts(n)
    _same(lv.rw_sample(xs, 2, M.STEP, seed=SEED, data=data, layout='auto'),
          lv.rw_sample(xs, 2, M.STEP, seed=SEED, data=data, layout='thread'))
    if lv.WAVE_MAX_CHAINS >= 5:
        _same(lv.rw_sample(x0[:5], 13, M.STEP, seed=SEED, data=data, layout='auto'),
              lv.rw_sample(x0[:5], 13, M.STEP, seed=SEED, data=data, layout='wave'))
    d = lv.rw_sample(x0[:5], 13, M.STEP, seed=SEED, data=data, device_out=True, layout='wave')
    assert d.samples.is_cuda and d.log_p.is_cuda and d.accepted.dtype == torch.int64
    np.testing.assert_array_equal(d.samples.cpu().numpy(), few['samples'])
    np.testing.assert_array_equal(d.accepted.cpu().numpy(), few['accepted'])
