"""Random-walk Metropolis sampler on the GPU (csrc/lv_mcmc.hip, lotka_volterra.rw_sample) against the host
restatement of tests/mcmc_ref.py: the Metropolis loop over oracle.lv_numpy.log_target_density (scipy) and the
Python Philox4x64-10 / noise mapping.

The main parity test compares chains row for row.  That holds because every accept / reject decision of the
fixed input has a relative margin above 1e-7 (tests/test_lv_mcmc_cpu.py asserts it; smallest 2.1e-6) while the
densities agree with scipy to RTOL = 1e-8; the proposal x + step * z is one multiply and one add on both sides,
so accepted rows are equal bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import mcmc_ref as M  # noqa: E402
from tests.test_lv_mcmc_cpu import MOMENT_SEED  # noqa: E402

RTOL = 1e-8          # observed on MI355X: log_p 1.4e-11 against the scipy chain, 2.3e-12 against
#                      log_target_density (the pairwise-ordered sum); device noise 4.4e-16 absolute
NOISE_ATOL = 1e-13   # the angle 2 pi u carries ~7e-16 of rounding, the radius is at most 8.6, the device
#                      functions are good to a few ulp: ~1e-14, and 10 times that is allowed
SEED = 20261020


@pytest.fixture(scope='module')
def data():
    return lv.reference_data()


@pytest.fixture(scope='module')
def fixed(data):
    """rw_sample on the fixed input (supplied noise), computed once."""
    x0, z, log_u = M.fixed_input()
    return lv.rw_sample(x0, 41, M.STEP, noise=(z, log_u), data=data)


@pytest.fixture(scope='module')
def dev130(data):
    """130 chains (two full waves and a partial one) of 13 rows with device noise, noise returned."""
    x0 = _starts(130)
    return x0, lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, return_noise=True)


def _starts(n):
    rng = np.random.default_rng(42)
    return np.log(lv.THETA) + 0.02 * rng.normal(size=(n, 4))


def _same(a, b):
    for name in ('samples', 'log_p', 'accepted', 'n_failed'):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def test_fixed_input_matches_the_host_chain(fixed):
    samples, log_p, accepted, margins = M.fixed_reference()
    assert margins.min() > 1e-7
    err = np.abs(fixed.log_p - log_p) / np.abs(log_p)
    print('max rel err of log_p', err.max(), 'accepted', fixed.accepted.tolist())
    np.testing.assert_array_equal(fixed.accepted, accepted)
    np.testing.assert_array_equal(fixed.samples, samples)
    assert err.max() < RTOL, err.max()
    assert fixed.n_failed.tolist() == [0] * 10
    assert fixed.z is None and fixed.log_u is None
    # chains c and c + 5 share their noise but not their starts
    assert not np.array_equal(fixed.samples[0], fixed.samples[5])


def test_result_is_consistent_with_itself(fixed, data):
    s, lp = fixed.samples, fixed.log_p
    want = lv.log_target_density(s.reshape(-1, 4), data).reshape(lp.shape)
    err = np.abs(lp - want) / np.abs(want)
    print('max rel diff to log_target_density', err.max())
    assert err.max() < 1e-8, err.max()
    changed = np.any(s[:, 1:] != s[:, :-1], axis=2)
    np.testing.assert_array_equal(changed.sum(axis=1), fixed.accepted)
    # a rejected row repeats its predecessor's log_p bit for bit
    np.testing.assert_array_equal(lp[:, 1:][~changed], lp[:, :-1][~changed])
    assert np.all(lp[:, 1:][changed] != lp[:, :-1][changed])
    np.testing.assert_array_equal(s[:, 0], M.fixed_input()[0])


def test_device_noise_matches_the_host_generator(dev130, data):
    x0, r = dev130
    z, log_u = M.device_noise(SEED, 130, 12)
    assert r.z.shape == (130, 12, 4) and r.log_u.shape == (130, 12)
    print('max abs err z', np.abs(r.z - z).max(), 'log_u', np.abs(r.log_u - log_u).max())
    assert np.abs(r.z - z).max() < NOISE_ATOL
    assert np.abs(r.log_u - log_u).max() < NOISE_ATOL
    assert 0 < r.accepted.sum() < 130 * 12
    # the same chains from the recorded noise: bit-identical
    again = lv.rw_sample(x0, 13, M.STEP, noise=(r.z, r.log_u), data=data)
    _same(again, r)


def test_launch_geometry_does_not_matter(dev130, fixed, data):
    x0, r = dev130
    tail = lv.rw_sample(x0[64:], 13, M.STEP, seed=SEED, data=data, first_chain=64, return_noise=True)
    for name in ('samples', 'log_p', 'accepted', 'n_failed', 'z', 'log_u'):
        np.testing.assert_array_equal(getattr(tail, name), getattr(r, name)[64:], err_msg=name)
    split = lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, steps_per_launch=5, return_noise=True)
    for name in ('samples', 'log_p', 'accepted', 'n_failed', 'z', 'log_u'):
        np.testing.assert_array_equal(getattr(split, name), getattr(r, name), err_msg=name)
    fx0, fz, flu = M.fixed_input()
    _same(lv.rw_sample(fx0, 41, M.STEP, noise=(fz, flu), data=data, steps_per_launch=5), fixed)
    # without return_noise the kernel that records nothing draws the same noise
    _same(lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data), r)


def test_out_of_range_proposals_are_rejected_without_integrating(data):
    x0 = np.log(lv.THETA)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((1, 10, 4))
    log_u = np.log(rng.random((1, 10)))
    ref = lv.rw_sample(x0, 11, M.STEP, noise=(z, log_u), data=data)
    # two extra steps whose proposals land at log theta = +800 (exp: inf) and -800 (exp: 0); their log_u = -inf
    # would accept any proposal that had a density
    bad_hi = np.array([(800.0 - x0[0]) / M.STEP, 0.0, 0.0, 0.0])
    bad_lo = np.array([0.0, 0.0, (-800.0 - x0[2]) / M.STEP, 0.0])
    z2 = np.insert(z, [3, 6], [bad_hi, bad_lo], axis=1)
    log_u2 = np.insert(log_u, [3, 6], -np.inf, axis=1)
    got = lv.rw_sample(x0, 13, M.STEP, noise=(z2, log_u2), data=data)
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
        lv.rw_sample(np.array([800.0, 0.0, 0.0, 0.0]), 3, seed=1, data=data)
    with pytest.raises(ValueError, match='starting point'):          # the integration runs out of steps
        lv.rw_sample(np.log(lv.THETA), 3, seed=1, data=data, max_steps=3)
    one = lv.rw_sample(np.log(lv.THETA), 1, seed=1, data=data, return_noise=True)
    assert one.samples.shape == (1, 1, 4) and one.log_p.shape == (1, 1) and one.z.shape == (1, 0, 4)
    assert one.accepted.tolist() == [0] and one.n_failed.tolist() == [0]


def test_device_out_returns_tensors(dev130, data):
    x0, r = dev130
    d = lv.rw_sample(x0, 13, M.STEP, seed=SEED, data=data, device_out=True)
    assert d.samples.is_cuda and d.log_p.is_cuda and d.accepted.dtype == torch.int64
    np.testing.assert_array_equal(d.samples.cpu().numpy(), r.samples)
    np.testing.assert_array_equal(d.accepted.cpu().numpy(), r.accepted)


def test_noise_moments(data):
    """4096 chains, 3 rows: mean and variance of z and the mean of u = exp(log_u) within 5 standard errors
    (the host restatement is within 1 for this seed: tests/test_lv_mcmc_cpu.py)."""
    r = lv.rw_sample(np.tile(np.log(lv.THETA), (4096, 1)), 3, M.STEP, seed=MOMENT_SEED, data=data, return_noise=True)
    z, u = r.z, np.exp(r.log_u)
    n = z.size
    assert z.shape == (4096, 2, 4)
    assert abs(z.mean()) < 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert abs(u.mean() - 0.5) < 5.0 * np.sqrt(1.0 / 12.0 / u.size)
    assert np.all((u >= 0) & (u < 1))
    assert r.n_failed.sum() == 0


def test_failed_proposals_are_those_log_target_density_fails(data):
    """The sampler rejects a proposal for a failed integration exactly where log_target_density reports a
    non-zero status (both run csrc/lv_rk45.hpp).  log_u = -inf accepts every proposal that has a density, so
    a repeated row marks a failure; 25 of the 80 proposals need more than max_steps steps
    (tests/test_lv_mcmc_cpu.py holds that from scipy alone)."""
    import warnings
    x0, z, log_u = M.failing_input()
    max_steps = 23 + M.FAIL_K                          # 23: the start row's accepted steps
    r = lv.rw_sample(x0, 21, M.FAIL_STEP, noise=(z, log_u), data=data, max_steps=max_steps)
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
