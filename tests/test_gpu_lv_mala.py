"""MALA sampler on the GPU (csrc/lv_mcmc.hip: lv_mala_wave_kernel, lotka_volterra.mala_sample) against the host
restatement of tests/mala_ref.py (scipy) and against itself.

The device chain is compared with the host ONE STEP AT A TIME: every device row is evaluated on the host (log_p
and grad within RTOL, the tolerance tests/test_gpu_lv.py holds the LV gradient and density to against scipy),
and every step is replayed on the host from the device's previous row, its grad and the step's noise; the
replayed decision must be the device's wherever its margin exceeds 1e-7, and no step of the fixed input may
have a smaller one (tests/test_lv_mala_cpu.py holds 1e-6 on the host chain).  Proposals are checked bit for bit
from the returned arrays, and a chain is bit-identical to itself under every launch geometry.

Recorded on MI355X: fixed input log_p within 5.0e-14 and grad within 1.5e-11 of the host evaluation, smallest
replayed margin 7.9e-5, accepted 8, 5, 4, 4, 8 of 40; t_n = 1 and 2: log_p within 1.3e-16, grad within 4.4e-16; the
failing input fails 6, 9, 14 and 18 of its chains' 20 proposals (22 .. 67 accepted RK45 steps against max_steps 33)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import mala_ref as R  # noqa: E402

RTOL = 1e-8          # tests/test_gpu_lv.py: the project's LV tolerance against scipy
SEED = 20261020
T_NS = [1, 2, 63, 65, 130]
NAMES = ('samples', 'log_p', 'grad', 'accepted', 'n_failed')
EPS4 = np.array([0.003, 0.002, 0.003, 0.004])


@pytest.fixture(scope='module')
def data():
    return lv.reference_data()


def _cut(data, n):
    return lv.LvData(t=data.t[:n], y=data.y[:n], cov=data.cov, t_span=data.t_span, u_init=data.u_init)


def _starts(n):
    rng = np.random.default_rng(42)
    return np.log(lv.THETA) + 0.02 * rng.normal(size=(n, 4))


def _same(a, b, names=NAMES, rows=slice(None)):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name)[rows], err_msg=name)


def _grad_err(got, want):
    return np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)


def _clip(v, c):
    return np.minimum(np.maximum(v, -c), c)


def _proposals(run, eps, cap, z):
    """(samples[t-1] + clip(h * grad[t-1])) + eps * z[t], in NumPy from the returned arrays."""
    eps, h, w, c = R.constants(eps, cap)
    return (run.samples[:, :-1] + _clip(h * run.grad[:, :-1], c)) + eps * z, np.abs(h * run.grad[:, :-1]) > c


@pytest.fixture(scope='module')
def host_eval(data):
    """mala_ref.evaluate on the full data, once per distinct point."""
    return functools.lru_cache(maxsize=None)(lambda key: R.evaluate(np.frombuffer(key), data))


@pytest.fixture(scope='module')
def fixed(data):
    x0, z, log_u = R.fixed_input()
    return lv.mala_sample(x0, R.FIXED_ROWS, R.FIXED_EPS, noise=(z, log_u), drift_cap=R.FIXED_CAP, data=data)


def test_fixed_input_rows_match_the_host_evaluation(fixed, host_eval):
    lp_err, g_err = 0.0, 0.0
    for c in range(R.FIXED_CHAINS):
        for t in range(R.FIXED_ROWS):
            lp, g, _ = host_eval(fixed.samples[c, t].tobytes())
            lp_err = max(lp_err, abs(fixed.log_p[c, t] - lp) / abs(lp))
            g_err = max(g_err, float(_grad_err(fixed.grad[c, t], g)))
    print('max rel err: log_p', lp_err, 'grad', g_err)
    assert lp_err < RTOL and g_err < RTOL, (lp_err, g_err)
    assert fixed.n_failed.tolist() == [0] * R.FIXED_CHAINS
    assert fixed.z is None and fixed.log_u is None


def test_fixed_input_decisions_replay_on_the_host(fixed, host_eval):
    x0, z, log_u = R.fixed_input()
    eps, h, w, c = R.constants(R.FIXED_EPS, R.FIXED_CAP)
    np.testing.assert_array_equal(fixed.samples[:, 0], x0)
    margins = np.empty((R.FIXED_CHAINS, R.FIXED_ROWS - 1))
    moved = np.any(fixed.samples[:, 1:] != fixed.samples[:, :-1], axis=2)
    for ch in range(R.FIXED_CHAINS):
        for k in range(R.FIXED_ROWS - 1):
            x, g = fixed.samples[ch, k], fixed.grad[ch, k]
            lp = host_eval(x.tobytes())[0]
            d = R.drift(g, h, c)
            p = (x + d) + eps * z[ch, k]
            lp_new, g_new, _ = host_eval(p.tobytes())
            ok, margins[ch, k] = R.decide(x, lp, d, p, lp_new, g_new, log_u[ch, k], h, w, c)
            if margins[ch, k] > 1e-7:
                assert ok == moved[ch, k], (ch, k, margins[ch, k])
                if ok:
                    np.testing.assert_array_equal(fixed.samples[ch, k + 1], p)
    print('accepted', fixed.accepted.tolist(), 'smallest replayed margin', margins.min())
    assert margins.min() > 1e-7, margins.min()              # no step is left out
    np.testing.assert_array_equal(fixed.accepted, moved.sum(axis=1))
    # with margins this far above the values' error the device takes the host chain's decisions
    np.testing.assert_array_equal(fixed.accepted, R.fixed_reference()['accepted'])


@pytest.mark.parametrize('cap', [0.5, np.inf])
def test_proposal_arithmetic_is_numpys_bit_for_bit(data, cap):
    """A vector step size.  cap = 0.5 from the fixed input's starts with device noise: some drift components are
    clipped and some are not.  cap = inf from starts within 0.001 of log(THETA) at half the step with supplied
    noise: from the fixed input's starts an uncapped drift of ~0.15 overshoots the posterior (width ~0.005) and
    every proposal is rejected; this input was chosen on the host, where the restated chains accept 6, 6, 2, 1
    and 0 of their 12 proposals with margins above 1e-4."""
    if np.isfinite(cap):
        eps4 = EPS4
        run = lv.mala_sample(R.fixed_input()[0], 13, eps4, seed=SEED, drift_cap=cap, data=data, return_noise=True)
        z = run.z
    else:
        eps4 = 0.5 * EPS4
        x0 = np.log(R.THETA) + 0.001 * np.random.default_rng(7).standard_normal((5, 4))
        z, log_u = np.empty((5, 12, 4)), np.empty((5, 12))
        for c in range(5):
            rng = np.random.default_rng(300 + c)
            z[c] = rng.standard_normal((12, 4))
            log_u[c] = np.log(rng.random(12))
        run = lv.mala_sample(x0, 13, eps4, noise=(z, log_u), drift_cap=cap, data=data)
        assert run.accepted.tolist() == [6, 6, 2, 1, 0]
    prop, clipped = _proposals(run, eps4, cap, z)
    moved = np.any(run.samples[:, 1:] != run.samples[:, :-1], axis=2)
    print('cap', cap, 'accepted', run.accepted.tolist(), 'clipped', int(clipped.sum()), 'of', clipped.size)
    if np.isfinite(cap):
        assert clipped.any() and not clipped.all()
    else:
        assert not clipped.any()
    assert moved.any()
    np.testing.assert_array_equal(run.accepted, moved.sum(axis=1))
    np.testing.assert_array_equal(run.samples[:, 1:][moved], prop[moved])
    for name in ('samples', 'log_p', 'grad'):                 # a rejected step repeats the row
        a = getattr(run, name)
        np.testing.assert_array_equal(a[:, 1:][~moved], a[:, :-1][~moved], err_msg=name)


@pytest.mark.parametrize('t_n', T_NS)
def test_launch_geometry_does_not_matter(data, t_n):
    sub = _cut(data, t_n)
    x0 = _starts(9)                                  # 9 chains: two full blocks of 4 waves and one wave
    names = NAMES + ('z', 'log_u')
    kw = dict(seed=SEED, drift_cap=2.0, data=sub)
    r = lv.mala_sample(x0, 13, EPS4, return_noise=True, **kw)
    assert np.all(np.isfinite(r.log_p)) and np.all(np.isfinite(r.grad)) and r.n_failed.sum() == 0
    assert r.accepted.sum() > 0
    for spl in (1, 5):                               # 12 steps: 12 launches; 5 + 5 + 2
        _same(lv.mala_sample(x0, 13, EPS4, return_noise=True, steps_per_launch=spl, **kw), r, names)
    _same(lv.mala_sample(x0[4:], 13, EPS4, return_noise=True, first_chain=4, **kw), r, names, slice(4, None))
    _same(lv.mala_sample(x0, 13, EPS4, **kw), r)                        # the kernel that records nothing
    _same(lv.mala_sample(x0, 13, EPS4, noise=(r.z, r.log_u), drift_cap=2.0, data=sub), r)
    for n in (1, 4, 5):                              # one wave of four, a full block, a full block and one wave
        _same(lv.mala_sample(x0[:n], 13, EPS4, return_noise=True, **kw), r, names, slice(0, n))


def test_device_noise_equals_rw_samples(data):
    sub = _cut(data, 65)
    x0 = _starts(9)
    m = lv.mala_sample(x0[2:], 13, 0.003, seed=SEED, data=sub, first_chain=2, return_noise=True)
    for layout in ('wave', 'thread'):
        rw = lv.rw_sample(x0[2:], 13, seed=SEED, data=sub, first_chain=2, return_noise=True, layout=layout)
        np.testing.assert_array_equal(m.z, rw.z)
        np.testing.assert_array_equal(m.log_u, rw.log_u)


@pytest.mark.parametrize('t_n', [1, 2])
def test_one_and_two_observations(data, t_n):
    """With at most two observation times only lanes 0 and 1 hold a term: log_p and grad must not depend on the
    split.  Against the restated density and against grad_log_posterior (the thread-per-point kernels) at the
    device rows."""
    sub = _cut(data, t_n)
    x0 = _starts(5)
    r = lv.mala_sample(x0, 9, 0.05, seed=SEED, drift_cap=1.0, data=sub)
    assert r.accepted.sum() > 0 and r.n_failed.sum() == 0
    rows = r.samples.reshape(-1, 4)
    theta = np.exp(rows)
    want_g = theta * lv.grad_log_posterior(theta, sub)
    want_lp = np.array([R.evaluate(x, sub)[0] for x in rows])
    host_g = np.array([R.evaluate(x, sub)[1] for x in rows])
    lp_err = np.abs(r.log_p.reshape(-1) - want_lp) / np.abs(want_lp)
    got_g = r.grad.reshape(-1, 4)
    print('max rel err: log_p', lp_err.max(), 'grad vs grad_log_posterior', _grad_err(got_g, want_g).max(),
          'grad vs host', _grad_err(got_g, host_g).max())
    assert lp_err.max() < RTOL
    assert _grad_err(got_g, want_g).max() < RTOL
    assert _grad_err(got_g, host_g).max() < RTOL


def test_failed_proposals_are_those_that_need_more_steps(data):
    """tests/mcmc_ref.failing_input()'s scheme: log_u = -inf accepts every proposal that has a density, max_steps is
    one more than the start row's accepted-step count for the 10-state system; the steps of every proposal are
    recounted on the host (tests/test_lv_mala_cpu.py holds that some, and not all, need more)."""
    from oracle import lv_numpy as ol
    x0, z, log_u = R.failing_input()
    max_steps = R.failing_max_steps()
    r = lv.mala_sample(x0, 21, R.FAIL_EPS, noise=(z, log_u), drift_cap=R.FAIL_CAP, data=data, max_steps=max_steps)
    prop, _ = _proposals(r, R.FAIL_EPS, R.FAIL_CAP, z)
    counts = np.array([ol.n_steps(np.exp(p), sensitivity=True) for p in prop.reshape(-1, 4)]).reshape(4, 20)
    bad = counts > max_steps
    print('failed proposals', bad.sum(axis=1).tolist(), 'accepted steps', counts.min(), '..', counts.max())
    assert 0 < bad.sum() < bad.size
    repeats = np.all(r.samples[:, 1:] == r.samples[:, :-1], axis=2)
    np.testing.assert_array_equal(repeats, bad)
    np.testing.assert_array_equal(r.n_failed, bad.sum(axis=1))
    np.testing.assert_array_equal(r.accepted, (~bad).sum(axis=1))
    np.testing.assert_array_equal(r.samples[:, 1:][~bad], prop[~bad])
    np.testing.assert_array_equal(r.log_p[:, 1:][bad], r.log_p[:, :-1][bad])
    np.testing.assert_array_equal(r.grad[:, 1:][bad], r.grad[:, :-1][bad])
    assert np.all(np.isfinite(r.log_p)) and np.all(np.isfinite(r.grad))


def test_out_of_range_proposals_are_rejected_without_integrating(data):
    sub = _cut(data, 130)
    x0 = np.log(lv.THETA)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((1, 10, 4))
    log_u = np.log(rng.random((1, 10)))
    eps = 0.003
    ref = lv.mala_sample(x0, 11, eps, noise=(z, log_u), drift_cap=1.0, data=sub)
    # two extra steps whose proposals land near log theta = +800 (exp: inf) and -800 (exp: 0); log_u = -inf would
    # accept any proposal that had a density
    z2 = np.insert(z, [3, 6], [[800.0 / eps, 0, 0, 0], [0, 0, -800.0 / eps, 0]], axis=1)
    log_u2 = np.insert(log_u, [3, 6], -np.inf, axis=1)
    got = lv.mala_sample(x0, 13, eps, noise=(z2, log_u2), drift_cap=1.0, data=sub)
    assert got.n_failed.tolist() == [2] and ref.n_failed.tolist() == [0]
    np.testing.assert_array_equal(got.accepted, ref.accepted)
    for name in ('samples', 'log_p', 'grad'):       # rows 4 and 8 repeat; the chain goes on as without them
        np.testing.assert_array_equal(np.delete(getattr(got, name), [4, 8], axis=1), getattr(ref, name), err_msg=name)
        np.testing.assert_array_equal(getattr(got, name)[0, [4, 8]], getattr(got, name)[0, [3, 7]], err_msg=name)


def test_a_start_that_cannot_be_evaluated_raises(data):
    sub = _cut(data, 63)
    with pytest.raises(ValueError, match='starting point'):
        lv.mala_sample(np.array([800.0, 0.0, 0.0, 0.0]), 3, 0.003, seed=1, data=sub)       # theta overflows
    with pytest.raises(ValueError, match='starting point'):                                # out of RK45 steps
        lv.mala_sample(np.log(lv.THETA), 3, 0.003, seed=1, data=sub, max_steps=3)
    one = lv.mala_sample(np.log(lv.THETA), 1, 0.003, seed=1, data=sub, return_noise=True)
    assert one.samples.shape == (1, 1, 4) and one.grad.shape == (1, 1, 4) and one.log_p.shape == (1, 1)
    assert one.z.shape == (1, 0, 4) and one.accepted.tolist() == [0] and one.n_failed.tolist() == [0]


def test_device_tensors_feed_thin_chains(data):
    from stein_thinning.thinning import thin_chains
    x0 = _starts(3)
    kw = dict(seed=SEED, drift_cap=1.0, data=_cut(data, 130))
    run = lv.mala_sample(x0, 60, 0.001, device_out=True, **kw)
    assert run.samples.is_cuda and run.grad.is_cuda and run.log_p.is_cuda and run.accepted.dtype == torch.int64
    host = lv.mala_sample(x0, 60, 0.001, **kw)
    for name in NAMES:
        np.testing.assert_array_equal(getattr(run, name).cpu().numpy(), getattr(host, name), err_msg=name)
    got = thin_chains(list(run.samples), list(run.grad), 10)
    want = thin_chains(list(host.samples), list(host.grad), 10)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a.cpu() if hasattr(a, 'cpu') else a), b)
