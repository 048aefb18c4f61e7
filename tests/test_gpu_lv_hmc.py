"""HMC sampler on the GPU (csrc/lv_mcmc.hip: lv_hmc_wave_kernel, lotka_volterra.hmc_sample) against the host
restatement of tests/hmc_ref.py (scipy) and against itself.

Values: every device row is evaluated on the host (log_p and grad within RTOL, the tolerance tests/test_gpu_lv.py
holds the LV gradient and density to against scipy).  Arithmetic: a one-stage step is NumPy's bit for bit from the
returned arrays, and a trajectory of L stages is bit for bit L one-stage device calls chained through (q, r) --
so the accept decision of EVERY step is recomputed in NumPy from device values alone, with nothing re-evaluated on
another machine and no step left out.  A chain is bit-identical to itself under every launch geometry.

Recorded on MI355X: fixed input log_p within 5.5e-14 and grad within 1.3e-11 of the host evaluation, accepted 7, 6, 2,
8, 8 of 12; chained one-stage calls: smallest |a - log_u| 1.2e-2, 8.7e-3, 8.0e-4 for L = 2, 3, 5; one-stage HMC against
MALA: rows within 8.2e-16, log_p within 8.6e-12; t_n = 1 and 2: log_p equal, grad within 3.8e-16; the failing input
fails 4, 7, 3 and 6 of its chains' 12 trajectories, 10 of them at stage 1 (21 .. 44 accepted RK45 steps against
max_steps 33)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import hmc_ref as R  # noqa: E402

RTOL = 1e-8          # tests/test_gpu_lv.py: the project's LV tolerance against scipy
SEED = 20261021
T_NS = [1, 2, 63, 65, 130]
NAMES = ('samples', 'log_p', 'grad', 'accepted', 'n_failed')
# with the first 130 observations the posterior is ~0.02 wide: on the host these steps and this cap give mixed
# decisions (4 .. 11 of 12 accepted for L = 1 .. 5) and both clipped and unclipped kick components
EPS4 = np.array([0.02, 0.015, 0.02, 0.025])
CAP = 0.2


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


def _hk(g, eps, cap):
    return 0.5 * R.clip(eps * g, np.full(4, cap))


def _kinetic(r):
    s = np.zeros(r.shape[:-1])
    for j in range(4):
        s = s + r[..., j] * r[..., j]
    return 0.5 * s


def _one_stage(q, r, eps, cap, data, **kw):
    """One-stage device trajectories from the points q (n, 4) with momenta r (n, 4), each its own chain, accepted
    whenever they have a density (log_u = -inf): row 0 is q with g(q), row 1 the end point with its log_p and grad."""
    n = q.shape[0]
    return lv.hmc_sample(q, 2, eps, 1, noise=(r[:, None, :], np.full((n, 1), -np.inf)), kick_cap=cap, data=data, **kw)


@pytest.fixture(scope='module')
def fixed(data):
    x0, z, log_u = R.fixed_input()
    return lv.hmc_sample(x0, R.FIXED_ROWS, R.FIXED_EPS, R.FIXED_L, noise=(z, log_u), kick_cap=R.FIXED_CAP, data=data)


def test_fixed_input_rows_match_the_host_evaluation(fixed, data):
    """Every row of the fixed-input run (L = 3, cap 0.5, full data) against scipy at the device row."""
    ev = functools.lru_cache(maxsize=None)(lambda key: R.evaluate(np.frombuffer(key), data))
    lp_err, g_err = 0.0, 0.0
    for c in range(R.FIXED_CHAINS):
        for t in range(R.FIXED_ROWS):
            lp, g, _ = ev(fixed.samples[c, t].tobytes())
            lp_err = max(lp_err, abs(fixed.log_p[c, t] - lp) / abs(lp))
            g_err = max(g_err, float(_grad_err(fixed.grad[c, t], g)))
    print('max rel err: log_p', lp_err, 'grad', g_err, 'accepted', fixed.accepted.tolist())
    assert lp_err < RTOL and g_err < RTOL, (lp_err, g_err)
    np.testing.assert_array_equal(fixed.samples[:, 0], R.fixed_input()[0])
    assert fixed.n_failed.tolist() == [0] * R.FIXED_CHAINS
    assert fixed.z is None and fixed.log_u is None
    moved = np.any(fixed.samples[:, 1:] != fixed.samples[:, :-1], axis=2)
    np.testing.assert_array_equal(fixed.accepted, moved.sum(axis=1))
    # the host chain's smallest margin (1.0e-4, tests/test_lv_hmc_cpu.py holds 1e-6) is far above the values' error
    np.testing.assert_array_equal(fixed.accepted, R.fixed_reference()['accepted'])


@pytest.mark.parametrize('cap', [CAP, np.inf])
def test_one_stage_is_numpys_bit_for_bit(data, cap):
    """L = 1 with a vector step size: every moved row is x + eps * (z + 0.5 * clip(eps * grad_prev, c)) in NumPy from
    the returned arrays; a rejected step repeats row, log_p and grad.  With the cap some kick components are clipped
    and some are not."""
    sub = _cut(data, 130)
    run = lv.hmc_sample(R.fixed_input()[0], 13, EPS4, 1, seed=SEED, kick_cap=cap, data=sub, return_noise=True)
    kick = EPS4 * run.grad[:, :-1]
    clipped = np.abs(kick) > cap
    prop = run.samples[:, :-1] + EPS4 * (run.z + 0.5 * R.clip(kick, np.full(4, cap)))
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


@pytest.mark.parametrize('n_leapfrog', [2, 3, 5])
def test_l_stages_are_l_chained_one_stage_steps_bit_for_bit(data, n_leapfrog):
    """Every step of a 5-chain, 13-row run is rebuilt from one-stage device calls (all 60 steps of a stage as
    separate chains of one call): stage l + 1 starts at the returned q^l with the momentum (r' + hk(q^l)) formed in
    NumPy from the returned grad.  End point, log_p and grad are the device trajectory's bits, and the decision
    recomputed in NumPy from those values is the device's for every step."""
    sub = _cut(data, 130)
    run = lv.hmc_sample(R.fixed_input()[0], 13, EPS4, n_leapfrog, seed=SEED, kick_cap=CAP, data=sub, return_noise=True)
    assert run.n_failed.sum() == 0
    x, g, lp = (getattr(run, name)[:, :-1].reshape(60, -1) for name in ('samples', 'grad', 'log_p'))
    z, log_u = run.z.reshape(60, 4), run.log_u.reshape(60)
    q, r = x, z
    for stage in range(n_leapfrog):
        one = _one_stage(q, r, EPS4, CAP, sub)
        assert one.accepted.tolist() == [1] * 60 and one.n_failed.sum() == 0
        np.testing.assert_array_equal(one.samples[:, 0], q)
        if stage == 0:
            np.testing.assert_array_equal(one.grad[:, 0], g)
            np.testing.assert_array_equal(one.log_p[:, 0], lp[:, 0])
        r = (r + _hk(one.grad[:, 0], EPS4, CAP)) + _hk(one.grad[:, 1], EPS4, CAP)
        q = one.samples[:, 1]
    a = (one.log_p[:, 1] - lp[:, 0]) + (_kinetic(z) - _kinetic(r))
    accept = log_u < a
    moved = np.any(run.samples[:, 1:] != run.samples[:, :-1], axis=2).reshape(60)
    print('L', n_leapfrog, 'accepted', run.accepted.tolist(), 'smallest |a - log_u|', np.abs(a - log_u).min())
    np.testing.assert_array_equal(moved, accept)             # EVERY step
    np.testing.assert_array_equal(run.accepted, moved.reshape(5, 12).sum(axis=1))
    assert moved.any()
    for name, end in (('samples', q), ('log_p', one.log_p[:, 1:2]), ('grad', one.grad[:, 1])):
        nxt = getattr(run, name)[:, 1:].reshape(60, -1)
        prev = getattr(run, name)[:, :-1].reshape(60, -1)
        np.testing.assert_array_equal(nxt[moved], end[moved], err_msg=name)
        np.testing.assert_array_equal(nxt[~moved], prev[~moved], err_msg=name)


def test_one_stage_takes_mala_samples_decisions(data):
    """The cap = inf input of test_gpu_lv_mala.py::test_proposal_arithmetic_is_numpys_bit_for_bit (starts within
    0.001 of log(THETA), half its step, margins above 1e-4 on the host): MALA is one-stage HMC up to rounding, so
    the same noise gives the same decisions."""
    eps4 = 0.5 * np.array([0.003, 0.002, 0.003, 0.004])
    x0 = np.log(R.THETA) + 0.001 * np.random.default_rng(7).standard_normal((5, 4))
    z, log_u = np.empty((5, 12, 4)), np.empty((5, 12))
    for c in range(5):
        rng = np.random.default_rng(300 + c)
        z[c] = rng.standard_normal((12, 4))
        log_u[c] = np.log(rng.random(12))
    mala = lv.mala_sample(x0, 13, eps4, noise=(z, log_u), drift_cap=np.inf, data=data)
    hmc = lv.hmc_sample(x0, 13, eps4, 1, noise=(z, log_u), kick_cap=np.inf, data=data)
    print('largest row difference', np.abs(hmc.samples - mala.samples).max(), 'log_p',
          np.abs(hmc.log_p - mala.log_p).max())
    assert mala.accepted.tolist() == [6, 6, 2, 1, 0]
    assert hmc.accepted.tolist() == [6, 6, 2, 1, 0]
    np.testing.assert_array_equal(hmc.samples[:, 0], mala.samples[:, 0])
    np.testing.assert_array_equal(hmc.log_p[:, 0], mala.log_p[:, 0])         # the same evaluation of the same start
    np.testing.assert_array_equal(hmc.grad[:, 0], mala.grad[:, 0])


@pytest.mark.parametrize('t_n', T_NS)
def test_launch_geometry_does_not_matter(data, t_n):
    sub = _cut(data, t_n)
    x0 = _starts(9)                                  # 9 chains: two full blocks of 4 waves and one wave
    names = NAMES + ('z', 'log_u')
    kw = dict(seed=SEED, kick_cap=CAP, data=sub)
    r = lv.hmc_sample(x0, 13, EPS4, 3, return_noise=True, **kw)
    assert np.all(np.isfinite(r.log_p)) and np.all(np.isfinite(r.grad)) and r.n_failed.sum() == 0
    assert r.accepted.sum() > 0
    for spl in (1, 5):                               # 12 steps: 12 launches; 5 + 5 + 2
        _same(lv.hmc_sample(x0, 13, EPS4, 3, return_noise=True, steps_per_launch=spl, **kw), r, names)
    _same(lv.hmc_sample(x0[4:], 13, EPS4, 3, return_noise=True, first_chain=4, **kw), r, names, slice(4, None))
    _same(lv.hmc_sample(x0, 13, EPS4, 3, **kw), r)                      # the kernel that records nothing
    _same(lv.hmc_sample(x0, 13, EPS4, 3, noise=(r.z, r.log_u), kick_cap=CAP, data=sub), r)
    for n in (1, 4, 5):                              # one wave of four, a full block, a full block and one wave
        _same(lv.hmc_sample(x0[:n], 13, EPS4, 3, return_noise=True, **kw), r, names, slice(0, n))


def test_device_noise_equals_rw_samples(data):
    sub = _cut(data, 65)
    x0 = _starts(9)
    m = lv.hmc_sample(x0[2:], 13, 0.003, 3, seed=SEED, data=sub, first_chain=2, return_noise=True)
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
    r = lv.hmc_sample(x0, 9, 0.05, 2, seed=SEED, kick_cap=1.0, data=sub)
    assert r.accepted.sum() > 0 and r.n_failed.sum() == 0
    rows = r.samples.reshape(-1, 4)
    theta = np.exp(rows)
    want_g = theta * lv.grad_log_posterior(theta, sub)
    host = [R.evaluate(x, sub) for x in rows]
    want_lp = np.array([h[0] for h in host])
    host_g = np.array([h[1] for h in host])
    lp_err = np.abs(r.log_p.reshape(-1) - want_lp) / np.abs(want_lp)
    got_g = r.grad.reshape(-1, 4)
    print('max rel err: log_p', lp_err.max(), 'grad vs grad_log_posterior', _grad_err(got_g, want_g).max(),
          'grad vs host', _grad_err(got_g, host_g).max())
    assert lp_err.max() < RTOL
    assert _grad_err(got_g, want_g).max() < RTOL
    assert _grad_err(got_g, host_g).max() < RTOL


def test_failed_trajectories_are_those_with_a_stage_that_needs_more_steps(data):
    """tests/mala_ref.failing_input()'s scheme with L = 2: log_u = -inf accepts every trajectory that has a density,
    max_steps is one more than the start row's accepted-step count.  The intermediate point of every step comes
    from a one-stage device call with the default max_steps (bit for bit the trajectory's, see above), the end point
    from a second one; their RK45 steps are recounted on the host (tests/test_lv_hmc_cpu.py holds that some
    trajectories and not all need more, at either stage)."""
    from oracle import lv_numpy as ol
    x0, z, log_u = R.failing_input()
    max_steps = R.failing_max_steps()
    C, S = R.FAIL_CHAINS, R.FAIL_ROWS - 1
    r = lv.hmc_sample(x0, R.FAIL_ROWS, R.FAIL_EPS, R.FAIL_L, noise=(z, log_u), kick_cap=R.FAIL_CAP, data=data,
                      max_steps=max_steps)
    assert R.FAIL_L == 2
    x = r.samples[:, :-1].reshape(C * S, 4)
    one = _one_stage(x, z.reshape(C * S, 4), R.FAIL_EPS, R.FAIL_CAP, data)
    assert one.accepted.tolist() == [1] * (C * S)
    np.testing.assert_array_equal(one.grad[:, 0], r.grad[:, :-1].reshape(C * S, 4))
    q1 = one.samples[:, 1]
    r1 = (z.reshape(C * S, 4) + _hk(one.grad[:, 0], R.FAIL_EPS, R.FAIL_CAP)) + _hk(one.grad[:, 1], R.FAIL_EPS, R.FAIL_CAP)
    two = _one_stage(q1, r1, R.FAIL_EPS, R.FAIL_CAP, data)
    assert two.accepted.tolist() == [1] * (C * S)
    q2 = two.samples[:, 1]
    n1 = np.array([ol.n_steps(np.exp(p), sensitivity=True) for p in q1])
    n2 = np.array([ol.n_steps(np.exp(p), sensitivity=True) for p in q2])
    bad = ((n1 > max_steps) | (n2 > max_steps)).reshape(C, S)
    print('failed trajectories', bad.sum(axis=1).tolist(), 'at stage 1', int((n1 > max_steps).sum()), 'accepted steps',
          min(n1.min(), n2.min()), '..', max(n1.max(), n2.max()), 'max_steps', max_steps)
    assert 0 < bad.sum() < bad.size
    repeats = np.all(r.samples[:, 1:] == r.samples[:, :-1], axis=2)
    np.testing.assert_array_equal(repeats, bad)
    np.testing.assert_array_equal(r.n_failed, bad.sum(axis=1))                # once per trajectory
    np.testing.assert_array_equal(r.accepted, (~bad).sum(axis=1))
    np.testing.assert_array_equal(r.samples[:, 1:][~bad], q2.reshape(C, S, 4)[~bad])
    np.testing.assert_array_equal(r.log_p[:, 1:][~bad], two.log_p[:, 1].reshape(C, S)[~bad])
    np.testing.assert_array_equal(r.grad[:, 1:][~bad], two.grad[:, 1].reshape(C, S, 4)[~bad])
    np.testing.assert_array_equal(r.log_p[:, 1:][bad], r.log_p[:, :-1][bad])
    np.testing.assert_array_equal(r.grad[:, 1:][bad], r.grad[:, :-1][bad])
    assert np.all(np.isfinite(r.samples)) and np.all(np.isfinite(r.log_p)) and np.all(np.isfinite(r.grad))


def test_out_of_range_trajectories_are_rejected_without_integrating(data):
    sub = _cut(data, 130)
    x0 = np.log(lv.THETA)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((1, 10, 4))
    log_u = np.log(rng.random((1, 10)))
    eps = 0.02
    ref = lv.hmc_sample(x0, 11, eps, 2, noise=(z, log_u), kick_cap=CAP, data=sub)
    # two extra steps whose first stage lands near log theta = +800 (exp: inf) and -800 (exp: 0); log_u = -inf would
    # accept any trajectory that had a density
    z2 = np.insert(z, [3, 6], [[800.0 / eps, 0, 0, 0], [0, 0, -800.0 / eps, 0]], axis=1)
    log_u2 = np.insert(log_u, [3, 6], -np.inf, axis=1)
    got = lv.hmc_sample(x0, 13, eps, 2, noise=(z2, log_u2), kick_cap=CAP, data=sub)
    assert got.n_failed.tolist() == [2] and ref.n_failed.tolist() == [0]
    np.testing.assert_array_equal(got.accepted, ref.accepted)
    for name in ('samples', 'log_p', 'grad'):       # rows 4 and 8 repeat; the chain goes on as without them
        np.testing.assert_array_equal(np.delete(getattr(got, name), [4, 8], axis=1), getattr(ref, name), err_msg=name)
        np.testing.assert_array_equal(getattr(got, name)[0, [4, 8]], getattr(got, name)[0, [3, 7]], err_msg=name)


def test_a_start_that_cannot_be_evaluated_raises(data):
    sub = _cut(data, 63)
    with pytest.raises(ValueError, match='starting point'):
        lv.hmc_sample(np.array([800.0, 0.0, 0.0, 0.0]), 3, 0.003, 2, seed=1, data=sub)     # theta overflows
    with pytest.raises(ValueError, match='starting point'):                                # out of RK45 steps
        lv.hmc_sample(np.log(lv.THETA), 3, 0.003, 2, seed=1, data=sub, max_steps=3)
    one = lv.hmc_sample(np.log(lv.THETA), 1, 0.003, 2, seed=1, data=sub, return_noise=True)
    assert one.samples.shape == (1, 1, 4) and one.grad.shape == (1, 1, 4) and one.log_p.shape == (1, 1)
    assert one.z.shape == (1, 0, 4) and one.accepted.tolist() == [0] and one.n_failed.tolist() == [0]


def test_device_tensors_feed_thin_chains(data):
    from stein_thinning.thinning import thin_chains
    x0 = _starts(3)
    kw = dict(seed=SEED, kick_cap=CAP, data=_cut(data, 130))
    run = lv.hmc_sample(x0, 60, 0.01, 2, device_out=True, **kw)
    assert run.samples.is_cuda and run.grad.is_cuda and run.log_p.is_cuda and run.accepted.dtype == torch.int64
    host = lv.hmc_sample(x0, 60, 0.01, 2, **kw)
    for name in NAMES:
        np.testing.assert_array_equal(getattr(run, name).cpu().numpy(), getattr(host, name), err_msg=name)
    got = thin_chains(list(run.samples), list(run.grad), 10)
    want = thin_chains(list(host.samples), list(host.grad), 10)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a.cpu() if hasattr(a, 'cpu') else a), b)
