"""The Lotka-Volterra kernels (csrc/lv.hip) on every input tests/test_gpu_lv.py holds fixed: dense
covariances, theta wide enough to mix points on both sides of the 64-step table, other tolerances, span and
initial state, short / repeated / out-of-span observation grids, the recorded step table against scipy's
``sol.t``, the failure statuses (max_steps, non-finite theta), batch shapes and chunks.

Reference: scipy through oracle/lv_numpy.py, on the input sets of tests/lv_ref.py.  Tolerance: RTOL = 1e-8 of
tests/test_gpu_lv.py (gradient: max|got - want| / max|want| per row; log density: relative).
tests/test_lv_ref_cpu.py shows on the same sets that scipy's own reordering noise stays under 1e-9 and that
no point is nearer than 1e-5 to a flipped step decision, so the bound keeps a factor 10 over the reference.
One row is over that cap (THETA * 8, log density only, lv_ref.LOG_DENSITY_EXCEPTIONS): it is held to 10 x
its own recorded noise.  The step table is held to 10 x the recorded drift of scipy's step times and states
(lv_ref.RECORDED), its observation ranges to the exact integers.
"""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from oracle import lv_numpy as ol  # noqa: E402
from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import lv_ref as R  # noqa: E402
from tests.test_gpu_lv import RTOL  # noqa: E402

FORMS_TOL = 1e-11        # two-phase against single-phase (tests/test_gpu_lv.py)
STEP_CAP, STEP_REC = 64, 56


def _abi(th, data, rtol=lv.RTOL, atol=lv.ATOL, max_steps=lv.MAX_STEPS, two_phase=True):
    """The gradient through the C ABI: st_lv_grad_log_posterior_ws (record, phase B, overflow fallback) or
    st_lv_grad_log_posterior (the single-phase kernel; no st_tune key selects it).  Returns (out, status) and,
    for the two-phase entry, the workspace it leaves: (steps (n, 64, 56), nsteps (n,)).

    Workspace layout (capi.hip st_lv_grad_log_posterior_ws, lv.hip kLvStepRec): n x 64 step records of 56
    doubles -- t_old, 1 / h, k_begin, k_end, y_old[10], hQ[10][4], 2 of padding -- then, at byte offset
    n * 64 * 56 * 8, the int32 count of recorded steps per point."""
    th = np.ascontiguousarray(th, dtype=np.float64)
    t, y, s = lv._settings(data, rtol, atol)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(data.cov, dtype=np.float64)))
    dev = nat.require_device()
    L = nat.lib()
    n = th.shape[0]
    out = torch.empty((n, 4), dtype=torch.float64, device=dev)
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    thd, td, yd = (torch.from_numpy(a).to(dev) for a in (th, t, y))
    if not two_phase:
        nat.check(L.st_lv_grad_log_posterior(
            nat.ptr(thd), n, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data, cinv.ctypes.data, int(max_steps),
            nat.ptr(out), nat.ptr(status), nat.stream_handle()), 'st_lv_grad_log_posterior')
        return out.cpu().numpy(), status.cpu().numpy()
    wb = int(L.st_lv_grad_workspace_bytes(n, t.size))
    assert wb == n * (STEP_CAP * STEP_REC * 8 + 8)
    work = torch.zeros((wb + 7) // 8, dtype=torch.float64, device=dev)
    nat.check(L.st_lv_grad_log_posterior_ws(
        nat.ptr(thd), n, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data, cinv.ctypes.data, int(max_steps),
        nat.ptr(out), nat.ptr(status), nat.ptr(work), wb, nat.stream_handle()), 'st_lv_grad_log_posterior_ws')
    w = work.cpu().numpy()
    steps = w[:n * STEP_CAP * STEP_REC].reshape(n, STEP_CAP, STEP_REC)
    nsteps = w.view(np.int32)[2 * n * STEP_CAP * STEP_REC:][:n]
    return out.cpu().numpy(), status.cpu().numpy(), (steps, nsteps)


def _quiet(f, *args, **kw):
    """f(...) with the status warning an error: no status may reach the caller on a good batch."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        return f(*args, **kw)


def _check_gradient(s, label=''):
    """Both forms of the gradient on set ``s`` against scipy within RTOL, and against each other."""
    want = R.gradient(s)
    two = _quiet(lv.grad_log_posterior, s.theta, s.data, rtol=s.rtol, atol=s.atol)
    one, status = _abi(s.theta, s.data, s.rtol, s.atol, two_phase=False)
    assert not status.any()
    e2, e1, ef = R.grad_error(two, want), R.grad_error(one, want), R.grad_error(two, one)
    print(f'{s.name}{label}: gradient against scipy: two-phase {e2.max():.2e}, single-phase {e1.max():.2e} '
          f'(bound {RTOL:g}); between the forms {ef.max():.2e} (bound {FORMS_TOL:g})')
    assert e2.max() < RTOL, (int(e2.argmax()), e2.max())
    assert e1.max() < RTOL, (int(e1.argmax()), e1.max())
    assert ef.max() < FORMS_TOL, (int(ef.argmax()), ef.max())
    return two, one


def _check_log_density(s, label=''):
    want = R.log_density(s)
    got = _quiet(lv.log_target_density, np.log(s.theta), s.data, rtol=s.rtol, atol=s.atol)
    err = np.abs(got - want) / np.abs(want)
    bound = np.full(len(want), RTOL)
    for row, delta in R.LOG_DENSITY_EXCEPTIONS.get(s.name, {}).items():
        print(f'{s.name}: log density row {row}: {err[row]:.2e} (bound {R.DRIFT_FACTOR * delta:g}, 10 x its noise)')
        bound[row] = R.DRIFT_FACTOR * delta
    rest = np.where(bound == RTOL, err, 0.0)
    print(f'{s.name}{label}: log density against scipy {rest.max():.2e} (bound {RTOL:g})')
    assert np.all(err < bound), (int(np.argmax(err / bound)), err.max())
    return got


# ---- a. dense covariance

@pytest.mark.parametrize('name', ['cov_pos', 'cov_neg', 'cov_asym'])
def test_dense_covariance_gradient(name):
    """cinv[1], cinv[2] are non-zero; 'cov_asym' hands the kernels a non-symmetric C^-1 (the ABI takes four
    doubles, row-major), the one input that tells cinv[1] from cinv[2]."""
    s = R.input_sets()[name]
    cinv = np.linalg.inv(s.data.cov)
    assert abs(cinv[0, 1]) > 1 and abs(cinv[1, 0]) > 1
    assert (name == 'cov_asym') == (abs(cinv[0, 1] - cinv[1, 0]) > 1)
    _check_gradient(s)


@pytest.mark.parametrize('name', ['cov_pos', 'cov_neg'])
def test_dense_covariance_log_density(name):
    """The whitening matrix PsdFactor.U is dense and not symmetric: z = r U, not r U^T."""
    from stein_thinning.proxy import PsdFactor
    s = R.input_sets()[name]
    U = PsdFactor(s.data.cov, allow_singular=False).U
    assert abs(U[0, 1] - U[1, 0]) > 0.1 and np.abs(U @ U.T - np.linalg.inv(s.data.cov)).max() < 1e-10
    _check_log_density(s)


# ---- b. wide theta: points on both sides of the 64-step table in one batch

def test_wide_theta_mixed_overflow_gradient():
    s = R.input_sets()['wide']
    n_acc = np.array([ol.n_steps(th) for th in s.theta])
    assert n_acc.min() < 64 < n_acc.max() and len(n_acc) <= 64          # both kinds in one 64-thread block
    rec = R.record_counts(s)
    over = rec > STEP_CAP
    assert np.array_equal(over, n_acc > 64) and not np.any(np.abs(rec - 64.5) < 2)
    assert any(0 < over[b:b + 8].sum() < 8 for b in range(0, len(over) - 7, 8))   # and in one phase-B block
    two, one = _check_gradient(s)
    out, status, (_, nsteps) = _abi(s.theta, s.data)
    assert not status.any(), status                                     # the overflow status stays inside
    np.testing.assert_array_equal(out, two)
    np.testing.assert_array_equal(nsteps[over], STEP_CAP)
    np.testing.assert_array_equal(nsteps[~over], rec[~over])
    # overflowed rows are the single-phase kernel's, bit for bit
    np.testing.assert_array_equal(two[over], one[over])
    assert not np.array_equal(two[~over], one[~over])                  # (the others are phase B's)


def test_wide_theta_log_density():
    _check_log_density(R.input_sets()['wide'])


# ---- c. tolerances, span, initial state

@pytest.mark.parametrize('name', ['tol5', 'tol7_dense', 'tol7_sparse', 'loose', 'span', 'span_tol5'])
def test_tolerances_span_and_initial_state(name):
    s = R.input_sets()[name]
    rec = R.record_counts(s)
    acc = np.array([R.solve(th, s).accepted for th in s.theta])
    if name == 'tol7_dense':
        assert rec.min() > STEP_CAP            # every point overflows
    if name == 'tol7_sparse':
        assert acc.min() > 100 and rec.max() == 40 == len(s.data.t)   # phase B across many unrecorded steps
    if name.startswith('span'):
        assert tuple(s.data.t_span) == (1.0, 9.5) and tuple(s.data.u_init) == (0.8, 1.7)
        assert s.data.t[0] < 1.0 and s.data.t[-1] > 9.5
    two, one = _check_gradient(s)
    if name == 'tol7_dense':
        np.testing.assert_array_equal(two, one)
    _check_log_density(s)


# ---- d. observation grids

GRIDS = [f'grid_{n}' for n in R.SMALL_T_N] + ['grid_repeats', 'grid_outside', 'grid_sol_t']


@pytest.mark.parametrize('name', GRIDS)
def test_observation_grids(name):
    s = R.input_sets()[name]
    t = s.data.t
    if name == 'grid_repeats':
        c = np.unique(t, return_counts=True)[1]
        assert (c == 3).sum() >= 3 and (c == 2).sum() >= 3
    if name == 'grid_outside':
        assert t[0] < s.data.t_span[0] and t[-1] > s.data.t_span[1]
    _check_gradient(s)
    _check_log_density(s)


@pytest.mark.parametrize('name', ['grid_3', 'grid_65'])
def test_small_grid_with_observations_in_global_memory(name):
    """st_tune key 17 = 1: phase B reads the observations from global memory (4 points per block)."""
    L = nat.lib()
    assert L.st_tune(17, 1) == 0
    try:
        _check_gradient(R.input_sets()[name], ' (key 17 = 1)')
    finally:
        L.st_tune(17, -1)


# ---- e. the step table against sol.t

@pytest.mark.parametrize('name', R.STEP_TABLE_SETS)
def test_step_table_matches_scipys_steps(name):
    """What phase A leaves in the workspace, record by record, against scipy's accepted steps: as many
    records as scipy has segments that hold an observation, each with that segment's ends, its state at the
    left end and exactly np.searchsorted's observation range."""
    s = R.input_sets()[name]
    t_obs = np.asarray(s.data.t)
    span = s.data.t_span[1] - s.data.t_span[0]
    t_tol = R.DRIFT_FACTOR * R.RECORDED[name][3] * span
    y_tol = R.DRIFT_FACTOR * R.RECORDED[name][4]
    assert t_tol < R.BOUNDARY_DISTANCE * span
    out, status, (steps, nsteps) = _abi(s.theta, s.data, s.rtol, s.atol)
    assert not status.any()
    worst_t = worst_y = 0.0
    checked = 0
    for i, th in enumerate(s.theta):
        sol = R.solve(th, s)
        want = R.records(sol, t_obs)
        if len(want) > STEP_CAP:
            assert nsteps[i] == STEP_CAP
            continue
        assert nsteps[i] == len(want), (i, nsteps[i], len(want))
        r = steps[i, :len(want)]
        seg = np.array([w[0] for w in want])
        np.testing.assert_array_equal(r[:, 2], [w[1] for w in want])
        np.testing.assert_array_equal(r[:, 3], [w[2] for w in want])
        worst_t = max(worst_t, np.abs(r[:, 0] - sol.t[seg]).max(), np.abs(r[:, 0] + 1.0 / r[:, 1] - sol.t[seg + 1]).max())
        yscale = np.abs(sol.y).max(axis=1)
        worst_y = max(worst_y, (np.abs(r[:, 4:14] - sol.y[:, seg].T) / yscale[None, :]).max())
        checked += 1
    print(f'{name}: {checked} of {len(s.theta)} points in the table; step times off by {worst_t:.2e} (bound {t_tol:.2e}), '
          f'states by {worst_y:.2e} (bound {y_tol:.2e})')
    assert checked >= len(s.theta) // 2
    assert worst_t <= t_tol
    assert worst_y <= y_tol


@pytest.mark.parametrize('row', [0, 5])
def test_segment_rule_on_the_kernels_own_step_boundaries(row):
    """OdeSolution's rule: an observation at a step boundary t_j belongs to the segment that ends there,
    (t_j-1, t_j].  The step sequence does not depend on the observations, so a first run gives the kernel's
    own boundaries, bit for bit (the t_old of every record after the first); a second run observes exactly at
    them and halfway between.  Expected ranges: np.searchsorted(.., 'right') on scipy's step times with the
    kernel's own value put in place of each one it reported."""
    import types
    s = R.input_sets()['table_dense']
    th = s.theta[row:row + 1]
    sol = R.solve(th[0], s)
    _, status, (steps, nsteps) = _abi(th, s.data)
    assert status[0] == 0 and nsteps[0] > 20
    bounds = steps[0, 1:nsteps[0], 0].copy()
    t_tol = R.DRIFT_FACTOR * R.RECORDED['table_dense'][3] * 25.0
    idx = np.abs(sol.t[None, :] - bounds[:, None]).argmin(axis=1)
    assert np.abs(sol.t[idx] - bounds).max() <= t_tol and len(set(idx)) == len(idx)
    t_kernel = sol.t.copy()
    t_kernel[idx] = bounds
    edges = np.concatenate([[0.0], bounds, [25.0]])
    mids = 0.5 * (edges[:-1] + edges[1:])
    assert np.abs(mids[:, None] - t_kernel[None, :]).min() > R.BOUNDARY_DISTANCE * 25.0
    grid = np.sort(np.concatenate([bounds, mids]))
    data = R.on_grid(grid)
    want = R.records(types.SimpleNamespace(t=t_kernel), grid)
    got, status, (steps2, nsteps2) = _abi(th, data)
    assert status[0] == 0 and nsteps2[0] == len(want)
    r = steps2[0, :len(want)]
    np.testing.assert_array_equal(r[:, 0], t_kernel[[w[0] for w in want]])
    np.testing.assert_array_equal(r[:, 2], [w[1] for w in want])
    np.testing.assert_array_equal(r[:, 3], [w[2] for w in want])
    # every boundary time is the last observation of a record
    assert set(np.searchsorted(grid, bounds, 'right')) <= set(r[:, 3].astype(int))
    ref = ol.grad_from_solution(sol, th[0], data.t, data.y, data.cov)
    assert R.grad_error(got, ref[None, :]).max() < RTOL


# ---- f. max_steps (status 2)

def test_max_steps_boundary_gradient():
    """max_steps = scipy's step count N of the 10-state system succeeds with the default run's bits;
    N - 1 ends as status 2 and NaN, in both forms."""
    s = R.input_sets()['scale04']
    th = s.theta[2:3]
    n = ol.n_steps(th[0])
    free = _quiet(lv.grad_log_posterior, th, s.data)
    np.testing.assert_array_equal(_quiet(lv.grad_log_posterior, th, s.data, max_steps=n), free)
    with pytest.warns(RuntimeWarning, match=r'failed for 1 parameter point\(s\) \(first: 0, status 2\)'):
        assert np.isnan(lv.grad_log_posterior(th, s.data, max_steps=n - 1)).all()
    one_free = _abi(th, s.data, two_phase=False)[0]
    out, status = _abi(th, s.data, max_steps=n, two_phase=False)
    assert status[0] == 0 and np.array_equal(out, one_free)
    out, status = _abi(th, s.data, max_steps=n - 1, two_phase=False)
    assert status[0] == 2 and np.isnan(out).all()


def test_max_steps_boundary_log_density():
    """The same with N of the 2-state system (its own step sequence)."""
    s = R.input_sets()['scale04']
    th = s.theta[2:3]
    n, n10 = ol.n_steps(th[0], sensitivity=False), ol.n_steps(th[0])
    assert n < n10
    free = _quiet(lv.log_target_density, np.log(th), s.data)
    np.testing.assert_array_equal(_quiet(lv.log_target_density, np.log(th), s.data, max_steps=n), free)
    with pytest.warns(RuntimeWarning, match=r'failed for 1 parameter point\(s\) \(first: 0, status 2\)'):
        assert np.isnan(lv.log_target_density(np.log(th), s.data, max_steps=n - 1)).all()


def test_max_steps_in_a_mixed_batch():
    """max_steps = 40 on points that need 23 to 56 steps: exactly the rows over 40 are NaN with status 2,
    the warning counts them and names the first, every other row keeps the unrestricted run's bits."""
    s = R.input_sets()['scale04']
    n = np.array([ol.n_steps(th) for th in s.theta])
    bad = n > 40
    assert 3 <= bad.sum() <= len(n) - 3 and n.min() == 23 and n.max() == 56
    first = int(np.flatnonzero(bad)[0])
    free = _quiet(lv.grad_log_posterior, s.theta, s.data)
    with pytest.warns(RuntimeWarning, match=rf'failed for {bad.sum()} parameter point\(s\) \(first: {first}, status 2\)'):
        got = lv.grad_log_posterior(s.theta, s.data, max_steps=40)
    assert np.array_equal(np.isnan(got).all(axis=1), bad) and np.array_equal(np.isnan(got).any(axis=1), bad)
    np.testing.assert_array_equal(got[~bad], free[~bad])
    out, status, _ = _abi(s.theta, s.data, max_steps=40)
    np.testing.assert_array_equal(status, np.where(bad, 2, 0))
    np.testing.assert_array_equal(out, got)
    one_free = _abi(s.theta, s.data, two_phase=False)[0]
    out, status = _abi(s.theta, s.data, max_steps=40, two_phase=False)
    np.testing.assert_array_equal(status, np.where(bad, 2, 0))
    assert np.array_equal(np.isnan(out).all(axis=1), bad)
    np.testing.assert_array_equal(out[~bad], one_free[~bad])


def test_overflow_then_max_steps_ends_as_status_2():
    """THETA * 4 takes 115 steps: it overflows the step table at the 65th and then hits max_steps = 100 in
    the single-phase rerun.  The caller sees status 2 and NaN, never the internal overflow status; the good
    neighbour keeps its bits."""
    s = R.input_sets()['wide']
    th = np.stack([s.theta[50], lv.THETA])
    assert ol.n_steps(th[0]) == 115 and ol.n_steps(th[1]) < 64
    out, status, (_, nsteps) = _abi(th, s.data, max_steps=100)
    assert status.tolist() == [2, 0] and nsteps[0] == STEP_CAP
    assert np.isnan(out[0]).all()
    np.testing.assert_array_equal(out[1], _quiet(lv.grad_log_posterior, lv.THETA, s.data)[0])


# ---- g. non-finite theta (status 1)

def test_non_finite_theta_rows_fail_alone():
    """A NaN or +inf coordinate makes every error norm NaN: never < 1, so the step shrinks by
    fmax(0.2, NaN) = 0.2 per attempt from at most t1 - t0 until it is below min_step (ten times the smallest
    subnormal at t = 0; ~465 attempts, or at once when the initial step is already 0) and the point ends with
    status 1.  The bad rows are NaN with a non-zero status and a warning; the good rows keep their bits."""
    s = R.input_sets()['scale04']
    th = s.theta[:9].copy()
    th[3, 2] = np.nan
    th[6, 0] = np.inf
    bad = np.zeros(9, dtype=bool)
    bad[[3, 6]] = True
    free = _quiet(lv.grad_log_posterior, s.theta[:9], s.data)
    with pytest.warns(RuntimeWarning, match=r'failed for 2 parameter point\(s\) \(first: 3, status 1\)'):
        got = lv.grad_log_posterior(th, s.data)
    assert np.isnan(got[bad]).all()
    np.testing.assert_array_equal(got[~bad], free[~bad])
    out, status = _abi(th, s.data, two_phase=False)
    assert np.array_equal(status != 0, bad) and np.isnan(out[bad]).all()
    np.testing.assert_array_equal(out[~bad], _abi(s.theta[:9], s.data, two_phase=False)[0][~bad])
    out, status, _ = _abi(th, s.data)
    assert np.array_equal(status != 0, bad) and not (status == 3).any()
    free = _quiet(lv.log_target_density, np.log(s.theta[:9]), s.data)
    with np.errstate(invalid='ignore'):
        lth = np.log(th)
    with pytest.warns(RuntimeWarning, match=r'failed for 2 parameter point\(s\) \(first: 3, status 1\)'):
        got = lv.log_target_density(lth, s.data)
    assert np.isnan(got[bad]).all()
    np.testing.assert_array_equal(got[~bad], free[~bad])


# ---- h. batch shape and chunks

BATCH = R.points(129, 0.3, 25)


@pytest.fixture(scope='module')
def full_batch():
    d = R.reference_data()
    return (_quiet(lv.grad_log_posterior, BATCH, d), _abi(BATCH, d, two_phase=False)[0],
            _quiet(lv.log_target_density, np.log(BATCH), d))


@pytest.mark.parametrize('n', [1, 7, 8, 9, 63, 64, 65, 129])
def test_rows_do_not_depend_on_the_batch(full_batch, n):
    """f(theta[:n]) is f(theta)[:n], bit for bit: partial 64-thread blocks, partial 8-point phase-B blocks."""
    d = R.reference_data()
    two, one, dens = full_batch
    np.testing.assert_array_equal(_quiet(lv.grad_log_posterior, BATCH[:n], d), two[:n])
    np.testing.assert_array_equal(_abi(BATCH[:n], d, two_phase=False)[0], one[:n])
    np.testing.assert_array_equal(_quiet(lv.log_target_density, np.log(BATCH[:n]), d), dens[:n])


def test_log_target_density_chunks(full_batch):
    d = R.reference_data()
    np.testing.assert_array_equal(_quiet(lv.log_target_density, np.log(BATCH[:30]), d, chunk=7), full_batch[2][:30])
