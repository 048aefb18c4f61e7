"""The conditions the GPU edge tests of the Lotka-Volterra kernels rely on (tests/test_gpu_lv_edges.py),
checked without a device on the input sets of tests/lv_ref.py: the extended oracle keeps its defaults, every
selected point is far from a flipped step decision, scipy's own reordering noise is under the cap the 1e-8
bound of the GPU tests assumes, and no observation of a step-table set sits next to a step boundary.  A GPU
failure on these inputs is then the kernel's, not the inputs'."""
import json
import os

import numpy as np
import pytest

from oracle import lv_numpy as ol
from tests import lv_ref as R

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'lv_reference.json')))
NAMES = list(R.RECORDED)

needs_sequential = pytest.mark.skipif(not R.sequential_available(),
                                      reason="this scipy lacks the private names the sequential-order solver replaces")


def test_every_input_set_has_recorded_constants():
    assert set(R.input_sets()) == set(R.RECORDED)
    assert set(R.STEP_TABLE_SETS) <= set(R.RECORDED) and set(R.LOG_DENSITY_EXCEPTIONS) <= set(R.RECORDED)


def test_extended_oracle_keeps_its_defaults():
    """rtol / atol / t_span / u_init passed through to solve_ivp: at the defaults, given or not, the values
    the reference module itself produced (tests/golden/lv_reference.json), bit for bit."""
    d = R.reference_data()
    for lt, want in zip(GOLDEN['log_theta'], GOLDEN['log_target_density']):
        lt = np.array(lt)
        assert ol.log_target_density(lt, d.t, d.y, d.cov) == want
        assert ol.log_target_density(lt, d.t, d.y, d.cov, t_span=tuple(GOLDEN['t_span']),
                                     u_init=tuple(GOLDEN['u_init']), rtol=1e-3, atol=1e-6) == want
        th = np.exp(lt)
        g = ol.grad_log_posterior(th, d.t, d.y, d.cov)
        assert np.array_equal(g, ol.grad_log_posterior(th, d.t, d.y, d.cov, (0, 25), (1., 1.), 1e-3, 1e-6))
        assert ol.n_steps(th) == ol.n_steps(th, rtol=1e-3, atol=1e-6) == R.solution(th).accepted


def test_oracle_passes_tolerances_span_and_state_on():
    """Each argument reaches the solver: it moves the step count or the ends of sol.t."""
    th = np.exp(np.array(GOLDEN['log_theta'][0]))
    assert ol.n_steps(th, rtol=1e-7, atol=1e-10) > 2 * ol.n_steps(th)
    assert ol.n_steps(th, rtol=1e-3, atol=1e-3) < ol.n_steps(th, rtol=1e-3, atol=1e-12)
    sol = ol.solve(th, (1.0, 9.5), (0.8, 1.7))
    assert sol.t[0] == 1.0 and sol.t[-1] == 9.5 and sol.y[:2, 0].tolist() == [0.8, 1.7] and not sol.y[2:, 0].any()


def test_recorder_does_not_move_scipy():
    """The recording subclass is scipy's RK45: same steps and values, bit for bit; one logged norm per attempt."""
    th = R.input_sets()['wide'].theta[50]
    sol, plain = R.solution(th), ol.solve(th)
    assert np.array_equal(sol.t, plain.t) and np.array_equal(sol.y, plain.y)
    assert sol.accepted == len(plain.t) - 1 and sol.rejected > 0
    assert 6 * (sol.accepted + sol.rejected) + 2 == plain.nfev == sol.nfev
    assert np.sum(sol.error_norms < 1) == sol.accepted


@needs_sequential
@pytest.mark.parametrize('name', NAMES)
def test_sequence_stability_and_noise_cap(name):
    """Every point of the set: margin >= 1e-5, the sequential-order solve takes scipy's accepted and rejected
    counts, and delta <= 1e-9 for the gradient and the log density (the listed exception apart: its row is
    measured against its own recorded delta).  The figures are those of lv_ref.RECORDED, measured again; another
    BLAS may move them by rounding, never over the cap."""
    s = R.input_sets()[name]
    got, same = R.measure(s)
    print(f"    '{name}': ({', '.join(f'{v:.1e}' for v in got)}),")
    dg, dl, margin, dt, dy = got
    assert same
    assert margin >= R.MARGIN_MIN
    assert dg <= R.NOISE_CAP and dl <= R.NOISE_CAP
    rec = R.RECORDED[name]
    for value, recorded in zip((dg, dl, dt, dy), (rec[0], rec[1], rec[3], rec[4])):
        assert value <= R.DRIFT_FACTOR * recorded
    assert margin >= rec[2] / R.DRIFT_FACTOR
    for row, recorded in R.LOG_DENSITY_EXCEPTIONS.get(name, {}).items():
        one = R.InputSet(name + '_row', s.theta[row:row + 1], s.data, s.rtol, s.atol)
        w = R.log_density(one)
        delta = abs(R.log_density(one, True)[0] - w[0]) / abs(w[0])
        print(f'    exception row {row}: {delta:.1e}')
        assert R.NOISE_CAP < delta <= R.DRIFT_FACTOR * recorded


@pytest.mark.parametrize('name', R.STEP_TABLE_SETS)
def test_boundary_distance_of_the_step_table_sets(name):
    """No observation within 1e-6 (t1 - t0) of an interior step boundary of any point, and 10 x the recorded
    drift of the step times stays below that distance: the step table's observation ranges are then the
    same integers for any solver whose step times are within the drift of scipy's."""
    s = R.input_sets()[name]
    dist = R.boundary_distance(s)
    print(name, 'boundary distance', dist)
    assert dist >= R.BOUNDARY_DISTANCE
    assert R.DRIFT_FACTOR * R.RECORDED[name][3] < R.BOUNDARY_DISTANCE


def test_grid_sol_t_sits_on_the_boundaries():
    """The one set that places observations on step boundaries on purpose."""
    s = R.input_sets()['grid_sol_t']
    assert np.array_equal(s.data.t, R.solution(s.theta[0]).t) and R.boundary_distance(s) == 0.0


def test_wide_set_mixes_both_sides_of_the_step_table():
    """Accepted steps on both sides of 64 within the one 64-thread block and within an 8-point phase-B block."""
    s = R.input_sets()['wide']
    n = np.array([ol.n_steps(th) for th in s.theta])
    assert len(n) <= 64 and n.min() < 30 and n.max() > 200
    over = n > 64
    assert any(0 < over[b:b + 8].sum() < len(over[b:b + 8]) for b in range(0, len(n), 8))
    assert [int(v) for v in n[48:]] == [18, 60, 115, 227]
