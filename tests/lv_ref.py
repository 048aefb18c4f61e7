"""Shared helper of the Lotka-Volterra edge tests (tests/test_lv_ref_cpu.py, tests/test_gpu_lv_edges.py):
the input sets, scipy's solution of each point (solved once and shared; the inputs go to torch.from_numpy,
so they stay writable: no test writes to them), and a measure of how far scipy's own values move when
nothing but the order of its sums changes.

The kernel (csrc/lv.hip) claims scipy's step sequence.  The only discontinuous decision of the step
controller is ``error_norm < 1``; ``recorder()`` is an RK45 subclass that logs every attempt's error norm, so

  margin(point) = min over attempts |error_norm - 1|

says how far a point is from a flipped decision.  ``recorder(sequential=True)`` forms the stage sums, the
error estimate and the dense-output Q as left-to-right sums in the kernel's order (K[0] c0 + K[1] c1 + ...)
where scipy calls np.dot: the relative difference delta between the two (max|diff| / max|want| per row) is
the reference's own reordering noise.  No implementation that sums in another order can be held below it;
the GPU tests hold the kernels to 1e-8, and every input set below keeps delta <= NOISE_CAP = 1e-9.  The
sequential variant touches private scipy names (rk.rk_step, RungeKutta._estimate_error,
._dense_output_impl, rk.RkDenseOutput): only CPU tests use it, and ``sequential_available()`` says whether
this scipy has them.

RECORDED holds, per input set, what tests/test_lv_ref_cpu.py measures again (scipy 1.15.3, NumPy 2.x with
OpenBLAS): delta of the gradient, delta of the log density, the smallest margin over both systems, and
the drift of the step times and of the states at them (scipy against the sequential variant, relative to
the span / to max|y| per row).  The step-table test (tests/test_gpu_lv_edges.py) allows 10 x the drift.
"""
import contextlib
import functools
from dataclasses import dataclass

import numpy as np

from oracle import lv_numpy as ol
from stein_thinning import lotka_volterra as lv

NOISE_CAP = 1e-9          # delta of every input set (a condition on the inputs, not a tolerance)
MARGIN_MIN = 1e-5         # smallest |error_norm - 1| of every selected point
BOUNDARY_DISTANCE = 1e-6  # x (t1 - t0): no observation this near a step boundary in the step-table sets
DRIFT_FACTOR = 10.0

COV_POS = np.array([[0.05, 0.02], [0.02, 0.03]])
COV_NEG = np.array([[0.06, -0.03], [-0.03, 0.04]])
COV_ASYM = np.array([[0.05, 0.03], [0.01, 0.03]])


@dataclass(frozen=True)
class InputSet:
    name: str
    theta: np.ndarray
    data: lv.LvData
    rtol: float = lv.RTOL
    atol: float = lv.ATOL
    log_density: bool = True      # False: a covariance only the gradient accepts

    @property
    def solver(self):
        return dict(rtol=self.rtol, atol=self.atol, t_span=tuple(self.data.t_span), u_init=tuple(self.data.u_init))


def points(n, scale, seed):
    """n draws of log-scale ``scale`` around the data-generating theta."""
    rng = np.random.default_rng(seed)
    return np.exp(np.log(lv.THETA) + scale * rng.normal(size=(n, 4)))


@functools.lru_cache(maxsize=None)
def reference_data():
    return lv.reference_data()


def on_grid(t, cov=None, t_span=lv.T_SPAN, u_init=lv.U_INIT):
    """The reference observations interpolated to the times ``t``."""
    d = reference_data()
    t = np.asarray(t, dtype=np.float64)
    y = np.stack([np.interp(t, d.t, d.y[:, 0]), np.interp(t, d.t, d.y[:, 1])], axis=1)
    return lv.LvData(t=t, y=y, cov=lv.C.copy() if cov is None else np.array(cov), t_span=t_span, u_init=u_init)


SMALL_T_N = [1, 2, 3, 63, 64, 65, 129]
WIDE_EXTRA = [0.5, 2.0, 4.0, 8.0]


@functools.lru_cache(maxsize=None)
def input_sets():
    """name -> InputSet, every set of tests/test_gpu_lv_edges.py that is compared with scipy."""
    d = reference_data()
    sets = []

    def add(name, theta, data, rtol=lv.RTOL, atol=lv.ATOL, log_density=True):
        sets.append(InputSet(name, np.ascontiguousarray(theta), data, rtol, atol, log_density))

    # a. dense covariance
    th_a = points(24, 0.1, 21)
    add('cov_pos', th_a, lv.LvData(t=d.t, y=d.y, cov=COV_POS.copy()))
    add('cov_neg', th_a, lv.LvData(t=d.t, y=d.y, cov=COV_NEG.copy()))
    # the gradient's C^-1 reaches the kernels as four doubles, row-major: a non-symmetric matrix tells
    # cinv[1] from cinv[2], which every covariance leaves equal
    add('cov_asym', th_a, lv.LvData(t=d.t, y=d.y, cov=COV_ASYM.copy()), log_density=False)
    # b. wide theta: both sides of the 64-step table in one batch
    add('wide', np.concatenate([points(48, 1.0, 31), lv.THETA[None, :] * np.array(WIDE_EXTRA)[:, None]]), d)
    # c. tolerances, span, initial state
    th_c = points(12, 0.1, 23)
    add('tol5', th_c, d, 1e-5, 1e-8)
    add('tol7_dense', th_c, d, 1e-7, 1e-10)
    add('tol7_sparse', th_c, on_grid(np.linspace(0.3, 24.8, 40)), 1e-7, 1e-10)
    add('loose', th_c, d, *LOOSE_TOL)
    add('span', th_c, on_grid(np.linspace(0.8, 9.7, 700), t_span=(1.0, 9.5), u_init=(0.8, 1.7)))
    add('span_tol5', th_c, on_grid(np.linspace(0.8, 9.7, 700), t_span=(1.0, 9.5), u_init=(0.8, 1.7)), 1e-5, 1e-8)
    # d. observation grids
    th_d = points(12, 0.1, 24)
    for t_n in SMALL_T_N:
        add(f'grid_{t_n}', th_d, on_grid(np.linspace(0.7, 24.3, t_n)))
    base = np.linspace(0.5, 24.5, 31)
    add('grid_repeats', th_d, on_grid(np.repeat(base, np.where(np.arange(31) % 5 == 2, 3, np.where(np.arange(31) % 5 == 4, 2, 1)))))
    add('grid_outside', th_d, on_grid(np.linspace(-0.4, 25.3, 90)))
    add('grid_sol_t', np.concatenate([lv.THETA[None, :], th_d[:11]]), on_grid(solution(lv.THETA).t))
    # f. the max_steps boundary: the scale-0.4 points of tests/test_gpu_lv.py
    add('scale04', points(20, 0.4, 3), d)
    # e. the step table against sol.t: grids that keep BOUNDARY_DISTANCE from every step boundary
    add('table_wide', sets[3].theta, on_grid(np.linspace(0.05, 24.95, 150)))
    add('table_dense', th_d, on_grid(np.linspace(0.0, 25.0, 1203)))
    return {s.name: s for s in sets}


LOOSE_TOL = (1e-2, 1e-5)
# the sets whose step table is read back and pinned to sol.t: every observation keeps BOUNDARY_DISTANCE
# from every step boundary
STEP_TABLE_SETS = ['table_wide', 'table_dense', 'tol7_sparse', 'span', 'grid_3', 'grid_64', 'grid_repeats',
                   'grid_outside']

# The one point over the cap: THETA * 8 (row 51 of 'wide'), whose 2-state solution takes 176 steps: scipy's
# own log density moves by 8.3e-7 (relative) when its sums are reordered.
# Its gradient is under the cap (4.8e-12).  The GPU test holds that row's log density to 10 x this delta (the
# factor covers the kernel's further reassociations: Horner dense output, numpy-pairwise sum) and every other
# row of the set to 1e-8.
LOG_DENSITY_EXCEPTIONS = {'wide': {51: 8.3e-07}, 'table_wide': {51: 8.3e-07}}

# name: (delta gradient, delta log density, smallest margin, drift of sol.t / span, drift of sol.y)
RECORDED = {
    'cov_pos': (1.8e-12, 1.7e-10, 3.9e-04, 4.2e-12, 9.6e-11),
    'cov_neg': (2.3e-12, 2.7e-10, 3.9e-04, 4.2e-12, 9.6e-11),
    'cov_asym': (2.0e-12, 0.0, 3.9e-04, 4.2e-12, 9.6e-11),      # (gradient only)
    'wide': (5.4e-10, 6.7e-11, 9.1e-04, 5.0e-10, 7.6e-08),
    'tol5': (3.5e-15, 5.6e-14, 4.0e-04, 1.9e-12, 2.3e-11),
    'tol7_dense': (7.4e-15, 9.2e-15, 9.9e-05, 3.4e-10, 5.6e-09),
    'tol7_sparse': (7.4e-15, 1.4e-14, 9.9e-05, 3.4e-10, 5.6e-09),
    'loose': (5.1e-10, 6.2e-10, 1.7e-02, 2.4e-10, 8.7e-09),
    'span': (4.1e-11, 1.8e-12, 3.0e-03, 3.6e-12, 4.7e-11),
    'span_tol5': (4.1e-11, 4.9e-13, 6.7e-03, 2.2e-10, 2.3e-09),
    'grid_1': (5.9e-15, 2.8e-14, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_2': (1.4e-12, 1.0e-11, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_3': (7.9e-13, 6.5e-12, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_63': (9.0e-13, 1.5e-11, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_64': (1.0e-12, 7.1e-12, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_65': (1.0e-12, 5.9e-12, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_129': (1.1e-12, 7.0e-12, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_repeats': (1.1e-12, 5.9e-12, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_outside': (3.8e-10, 5.1e-12, 1.2e-02, 1.7e-11, 2.1e-10),
    'grid_sol_t': (9.8e-13, 1.3e-11, 1.2e-02, 1.7e-11, 2.1e-10),
    'scale04': (1.7e-10, 3.7e-11, 7.4e-04, 7.8e-11, 1.9e-09),
    'table_wide': (4.0e-10, 9.2e-11, 9.1e-04, 5.0e-10, 7.6e-08),
    'table_dense': (8.1e-13, 1.5e-11, 1.2e-02, 1.7e-11, 2.1e-10),
}


def _scipy_private():
    from scipy.integrate import RK45
    from scipy.integrate._ivp import rk
    for obj, name in ((rk, 'rk_step'), (rk, 'RkDenseOutput'), (RK45, '_estimate_error'),
                      (RK45, '_estimate_error_norm'), (RK45, '_dense_output_impl')):
        if not hasattr(obj, name):
            return None
    return rk


def sequential_available():
    return _scipy_private() is not None


def _lsum(rows, coef):
    """rows[0] coef[0] + rows[1] coef[1] + ..., left to right, per component."""
    s = rows[0] * coef[0]
    for j in range(1, len(coef)):
        s = s + rows[j] * coef[j]
    return s


def _rk_step_sequential(fun, t, y, f, h, A, B, C, K):
    """scipy's rk.rk_step with the np.dot calls written as left-to-right sums."""
    K[0] = f
    for s in range(1, len(C)):
        dy = _lsum(K[:s], A[s, :s]) * h
        K[s] = fun(t + C[s] * h, y + dy)
    y_new = y + h * _lsum(K[:-1], B)
    f_new = fun(t + h, y_new)
    K[-1] = f_new
    return y_new, f_new


def recorder(sequential=False):
    """(solver class for solve_ivp's ``method=``, the list its instances append every error norm to)."""
    from scipy.integrate import RK45
    log = []

    class Recorder(RK45):
        def _estimate_error_norm(self, K, h, scale):
            e = super()._estimate_error_norm(K, h, scale)
            log.append(float(e))
            return e

    if sequential:
        rk = _scipy_private()

        class Recorder(Recorder):   # noqa: F811
            def _estimate_error(self, K, h):
                return _lsum(K, self.E) * h

            def _dense_output_impl(self):
                Q = np.stack([_lsum(self.K, self.P[:, q]) for q in range(self.P.shape[1])], axis=1)
                return rk.RkDenseOutput(self.t_old, self.t, self.y_old, Q)

    return Recorder, log


@contextlib.contextmanager
def _sequential_rk_step():
    rk = _scipy_private()
    saved = rk.rk_step
    rk.rk_step = _rk_step_sequential
    try:
        yield
    finally:
        rk.rk_step = saved


@functools.lru_cache(maxsize=None)
def _solve(theta, rtol, atol, t_span, u_init, sensitivity, sequential):
    method, log = recorder(sequential)
    with (_sequential_rk_step() if sequential else contextlib.nullcontext()):
        sol = ol.solve(np.array(theta), t_span, u_init, rtol, atol, sensitivity, method=method)
    assert sol.status == 0
    sol.error_norms = np.array(log)
    sol.margin = float(np.abs(sol.error_norms - 1.0).min())
    sol.accepted = len(sol.t) - 1
    sol.rejected = len(log) - sol.accepted
    return sol


def solution(theta, rtol=lv.RTOL, atol=lv.ATOL, t_span=lv.T_SPAN, u_init=lv.U_INIT, sensitivity=True,
             sequential=False):
    """scipy's ``sol`` (``sol.t``, ``sol.y``, ``sol.sol``) at one parameter point, with the recorder's
    ``error_norms``, ``margin``, ``accepted`` and ``rejected``.  Solved once per argument set; shared."""
    return _solve(tuple(float(x) for x in theta), float(rtol), float(atol), tuple(float(x) for x in t_span),
                  tuple(float(x) for x in u_init), bool(sensitivity), bool(sequential))


def solve(theta, s, sensitivity=True, sequential=False):
    """``solution`` with the solver settings of input set ``s``."""
    return solution(theta, sensitivity=sensitivity, sequential=sequential, **s.solver)


_values = {}


def _shared(kind, s, sequential, make):
    key = (kind, s.name, sequential)
    if key not in _values:
        v = make()
        v.setflags(write=False)
        _values[key] = v
    return _values[key]


def gradient(s, sequential=False):
    """(n, 4): scipy's grad_log_posterior of every point of set ``s`` (computed once, read-only)."""
    return _shared('gradient', s, sequential, lambda: _gradient(s, sequential))


def log_density(s, sequential=False):
    """(n,): scipy's log_target_density at log(theta) of every point of set ``s`` (computed once, read-only)."""
    return _shared('log_density', s, sequential, lambda: _log_density(s, sequential))


def _gradient(s, sequential):
    d = s.data
    return np.stack([ol.grad_from_solution(solve(th, s, True, sequential), th, d.t, d.y, d.cov) for th in s.theta])


def _log_density(s, sequential):
    d = s.data
    return np.array([ol.log_density_from_solution(solve(np.exp(lt), s, False, sequential), lt, d.t, d.y, d.cov)
                     for lt in np.log(s.theta)])


def grad_error(got, want):
    """max|got - want| / max|want| per row."""
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def measure(s):
    """(delta gradient, delta log density without the set's LOG_DENSITY_EXCEPTIONS, smallest margin,
    step-time drift / span, state drift) of set ``s``, and whether the sequential variant took scipy's accepted / rejected counts at every point."""
    dg = float(grad_error(gradient(s, True), gradient(s)).max())
    dl = 0.0
    if s.log_density:
        w = log_density(s)
        dl = np.abs(log_density(s, True) - w) / np.abs(w)
        dl[list(LOG_DENSITY_EXCEPTIONS.get(s.name, {}))] = 0.0
        dl = float(dl.max())
    margin, dt, dy, same = np.inf, 0.0, 0.0, True
    span = s.data.t_span[1] - s.data.t_span[0]
    for sens, thetas in ((True, s.theta), (False, np.exp(np.log(s.theta)))):
        for th in thetas:
            a, b = solve(th, s, sens), solve(th, s, sens, True)
            margin = min(margin, a.margin, b.margin)
            if (a.accepted, a.rejected) != (b.accepted, b.rejected):
                same = False
                continue
            if sens:
                dt = max(dt, float(np.abs(a.t - b.t).max() / span))
                dy = max(dy, float((np.abs(a.y - b.y).max(axis=1) / np.abs(a.y).max(axis=1)).max()))
    return (dg, dl, margin, dt, dy), same


def records(sol, t_obs):
    """The step table scipy's solution implies on the observation times ``t_obs``: (segment index j,
    k_begin, k_end) of every segment (t_j, t_j+1] that holds an observation, in order; the first segment
    also takes the times up to t_0, the last those after t_n (OdeSolution extrapolates there)."""
    ends = np.searchsorted(t_obs, sol.t[1:], 'right')
    ends[-1] = len(t_obs)
    begins = np.concatenate([[0], ends[:-1]])
    return [(j, int(b), int(e)) for j, (b, e) in enumerate(zip(begins, ends)) if e > b]


def record_counts(s):
    """Recorded steps per point of ``s``: more than 64 overflow the step table."""
    return np.array([len(records(solve(th, s), np.asarray(s.data.t))) for th in s.theta])


def boundary_distance(s):
    """Smallest |t_obs - step boundary| / (t1 - t0) over the points of ``s`` (interior boundaries of the
    sensitivity system: the step table's)."""
    t = np.asarray(s.data.t)
    span = s.data.t_span[1] - s.data.t_span[0]
    best = np.inf
    for th in s.theta:
        b = solve(th, s).t[1:-1]
        if b.size:
            best = min(best, float(np.abs(t[:, None] - b[None, :]).min() / span))
    return best
