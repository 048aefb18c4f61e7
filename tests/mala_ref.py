"""Host restatement of the MALA sampler (csrc/lv_mcmc.hip: lv_mala_wave_kernel, lotka_volterra.mala_sample) --
TEST INFRASTRUCTURE ONLY.  NumPy over scipy: ONE oracle.lv_numpy.solve(theta, sensitivity=True) per point gives
the log density (from the first two states of the 10-state solution: its step sequence is not the 2-state one
of oracle.lv_numpy.log_target_density, so this, not log_target_density, is the oracle of the sampler's log_p)
and the gradient with respect to log theta (grad_from_solution times theta).  Every step of the Metropolis loop
also returns its relative margin |a - log_u| / max(|lp_new|, |lp|), a = (lp_new - lp) + (qf - qr)."""
from __future__ import annotations

import functools

import numpy as np
import scipy.stats as stats

from oracle import lv_numpy as ol

THETA = np.array([0.67, 1.33, 1., 1.])


def evaluate(x, data, rtol=1e-3, atol=1e-6, max_steps=None):
    """(lp, g (4,), accepted RK45 steps) at x = log theta; lp and g are NaN when theta is out of range or the
    10-state integration takes more than max_steps accepted steps."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over='ignore', under='ignore'):
        theta = np.exp(x)
    if not (np.all(np.isfinite(theta)) and np.all(theta != 0)):
        return np.nan, np.full(4, np.nan), 0
    sol = ol.solve(theta, data.t_span, data.u_init, rtol, atol, sensitivity=True)
    n = len(sol.t) - 1
    if max_steps is not None and n > max_steps:
        return np.nan, np.full(4, np.nan), n
    # oracle.lv_numpy.log_density_from_solution's two lines, on the first two states
    u = sol.sol(data.t).T[:, :2]
    log_likelihood = np.sum(stats.multivariate_normal.logpdf(data.y - u, mean=[0, 0], cov=data.cov))
    lp = log_likelihood + np.sum(stats.norm.logpdf(x))
    g = ol.grad_from_solution(sol, theta, data.t, data.y, data.cov) * theta
    return float(lp), g, n


def constants(step_size, drift_cap):
    """(eps, h, w, c) as mala_sample computes them on the host."""
    eps = np.full(4, float(step_size)) if np.ndim(step_size) == 0 else np.asarray(step_size, dtype=np.float64)
    return eps, 0.5 * eps * eps, 0.5 / (eps * eps), float(drift_cap) * eps


def drift(g, h, c):
    return np.minimum(np.maximum(h * g, -c), c)


def quad(w, r):
    q = 0.0
    for j in range(4):
        q += w[j] * r[j] * r[j]
    return q


def decide(x, lp, d, p, lp_new, g_new, log_u, h, w, c):
    """(accept, margin) of one step: x, lp and the drift d = d(x) that formed p; lp_new, g_new at p."""
    rf = (p - x) - d
    rr = (x - p) - drift(g_new, h, c)
    a = (lp_new - lp) + (quad(w, rf) - quad(w, rr))
    if not np.isfinite(lp_new):
        return False, np.inf
    return bool(log_u < a), abs(a - log_u) / max(abs(lp_new), abs(lp))


def chain(x0, z, log_u, step_size, drift_cap, ev):
    """One chain: rows (steps + 1, 4), log_p, grad (steps + 1, 4), accepted, n_failed, margins (steps),
    clipped (steps, 4) -- whether the drift component of the step's proposal was clipped."""
    eps, h, w, c = constants(step_size, drift_cap)
    steps = z.shape[0]
    rows, grad, log_p = np.empty((steps + 1, 4)), np.empty((steps + 1, 4)), np.empty(steps + 1)
    margins, clipped = np.empty(steps), np.empty((steps, 4), dtype=bool)
    x = np.array(x0, dtype=np.float64)
    lp, g, _ = ev(x)
    rows[0], log_p[0], grad[0] = x, lp, g
    accepted = failed = 0
    for k in range(steps):
        d = drift(g, h, c)
        clipped[k] = np.abs(h * g) > c
        p = (x + d) + eps * z[k]
        lp_new, g_new, _ = ev(p)
        if not np.isfinite(lp_new):
            failed += 1
        ok, margins[k] = decide(x, lp, d, p, lp_new, g_new, log_u[k], h, w, c)
        if ok:
            x, lp, g = p, lp_new, g_new
            accepted += 1
        rows[k + 1], log_p[k + 1], grad[k + 1] = x, lp, g
    return rows, log_p, grad, accepted, failed, margins, clipped


# the fixed input: chosen on the host (tests/test_lv_mala_cpu.py holds the conditions)
FIXED_CHAINS, FIXED_ROWS = 5, 41
FIXED_SEED, FIXED_OFFSET = 2026, 0.01
FIXED_EPS, FIXED_CAP = 0.003, 1.0


@functools.lru_cache(maxsize=None)
def fixed_input():
    """5 chains of 41 rows started at log(THETA) + FIXED_OFFSET * N(0, I) (default_rng(FIXED_SEED)); chain c takes
    z = default_rng(200 + c).standard_normal((40, 4)), then log_u = log(random(40)).  Returns x0, z, log_u; the
    step size is FIXED_EPS and the drift cap FIXED_CAP.  The reference's far theta_inits are NOT part of it: with
    large drifts scipy's integrations at the proposals crawl."""
    x0 = np.log(THETA) + FIXED_OFFSET * np.random.default_rng(FIXED_SEED).standard_normal((FIXED_CHAINS, 4))
    z = np.empty((FIXED_CHAINS, FIXED_ROWS - 1, 4))
    log_u = np.empty((FIXED_CHAINS, FIXED_ROWS - 1))
    for c in range(FIXED_CHAINS):
        rng = np.random.default_rng(200 + c)
        z[c] = rng.standard_normal((FIXED_ROWS - 1, 4))
        log_u[c] = np.log(rng.random(FIXED_ROWS - 1))
    for a in (x0, z, log_u):
        a.setflags(write=False)
    return x0, z, log_u


def reference_data():
    from stein_thinning import lotka_volterra as lv
    return lv.reference_data()


@functools.lru_cache(maxsize=None)
def fixed_reference():
    """The host chains on fixed_input(): dict of samples (5, 41, 4), log_p (5, 41), grad (5, 41, 4), accepted (5,),
    n_failed (5,), margins (5, 40), clipped (5, 40, 4).  Computed once per process (~200 scipy integrations)."""
    data = reference_data()
    x0, z, log_u = fixed_input()
    out = [chain(x0[c], z[c], log_u[c], FIXED_EPS, FIXED_CAP, lambda x: evaluate(x, data))
           for c in range(FIXED_CHAINS)]
    names = ('samples', 'log_p', 'grad', 'accepted', 'n_failed', 'margins', 'clipped')
    res = {name: np.stack([np.asarray(o[q]) for o in out]) for q, name in enumerate(names)}
    for a in res.values():
        a.setflags(write=False)
    return res


# the input of the failed-proposal tests (tests/mcmc_ref.failing_input()'s scheme)
FAIL_EPS, FAIL_CAP, FAIL_SEED, FAIL_K = 0.3, 1.0, 4, 1


@functools.lru_cache(maxsize=None)
def failing_input():
    """4 chains of 21 rows from log(THETA), z = default_rng(FAIL_SEED).standard_normal((4, 20, 4)), log_u = -inf (a
    proposal that has a density is accepted unless its reverse drift is NaN, so a repeated row marks a failure),
    step size FAIL_EPS with drift cap FAIL_CAP, to be run with max_steps = FAIL_K more than the accepted-step
    count of the 10-state integration at THETA (failing_max_steps())."""
    x0 = np.tile(np.log(THETA), (4, 1))
    z = np.random.default_rng(FAIL_SEED).standard_normal((4, 20, 4))
    log_u = np.full((4, 20), -np.inf)
    for a in (x0, z, log_u):
        a.setflags(write=False)
    return x0, z, log_u


@functools.lru_cache(maxsize=None)
def failing_max_steps():
    return ol.n_steps(THETA, sensitivity=True) + FAIL_K
