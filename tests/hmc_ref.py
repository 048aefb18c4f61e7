"""Host restatement of the HMC sampler (csrc/lv_mcmc.hip: lv_hmc_wave_kernel, lotka_volterra.hmc_sample) -- TEST
INFRASTRUCTURE ONLY.  NumPy over tests/mala_ref.evaluate (scipy's 10-state solution: log density and gradient with
respect to log theta from ONE integration per point), in the kernel's order of operations:
    hk(q) = 0.5 * clip(eps * g(q), -c, c);  r' = r + hk(q);  q' = q + eps * r';  r'' = r' + hk(q')     (one stage)
    accept exactly when log_u < (lp(q^L) - lp(x)) + (K(r^0) - K(r^L)),  K(r) = 0.5 * (((r0 r0 + r1 r1) + r2 r2) + r3 r3)
Every step of the Metropolis loop also returns its relative margin |a - log_u| / max(|lp_new|, |lp|)."""
from __future__ import annotations

import functools

import numpy as np

from oracle import lv_numpy as ol
from tests import mala_ref as MR

THETA = MR.THETA
evaluate = MR.evaluate
reference_data = MR.reference_data


def constants(step_size, kick_cap):
    """(eps (4,), c (4,)) as hmc_sample hands them over."""
    eps = np.full(4, float(step_size)) if np.ndim(step_size) == 0 else np.asarray(step_size, dtype=np.float64)
    return eps, np.full(4, float(kick_cap))


def clip(v, c):
    return np.minimum(np.maximum(v, -c), c)            # (a NaN stays a NaN, as in the kernel)


def half_kick(g, eps, c):
    return 0.5 * clip(eps * g, c)


def kinetic(r):
    s = 0.0
    for j in range(4):
        s += r[j] * r[j]
    return 0.5 * s


def trajectory(q, g, r, eps, c, n_leapfrog, ev):
    """n_leapfrog stages from (q, r) with g = g(q).  Returns q^L, lp(q^L), g(q^L), r^L and, per stage, the point
    q^l, the accepted RK45 steps of its evaluation (0 when it ran none) and whether each kick component that led
    to it was clipped."""
    q, g, r = (np.array(a, dtype=np.float64) for a in (q, g, r))
    lp = np.nan
    points, counts, clipped = [], [], []
    for _ in range(n_leapfrog):
        with np.errstate(invalid='ignore'):
            clipped.append(np.abs(eps * g) > c)
            rp = r + half_kick(g, eps, c)
            q = q + eps * rp
            lp, g, n = ev(q)
            r = rp + half_kick(g, eps, c)
        points.append(q)
        counts.append(n)
    return q, lp, g, r, np.array(points), np.array(counts), np.array(clipped)


def decide(lp, lp_new, k0, k1, log_u):
    """(accept, margin) of one step from the densities at both ends and the kinetic energies K(r^0), K(r^L)."""
    if not np.isfinite(lp_new):
        return False, np.inf
    with np.errstate(invalid='ignore'):
        a = (lp_new - lp) + (k0 - k1)
    return bool(log_u < a), abs(a - log_u) / max(abs(lp_new), abs(lp))


def chain(x0, z, log_u, step_size, kick_cap, n_leapfrog, ev):
    """One chain: rows (steps + 1, 4), log_p, grad (steps + 1, 4), accepted, n_failed, margins (steps), clipped
    (steps, L, 4), counts (steps, L): accepted RK45 steps of every stage."""
    eps, c = constants(step_size, kick_cap)
    steps = z.shape[0]
    rows, grad, log_p = np.empty((steps + 1, 4)), np.empty((steps + 1, 4)), np.empty(steps + 1)
    margins = np.empty(steps)
    clipped = np.empty((steps, n_leapfrog, 4), dtype=bool)
    counts = np.empty((steps, n_leapfrog), dtype=np.int64)
    x = np.array(x0, dtype=np.float64)
    lp, g, _ = ev(x)
    rows[0], log_p[0], grad[0] = x, lp, g
    accepted = failed = 0
    for k in range(steps):
        q, lp_new, g_new, r, _, counts[k], clipped[k] = trajectory(x, g, z[k], eps, c, n_leapfrog, ev)
        if not np.isfinite(lp_new):
            failed += 1                                     # once per trajectory
        ok, margins[k] = decide(lp, lp_new, kinetic(z[k]), kinetic(r), log_u[k])
        if ok:
            x, lp, g = q, lp_new, g_new
            accepted += 1
        rows[k + 1], log_p[k + 1], grad[k + 1] = x, lp, g
    return rows, log_p, grad, accepted, failed, margins, clipped, counts


# the fixed input: chosen on the host (tests/test_lv_hmc_cpu.py holds the conditions)
FIXED_CHAINS, FIXED_ROWS, FIXED_L = 5, 13, 3
FIXED_SEED, FIXED_OFFSET = 2027, 0.01
FIXED_EPS, FIXED_CAP = 0.002, 0.5


@functools.lru_cache(maxsize=None)
def fixed_input():
    """5 chains of 13 rows started at log(THETA) + FIXED_OFFSET * N(0, I) (default_rng(FIXED_SEED)); chain c takes
    z = default_rng(400 + c).standard_normal((12, 4)), then log_u = log(random(12)).  Returns x0, z, log_u; the
    step size is FIXED_EPS, the kick cap FIXED_CAP and the trajectory length FIXED_L."""
    x0 = np.log(THETA) + FIXED_OFFSET * np.random.default_rng(FIXED_SEED).standard_normal((FIXED_CHAINS, 4))
    z = np.empty((FIXED_CHAINS, FIXED_ROWS - 1, 4))
    log_u = np.empty((FIXED_CHAINS, FIXED_ROWS - 1))
    for c in range(FIXED_CHAINS):
        rng = np.random.default_rng(400 + c)
        z[c] = rng.standard_normal((FIXED_ROWS - 1, 4))
        log_u[c] = np.log(rng.random(FIXED_ROWS - 1))
    for a in (x0, z, log_u):
        a.setflags(write=False)
    return x0, z, log_u


NAMES = ('samples', 'log_p', 'grad', 'accepted', 'n_failed', 'margins', 'clipped', 'counts')


def _stack(out):
    res = {name: np.stack([np.asarray(o[q]) for o in out]) for q, name in enumerate(NAMES)}
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def fixed_reference():
    """The host chains on fixed_input(): dict of samples (5, 13, 4), log_p (5, 13), grad (5, 13, 4), accepted (5,),
    n_failed (5,), margins (5, 12), clipped (5, 12, 3, 4), counts (5, 12, 3).  Computed once per process (~190
    scipy integrations)."""
    data = reference_data()
    x0, z, log_u = fixed_input()
    return _stack([chain(x0[c], z[c], log_u[c], FIXED_EPS, FIXED_CAP, FIXED_L, lambda x: evaluate(x, data))
                   for c in range(FIXED_CHAINS)])


# the input of the failed-trajectory tests (tests/mala_ref.failing_input()'s scheme)
FAIL_EPS, FAIL_CAP, FAIL_SEED, FAIL_K, FAIL_L = 0.15, 1.0, 4, 1, 2
FAIL_CHAINS, FAIL_ROWS = 4, 13


@functools.lru_cache(maxsize=None)
def failing_input():
    """4 chains of 13 rows from log(THETA), z = default_rng(FAIL_SEED).standard_normal((4, 12, 4)), log_u = -inf (a
    trajectory that has a density and a finite end momentum is accepted, so a repeated row marks a failure), step
    size FAIL_EPS with kick cap FAIL_CAP and FAIL_L stages, to be run with max_steps = FAIL_K more than the
    accepted-step count of the 10-state integration at THETA (failing_max_steps())."""
    x0 = np.tile(np.log(THETA), (FAIL_CHAINS, 1))
    z = np.random.default_rng(FAIL_SEED).standard_normal((FAIL_CHAINS, FAIL_ROWS - 1, 4))
    log_u = np.full((FAIL_CHAINS, FAIL_ROWS - 1), -np.inf)
    for a in (x0, z, log_u):
        a.setflags(write=False)
    return x0, z, log_u


@functools.lru_cache(maxsize=None)
def failing_max_steps():
    return ol.n_steps(THETA, sensitivity=True) + FAIL_K
