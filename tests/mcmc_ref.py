"""Host restatement of the random-walk Metropolis sampler (csrc/lv_mcmc.hip, lotka_volterra.rw_sample) --
TEST INFRASTRUCTURE ONLY: a Python Philox4x64-10 (checked against np.random.Philox by
tests/test_lv_mcmc_cpu.py), the sampler's mapping from raw Philox values to noise, and the Metropolis loop
over oracle.lv_numpy.log_target_density (scipy's solve_ivp).  Every decision of the loop also returns its
relative margin |(lp_new - lp) - log_u| / max(|lp_new|, |lp|): a GPU chain can only be compared row for
row with this one where the margins are far above the 1e-8 the LV values are held to against scipy."""
from __future__ import annotations

import functools

import numpy as np

MASK = (1 << 64) - 1
M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B

# code/src/lotka_volterra.py: theta_inits
THETA_INITS = np.array([[0.55, 1., 0.8, 0.8], [1.5, 1., 0.8, 0.8], [1.3, 1.33, 0.5, 0.8], [0.55, 3., 3., 0.8],
                        [0.55, 1., 1.5, 1.5]])
THETA = np.array([0.67, 1.33, 1., 1.])
STEP = 0.0025


def philox4x64_10(counter, key):
    """One Philox4x64-10 block: counter (4 words), key (2 words) -> 4 words."""
    c = [int(v) & MASK for v in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k0, p1 & MASK, (p0 >> 64) ^ c[3] ^ k1, p0 & MASK]
    return c


def raw(seed, chain, t):
    """The eight raw values of step t >= 1 of chain `chain`: the blocks with counter word 0 = 2t - 1 and 2t
    (np.random.Philox(key=[seed, chain], counter=[0, 0, 0, 0]).random_raw(8 t)[8 (t - 1):])."""
    return philox4x64_10([2 * t - 1, 0, 0, 0], [seed, chain]) + philox4x64_10([2 * t, 0, 0, 0], [seed, chain])


def noise_from_raw(r):
    """(z (4,), log_u) from r0 .. r7."""
    u = np.array([((v >> 11) + 1) for v in r[:4]], dtype=np.float64) * 2.0 ** -53
    z = np.empty(4)
    for k in (0, 2):
        rad, ang = np.sqrt(-2.0 * np.log(u[k])), 2 * np.pi * u[k + 1]
        z[k], z[k + 1] = rad * np.cos(ang), rad * np.sin(ang)
    with np.errstate(divide='ignore'):
        log_u = np.log(np.float64(r[4] >> 11) * 2.0 ** -53)
    return z, float(log_u)


def device_noise(seed, chains, steps, first_chain=0, first_step=1):
    """z (chains, steps, 4), log_u (chains, steps) of the device generator."""
    z = np.empty((chains, steps, 4))
    log_u = np.empty((chains, steps))
    for c in range(chains):
        for k in range(steps):
            z[c, k], log_u[c, k] = noise_from_raw(raw(seed, first_chain + c, first_step + k))
    return z, log_u


def metropolis(x0, z, log_u, log_density, step=STEP):
    """One chain: rows (steps + 1, 4), log_p (steps + 1), accepted, margins (steps) -- proposal
    x + step * z[k], accepted exactly when log_u[k] < lp_new - lp."""
    steps = z.shape[0]
    rows = np.empty((steps + 1, 4))
    log_p = np.empty(steps + 1)
    margins = np.empty(steps)
    x = np.array(x0, dtype=np.float64)
    lp = log_density(x)
    rows[0], log_p[0] = x, lp
    accepted = 0
    for k in range(steps):
        p = x + step * z[k]
        lp_new = log_density(p)
        margins[k] = abs((lp_new - lp) - log_u[k]) / max(abs(lp_new), abs(lp))
        if log_u[k] < lp_new - lp:
            x, lp = p, lp_new
            accepted += 1
        rows[k + 1], log_p[k + 1] = x, lp
    return rows, log_p, accepted, margins


@functools.lru_cache(maxsize=None)
def fixed_input():
    """The fixed input of the main parity test: 10 chains of 41 rows; the starts are the log of the
    reference's five theta_inits, then five copies of log(THETA); chains c and c + 5 both take their noise
    from default_rng(100 + c): z = standard_normal((40, 4)), then log_u = log(random(40))."""
    x0 = np.concatenate([np.log(THETA_INITS), np.tile(np.log(THETA), (5, 1))])
    z = np.empty((10, 40, 4))
    log_u = np.empty((10, 40))
    for c in range(5):
        rng = np.random.default_rng(100 + c)
        z[c] = z[c + 5] = rng.standard_normal((40, 4))
        log_u[c] = log_u[c + 5] = np.log(rng.random(40))
    for a in (x0, z, log_u):
        a.setflags(write=False)
    return x0, z, log_u


@functools.lru_cache(maxsize=None)
def fixed_reference():
    """The oracle's chains on fixed_input(): samples (10, 41, 4), log_p (10, 41), accepted (10,),
    margins (10, 40).  Computed once per process (~400 scipy integrations), read-only."""
    from oracle import lv_numpy as ol
    from stein_thinning import lotka_volterra as lv
    data = lv.reference_data()
    x0, z, log_u = fixed_input()

    def dens(x):
        return ol.log_target_density(x, data.t, data.y, data.cov)
    out = [metropolis(x0[c], z[c], log_u[c], dens) for c in range(10)]
    res = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out]),
           np.stack([o[3] for o in out]))
    for a in res:
        a.setflags(write=False)
    return res


FAIL_STEP, FAIL_SEED, FAIL_K = 0.3, 4, 1


@functools.lru_cache(maxsize=None)
def failing_input():
    """The input of the failed-proposal tests: 4 chains of 21 rows from log(THETA), z = default_rng(FAIL_SEED)
    .standard_normal((4, 20, 4)), log_u = -inf (a proposal that has a density is accepted, so a repeated row
    marks a failure), proposal step FAIL_STEP, to be run with max_steps = FAIL_K more than the start row's
    accepted-step count (23).  Chosen on the host among seeds 1 .. 5 and k = 0 .. 4 (tests/test_lv_mcmc_cpu.py
    holds the conditions): 25 of the 80 proposals need more steps."""
    x0 = np.tile(np.log(THETA), (4, 1))
    z = np.random.default_rng(FAIL_SEED).standard_normal((4, 20, 4))
    log_u = np.full((4, 20), -np.inf)
    for a in (x0, z, log_u):
        a.setflags(write=False)
    return x0, z, log_u
