"""Host restatement of the HMC sampler with a per-chain step size, a dense metric and dual averaging (csrc/lv_mcmc.hip:
lv_hmc_metric_wave_kernel, lotka_volterra.hmc_metric_sample / hmc_warmup) -- TEST INFRASTRUCTURE ONLY.  NumPy, batched
over chains (leading axis), in the kernel's order of operations:
    f_j = Lam_jj g_j + sum_{k > j} Lam_kj g_k;  hk = 0.5 * clip(eps * f, -c, c);  r' = r + hk(q)
    v_j = sum_{k <= j} Lam_jk r'_k (from the k = 0 term);  q' = q + eps * v;  r'' = r' + hk(q')          (one stage)
    a = (lp(q^L) - lp(x)) + (K(r^0) - K(r^L));  accept when log_u < a;  alpha = min(1, exp(a)), 0 for a NaN a
    m += 1; eta = 1 / (m + 10); sbar = (1 - eta) sbar + eta (delta - alpha); ell = mu - (sbar sqrt(m)) / 0.05;
    w = m ** -0.75; xbar = (1 - w) xbar + w ell; eps = exp(ell)                                   (dual averaging)
``ev(q)`` evaluates a batch of points: (lp (chains,), g (chains, 4)).

Everything here gives the same bits on every CPU: only IEEE element-wise operations (+, -, *, /, sqrt, comparisons) in a
written order, and exp / pow / log through the C library one value at a time (``elementwise``) -- never NumPy's own exp,
power or log, whose SIMD variants differ by an ulp between CPUs, and no BLAS or LAPACK call, whose summation order
depends on the CPU.  The chains are chaotic, so one ulp anywhere gives another realisation."""
from __future__ import annotations

import math

import numpy as np

GAMMA, T0, KAPPA = 0.05, 10.0, 0.75


def elementwise(fn, a, *args):
    """fn (a math-module function) of every element of a, one call per value; an overflow gives inf."""
    a = np.asarray(a, dtype=np.float64)

    def one(v):
        try:
            return fn(v, *args)
        except OverflowError:
            return math.inf
    return np.array([one(float(v)) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def clip(v, c):
    return np.minimum(np.maximum(v, -c), c)            # (a NaN stays a NaN, as in the kernel)


def half_kick(g, eps, lam, c):
    """hk (chains, 4) from g (chains, 4), eps (chains,), lam (chains, 4, 4), c (4,)."""
    hk = np.empty_like(g)
    for j in range(4):
        f = lam[:, j, j] * g[:, j]
        for k in range(j + 1, 4):
            f = f + lam[:, k, j] * g[:, k]
        hk[:, j] = 0.5 * clip(eps * f, c[j])
    return hk


def velocity(rp, lam):
    v = np.empty_like(rp)
    for j in range(4):
        s = lam[:, j, 0] * rp[:, 0]
        for k in range(1, j + 1):
            s = s + lam[:, j, k] * rp[:, k]
        v[:, j] = s
    return v


def kinetic(r):
    s = np.zeros(r.shape[0])
    for j in range(4):
        s = s + r[:, j] * r[:, j]
    return 0.5 * s


def trajectory(q, g, r, eps, lam, c, n_leapfrog, ev):
    """n_leapfrog stages from (q, r) with g = g(q), batched.  Returns q^L, lp(q^L), g(q^L), r^L."""
    q, g, r = (np.array(a, dtype=np.float64) for a in (q, g, r))
    lp = np.full(q.shape[0], np.nan)
    with np.errstate(invalid='ignore', over='ignore'):
        for _ in range(n_leapfrog):
            rp = r + half_kick(g, eps, lam, c)
            q = q + eps[:, None] * velocity(rp, lam)
            lp, g = ev(q)
            r = rp + half_kick(g, eps, lam, c)
    return q, lp, g, r


def accept_stat(a):
    """alpha = min(1, exp(a)); 0 where a is NaN."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 0.0, np.minimum(1.0, elementwise(math.exp, np.where(np.isnan(a), 0.0, a))))


def da_update(da, alpha, delta):
    """One dual-averaging update of the state da (chains, 5) = eps, m, sbar, xbar, mu with the step's alpha."""
    _, m, sbar, xbar, mu = (da[:, q] for q in range(5))
    m = m + 1.0
    eta = 1.0 / (m + T0)
    sbar = (1.0 - eta) * sbar + eta * (delta - alpha)
    ell = mu - (sbar * np.sqrt(m)) / GAMMA
    w = elementwise(math.pow, m, -KAPPA)
    xbar = (1.0 - w) * xbar + w * ell
    eps = elementwise(math.exp, ell)
    return np.stack([eps, m, sbar, xbar, mu], axis=1)


class Chains:
    """The kernel's Metropolis loop on the host for a batch of chains: state x, lp, g; ``run`` is a segment runner
    for lotka_volterra.hmc_warmup_schedule (adapt) and also runs fixed-eps steps."""

    def __init__(self, x0, ev, noise, n_leapfrog, cap=np.inf, delta=0.8):
        """noise(t) -> (z (chains, 4), log_u (chains,)) for global step t = 1, 2, ..."""
        self.x = np.array(x0, dtype=np.float64)
        self.ev, self.noise, self.L, self.c, self.delta = ev, noise, n_leapfrog, np.full(4, float(cap)), delta
        self.lp, self.g = ev(self.x)
        self.accepted = np.zeros(self.x.shape[0], dtype=np.int64)
        self.alphas, self.eps_used = [], []

    def step(self, t, eps, lam):
        z, log_u = self.noise(t)
        q, lp_new, g_new, r = trajectory(self.x, self.g, z, eps, lam, self.c, self.L, self.ev)
        with np.errstate(invalid='ignore'):
            a = (lp_new - self.lp) + (kinetic(z) - kinetic(r))
            ok = log_u < a
        self.x = np.where(ok[:, None], q, self.x)
        self.g = np.where(ok[:, None], g_new, self.g)
        self.lp = np.where(ok, lp_new, self.lp)
        self.accepted += ok
        alpha = accept_stat(a)
        self.alphas.append(alpha)
        self.eps_used.append(np.array(eps))
        return alpha

    def run(self, start, stop, lam, da):
        """Steps [start, stop) (global steps start + 1 .. stop) with adaptation: (rows, da after them)."""
        da = np.array(da, dtype=np.float64)
        rows = np.empty((self.x.shape[0], stop - start, 4))
        for k in range(start, stop):
            alpha = self.step(k + 1, da[:, 0], lam)
            da = da_update(da, alpha, self.delta)
            rows[:, k - start] = self.x
        return rows, da


def gaussian(precision):
    """ev for the target N(0, precision^-1): lp = -0.5 x^T P x, g = -P x, every sum from its j = 0 term, j ascending."""
    def ev(q):
        px = np.empty_like(q)
        for j in range(4):
            s = precision[j, 0] * q[:, 0]
            for k in range(1, 4):
                s = s + precision[j, k] * q[:, k]
            px[:, j] = s
        quad = q[:, 0] * px[:, 0]
        for j in range(1, 4):
            quad = quad + q[:, j] * px[:, j]
        return -0.5 * quad, -px
    return ev


def window_metric(rows):
    """lotka_volterra.hmc_window_metric's definition for rows (chains, n, 4) in a written order: the mean and the
    covariance summed over the rows in order, a hand-written Cholesky factorisation -- the same bits on every CPU."""
    rows = np.asarray(rows, dtype=np.float64)
    C, n, _ = rows.shape
    mean = np.zeros((C, 4))
    for t in range(n):
        mean = mean + rows[:, t]
    mean = mean / n
    cov = np.zeros((C, 4, 4))
    for t in range(n):
        d = rows[:, t] - mean
        cov = cov + d[:, :, None] * d[:, None, :]
    sigma = (n / (n + 5.0)) * (cov / (n - 1)) + (1e-3 * 5.0 / (n + 5.0)) * np.eye(4)
    lam = np.zeros((C, 4, 4))
    for j in range(4):
        s = sigma[:, j, j]
        for k in range(j):
            s = s - lam[:, j, k] * lam[:, j, k]
        lam[:, j, j] = np.sqrt(s)
        for i in range(j + 1, 4):
            s = sigma[:, i, j]
            for k in range(j):
                s = s - lam[:, i, k] * lam[:, j, k]
            lam[:, i, j] = s / lam[:, j, j]
    return lam


def regularised_cov(rows):
    """Stan's regularised covariance of rows (n, 4) in NumPy: n / (n + 5) cov + 1e-3 * 5 / (n + 5) I."""
    n = rows.shape[0]
    return n / (n + 5.0) * np.cov(rows, rowvar=False) + 1e-3 * 5.0 / (n + 5.0) * np.eye(4)
