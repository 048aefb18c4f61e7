"""Host restatement of the no-U-turn sampler (csrc/lv_mcmc.hip: lv_nuts_wave_kernel, lotka_volterra.nuts_sample;
DESIGN.md section 22) -- TEST INFRASTRUCTURE ONLY.  One chain, one step at a time, in the kernel's order of operations:
    K0 = K(z); both ends (x, z, g); rho = z; W = 0; the proposal is the row
    doubling j = 0 .. max_depth - 1: direction v and log u_T from the draws of the doubling's first stage; 2^j leaves
    from the end on side v; leaf n = (q, r):  a_n = (lp(q) - lp) + (K0 - K(r))
        sum_alpha += min(1, exp(a_n)) (0 for a NaN);  a NaN a_n or a_n < -1000: divergent, stop
        W' = a_0, then W' = lse(W', a_n);  leaf n > 0 becomes the sub-tree's proposal when log u_l < a_n - W'
        rho' = r_0, then rho' = rho' + r_n;  even n: checkpoint (r_n, rho') in slot popcount(n >> 1)
        odd n: every aligned block of 2^k leaves that ends at n, smallest first: rho_b = (rho' - rho'_a) + r_a;
               it turns when NOT (dot(rho_b, r_a) > 0 AND dot(rho_b, r_n) > 0): stop
    complete sub-tree: its proposal replaces the tree's when log u_T < W' - W; W = lse(W, W'); rho = rho + rho'; the
    end on side v is the last leaf; stop when the whole tree turns
The rules of tests/hmc_adapt_ref.py hold: IEEE element-wise operations in a written order, exp / log / log1p through
the C library one value at a time, no BLAS.  ``stage(q, g, r, v)`` -> (q', lp', g', r') is one leapfrog stage in direction
v: ``host_stage`` (hmc_adapt_ref.trajectory with an ``ev``) or a device one-stage call.  ``step_gen`` is the same step as
a generator that yields the stage requests, so that a test can drive several chains in lock-step."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from tests import hmc_adapt_ref as A

MASK = (1 << 64) - 1
M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def philox4x64_10(c0, c1, k0, k1):
    """One Philox4x64-10 block for counter (c0, c1, 0, 0) and key (k0, k1), in Python integers."""
    c = [c0 & MASK, c1 & MASK, 0, 0]
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k0, p1 & MASK, (p0 >> 64) ^ c[3] ^ k1, p0 & MASK]
    return c


def _log(v):
    return math.log(v) if v > 0.0 else -math.inf


def tree_draws(seed, chain, t):
    """draws(l) -> (log u_l, v, log u_T) of stage l = 1, 2, ... of step t: the block with counter (t, l, 0, 0)."""
    def draws(ell):
        r = philox4x64_10(t, ell, seed, chain)
        return _log((r[0] >> 11) * 2.0 ** -53), (1 if r[1] >> 63 == 0 else -1), _log((r[2] >> 11) * 2.0 ** -53)
    return draws


def lse(p, s):
    return max(p, s) + math.log1p(math.exp(-abs(p - s)))


def dot(a, b):
    s = a[0] * b[0]
    for j in range(1, 4):
        s = s + a[j] * b[j]
    return s


def kinetic(r):
    s = 0.0
    for j in range(4):
        s = s + r[j] * r[j]
    return 0.5 * s


def turns(rho, ra, rb):
    return not (dot(rho, ra) > 0.0 and dot(rho, rb) > 0.0)


def brute_turns(leaves):
    """The U-turn test of a block from its stored leaf momenta: rho summed directly, in leaf order."""
    rho = np.array(leaves[0], dtype=np.float64)
    for r in leaves[1:]:
        rho = rho + r
    return turns(rho, leaves[0], leaves[-1])


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


@dataclass
class Step:
    x: np.ndarray                     # the new row
    lp: float
    g: np.ndarray
    accept_stat: float
    step_size: float
    tree_depth: int
    n_leapfrog: int
    divergent: bool
    replaced: bool                    # the row's proposal was replaced at least once (counts in ``accepted``)
    reason: str                       # 'inner', 'whole', 'max_depth' or 'divergent'
    block: int = 0                    # 'inner': the leaves of the block that turned
    subtree: int = 0                  # the leaves of the last sub-tree begun
    nan: bool = False                 # 'divergent': the stage had no density
    directions: list = field(default_factory=list)
    margins: list = field(default_factory=list)       # |log u - (a_n - W')| and |log u_T - (W' - W)| of every decision
    checks: list = field(default_factory=list)        # brute=True: (checkpoint decision, brute-force decision) per block


def step_gen(x, lp, g, z, eps, max_depth, draws, brute=False):
    """The step as a generator: yields (q, g(q), r, v) and is sent the stage's (q', lp', g', r'); returns ``Step``."""
    x, g, z = (np.array(a, dtype=np.float64) for a in (x, g, z))
    lp = float(lp)
    k0 = kinetic(z)
    ends = {1: (x, z, g), -1: (x, z, g)}
    rho, w = z.copy(), 0.0
    prop, replaced = (x, lp, g), False
    suma, ell, depth = 0.0, 0, 0
    out = dict(reason='max_depth', block=0, subtree=0, nan=False, directions=[], margins=[], checks=[])
    divergent = False
    for j in range(max_depth):
        size, ck, leaves, stop = 1 << j, {}, [], False
        out['subtree'] = size
        for n in range(size):
            log_u, v_new, log_ut_new = draws(ell + 1)
            if n == 0:
                v, log_ut = v_new, log_ut_new
                q, r, gq = ends[v]
                depth += 1
                out['directions'].append(v)
            q, lpq, gq, r = yield q, gq, r, v
            q, gq, r, lpq = np.array(q, dtype=np.float64), np.array(gq, dtype=np.float64), \
                np.array(r, dtype=np.float64), float(lpq)
            ell += 1
            a = (lpq - lp) + (k0 - kinetic(r))
            if a == a:
                suma = suma + min(1.0, _exp(a))
            if a != a or a < -1000.0:
                divergent, stop = True, True
                out.update(reason='divergent', nan=a != a)
                break
            if n == 0:
                wp, sub, rhop = a, (q, lpq, gq), r.copy()
            else:
                wp = lse(wp, a)
                out['margins'].append(abs(log_u - (a - wp)))
                if log_u < a - wp:
                    sub = (q, lpq, gq)
                rhop = rhop + r
            leaves.append(r.copy())
            if n % 2 == 0:
                ck[bin(n >> 1).count('1')] = (r.copy(), rhop.copy())
            else:
                kk = 1
                while (n >> (kk - 1)) & 1:
                    m = n & ~((1 << kk) - 1)
                    ra, rhoa = ck[bin(m >> 1).count('1')]
                    turned = turns((rhop - rhoa) + ra, ra, r)
                    if brute:
                        out['checks'].append((turned, brute_turns(leaves[m:n + 1])))
                    if turned:
                        stop = True
                        out.update(reason='inner', block=1 << kk)
                        break
                    kk += 1
            if stop:
                break
        if stop:
            break
        out['margins'].append(abs(log_ut - (wp - w)))
        if log_ut < wp - w:
            prop, replaced = sub, True
        w = lse(w, wp)
        rho = rho + rhop
        ends[v] = (q, r, gq)
        if turns(rho, ends[-1][1], ends[1][1]):
            out['reason'] = 'whole'
            break
    return Step(prop[0], prop[1], prop[2], suma / ell, float(eps), depth, ell, divergent, replaced, **out)


def host_stage(ev, eps, lam, c):
    """stage(q, g, r, v) from hmc_adapt_ref.trajectory: the one-stage trajectory with eps replaced by v * eps."""
    lam1, c = np.asarray(lam, dtype=np.float64)[None], np.asarray(c, dtype=np.float64)

    def stage(q, g, r, v):
        q2, lp2, g2, r2 = A.trajectory(q[None], g[None], r[None], np.array([v * float(eps)]), lam1, c, 1, ev)
        return q2[0], lp2[0], g2[0], r2[0]
    return stage


def step(x, lp, g, z, eps, lam, c, max_depth, draws, stage=None, ev=None, brute=False):
    """One NUTS step from the row (x, lp, g) with momentum z.  ``stage``: see the module docstring; or ``ev``, from
    which ``host_stage(ev, eps, lam, c)`` is built."""
    if stage is None:
        stage = host_stage(ev, eps, lam, c)
    gen = step_gen(x, lp, g, z, eps, max_depth, draws, brute)
    try:
        req = next(gen)
        while True:
            req = gen.send(stage(*req))
    except StopIteration as done:
        return done.value
