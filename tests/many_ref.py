"""Shared inputs and host references of the thin_many tests (tests/test_thin_many_cpu.py, tests/test_gpu_thin_many.py).

Chains look like random-walk Metropolis output: about 75 % of the rows repeat the row before them bit for bit, so
exact ties occur at every greedy step and must go to the lowest index.  The gradient is the score of a Gaussian
target, the gradient-free proxy a slightly wider Gaussian.  Every reference (the NumPy oracle's indices, the C bit
model's indices and running sums on the oracle's standardised rows) is computed once per case and cached."""
import ctypes
import functools

import numpy as np

M = 20
DIMS = (2, 4)
PRECONS = ('id', 'med', 0.7)
BASE_NS = (2, 63, 64, 65, 256, 257, 1000, 1001, 1500)
SEED = 20261021


@functools.lru_cache(maxsize=None)
def native_lib():
    """The C-ABI library, loaded without touching a GPU (host-only queries: max_n, plan); built first when the
    tree holds none."""
    import os

    import __graft_entry__ as ge
    from stein_thinning import _native
    if not os.path.exists(ge.HIP_LIB):
        ge.build()
    return _native.load_library(ge.HIP_LIB)


def max_n(d, weights=False):
    return int(native_lib().st_greedy_many_max_n(d, 1 if weights else 0))


def plan(n, d, weights=False):
    t, r = ctypes.c_int32(0), ctypes.c_int32(0)
    assert native_lib().st_greedy_many_plan(n, d, 1 if weights else 0, ctypes.byref(t), ctypes.byref(r)) == 0
    return t.value, r.value


@functools.lru_cache(maxsize=None)
def plan_changes(d):
    """Every n at which the launcher's (threads, rows per thread) differs from that of n + 1."""
    lib = native_lib()
    t, r = ctypes.c_int32(0), ctypes.c_int32(0)
    plans = []
    for n in range(1, max_n(d) + 1):
        assert lib.st_greedy_many_plan(n, d, 0, ctypes.byref(t), ctypes.byref(r)) == 0
        plans.append((t.value, r.value))
    return tuple(n for n in range(1, max_n(d)) if plans[n - 1] != plans[n])


@functools.lru_cache(maxsize=None)
def parity_ns(d):
    ns = set(BASE_NS) | {max_n(d) - 1, max_n(d)}
    for n in plan_changes(d):
        ns |= {n, n + 1}
    return tuple(sorted(ns))


def parity_cases():
    return [(d, n, p) for d in DIMS for n in parity_ns(d) for p in PRECONS]


def rw_chains(C, n, d, seed=SEED, accept=0.25):
    """(x, g): (C, n, d) chains with ~75 % repeated rows and the score of N(mu, diag(s2)) at them."""
    rng = np.random.default_rng([seed, C, n, d])
    mu = np.linspace(-1.0, 2.0, d)
    s2 = np.linspace(0.5, 3.0, d)
    x = np.empty((C, n, d))
    for c in range(C):
        moved = rng.random(n) < accept
        moved[:min(n, 3)] = True               # the first rows differ: no chain is constant in a column
        step = rng.normal(size=(n, d)) * np.sqrt(s2) * 0.7
        x[c] = mu + rng.normal(size=d) + np.cumsum(np.where(moved[:, None], step, 0.0), axis=0)
    g = -(x - mu) / s2
    return x, g


def gf_inputs(x):
    """(log_p, log_q, gradient_q) for chains x: the target N(mu, diag(s2)) and a 30 % wider proxy."""
    d = x.shape[-1]
    mu = np.linspace(-1.0, 2.0, d)
    s2 = np.linspace(0.5, 3.0, d)
    q2 = 1.3 * s2
    log_p = -0.5 * np.sum((x - mu) ** 2 / s2, axis=-1)
    log_q = -0.5 * np.sum((x - mu) ** 2 / q2, axis=-1)
    return log_p, log_q, -(x - mu) / q2


def chains_per_case(n):
    return 3 if n >= 1000 else 5


def scales(s, precon):
    """(linv_scale, linv_trace) as thin() takes them from the oracle's preconditioner."""
    from oracle import stein_numpy as o
    linv = o.make_precon(s, precon) if isinstance(precon, str) else np.linalg.inv(precon * np.identity(s.shape[1]))
    return float(linv[0, 0]), float(np.trace(linv))


@functools.lru_cache(maxsize=None)
def parity_reference(d, n, precon):
    """x, g and per chain: the NumPy oracle's indices, the C bit model's (exact arithmetic) indices and final
    running sums on the oracle's standardised rows."""
    from oracle import stein_numpy as o
    from tests import oracle_c
    x, g = rw_chains(chains_per_case(n), n, d)
    ref = []
    for c in range(x.shape[0]):
        s, gs = o._validate_and_standardize(x[c], g[c], True)
        l, tr = scales(s, precon)
        cidx, cA = oracle_c.greedy(s, gs, None, l, tr, M, arith='exact')
        ref.append((o.thin(x[c], g[c], M, preconditioner=precon), cidx, cA))
    return x, g, ref
