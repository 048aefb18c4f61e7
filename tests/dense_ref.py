"""Shared data and CPU references of the dense-preconditioner tests (test_dense_cpu.py, test_gpu_dense.py).

Data recipe: a correlated Gaussian, rng = default_rng(seed); Amix = N(0, 1)^(d x d) + 2 I;
x = N(0, 1)^(n x d) Amix'; g = -x inv(Amix Amix') (its exact score); gradient-free weights
w = exp(u - min u), u ~ U(0, 2) (log_p = 0, log_q = u: what thin_gf computes from them).  The sample is
standardised by the oracle and L = make_precon(xs, 'smpcov') of the package under test; the oracle
integrand is oracle.stein_numpy.vfk0_imq with that L (the oracle's make_precon has no 'smpcov').
Every case is computed once per process and shared (lru_cache); callers must not modify the arrays.
"""
import functools

import numpy as np

from oracle import stein_numpy as o

# (n, d, seed, gradient-free, m) of the greedy tests; the oracle's per-step margin must be >= MARGIN_MIN
GREEDY_CASES = [(1500, 2, 7, False, 40), (1500, 4, 7, False, 40), (1500, 8, 7, False, 40),
                (1500, 12, 7, False, 40), (1500, 4, 7, True, 40), (20000, 4, 3, False, 30)]
PAIR_DIMS = [1, 2, 3, 4, 5, 8, 9, 16]   # pair tests: n = PAIR_N rows, seed 7, Langevin and gradient-free
PAIR_N = 300
CHAIN_SEEDS = [7, 8, 9]                 # thin_chains: three chains of n = 1500, d = 4, m = 40
KSD_CASES = [(4, False), (4, True), (12, False)]   # KSD / Gram tests: n = 1500, seed 7
MARGIN_MIN = 1e-9
FACTOR = 8   # GPU error bound: FACTOR x the NumPy reference's own error against long double


def raw(n, d, seed):
    rng = np.random.default_rng(seed)
    amix = rng.normal(size=(d, d)) + 2 * np.identity(d)
    x = rng.normal(size=(n, d)) @ amix.T
    g = -x @ np.linalg.inv(amix @ amix.T)
    u = rng.uniform(0, 2, size=n)
    return x, g, u


@functools.lru_cache(maxsize=None)
def case(n, d, seed=7, gf=False):
    from stein_thinning.kernel import make_precon
    x, g, u = raw(n, d, seed)
    xs, gs = o._validate_and_standardize(x, g, True)
    L = make_precon(xs, 'smpcov')
    w = np.exp(o._log_weights(np.zeros(n), u, None)) if gf else None
    return dict(x=x, g=g, log_p=np.zeros(n), log_q=u, xs=xs, gs=gs, L=L, tr=float(np.trace(L)), w=w, n=n, d=d)


def integrand(c):
    xs, gs, L, w = c['xs'], c['gs'], c['L'], c['w']

    def f(i1, i2):
        k = o.vfk0_imq(xs[i1], xs[i2], gs[i1], gs[i2], L)
        return k if w is None else k * w[i1] * w[i2]
    return f


@functools.lru_cache(maxsize=None)
def greedy(n, d, seed, gf, m):
    """The oracle's greedy run: (indices, final running sums, smallest per-step margin
    (second-smallest - smallest running sum) / max |sum|)."""
    f = integrand(case(n, d, seed, gf))
    idx = np.empty(m, dtype=np.uint32)
    k0 = f(slice(None), slice(None)).copy()
    margin = np.inf
    for i in range(m):
        if i:
            k0 += 2 * f(slice(None), [idx[i - 1]])
        idx[i] = np.argmin(k0)
        two = np.partition(k0, 1)[:2]
        margin = min(margin, (two[1] - two[0]) / np.max(np.abs(k0)))
    assert np.array_equal(idx, o._greedy_search(m, f))
    return idx, k0, margin


def longdouble_ok():
    return np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def pair_ld(c, i1, i2):
    """(k, scale) of the reference formula in np.longdouble for rows i1 against i2: scale = |t1| + |t2| + |t3|
    (times w_i w_j for the gradient-free kernel)."""
    ld = np.longdouble
    xs, gs, L = c['xs'].astype(ld), c['gs'].astype(ld), c['L'].astype(ld)
    amb = xs[i1].T - xs[i2].T
    smb = gs[i1].T - gs[i2].T
    qf = 1 + np.sum(np.dot(L, amb) * amb, axis=0)
    t1 = -3 * np.sum(np.dot(np.dot(L, L), amb) * amb, axis=0) / qf ** ld(2.5)
    t2 = (np.trace(L) + np.sum(np.dot(L, smb) * amb, axis=0)) / qf ** ld(1.5)
    t3 = np.sum(gs[i1].T * gs[i2].T, axis=0) / np.sqrt(qf)
    k, scale = t1 + t2 + t3, np.abs(t1) + np.abs(t2) + np.abs(t3)
    if c['w'] is not None:
        ww = c['w'].astype(ld)[i1] * c['w'].astype(ld)[i2]
        k, scale = k * ww, scale * ww
    return k, scale


def pair_set(n, count=4000, seed=11):
    """`count` random pairs plus every i = j."""
    rng = np.random.default_rng(seed)
    i1 = np.concatenate([rng.integers(0, n, count), np.arange(n)])
    i2 = np.concatenate([rng.integers(0, n, count), np.arange(n)])
    return i1, i2


def rho(values, k_ld, scale):
    return float(np.max(np.abs(values.astype(np.longdouble) - k_ld) / scale))


def ksd_ld(c, rows):
    """Cumulative KSD of the rows (in this order) in np.longdouble."""
    rows = np.asarray(rows)
    m = rows.shape[0]
    a, b = np.meshgrid(rows, rows, indexing='ij')
    k, _ = pair_ld(c, a.reshape(-1), b.reshape(-1))
    k = k.reshape(m, m)
    inc = 2 * np.sum(np.tril(k, -1), axis=1) + np.diag(k)   # what row i adds: 2 sum_{a<i} k(i, a) + k(i, i)
    return np.sqrt(np.cumsum(inc)) / np.arange(1, m + 1)
