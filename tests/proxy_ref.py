"""Shared recipes, long-double reference and per-element error bounds of the proxy producers' edge tests
(csrc/proxy.hip, st_proxy_logpdf_grad): test_proxy_ref_cpu.py and test_gpu_proxy_edges.py.  No GPU and no
package import here (NumPy; scipy only inside ``factors``).  np.longdouble is the yardstick
(dense_ref.longdouble_ok).

Everything is stated at the ABI's level, on the inputs as the kernel receives them: x (n, d), loc (d),
U (d, d) = scipy's _PSD factor (U U^T = pinv(cov)), P (d, d) = np.linalg.inv(cov), df (0: Gaussian) and
c_log.  ``reference`` evaluates in long double

    dev = x - loc,   y = P dev,   m_U = |dev U|^2,   m_P = dev . y
    Gaussian:   lq = -0.5 (c_log + m),                          grad = -y
    Student-t:  lq = c_log - t log1p(m / df),  t = (df + d) / 2,  grad = -(df + d) / (df + m_P) y

with lq in both forms (m = m_U: scipy's; m = m_P: what the matrix-core kernels evaluate).  The two forms
differ by the gap between the host's two float64 factors (U U^T against P), which grows with cond(cov):
``gap = |m_P - m_U|`` is taken from this reference, never from a GPU output.

Bounds (u = 2^-53; first order in u; they hold for ANY summation order and with or without fma, so one set
serves every kernel variant).  Abbreviations, all in long double:

    Y_j = sum_k |P_jk| |dev_k|        S_P = sum_j |dev_j| Y_j        Z_j = sum_k |dev_k| |U_kj|

* dev: one rounding per element, |fl(dev_k) - dev_k| <= u |dev_k|.
* y_j, a d-term dot product of P's row with the rounded dev: d products and d - 1 adds in any order give
  d u Y_j, the rounding of dev one more u Y_j: (d + 1) u Y_j.
      tol_y[j] = (d + 4) u Y_j                                        (3 u Y_j to spare)
* m_P = sum_j dev_j y_j: the error of y_j weighs |dev_j| ((d + 1) u S_P), the rounding of dev_j another
  u S_P, the d products and d - 1 adds d u S_P: (2 d + 2) u S_P.
      tol_mP = (2 d + 6) u S_P                                        (4 u S_P >= 4 u m_P to spare)
* m_U = sum_j z_j^2, z_j = sum_k dev_k U_kj: z_j is off by (d + 1) u Z_j as y_j above, so z_j^2 by
  2 (d + 1) u Z_j^2 plus its own rounding u z_j^2; the d - 1 adds of non-negative squares add (d - 1) u m_U:
  (2 d + 2) u sum Z_j^2 + d u m_U.
      tol_mU = (2 d + 4) u sum_j Z_j^2 + (d + 3) u m_U               (>= 5 u m_U to spare)
* Gaussian lq = -0.5 (c_log + m): the add rounds to u |c_log + m| = 2 u |lq|; the halving is exact.
      tol_lq = tol_m / 2 + u (|c_log| + |ref|)
* Student-t lq = c_log + (-t) log(1 + (1 / df) m), scipy's formula, which the kernels take over.  With
  a = m / df: the argument w = 1 + a carries the error of m (tol_m / df), the roundings of 1 / df and of
  the product (2 u a) and of the add (u (1 + a)); the spare 4 u m / df of tol_m covers u a of these, leaving
  2 u (1 + a).  An absolute error e of w moves log w by e / (1 + a), times t.  The logarithm itself is good
  to one ulp on the device (2 u log w relative), t = 0.5 (df + d) is one rounding and t log w another:
  4 u t log1p(a).  The final add rounds to u |ref|.
      tol_lq = t (tol_m / df + 2 u (1 + a)) / (1 + a) + 4 u t log1p(a) + u (|c_log| + |ref|)
  The 2 u (1 + a) term is the rounding of ``1.0 + (1 / df) m`` and dominates for large df: t 2 u is about
  0.1 at df = 1e15.  That is the reference formula's own behaviour (scipy has it too), not a defect of the
  kernels.  (The issue that asked for these tests budgeted 2 u t log1p(a) for the logarithm's term.  That is
  a one-ulp logarithm alone and leaves nothing for the roundings of t and of the product; they matter for
  the far-tail rows, where t log1p(a) is all of lq: a correct float64 evaluation with another logarithm
  could miss that budget, so the worst case, 4 u, is used.  Every other form is the issue's.)
* Student-t grad_j = coef y_j, coef = (-(df + d) / df) / (1 + m_P / df) = -(df + d) / (df + m_P): the
  roundings of df + d, of the division by df, of the add, of the last division and of coef y_j are 5 u;
  the rounding of m_P / df (u a / (1 + a)) is covered by tol_mP's spare part; the error of m_P moves the
  denominator by tol_mP / (df + m_P) relative.
      tol_g[j] = |coef| tol_y[j] + |coef| |y_j| (5 u + tol_mP / (df + m_P))
* Gaussian grad = -y: tol_y (the negation is exact).

Which reference each kernel is held to (``check``):
* the VALU kernel ('valu'): lq against the U form with tol_mU; its Student-t coefficient uses m_P;
* the matrix-core kernels ('mfma'): lq against the P form with tol_mP, and against the U form with
  tol_mP + gap in place of tol_m.
A row at loc has dev = 0 and every tolerance except lq's own rounding 0: its gradient must be exactly 0.

``emulate`` restates each kernel's operation order in float64 on the CPU (fma-free NumPy; NumPy's log in
place of the device's): test_proxy_ref_cpu.py keeps it inside these bounds on every recipe.

Recipes (``recipe(name, n, d)``; seeded, cached, read-only):
* 'benign': cov = A A^T / d + 0.3 I (cond <= 18), loc ~ N(0, 1), rows loc + 1.5 chol(cov) N(0, 1) -- the
  recipe of tests/test_gpu_proxy.py;
* 'scaled': the same with per-dimension scales s = exp(U(0, log spread)) (cov -> s s^T * cov, loc and the
  rows scaled along), spread = 1e4: cond up to about 1e8;
* 'shifted': the benign one with loc + 1e6 (unit spread around a far location);
* 'special' / 'special_scaled': on the benign / scaled covariance, row i at Mahalanobis radius
  RADII[i % 4] = 0 (x == loc exactly), 1e-6, 1.5, 1e4, and the whole 16-row block [64, 80) at 1e140
  (squares near 1e280: everything stays finite in float64).
"""
import functools

import numpy as np

U = 2.0 ** -53
LOG_2PI = float(np.log(2 * np.pi))
RECIPES = ['benign', 'scaled', 'shifted', 'special', 'special_scaled']
RADII = [0.0, 1e-6, 1.5, 1e4]
FAR_BLOCK = (64, 80)
FAR_RADIUS = 1e140
MFMA_DIMS = [17, 18, 24, 25, 63, 64]                 # the matrix-core kernels' range: every (T, S) edge
VALU_DIMS = [1, 3, 4, 5, 15, 16, 65, 127, 128]       # nc < 4 remainder columns; > 64 KB of LDS above d = 60
EDGE_DIMS = [17, 18, 63, 64]
EDGE_N = [1, 15, 16, 17, 63, 64, 65, 127]
DFS = [0.0, 1e-3, 1.0, 30.5, 1e6, 1e15]              # 0: the Gaussian proxy
TILED_ROWS = 509                                     # distinct rows of the deep grid-stride cases (a prime)


# ------------------------------------------------------------------------------------------ recipes
@functools.lru_cache(maxsize=None)
def recipe(name, n, d, spread=1e4):
    """dict(x (n, d), loc (d), cov (d, d)), read-only."""
    rng = np.random.default_rng([RECIPES.index(name), n, d])
    a = rng.normal(size=(d, d))
    cov = a @ a.T / d + 0.3 * np.eye(d)
    cov = np.tril(cov) + np.tril(cov, -1).T
    loc = rng.normal(size=d)
    z = rng.normal(size=(n, d))
    scale = np.ones(d)
    if name in ('scaled', 'special_scaled'):
        scale = np.exp(rng.uniform(0.0, np.log(spread), size=d))
    if name in ('special', 'special_scaled'):
        z = z / np.sqrt(np.sum(z * z, axis=1, keepdims=True))      # unit directions in whitened space
        radius = np.array(RADII)[np.arange(n) % len(RADII)]
        radius[FAR_BLOCK[0]:FAR_BLOCK[1]] = FAR_RADIUS
        step = (z @ np.linalg.cholesky(cov).T) * radius[:, None]
    else:
        step = (z @ np.linalg.cholesky(cov).T) * 1.5
    cov = np.outer(scale, scale) * cov
    loc = loc * scale
    if name == 'shifted':
        loc = loc + 1e6
    x = loc + step * scale
    if name in ('special', 'special_scaled'):
        x[radius == 0.0] = loc
    assert np.all(np.isfinite(x))
    out = dict(x=x, loc=loc, cov=cov)
    for v in out.values():
        v.setflags(write=False)
    return out


def at_loc(name, n):
    """Indices of the rows that sit exactly at loc (special recipes), none otherwise."""
    if name not in ('special', 'special_scaled'):
        return np.empty(0, dtype=np.int64)
    i = np.arange(n)
    return i[(i % len(RADII) == 0) & ~((i >= FAR_BLOCK[0]) & (i < FAR_BLOCK[1]))]


@functools.lru_cache(maxsize=None)
def _psd(name, n, d, spread):
    import scipy.linalg
    cov = recipe(name, n, d, spread)['cov']
    s, u = scipy.linalg.eigh(cov, lower=True, check_finite=True)
    eps = 1e6 * np.finfo(np.float64).eps * np.max(abs(s))
    assert np.min(s) > eps, 'the recipe must be full rank to scipy'
    s_pinv = np.array([1 / v for v in s], dtype=float)
    # row-major, as the ABI takes them (eigh's vectors come column-major)
    out = np.ascontiguousarray(np.multiply(u, np.sqrt(s_pinv))), np.ascontiguousarray(np.linalg.inv(cov)), float(np.sum(np.log(s)))
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def factors(name, n, d, df, spread=1e4):
    """(U, P, c_log) of the recipe's covariance as the host computes them (stein_thinning.proxy restated:
    scipy's _PSD factor, np.linalg.inv, the constants in scipy's operation order); df = 0: Gaussian."""
    from scipy.special import gammaln
    whiten, precision, log_pdet = _psd(name, n, d, spread)
    if df == 0.0:
        c_log = d * LOG_2PI + log_pdet
    else:
        t = 0.5 * (df + d)
        c_log = gammaln(t) - gammaln(0.5 * df) - d / 2. * np.log(df * np.pi) - 0.5 * log_pdet
    return whiten, precision, float(c_log)


# ------------------------------------------------------------------------------------------ reference
def reference(x, loc, whiten, precision, df, c_log):
    """Long-double values and the docstring's tolerances: a dict with lq_U, lq_P, grad, tol_lq_U (VALU),
    tol_lq_P, tol_lq_PU (matrix cores against the P and the U form), tol_g, and m_U, m_P, tol_mU, tol_mP,
    gap (all long double)."""
    ld = np.longdouble
    u = ld(U)
    n, d = x.shape
    dev = x.astype(ld) - np.asarray(loc).astype(ld)
    Pl, Ul = np.asarray(precision).astype(ld), np.asarray(whiten).astype(ld)
    adev = np.abs(dev)
    y = dev @ Pl.T
    Y = adev @ np.abs(Pl).T
    z = dev @ Ul
    Z = adev @ np.abs(Ul)
    m_P = np.sum(dev * y, axis=1)
    m_U = np.sum(z * z, axis=1)
    tol_y = (d + 4) * u * Y
    tol_mP = (2 * d + 6) * u * np.sum(adev * Y, axis=1)
    tol_mU = (2 * d + 4) * u * np.sum(Z * Z, axis=1) + (d + 3) * u * m_U
    gap = np.abs(m_P - m_U)
    c = ld(c_log)
    dfl = ld(df)

    def lq_and_tol(m, tol_m):
        if df == 0.0:
            ref = -(c + m) / 2
            return ref, tol_m / 2 + u * (abs(c) + np.abs(ref))
        t = (dfl + d) / 2
        a = m / dfl
        ref = c - t * np.log1p(a)
        tol = t * (tol_m / dfl + 2 * u * (1 + a)) / (1 + a) + 4 * u * t * np.log1p(a) + u * (abs(c) + np.abs(ref))
        return ref, tol

    lq_U, tol_lq_U = lq_and_tol(m_U, tol_mU)
    lq_P, tol_lq_P = lq_and_tol(m_P, tol_mP)
    _, tol_lq_PU = lq_and_tol(m_U, tol_mP + gap)
    if df == 0.0:
        grad, tol_g = -y, tol_y
    else:
        coef = -(dfl + d) / (dfl + m_P)
        grad = coef[:, None] * y
        tol_g = np.abs(coef)[:, None] * (tol_y + np.abs(y) * (5 * u + tol_mP / (dfl + m_P))[:, None])
    return dict(lq_U=lq_U, lq_P=lq_P, grad=grad, tol_lq_U=tol_lq_U, tol_lq_P=tol_lq_P, tol_lq_PU=tol_lq_PU,
                tol_g=tol_g, m_U=m_U, m_P=m_P, tol_mU=tol_mU, tol_mP=tol_mP, gap=gap)


def kernel_kind(mode, d):
    """'mfma' where st_tune key 7 = mode sends dimension d to a matrix-core kernel, else 'valu'."""
    return 'mfma' if mode != 1 and 16 < d <= 64 else 'valu'


def _ratio(err, tol):
    """max err / tol with 0 / 0 = 0 and anything else over 0 = inf; a NaN error counts as inf."""
    err, tol = np.asarray(err, dtype=np.longdouble), np.asarray(tol, dtype=np.longdouble)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


def check(kind, lq, grad, r, rows=None, what=''):
    """Every element of (lq, grad) within the bounds of ``r`` (a ``reference`` dict, restricted to ``rows``
    when given) for a kernel of ``kind`` ('valu' or 'mfma'); returns the worst error / bound ratios."""
    sel = slice(None) if rows is None else rows
    ld = np.longdouble
    lq, grad = np.asarray(lq).astype(ld), np.asarray(grad).astype(ld)
    out = {}
    if kind == 'valu':
        out['lq_U'] = _ratio(np.abs(lq - r['lq_U'][sel]), r['tol_lq_U'][sel])
    else:
        out['lq_P'] = _ratio(np.abs(lq - r['lq_P'][sel]), r['tol_lq_P'][sel])
        out['lq_U'] = _ratio(np.abs(lq - r['lq_U'][sel]), r['tol_lq_PU'][sel])
    out['grad'] = _ratio(np.abs(grad - r['grad'][sel]), r['tol_g'][sel])
    for name, v in out.items():
        assert v <= 1.0, f'{what}: {kind} kernel, {name}: worst error / bound = {v:.3g}'
    return out


# ------------------------------------------------------------------------------------------ emulation
def _kmap(s, lk):
    return 8 * (s >> 1) + 2 * lk + (s & 1)


def emulate(variant, x, loc, whiten, precision, df, c_log):
    """(lq, grad) of kernel ``variant`` (st_tune key 7: 1 VALU, 2 LDS-tiled matrix cores, 3 / 4 the streaming
    forms, which share one order) in float64 with the kernel's summation order, unfused:
    * 1: z_j and y_j sequential over k; the squares z_j^2 summed per wave (columns 4 w + 16 i .. + 3, in
      order), the four wave sums added ((0 + 1) + 2) + 3; the Student-t coefficient from dev . y sequential;
    * 2: y_j over k in order (four k per matrix instruction); dev . y in four strided partial sums
      (j = q, q + 4, ...) added (0 + 1) + (2 + 3);
    * 3, 4: y_j over the steps s with k = kmap(s, 0 .. 3) inside a step; dev . y in four partial sums (lane
      group lk owns k = kmap(s, lk)) added (0 + 1) + (2 + 3)."""
    x = np.asarray(x, dtype=np.float64)
    P, W = np.asarray(precision, dtype=np.float64), np.asarray(whiten, dtype=np.float64)
    n, d = x.shape
    with np.errstate(all='ignore'):
        dev = x - np.asarray(loc, dtype=np.float64)
        y = np.zeros((n, d))
        if variant in (1, 2):
            korder = list(range(d))
        else:
            S = 2 * ((d + 7) // 8)
            korder = [k for s in range(S) for k in (_kmap(s, lk) for lk in range(4)) if k < d]
            assert sorted(korder) == list(range(d))
        for k in korder:
            y = y + dev[:, k, None] * P[None, :, k]
        if variant == 1:
            z = np.zeros((n, d))
            for k in range(d):
                z = z + dev[:, k, None] * W[None, k, :]
            part = np.zeros((4, n))
            for j in range(d):
                w = (j // 4) % 4
                part[w] = part[w] + z[:, j] * z[:, j]
            maha = ((part[0] + part[1]) + part[2]) + part[3]
            my = np.zeros(n)
            for k in range(d):
                my = my + dev[:, k] * y[:, k]
        else:
            part = np.zeros((4, n))
            if variant == 2:
                for j in range(d):
                    part[j % 4] = part[j % 4] + dev[:, j] * y[:, j]
            else:
                for s in range(S):
                    for lk in range(4):
                        k = _kmap(s, lk)
                        if k < d:
                            part[lk] = part[lk] + dev[:, k] * y[:, k]
            maha = (part[0] + part[1]) + (part[2] + part[3])
            my = maha
        if df > 0.0:
            t = 0.5 * (df + d)
            lq = c_log + -t * np.log(1.0 + (1.0 / df) * maha)
            coef = (-(df + d) / df) / (1.0 + my / df)
            grad = coef[:, None] * y
        else:
            lq = -0.5 * (c_log + maha)
            grad = -y
    return lq, grad
