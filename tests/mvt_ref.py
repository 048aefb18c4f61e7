"""Shared helper of the multivariate-t fit tests (tests/test_mvt_cpu.py, tests/test_abi_mvt.py,
tests/test_gpu_mvt.py): the seeded recipe, the sample moments of the t likelihood in long double and in
float64 NumPy, the likelihood's value and analytic gradient from them, and the reference's own fit
(scipy's multivariate_t.logpdf under finite-difference L-BFGS-B), restated from the formulas:

  par = [mu (d), triu(A) (np.triu_indices order), df],  Sigma = A^T A,  U = inv(A)  (U U^T = inv(Sigma))
  z_i = (x_i - mu) @ U,  delta_i = |z_i|^2,  w_i = (df + d) / (df + delta_i)
  S0 = sum log(1 + delta_i / df),  S1 = sum w_i,  Sz = sum w_i z_i,  Szz = sum w_i z_i z_i^T
  c = gammaln((df + d) / 2) - gammaln(df / 2) - d / 2 log(df pi) - sum log|A_kk|
  NLL = -n c + (df + d) / 2 S0
  d/dmu = -U @ Sz,   d/dA = triu((n I - Szz) @ U^T)
  d/ddf = -n c' + S0 / 2 - (df + d) / (2 df) (n - df S1 / (df + d)),  c' = psi((df + d) / 2) / 2 - psi(df / 2) / 2 - d / (2 df)
  fit_mvt2: Sigma = exp(s) C, U = exp(-s / 2) U_C, d/ds = (n d - tr Szz) / 2

Recipe (``case(d, n, seed)``): ``rng = default_rng(seed)``; M standard normal (d, d), Sigma = (M M^T / d + I)
1e-2; loc = 0.1 N(0, 1); df = 5; rows = loc + (L g) / sqrt(chi2_5 / 5), L the lower Cholesky factor.

Tolerances.  MOMENT_RTOL = 1e-12 (the project's proxy tolerance) bounds every sum's error by 1e-12 *
sum |term|; the float64 NumPy moments hold it on every case (tests/test_mvt_cpu.py).  The fit bounds are
10 x the differences measured between the reference's finite-difference fit and the analytic-gradient
fit on the NumPy moments (scipy 1.15.3; tests/test_mvt_cpu.py re-measures and prints them):

  case                  |df diff|   max|Sigma diff| / max|Sigma|   max|mu diff|   fun (relative)   nfev
  fit_mvt  (4, 4000)    7.285e-06   6.012e-07                      1.676e-08      -5.8e-12         22 against 352
  fit_mvt  (2, 1000)    1.916e-05   1.044e-05                      6.941e-07      -1.9e-11         22 against 168
  fit_mvt  (9, 3000)    4.520e-06   1.314e-07                      1.479e-08      -1.5e-12         27 against 1512
  fit_mvt2 (4, 4000)    1.889e-05   7.298e-07                      (mu fixed)     -1.4e-12         11 against 33
  (fit_mvt2: Sigma = exp(s) C, so the relative difference is |exp(s' - s) - 1|.)
The float64 NumPy moments' largest error / sum |term| on the moment cases: 1.5e-15 (n = 300 001), 9.2e-16 on
the far rows.
"""
import functools

import numpy as np

MOMENT_RTOL = 1e-12
FTOL = 2.2e-9                       # L-BFGS-B's default ftol, by which both fits stop
FIT_CASES = [(4, 4000, 11), (2, 1000, 12), (9, 3000, 13)]    # (d, n, seed)
MU_BOUNDS, A_BOUNDS, DF_BOUNDS, SCALE_BOUNDS = (-1.0, 1.0), (-1.0, 1.0), (2.0, 30.0), (-20.0, 20.0)
# measured |reference fit - analytic NumPy fit|: (df, Sigma relative to max|Sigma|, mu), per FIT_CASES
# entry and then fit_mvt2 on the first; the GPU fits are held to BOUND_FACTOR x these
RECORDED = {
    (4, 4000): (7.285e-06, 6.012e-07, 1.676e-08),
    (2, 1000): (1.916e-05, 1.044e-05, 6.941e-07),
    (9, 3000): (4.520e-06, 1.314e-07, 1.479e-08),
    'fit_mvt2': (1.889e-05, 7.298e-07, 0.0),
}
BOUND_FACTOR = 10.0

MOMENT_DIMS = [1, 2, 4, 8, 9, 16]
MOMENT_ROWS = [1, 63, 64, 65, 257, 4097]
MOMENT_DFS = [2.0, 9.456, 30.0]


@functools.lru_cache(maxsize=None)
def case(d, n, seed):
    """(x, loc, sigma, df), read-only: computed once per shape and shared."""
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(d, d))
    sigma = (m @ m.T / d + np.eye(d)) * 1e-2
    loc = 0.1 * rng.normal(size=d)
    df = 5.0
    g = rng.normal(size=(n, d)) @ np.linalg.cholesky(sigma).T
    x = loc + g / np.sqrt(rng.chisquare(df, size=n) / df)[:, None]
    for arr in (x, loc, sigma):
        arr.setflags(write=False)
    return x, loc, sigma, df


def whitening(sigma):
    """(A, U): the upper Cholesky factor A (sigma = A^T A) and U = inv(A), upper triangular."""
    a = np.linalg.cholesky(sigma).T
    return a, np.triu(np.linalg.inv(a))


def pack(mu, a, df):
    return np.concatenate([mu, a[np.triu_indices(len(mu))], [df]])


def moments_ld(x, loc, whiten, df):
    """({S0, S1, Sz, Szz}, the same with |term| summed) in np.longdouble."""
    ld = np.longdouble
    d = x.shape[1]
    z = (x.astype(ld) - np.asarray(loc, dtype=ld)) @ np.asarray(whiten, dtype=ld)
    delta = np.sum(z * z, axis=1)
    dfl = ld(df)
    w = (dfl + d) / (dfl + delta)
    l = np.log1p(delta / dfl)
    wz = w[:, None] * z
    terms = wz[:, :, None] * z[:, None, :]
    sums = {'S0': np.sum(l), 'S1': np.sum(w), 'Sz': np.sum(wz, axis=0), 'Szz': np.sum(terms, axis=0)}
    mags = {'S0': np.sum(np.abs(l)), 'S1': np.sum(np.abs(w)), 'Sz': np.sum(np.abs(wz), axis=0),
            'Szz': np.sum(np.abs(terms), axis=0)}
    return sums, mags


def moments_np(x, loc, whiten, df, grad=True):
    """(S0, S1, Sz, Szz) in float64 NumPy (scipy's operation order for the log term)."""
    d = x.shape[1]
    z = (x - loc) @ whiten
    delta = np.sum(z * z, axis=1)
    s0 = float(np.sum(np.log(1 + (1. / df) * delta)))
    if not grad:
        return s0, None, None, None
    w = (df + d) / (df + delta)
    wz = w[:, None] * z
    return s0, float(np.sum(w)), np.sum(wz, axis=0), wz.T @ z


def check_moments(got, x, loc, whiten, df, rtol=MOMENT_RTOL):
    """Every sum of ``got`` = (S0, S1, Sz, Szz) within rtol * sum |term| of the long-double sums; returns
    the largest error / sum |term| seen."""
    sums, mags = moments_ld(x, loc, whiten, df)
    worst = 0.0
    for name, g in zip(('S0', 'S1', 'Sz', 'Szz'), got):
        err = np.abs(np.asarray(g, dtype=np.longdouble) - sums[name])
        mag = mags[name]
        assert np.all(np.isfinite(np.asarray(g, dtype=np.float64))), name
        assert np.all(err <= rtol * mag), (name, float(np.max(err)), float(np.max(mag)))
        with np.errstate(invalid='ignore', divide='ignore'):
            worst = max(worst, float(np.max(np.where(mag > 0, err / np.where(mag > 0, mag, 1), 0))))
    return worst


def numpy_backend(lik, loc, whiten, df, want_grad):
    """Stand-in for stein_thinning.proxy._mvt_moments on a host: the flat record from moments_np."""
    d = lik.d
    s0, s1, sz, szz = moments_np(np.asarray(lik.sample), loc, whiten, df, want_grad)
    out = np.zeros(2 + d + d * (d + 1) // 2)
    out[0] = s0
    if want_grad:
        out[1] = s1
        out[2:2 + d] = sz
        out[2 + d:] = (0.5 * (szz + szz.T))[np.triu_indices(d)]
    return out


def nll_grad(x, par):
    """(NLL, gradient) of the t likelihood at fit_mvt's parameter vector, in NumPy."""
    from scipy.special import gammaln, psi
    n, d = x.shape
    par = np.asarray(par, dtype=np.float64)
    mu, df = par[:d], par[-1]
    a = np.zeros((d, d))
    a[np.triu_indices(d)] = par[d:-1]
    u = np.triu(np.linalg.inv(a))
    s0, s1, sz, szz = moments_np(x, mu, u, df)
    c = gammaln((df + d) / 2) - gammaln(df / 2) - d / 2 * np.log(df * np.pi) - np.sum(np.log(np.abs(np.diag(a))))
    value = -n * c + (df + d) / 2 * s0
    dc = psi((df + d) / 2) / 2 - psi(df / 2) / 2 - d / (2 * df)
    g_df = -n * dc + s0 / 2 - (df + d) / (2 * df) * (n - df * s1 / (df + d))
    g_a = np.triu((n * np.eye(d) - szz) @ u.T)
    return float(value), np.concatenate([-u @ sz, g_a[np.triu_indices(d)], [g_df]])


def scipy_nll(x, par):
    """-sum multivariate_t.logpdf at fit_mvt's parameter vector: the reference's objective."""
    from scipy import stats
    d = x.shape[1]
    a = np.zeros((d, d))
    a[np.triu_indices(d)] = par[d:-1]
    return -np.sum(stats.multivariate_t.logpdf(x, loc=par[:d], shape=a.T @ a, df=par[-1]))


def start_and_bounds(x, mu_bounds=MU_BOUNDS, a_bounds=A_BOUNDS, df_bounds=DF_BOUNDS, df_init=4.):
    """The reference's start vector (sample mean, upper Cholesky factor of np.cov(ddof=d), df_init) and
    its list of (lower, upper) pairs."""
    d = x.shape[1]
    a = np.linalg.cholesky(np.atleast_2d(np.cov(x, rowvar=False, ddof=d))).T
    start = np.concatenate([np.mean(x, axis=0), a[np.triu_indices(d)], [df_init]])
    n_cov = d * (d + 1) // 2
    bounds = [tuple(mu_bounds)] * d + [tuple(a_bounds)] * n_cov + [tuple(df_bounds)]
    return start, bounds


@functools.lru_cache(maxsize=None)
def reference_fit(d, n, seed):
    """The reference's fit_mvt call on case(d, n, seed): value-only objective, scipy's finite differences."""
    from scipy.optimize import minimize
    x = case(d, n, seed)[0]
    start, bounds = start_and_bounds(x)
    return minimize(lambda par: scipy_nll(x, par), start, method='L-BFGS-B', bounds=bounds)


def mode_row(d, n, seed):
    """fit_mvt2's fixed location in the tests: the row nearest the sample mean (a stand-in for the
    notebook's row of highest log p)."""
    x = case(d, n, seed)[0]
    return x[np.argmin(np.sum((x - x.mean(axis=0)) ** 2, axis=1))].copy()


@functools.lru_cache(maxsize=None)
def reference_fit2(d, n, seed):
    """The reference's fit_mvt2 call on case(d, n, seed) with mu = mode_row."""
    from scipy import stats
    from scipy.optimize import minimize
    x = case(d, n, seed)[0]
    mu = mode_row(d, n, seed)
    cov = np.atleast_2d(np.cov(x, rowvar=False, ddof=d))
    return minimize(lambda b: -np.sum(stats.multivariate_t.logpdf(x, loc=mu, shape=np.exp(b[0]) * cov, df=b[1])),
                    np.array([0.0, 4.0]), method='L-BFGS-B', bounds=[SCALE_BOUNDS, DF_BOUNDS])


class numpy_moments:
    """``with numpy_moments(): ...`` -- stein_thinning.proxy runs on numpy_backend inside the block."""

    def __enter__(self):
        from stein_thinning import proxy
        self.saved = proxy._mvt_moments
        proxy._mvt_moments = numpy_backend
        return self

    def __exit__(self, *exc):
        from stein_thinning import proxy
        proxy._mvt_moments = self.saved
        return False


@functools.lru_cache(maxsize=None)
def numpy_fit(d, n, seed, jac='analytic'):
    """stein_thinning.proxy.fit_mvt on case(d, n, seed) with the NumPy moments."""
    from stein_thinning import proxy
    with numpy_moments():
        return proxy.fit_mvt(case(d, n, seed)[0], MU_BOUNDS, A_BOUNDS, DF_BOUNDS, jac=jac)


@functools.lru_cache(maxsize=None)
def numpy_fit2(d, n, seed):
    from stein_thinning import proxy
    with numpy_moments():
        return proxy.fit_mvt2(case(d, n, seed)[0], SCALE_BOUNDS, DF_BOUNDS, mode_row(d, n, seed))


def fit_differences(res, want, d):
    """(|df diff|, max|Sigma diff| / max|Sigma|, max|mu diff|) of two fit_mvt results."""
    a, b = np.zeros((d, d)), np.zeros((d, d))
    a[np.triu_indices(d)] = res.x[d:-1]
    b[np.triu_indices(d)] = want.x[d:-1]
    sa, sb = a.T @ a, b.T @ b
    return (abs(res.x[-1] - want.x[-1]), float(np.abs(sa - sb).max() / np.abs(sb).max()),
            float(np.abs(res.x[:d] - want.x[:d]).max()))


def fit2_differences(res, want):
    """The same for fit_mvt2 results (s, df): Sigma = exp(s) C, mu fixed."""
    return abs(res.x[1] - want.x[1]), abs(float(np.expm1(res.x[0] - want.x[0]))), 0.0


def moment_inputs(d, n):
    """(x, loc, U) of the moment tests at (d, n): the recipe's rows, its true location and the whitening
    of its true Sigma."""
    x, loc, sigma, _ = case(d, n, 1000 * d + n)
    return x, loc, whitening(sigma)[1]


def extreme_inputs(d=4, n=257):
    """name -> (x, loc, U, df): rows equal to loc (delta = 0), rows 1e6 scale lengths away (delta / df
    ~ 1e12), an upper-triangular U with negative diagonal entries."""
    x, loc, u = moment_inputs(d, n)
    a = np.linalg.inv(u)
    at_loc = x.copy()
    at_loc[::3] = loc
    far = x.copy()
    far[5::7] = loc + 1e6 * (np.ones(d) @ a) * np.where(np.arange(len(far[5::7])) % 2, 1.0, -1.0)[:, None]
    flip = u * np.where(np.arange(d) % 2 == 0, -1.0, 1.0)[None, :]
    return {'at_loc': (at_loc, loc, u, 5.0), 'all_at_loc': (np.tile(loc, (65, 1)), loc, u, 5.0),
            'far': (far, loc, u, 5.0), 'negative_diagonal': (x, loc, flip, 9.456)}
