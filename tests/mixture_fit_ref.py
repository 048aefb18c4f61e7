"""Shared helper of the mixture-fit tests (tests/test_mixture_fit_cpu.py, tests/test_gpu_mixture_fit.py): a
NumPy restatement of one EM pass (``stats``), of the M-step and of the whole EM loop (``em``), generic in dtype
so that it runs in ``np.longdouble``, and a derived rounding bound for every entry of the statistics.

Definitions (include/stein_thinning_hip.h, st_mixture_em_stats), for rows x_i of weight om_i and the factors
(a_c, mu_c, P_c) that ``stein_thinning.mixture.mixture_factors`` makes:

    dev_ic = x_i - mu_c,  l_ic = a_c - dev_ic . (P_c dev_ic) / 2,  log_p_i = logsumexp_c l_ic,  r_ic = exp(l_ic - log_p_i)
    LL = sum om_i log_p_i,  N_c = sum om_i r_ic,  S_c = sum om_i r_ic dev_ic,  Q_c = sum om_i r_ic dev_ic dev_ic^T

Rows of weight 0 are left out whatever they hold; a component with a_c = -inf is left out and its statistics
are 0.  The logsumexp is the stable one of tests/mixture_ref.py::stable (maximum first).

The bound (``stats(...)['bound']``, u = 2^-53, first order in u, then doubled for the second-order terms and
for exp / log being accurate to 1 ulp rather than correctly rounded).  The float64 kernel evaluates
  * dev_k with one rounding; y_j = sum_k P_jk dev_k and q = sum_j dev_j y_j by fma chains of length d:
    |dq| <= (2 d + 3) u qabs,  qabs = sum_jk |dev_j| |P_jk| |dev_k|;  l = a - q / 2: |dl| <= |dq| / 2 + u |l|;
  * log_p by a running-maximum logsumexp over k components (per component: one subtraction, one exp, one
    fma or add):  |dlog_p| <= sum_c r_c |dl_c| + u sum_c r_c |l_c - m| + (3 k + 6) u + u |log_p|;
  * r = exp(l - log_p): relative error rho_ic <= |dl_ic| + |dlog_p_i| + u |l_ic - log_p_i| + 2 u;
  * a term om r dev_i dev_j by two multiplications and an fma on two rounded dev: relative error rho + 4 u;
  * the sum of the n terms in some fixed order whose longest chain is at most ceil(n / 64) + 100 additions
    (a lane's tiles one after another, 6 tree levels, 4 waves, the block records):
    (ceil(n / 64) + 100) u sum |term|.
So for an entry with terms t_i:  bound = 2 [ sum_i |t_i| (rho_i + 4 u) + (ceil(n / 64) + 100) u sum_i |t_i| ],
and for LL (terms om_i log_p_i):  2 [ sum_i om_i |dlog_p_i| + (ceil(n / 64) + 101) u sum_i |om_i log_p_i| ].
The bound is a function of the inputs alone.  ``check`` asserts that it stays below VACUOUS = 1e-10 of the
entry's sum of absolute terms, so that it cannot grow until it says nothing.

RECORDED: the largest difference between the float64 and the long-double run of ``em`` from the same start on
``planted`` (final ll; weights, means and covariances relative to max |value|), measured by
tests/test_mixture_fit_cpu.py::test_recorded_spread on this restatement, rounded up to one digit.  EM is a
contraction only near its fixed point, so a free-running float64 run -- the restatement's or the GPU's --
may drift by that much from the long-double one; the GPU fit is held to ALLOW = 10 x RECORDED.
"""
import functools

import numpy as np

U = 2.0 ** -53
VACUOUS = 1e-10
RECORDED = 4e-15
ALLOW = 10 * RECORDED

ROWS = [1, 63, 64, 65, 257, 4099]
DIMS = [1, 2, 4, 8, 9, 16]
COMPONENTS = [1, 2, 3, 7, 32]
FIT_SHAPES = [(3000, 2, 2), (3000, 4, 3), (2000, 8, 2), (4000, 16, 2)]
FIT_TOLS = [1e-3, 1e-8]


def factors(weights, means, covs):
    """(a, means, precision) as stein_thinning.mixture.mixture_factors defines them, restated on np.linalg
    (slogdet for scipy's log-pseudo-determinant: equal to rounding for the positive definite covs here)."""
    w = np.asarray(weights, dtype=np.float64)
    mu = np.ascontiguousarray(means, dtype=np.float64)
    cv = np.asarray(covs, dtype=np.float64)
    d = mu.shape[1]
    sign, logdet = np.linalg.slogdet(cv)
    if np.any(sign <= 0):
        raise np.linalg.LinAlgError('covariance not positive definite')
    with np.errstate(divide='ignore'):
        a = np.log(w) - 0.5 * (d * np.log(2 * np.pi) + logdet)
    return a, mu, np.ascontiguousarray(np.linalg.inv(cv))


def stats(x, row_weights, fac, dtype=np.longdouble, want_bound=True):
    """One EM pass in ``dtype``: dict with LL, N (k,), S (k, d), Q (k, d, d), log_p (n,; NaN for the rows left
    out) and, with ``want_bound``, 'abs' and 'bound': dicts of the same four shapes holding each entry's sum of
    absolute terms and its rounding bound."""
    a64, mu64, p64 = fac
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    k = mu64.shape[0]
    om = np.ones(n) if row_weights is None else np.asarray(row_weights, dtype=np.float64)
    rows = om != 0
    comp = a64 != -np.inf
    xs, oms = x[rows].astype(dtype), om[rows].astype(dtype)
    a, mu, P = a64[comp].astype(dtype), mu64[comp].astype(dtype), p64[comp].astype(dtype)
    dev = xs[None, :, :] - mu[:, None, :]                                   # (k', n', d)
    y = np.einsum('cjk,cnk->cnj', P, dev)
    q = np.sum(dev * y, axis=-1)
    l = a[:, None] - q / 2                                                  # (k', n')
    m = np.max(l, axis=0)
    s = np.sum(np.exp(l - m), axis=0)
    log_p = m + np.log(s)
    r = np.exp(l - log_p)
    wr = oms * r
    out = {'LL': np.sum(oms * log_p)}
    N, S, Q = np.zeros(k, dtype), np.zeros((k, d), dtype), np.zeros((k, d, d), dtype)
    N[comp] = np.sum(wr, axis=1)
    S[comp] = np.einsum('cn,cni->ci', wr, dev)
    Q[comp] = np.einsum('cn,cni,cnj->cij', wr, dev, dev)
    Q = np.triu(Q) + np.triu(Q, 1).transpose(0, 2, 1)      # the record holds the upper triangle alone
    out.update(N=N, S=S, Q=Q)
    full = np.full(n, np.nan, dtype)
    full[rows] = log_p
    out['log_p'] = full
    if not want_bound:
        return out
    ad = np.abs(dev)
    qabs = np.einsum('cnj,cjk,cnk->cn', ad, np.abs(P), ad)
    dl = (2 * d + 3) * U * qabs / 2 + U * np.abs(l)
    dlp = np.sum(r * dl, axis=0) + U * np.sum(r * np.abs(l - m), axis=0) + (3 * k + 6) * U + U * np.abs(log_p)
    rho = dl + dlp + U * np.abs(l - log_p) + 2 * U                          # (k', n')
    chain = (-(-n // 64) + 100) * U
    def sums(v):   # sum_i v_ci |term factors|: the shapes of N, S, Q
        return (np.sum(v, axis=1), np.einsum('cn,cni->ci', v, ad), np.einsum('cn,cni,cnj->cij', v, ad, ad))
    ab = {'LL': np.sum(oms * np.abs(log_p)), 'N': np.zeros(k, dtype), 'S': np.zeros((k, d), dtype),
          'Q': np.zeros((k, d, d), dtype)}
    bd = {'LL': 2 * (np.sum(oms * dlp) + (chain + U) * ab['LL']), 'N': np.zeros(k, dtype),
          'S': np.zeros((k, d), dtype), 'Q': np.zeros((k, d, d), dtype)}
    for name, t_abs, t_err in zip(('N', 'S', 'Q'), sums(wr), sums(wr * (rho + 4 * U))):
        ab[name][comp] = t_abs
        bd[name][comp] = 2 * (t_err + chain * t_abs)
    out['abs'], out['bound'] = ab, bd
    return out


def check(got, want, what=''):
    """``got`` = (LL, N, S, Q) float64 against ``want = stats(...)``: every entry within its bound, the bound not
    vacuous.  Returns the worst error / bound ratio."""
    worst = 0.0
    for name, g in zip(('LL', 'N', 'S', 'Q'), got):
        g = np.asarray(g, dtype=np.longdouble)
        w, b, ab = want[name], want['bound'][name], want['abs'][name]
        assert np.all(b <= VACUOUS * ab), (what, name, 'vacuous bound', float(np.max(b / np.where(ab > 0, ab, 1))))
        err = np.abs(g - w)
        assert np.all(err <= b), (what, name, float(np.max(err)), float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), err))))
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1), 0)
        worst = max(worst, float(np.max(ratio)))
    return worst


def m_step(weight_sum, means, N, S, Q, reg_covar, dtype=np.float64):
    """N + 10 eps first; w = N / W, mu + S / N, Q / N - (S / N)(S / N)^T + reg_covar I; all in ``dtype``."""
    N = np.asarray(N, dtype=dtype) + 10 * np.finfo(np.float64).eps
    sn = np.asarray(S, dtype=dtype) / N[:, None]
    d = sn.shape[1]
    covs = np.asarray(Q, dtype=dtype) / N[:, None, None] - sn[:, :, None] * sn[:, None, :] + reg_covar * np.eye(d)
    return N / weight_sum, np.asarray(means, dtype=dtype) + sn, covs


def em(x, row_weights, weights, means, covs, tol=1e-3, max_iter=100, reg_covar=1e-6, dtype=np.float64,
       keep_path=False):
    """The EM loop of fit_mixture restated: dict with weights, means, covs (float64: the parameters the last
    ll was evaluated at), ll, n_iter, converged, history, margin = | |ll_t - ll_{t-1}| - tol | at the deciding
    evaluation (min over the evaluations that did not stop and the one that did) and, with ``keep_path``,
    the parameters of every evaluation.  The parameters pass through float64 between iterations (as they do
    on their way to the device); the statistics and the M-step run in ``dtype``."""
    x = np.asarray(x, dtype=np.float64)
    om = None if row_weights is None else np.asarray(row_weights, dtype=np.float64)
    W = float(x.shape[0]) if om is None else float(np.sum(om))
    weights, means, covs = (np.asarray(v, dtype=np.float64) for v in (weights, means, covs))
    history, path, margin, converged = [], [], np.inf, False
    for t in range(1, max_iter + 1):
        if keep_path:
            path.append((weights, means, covs))
        st = stats(x, om, factors(weights, means, covs), dtype, want_bound=False)
        history.append(float(st['LL'] / W))
        if t > 1:
            change = abs(history[-1] - history[-2])
            margin = min(margin, abs(change - tol))
            if change < tol:
                converged = True
                break
        if t == max_iter:
            break
        w, mu, cv = m_step(W, means, st['N'], st['S'], st['Q'], reg_covar, dtype)
        weights, means, covs = (np.asarray(v, dtype=np.float64) for v in (w, mu, cv))
    return dict(weights=weights, means=means, covs=covs, ll=history[-1], n_iter=len(history), converged=converged,
                history=history, margin=margin, path=path)


def inputs(n, d, k, weighted, centre=0.0):
    """Test inputs of the statistics: tests/mixture_ref.py's recipe (rows drawn from the mixture, spread 1.5)
    shifted by ``centre``, the parameters perturbed so that S_c is not near 0, and, ``weighted``, row weights
    from {0, 0.5, 1, 2, 3.25} (a fifth of them 0; never all)."""
    from tests import mixture_ref as M
    rng, weights, means, covs = M.parameters(d, k)
    x = M.rows(rng, n, weights, means, covs) + centre
    means = means + 0.1 * rng.normal(size=means.shape) + centre
    om = None
    if weighted:
        om = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 3.25]), size=n)
        om[0] = 1.0
    return x, om, weights, means, covs


@functools.lru_cache(maxsize=None)
def planted(n, d, k, seed=0):
    """A planted, well separated mixture and a rough start: (x, weights0, means0, covs0), read-only.  Component
    c = 0, 1, ... sits at 3 (c + 1) e_(c mod d) + N(0, 1) offsets, covariances A A^T / d + 0.5 I; the start is the true means
    moved by N(0, 0.7^2), the sample covariance and uniform weights."""
    rng = np.random.default_rng(1000 * d + 10 * k + seed)
    a = rng.normal(size=(k, d, d))
    covs = a @ a.transpose(0, 2, 1) / d + 0.5 * np.eye(d)
    means = rng.normal(size=(k, d))
    for c in range(k):
        means[c, c % d] += 3.0 * (c + 1)
    w = rng.dirichlet(np.full(k, 5.0))
    comp = rng.choice(k, size=n, p=w)
    chol = np.linalg.cholesky(covs)
    x = means[comp] + np.einsum('nij,nj->ni', chol[comp], rng.normal(size=(n, d)))
    means0 = means + 0.7 * rng.normal(size=(k, d))
    c = np.atleast_2d(np.cov(x, rowvar=False, bias=True))
    covs0 = np.repeat(c[None], k, axis=0)
    out = (x, np.full(k, 1.0 / k), means0, covs0)
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def planted_em(n, d, k, tol):
    """The float64 restatement's run on planted(n, d, k), computed once; asserts that its stopping decision is
    not marginal (| |dll| - tol | > 1 % of tol at every evaluation), so an equal n_iter can be demanded."""
    x, w0, m0, c0 = planted(n, d, k)
    run = em(x, None, w0, m0, c0, tol=tol, max_iter=200, keep_path=True)
    assert run['converged'] and run['margin'] > 0.01 * tol, (n, d, k, tol, run['n_iter'], run['margin'])
    return run


def spread(a, b):
    """The largest difference of two runs: ll absolute; weights, means, covs relative to max |value|."""
    out = abs(a['ll'] - b['ll'])
    for name in ('weights', 'means', 'covs'):
        out = max(out, float(np.max(np.abs(a[name] - b[name])) / np.max(np.abs(b[name]))))
    return out
