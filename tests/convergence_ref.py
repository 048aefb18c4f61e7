"""Oracle of stein_thinning.convergence: a NumPy restatement of the definitions of DESIGN.md section 20
(Vehtari et al. 2021), with the autocovariances summed directly in np.longdouble, scipy's average ranks, the
inverse normal cdf from mpmath at 40 digits, and the error bounds the GPU tests accept within.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u)); every one is derived from the kernels' summation plans
(csrc/convergence.hip), none is fitted:
* a series mean is m0 + mean(a - m0) with both sums of depth <= DM = ceil(h / 64) + 10, so
  |mu_dev - mu| <= delta = u |mu| + gamma_{DM + 2} (mean|a - mu| + gamma_DM mean|a|);
* a centred value carries eta_i = e_i + mean(e) + delta + u |a_i - mu| (e_i: what the input itself may be off
  by, e.g. the z of a rank);
* a lag sum of h - t products has depth <= D = max(h, 256 + ceil(h / 2048) + 74) + 2 on either plan, so
  |acov_dev - acov| <= [sum(|c_i| eta_{i+t} + eta_i |c_{i+t}| + eta_i eta_{i+t})
                        + gamma_D sum (|c_i| + eta_i)(|c_{i+t}| + eta_{i+t})] / h + u |acov|;
* the mean over S series adds gamma_{min(S, 256) + ceil(S / 256) + 1} mean_s |acov_s|.
These propagate through rho, tau, B and W to first order with the rounding of the host's own float64 steps.
"""
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# scipy.special.ndtri's worst error against mpmath over every rank r = 1 .. N of N = 2^20 + 3,
# p = (r - 0.375) / (N + 0.25), in ulps of the mpmath value (measured on the CPU)
E_NDTRI_ULP = 4.53
Z_TOL_ULP = max(4.0, 2.0 * E_NDTRI_ULP)

# (C, n, phi), seed: the shared case list
CASES = [
    ((1, 8, 0.0), 11),
    ((3, 9, 0.5), 12),
    ((4, 257, 0.5), 13),
    ((2, 1000, 0.9), 14),
    ((4, 4099, 0.99), 15),
    ((5, 2048, 0.999), 16),
    ((2049, 16, 0.3), 17),
]
QUANTITIES = ('mean', 'sd', 'bulk', 'tail05', 'tail95', 'fold')


def gamma(k):
    return k * U / (1 - k * U)


def ar1(C, n, phi, seed):
    """(C, n) AR(1) chains with unit innovations, started from the stationary law."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((C, n))
    x = np.empty((C, n))
    x[:, 0] = e[:, 0] / math.sqrt(1 - phi * phi) if phi < 1 else e[:, 0]
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


def case_column(k):
    (C, n, phi), seed = CASES[k]
    return ar1(C, n, phi, seed)


def stack_columns():
    """(4, 257, 5): five AR(1) columns of one shape, phi of five of the shared cases."""
    return np.stack([ar1(4, 257, phi, 100 + j) for j, phi in enumerate((0.0, 0.5, 0.9, 0.99, 0.999))], axis=2)


def ties_column():
    """(4, 2000): an AR(1) phi = 0.9 chain whose rows repeat a geometric number of times (>= 60 % ties)."""
    rng = np.random.default_rng(21)
    base = ar1(4, 2000, 0.9, 22)
    out = np.empty((4, 2000))
    for c in range(4):
        reps = rng.geometric(0.3, size=2000)
        out[c] = np.repeat(base[c], reps)[:2000]
    assert np.mean(out[:, 1:] == out[:, :-1]) >= 0.6
    return out


def shifted_column():
    x = ar1(4, 500, 0.3, 23)
    x[0] += 3 * x.std(ddof=1)
    return x


def split(a):
    n = a.shape[1]
    h = n // 2
    return np.concatenate([a[:, :h], a[:, n - h:]], axis=0)


def rank_p(b):
    """fp64 p of every entry of b, ranked over all entries at once (ties: the mean rank)."""
    from scipy.stats import rankdata
    r = rankdata(b.reshape(-1), method='average')
    return ((r - 0.375) / (b.size + 0.25)).reshape(b.shape)


_Z_CACHE = {}


def z_mp(p):
    """float64 rounding of the 40-digit inverse normal cdf at the fp64 p: one Newton step on mpmath's ncdf
    from scipy's ndtri (whose 1e-15 error the step squares)."""
    import mpmath
    from scipy.special import ndtri
    flat = np.asarray(p, dtype=np.float64).reshape(-1)
    uniq = np.unique(flat)
    with mpmath.workdps(40):
        for v, z0 in zip(uniq, ndtri(uniq)):
            if v not in _Z_CACHE:
                z = mpmath.mpf(float(z0))
                z = z - (mpmath.ncdf(z) - mpmath.mpf(float(v))) / mpmath.npdf(z)
                _Z_CACHE[v] = float(z)
    return np.array([_Z_CACHE[v] for v in flat]).reshape(np.shape(p))


def z_of(b):
    return z_mp(rank_p(b))


def z_input_error(z):
    """What a device z may be off by: Z_TOL_ULP ulps, plus the half ulp of rounding the mpmath value."""
    return (Z_TOL_ULP + 0.5) * np.spacing(np.abs(z))


def acov_ld(b, lag0=0, lag1=None):
    """(S, lag1 - lag0) biased centred autocovariances by the direct sum in long double."""
    S, h = b.shape
    lag1 = h if lag1 is None else lag1
    c = b.astype(LD) - b.astype(LD).mean(axis=1, keepdims=True)
    out = np.empty((S, lag1 - lag0), dtype=LD)
    for t in range(lag0, lag1):
        out[:, t - lag0] = (c[:, :h - t] * c[:, t:]).sum(axis=1) / h
    return out


def acov_fft64(b):
    """(S, h) the same autocovariances the way users of the reference get them: float64, zero-padded FFT."""
    S, h = b.shape
    c = b - b.mean(axis=1, keepdims=True)
    nfft = 2 ** int(math.ceil(math.log2(2 * h)))
    f = np.fft.rfft(c, nfft, axis=1)
    return np.fft.irfft(f * np.conj(f), nfft, axis=1)[:, :h] / h


def mean_depth(h):
    return -(-h // 64) + 10


def sum_depth(h):
    return max(h, 256 + -(-h // 2048) + 74) + 2


def mean_bound(b):
    """(S,) bound on |mu_dev - mu| of every series (no input error)."""
    h = b.shape[1]
    bl = b.astype(LD)
    mu = bl.mean(axis=1)
    dm = mean_depth(h)
    return U * np.abs(mu) + gamma(dm + 2) * (np.abs(bl - mu[:, None]).mean(axis=1) +
                                             gamma(dm) * np.abs(bl).mean(axis=1))


def acov_bound(b, lag0=0, lag1=None, e=None):
    """(S, lag1 - lag0) bound on |acov_dev - acov_ld| per element; e: (S, h) what each input may be off by."""
    S, h = b.shape
    lag1 = h if lag1 is None else lag1
    bl = b.astype(LD)
    mu = bl.mean(axis=1, keepdims=True)
    A = np.abs(bl - mu)
    e = np.zeros((S, h), dtype=LD) if e is None else np.asarray(e, dtype=LD)
    delta = mean_bound(b)[:, None] + e.mean(axis=1, keepdims=True)
    eta = (e + delta) * (1 + U) + U * A
    g = gamma(sum_depth(h))
    P = A + eta
    out = np.empty((S, lag1 - lag0), dtype=LD)
    for t in range(lag0, lag1):
        k = h - t
        pert = (A[:, :k] * eta[:, t:] + eta[:, :k] * A[:, t:] + eta[:, :k] * eta[:, t:]).sum(axis=1)
        mag = (P[:, :k] * P[:, t:]).sum(axis=1)
        exact = np.abs(((bl - mu)[:, :k] * (bl - mu)[:, t:]).sum(axis=1)) / h
        out[:, t - lag0] = (pert + g * mag) / h * (1 + 2 * U) + U * exact
    return out


def series_depth(S):
    return min(S, 256) + -(-S // 256) + 1


def acov_mean_bound(acs, bounds):
    """Bound on the chain-averaged values from the per-series values and bounds."""
    S = acs.shape[0]
    return bounds.mean(axis=0) + gamma(series_depth(S)) * (np.abs(acs) + bounds).mean(axis=0)


def geyer(ac, S, h, var_mu, eps_rho=None):
    """(ess, max_t, tau, rho, worst): the definition's Geyer passes in ac's dtype.  worst: the smallest
    margin / bound over every comparison made (rho_even + rho_odd against 0, the last rho_even against 0, each
    monotone comparison), bound taken from eps_rho (per-lag bound on rho); inf without eps_rho."""
    one = ac.dtype.type(1.0)
    mean_var = ac[0] * h / (h - 1)
    var_plus = mean_var * (h - 1) / h
    if S > 1:
        var_plus = var_plus + var_mu
    worst = np.inf
    er = (lambda *ts: sum(float(eps_rho[t]) for t in ts)) if eps_rho is not None else None

    def see(margin, *ts):
        nonlocal worst
        if er is not None:
            b = er(*ts)
            worst = min(worst, float(abs(margin)) / b if b > 0 else np.inf)

    rho = np.zeros(h, dtype=ac.dtype)
    rho_even = one
    rho[0] = rho_even
    rho_odd = 1 - (mean_var - ac[1]) / var_plus
    rho[1] = rho_odd
    t = 1
    while t < h - 3:
        see(rho_even + rho_odd, t - 1, t)
        if not rho_even + rho_odd > 0:
            break
        rho_even = 1 - (mean_var - ac[t + 1]) / var_plus
        rho_odd = 1 - (mean_var - ac[t + 2]) / var_plus
        if rho_even + rho_odd >= 0:
            rho[t + 1] = rho_even
            rho[t + 2] = rho_odd
        t += 2
    if t >= 3:
        see(rho_even + rho_odd, t - 1, t)      # the store test of the last pair taken
    max_t = t - 2
    see(rho_even, max(t - 1, 0))
    if rho_even > 0:
        rho[max_t + 1] = rho_even
    t = 1
    while t <= max_t - 2:
        see((rho[t + 1] + rho[t + 2]) - (rho[t - 1] + rho[t]), t - 1, t, t + 1, t + 2)
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2
            rho[t + 2] = rho[t + 1]
        t += 2
    tau = -1 + 2 * np.sum(rho[:max_t + 1]) + rho[max_t + 1]
    tau = max(tau, 1 / np.log10(ac.dtype.type(S * h)))
    return S * h / tau, max_t, tau, rho, worst


def ess_of(b, e=None, acov=None):
    """dict(ess, bound, worst, max_t, rhat, rhat_bound) of a (S, h) series; e: its input error; acov: another
    autocovariance routine (acov_fft64) in place of the long-double sum (then no bounds)."""
    S, h = b.shape
    bl = b.astype(LD)
    if float(bl.max() - bl.min()) < 1e-15:
        return dict(ess=float(S * h), bound=0.0, worst=np.inf, max_t=-1, rhat=np.nan, rhat_bound=np.nan)
    if acov is not None:
        acs = acov(b)
        mu = b.mean(axis=1)
        var_mu = np.var(mu, ddof=1) if S > 1 else 0.0
        ess, max_t, _, _, _ = geyer(acs.mean(axis=0), S, h, var_mu)
        return dict(ess=float(ess), max_t=max_t)
    return _ess_of_lags(b, e, min(h, 64))


def _ess_of_lags(b, e, K):
    """ess_of from the first K lags; doubles K until the positive sequence has ended inside them."""
    S, h = b.shape
    bl = b.astype(LD)
    acs = acov_ld(b, 0, K)
    bnd = acov_bound(b, 0, K, e=e)
    ac = acs.mean(axis=0)
    eps_ac = acov_mean_bound(acs, bnd)
    mu = bl.mean(axis=1)
    e_mean = np.zeros(S, dtype=LD) if e is None else np.asarray(e, dtype=LD).mean(axis=1)
    dmu = mean_bound(b) + e_mean
    if S > 1:
        var_mu = np.var(mu, ddof=1)
        eps_vm = (2 * np.abs(mu - mu.mean()) * 2 * dmu).sum() / (S - 1) + (4 * dmu * dmu).sum() / (S - 1) \
            + (S + 8) * U * var_mu
    else:
        var_mu, eps_vm = LD(0), LD(0)
    mv = ac[0] * h / (h - 1)
    vp = mv * (h - 1) / h + var_mu
    eps_mv = eps_ac[0] * h / (h - 1) + 2 * U * mv
    eps_vp = eps_ac[0] + eps_vm + 4 * U * vp
    rho_raw = 1 - (mv - ac) / vp
    eps_rho = (eps_mv + eps_ac) / vp + np.abs(mv - ac) / (vp * vp) * eps_vp + 4 * U * (1 + np.abs(rho_raw))
    eps_rho = eps_rho * (1 + 1e-6)
    try:
        ess, max_t, tau, rho, worst = geyer(ac, S, h, var_mu, eps_rho)
    except IndexError:
        return _ess_of_lags(b, e, min(h, 2 * K))
    k = max_t + 2
    eps_tau = 2 * eps_rho[:k].sum() + gamma(k + 4) * (1 + 2 * np.abs(rho[:k]).sum())
    bound = float(ess * (eps_tau / tau) * (1 + 1e-6) + 4 * U * ess)
    # rhat: B = h var(mu), W = mean var_s (ddof = 1)
    W = (acs[:, 0] * h / (h - 1)).mean()
    eps_W = (bnd[:, 0] * h / (h - 1)).mean() + (S + 8) * U * W
    B = h * var_mu
    r2 = (B / W + h - 1) / h
    eps_r2 = (h * eps_vm / W + B * eps_W / (W * W)) / h + 4 * U * r2
    rhat = np.sqrt(r2)
    return dict(ess=float(ess), bound=bound, worst=float(worst), max_t=max_t, rhat=float(rhat),
                rhat_bound=float(eps_r2 / (2 * rhat) + 2 * U * rhat))


def quantity_series(a):
    """The six (2C, h) float64 series of a (C, n) column and what each input may be off by on the device."""
    al = a.astype(LD)
    C, n = a.shape
    sp = split(a)
    m = np.mean(a)
    # the device forms (a - m_dev)^2 with its own mean: m_dev - m within the mean bound of the chains + np.mean's
    dm = float(mean_bound(a).mean() + (C + 2) * U * abs(al.mean()) + 140 * U * np.abs(al).mean())
    sq = (sp - m) ** 2
    e_sq = 2 * np.abs(sp - m) * dm + dm * dm + 4 * U * sq
    zb = z_of(sp)
    q05, q95 = np.quantile(a, 0.05), np.quantile(a, 0.95)
    zf = z_of(np.abs(sp - np.median(a)))
    return {
        'mean': (sp, None),
        'sd': (sq, e_sq),
        'bulk': (zb, z_input_error(zb)),
        'tail05': ((sp <= q05).astype(np.float64), None),
        'tail95': ((sp <= q95).astype(np.float64), None),
        'fold': (zf, z_input_error(zf)),
    }


def _nan_summary():
    return {k: (np.nan, np.nan) for k in ('mean', 'sd', 'mcse_mean', 'mcse_sd', 'ess_bulk', 'ess_tail', 'r_hat')}


def summary_column(a, acov=None):
    """{column: (value, bound)} of one (C, n) column, and under 'worst' the smallest decision margin / bound of
    each quantity.  acov: see ess_of (values only)."""
    if not np.all(np.isfinite(a)):
        return _nan_summary()
    C, n = a.shape
    N = C * n
    al = a.astype(LD)
    q = quantity_series(a)
    res = {k: ess_of(b, e, acov) for k, (b, e) in q.items() if acov is None or k not in ('fold',)}
    if acov is not None:
        return {'ess_mean': res['mean']['ess'], 'ess_sd': min(res['mean']['ess'], res['sd']['ess']),
                'ess_bulk': res['bulk']['ess'], 'ess_tail': min(res['tail05']['ess'], res['tail95']['ess'])}
    mean = al.mean()
    sd = np.sqrt(((al - mean) ** 2).sum() / (N - 1))
    # device: mean of the chains' means; SS = sum n v0_c + n sum (mu_c - mean)^2
    dmu = mean_bound(a)
    eps_mean = float(dmu.mean() + (C + 2) * U * abs(mean))
    mu_c = al.mean(axis=1)
    v0b = acov_bound(a, 0, 1)[:, 0]
    SS = ((al - mean) ** 2).sum()
    eps_SS = n * v0b.sum() + n * (2 * np.abs(mu_c - mean) * (dmu + eps_mean)).sum() \
        + n * ((dmu + eps_mean) ** 2).sum() + (2 * C + 8) * U * SS
    eps_sd = float(eps_SS / (2 * sd * (N - 1)) + 2 * U * sd) if sd > 0 else 0.0
    out = {'mean': (float(mean), eps_mean), 'sd': (float(sd), eps_sd)}

    def pick(names, op):
        vals = [res[k]['ess'] for k in names]
        return op(vals), max(res[k]['bound'] for k in names)
    ess_mean = (res['mean']['ess'], res['mean']['bound'])
    ess_sd = pick(('mean', 'sd'), min)
    out['ess_bulk'] = (res['bulk']['ess'], res['bulk']['bound'])
    out['ess_tail'] = pick(('tail05', 'tail95'), min)
    out['ess_mean'], out['ess_sd'] = ess_mean, ess_sd
    rb, rf = res['bulk'], res['fold']
    if np.isnan(rb['rhat']) or np.isnan(rf['rhat']):
        out['r_hat'] = (np.nan, np.nan)
    else:
        out['r_hat'] = (max(rb['rhat'], rf['rhat']), max(rb['rhat_bound'], rf['rhat_bound']))
    with np.errstate(all='ignore'):
        sdl = LD(sd)
        e1, b1 = LD(ess_mean[0]), ess_mean[1]
        v = sdl / np.sqrt(e1)
        out['mcse_mean'] = (float(v), float(v * (eps_sd / sd + 0.5 * b1 / e1 + 4 * U)) if sd > 0 else 0.0)
        e2, b2 = LD(ess_sd[0]), LD(ess_sd[1])

        def g(x):
            return np.expm1(1 + (x - 1) * np.log1p(-1 / x))     # e (1 - 1/x)^(x - 1) - 1 without its cancellation
        g0 = g(e2)
        # the host's float64 steps: (x - 1) log1p(-1 / x) is about -1 and carries 5 u, the sum with 1 one more,
        # expm1 two ulps of its value
        eps_g = max(abs(g(e2 + b2) - g0), abs(g(e2 - b2) - g0)) + 8 * U + 4 * U * g0
        v = sdl * np.sqrt(g0)
        out['mcse_sd'] = (float(v), float(eps_sd * np.sqrt(g0) + sdl * eps_g / (2 * np.sqrt(g0)) + 4 * U * v)
                          if sd > 0 else 0.0)
    out['worst'] = {k: r['worst'] for k, r in res.items()}
    out['max_t'] = {k: r['max_t'] for k, r in res.items()}
    return out


@functools.lru_cache(maxsize=None)
def case_summary(k):
    """summary_column of shared case k, computed once per process."""
    return summary_column(case_column(k))
