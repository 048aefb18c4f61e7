"""CPU references of the Student-t kernel density proxy (csrc/kde.hip: st_kde_t_logpdf_grad), shared by
test_kde_t_cpu.py and test_gpu_kde_t.py.  No GPU needed here (gm_thin_case alone imports the package); np.longdouble is the yardstick
(dense_ref.longdouble_ok).  Inputs come from side_ref.kde_case (coincident, near and far queries, weights
over 300 orders of magnitude, exact zeros, a whole zero-weight staging tile).

At the ABI's level: whitened p (n, d), q (m, d), logw (n), df = nu, log_norm (= log_norm_t), lower L.  With
h = (nu + d) / 2 and r2_ij = |p_i - q_j|^2, ``tkde_ld`` evaluates in long double

    a_ij = logw_i + log_norm - h log1p(r2_ij / nu),   log q_j = logsumexp_i a_ij,   s_ij = exp(a_ij - log q_j),
    g_ijl = (nu + d) / (nu + r2_ij) (p_il - q_jl),    v_jl = sum_i s_ij g_ijl,      grad_j = v_j L^T.

The kernel's order (``tkde_emulate`` restates it in float64; the kernel forms r2 with fma, the restatement
without, NumPy's exp / log / sqrt in place of the device's): r2 sequentially over the coordinates; r2min_j the
smallest r2 over the points of non-zero weight, lwmax the largest log weight; per pair den = nu + r2, rinv =
1 / den, rho = min((nu + r2min) rinv, 1), rho^h by a square-and-multiply chain (times sqrt(rho) for odd nu + d) when
nu + d is an integer <= 256 and exp(h log(rho)) otherwise, t = exp(logw_i - lwmax) rho^h; s = sum t and sm_l =
sum (t rinv) (p_il - q_jl) sequentially in i; log q = log(s) + (lwmax + (log_norm - h log1p(r2min / nu))), v =
((nu + d) / s) sm, grad by a sequential dot product with L's rows.

Bound, u = 2^-53.  Over the points that matter, P_j = {i: s_ij >= 2^-53}, and the nearest weighted point:

    X_ij = r2_ij / (nu + r2_ij),  Xmin_j the same for r2min_j       (how much of den is the computed r2)
    E_j  = max_{P_j} h log((nu + r2_ij) / (nu + r2min_j))            (the shifted exponent)
    W_j  = max_{P_j} (lwmax - logw_i),   M_j = h log1p(r2min_j / nu),   S_j = |log(sum_i t_ij)|

* r2: a sum of d non-negative terms, (d + 2) u relative (side_ref's argument).  den = nu + r2 is then off by
  ((d + 2) X + 1) u, the reciprocal is budgeted 2 u, the product with nu + r2min (itself ((d + 2) Xmin + 1) u)
  1 u:  eps_rho_ij = ((d + 2) (X_ij + Xmin_j) + 5) u -- the division by nu never happens per pair.
* the power multiplies that by h and adds its own roundings: at most 16 multiplications and a square root on
  the chain (h <= 128), or the log's ulp and the product's rounding on an exponent of size E_j and exp's ulp
  on the other path: budget (18 + 3 E_j) u for both.
* the weight factor exp(logw_i - lwmax): the subtraction's rounding enters as W_j u, exp and the product with
  the power 3 u.  Together, per term,

      eps_t_j = max_{P_j} h ((d + 2) (X_ij + Xmin_j) + 5) + 21 + 3 E_j + W_j            (units of u)

* the n-term sequential sum of non-negative terms: n u.  log(s): 2 u S_j.
* the shift put back: r2min / nu ((d + 3) u relative: h Xmin_j (d + 3) u on the result), log1p and the
  product with h (3 u M_j), and the two additions of log_norm and lwmax (each one rounding of a result no
  larger than the sum of the magnitudes); the last addition sits in the 2^-52 |ref| term:

      tau_j = u (n + eps_t_j + 2 S_j + h Xmin_j (d + 3) + 3 M_j + 2 (|lwmax| + |log_norm| + M_j))
      |log q_j - ref_j| <= tau_j + 2^-52 |ref_j|

* gradient: every error above is a relative perturbation of a term.  Those of t_ij are common to s and sm and
  reach the softmax mean v only through the spread MAD_jl = sum_i s_ij |g_ijl - v_jl|; those of the factor
  rinv (p - q) ((d + 2) + 2 + 1 + 1 + 2 roundings: (d + 8) u) and of the two sequential sums (n u each) do not
  cancel and scale with G_jl = sum_i s_ij |g_ijl| and |v_jl|; two more roundings for (nu + d) / s and its
  product.  Then the d-term product with L as in side_ref:

      tol_v_jl    = u (eps_t_j MAD_jl + (n + d + 8) G_jl + (n + 2) |v_jl|)
      tol_grad_jk = sum_l |L_kl| tol_v_jl + (d + 1) u sum_l |L_kl| |v_jl|

(points outside P_j carry less than u of the weight each: their own, larger, exponents enter at second order.)
The bound assumes the kernel's domain: non-zero weights within a ratio of 2^900 (``in_domain``).
"""
import numpy as np

U = 2.0 ** -53
MAX_INT_POWER = 256      # csrc/kde.hip kKdeTMaxIntPower
TKDE_DIMS_CPU = [1, 2, 4, 8, 9, 17]
TKDE_DIMS_GPU = [1, 2, 3, 4, 8, 9, 17]
TKDE_DFS = [1.0, 3.0, 2.5, 1e5]


def in_domain(logw):
    """The kernel's stated domain: the non-zero weights span a ratio of at most 2^900."""
    lw = np.asarray(logw, dtype=np.float64)
    lw = lw[np.isfinite(lw)]
    return lw.size == 0 or float(lw.max() - lw.min()) <= 900 * np.log(2.0)


def _r2_ld(p, q):
    ld = np.longdouble
    pl, ql = p.astype(ld), q.astype(ld)
    r2 = np.zeros((q.shape[0], p.shape[0]), dtype=ld)
    for k in range(p.shape[1]):
        dk = pl[None, :, k] - ql[:, k, None]
        r2 += dk * dk
    return r2


def unshifted_exponents(p, q, df):
    """h log1p(r2_ij / nu), (m, n) float64: what exp would see without the shift (weights aside)."""
    d = p.shape[1]
    return (np.longdouble(0.5 * (df + d)) * np.log1p(_r2_ld(p, q) / np.longdouble(df))).astype(np.float64)


def tkde_ld(p, q, logw, df, log_norm, L):
    """Long-double log q (m), grad (m, d) and the tolerances of the module docstring: a dict with logq,
    grad, tol_logq, tol_grad (long double) and eps_t (float64).  Needs at least one finite logw."""
    ld = np.longdouble
    n, d = p.shape
    pl, ql, Ll = p.astype(ld), q.astype(ld), np.asarray(L).astype(ld)
    lw = np.asarray(logw, dtype=np.float64).astype(ld)
    nu, h = ld(df), ld(0.5) * (ld(df) + d)
    r2 = _r2_ld(p, q)
    arg = lw[None, :] + (ld(log_norm) - h * np.log1p(r2 / nu))
    mx = np.max(arg, axis=1)
    t = np.exp(arg - mx[:, None])
    tot = np.sum(t, axis=1)
    logq = mx + np.log(tot)
    s = t / tot[:, None]
    coef = (nu + d) / (nu + r2)
    v = np.empty((q.shape[0], d), dtype=ld)
    mad = np.empty_like(v)
    gabs = np.empty_like(v)
    for l in range(d):
        g = coef * (pl[None, :, l] - ql[:, l, None])
        v[:, l] = np.sum(s * g, axis=1)
        mad[:, l] = np.sum(s * np.abs(g - v[:, l, None]), axis=1)
        gabs[:, l] = np.sum(s * np.abs(g), axis=1)
    # the quantities of the bound
    weighted = np.isfinite(lw)
    lwmax = np.max(lw[weighted])
    r2min = np.min(np.where(weighted[None, :], r2, ld(np.inf)), axis=1)
    carry = s >= ld(U)
    X = r2 / (nu + r2)
    Xmin = r2min / (nu + r2min)
    zero = ld(0)
    Xmax = np.max(np.where(carry, X, zero), axis=1)
    E = np.max(np.where(carry, h * np.log((nu + r2) / (nu + r2min)[:, None]), zero), axis=1)
    with np.errstate(invalid='ignore'):
        W = np.max(np.where(carry, (lwmax - lw)[None, :], zero), axis=1)
    M = h * np.log1p(r2min / nu)
    # log of the kernel's sum: log q minus the shift put back
    S = np.abs(logq - (lwmax + ld(log_norm) - M))
    u = ld(U)
    eps_t = h * ((d + 2) * (Xmax + Xmin) + 5) + 21 + 3 * E + W
    tau = u * (n + eps_t + 2 * S + h * Xmin * (d + 3) + 3 * M + 2 * (abs(lwmax) + abs(ld(log_norm)) + M))
    absL = np.abs(Ll)
    tol_v = u * (eps_t[:, None] * mad + (n + d + 8) * gabs + (n + 2) * np.abs(v))
    return dict(logq=logq, grad=v @ Ll.T, tol_logq=tau + 2 * u * np.abs(logq),
                tol_grad=tol_v @ absL.T + (d + 1) * u * (np.abs(v) @ absL.T), eps_t=eps_t.astype(np.float64))


def integer_path(df, d):
    """The kernel's rule for the multiplication chain: nu + d an integer of at most MAX_INT_POWER."""
    two_h = df + d
    return two_h == np.floor(two_h) and two_h <= MAX_INT_POWER


RT_TILE = 32            # csrc/kde.hip kKdeRowsRt: the runtime-d kernel pads its last tile to this many rows


def tkde_emulate(p, q, logw, df, log_norm, L, wrong=None):
    """Float64 restatement of kde_t_kernel's order (module docstring); returns (logq (m), grad (m, d)).
    Rows of zero weight are not skipped: as in the kernel they sit at the origin with the factor 0, and for
    d > 8 the last tile is padded with such rows up to a multiple of RT_TILE; rho is clamped to 1.
    ``wrong`` plants one deliberate mistake for the tests of the bound's teeth: 'h' raises to nu / 2 in
    place of (nu + d) / 2, 'coef' drops the 1 / (1 + r2 / nu) factor of the gradient coefficient,
    'unshifted' sums w_i (1 + r2 / nu)^-h with no shift, 'unclamped' leaves rho above 1 for a zero-weight or
    padding row that lies closer to the query than every weighted point."""
    assert wrong in (None, 'h', 'coef', 'unshifted', 'unclamped')
    m, d = q.shape
    n = p.shape[0]
    lw = np.asarray(logw, dtype=np.float64)
    nu = float(df)
    two_h = nu + d
    h = 0.5 * two_h
    integer = integer_path(nu, d) and wrong in (None, 'unclamped')
    hp = 0.5 * nu if wrong == 'h' else h
    weighted = lw != -np.inf
    npad = n if d <= 8 else -(-n // RT_TILE) * RT_TILE
    rows = np.zeros((npad, d))
    rows[:n][weighted] = p[weighted]                  # zero-weight and padding rows: the origin
    wfac = np.zeros(npad)
    lwmax = np.max(lw)
    if wrong == 'unshifted':
        lwmax = 0.0
    lwshift = 0.0 if lwmax == -np.inf else lwmax
    with np.errstate(under='ignore'):
        wfac[:n][weighted] = np.exp(lw[weighted] - lwshift)
    ss = np.zeros((m, npad))
    for k in range(d):
        dk = rows[None, :, k] - q[:, k, None]
        ss = ss + dk * dk
    keep = np.zeros(npad, dtype=bool)
    keep[:n] = weighted
    r2min = np.min(np.where(keep[None, :], ss, np.inf), axis=1)
    if wrong == 'unshifted':
        r2min = np.zeros(m)
    r2min = np.where(np.isinf(r2min), 0.0, r2min)
    dmin = nu + r2min
    s = np.zeros(m)
    sm = np.zeros((m, d))
    with np.errstate(under='ignore', over='ignore', divide='ignore', invalid='ignore'):
        for i in range(npad):
            den = nu + ss[:, i]
            rinv = 1.0 / den
            rho = dmin * rinv
            if wrong != 'unclamped':
                rho = np.minimum(rho, 1.0)
            if integer:
                b = rho.copy()
                e = int(two_h) // 2
                while not e & 1:
                    b = b * b
                    e >>= 1
                pw = np.sqrt(rho) * b if int(two_h) % 2 else b
                e >>= 1
                while e:
                    b = b * b
                    if e & 1:
                        pw = pw * b
                    e >>= 1
            else:
                pw = np.exp(hp * np.log(rho))
            t = wfac[i] * pw
            s = s + t
            tc = t * (1.0 / nu if wrong == 'coef' else rinv)
            sm = sm + tc[:, None] * (rows[i][None, :] - q)
        logq = np.log(s) + (lwshift + (log_norm - hp * np.log1p(r2min / nu)))
        v = ((2.0 * h) / s)[:, None] * sm
    grad = np.zeros((m, d))
    for l in range(d):
        grad = grad + v[:, l, None] * L[None, :, l]
    return logq, grad


def offset_case(n, m, d, zero_weights, seed=17):
    """Whitened inputs whose data sit far from the origin (N(0, 1) + 50 in every coordinate) with queries at
    and near the origin (rows 0 and 1), at data rows and near them: a zero-weight row (moved to the origin by
    the kernel) or a padding row of the runtime-d kernel is then much closer to queries 0 and 1 than every
    weighted point, r2 << r2min.  ``zero_weights``: every fifth weight exactly 0, else none.  Same keys as
    side_ref.kde_case; L a well-conditioned lower factor, log_norm left to the caller (log_norm_t)."""
    rng = np.random.default_rng([seed, n, m, d])
    p = rng.normal(size=(n, d)) + 50.0
    q = p[np.arange(m) % n] + 0.5 * rng.normal(size=(m, d))
    q[0] = 0.0
    if m > 1:
        q[1] = 0.01 * rng.normal(size=d)
    w = rng.uniform(0.1, 1.0, size=n)
    if zero_weights:
        w[4::5] = 0.0
    with np.errstate(divide='ignore'):
        logw = np.log(w / np.sum(w))
    L = np.tril(0.1 * rng.normal(size=(d, d))) + np.diag(rng.uniform(0.5, 2.0, size=d))
    return dict(n=n, m=m, d=d, p=p, q=q, w=w, logw=logw, L=L)


# (n, d, zero weights): d <= 8 needs a zero weight; d >= 9 with n % 32 != 0 has padding rows on every call
OFFSET_CASES = [(33, 4, True), (257, 8, True), (33, 9, False), (257, 17, True)]


def gm_thin_case(df=4.0):
    """The Gaussian-mixture fixture (n = 1000, d = 2) as kde_t_thin sees it: sample, log_p and the ABI-level
    inputs of its Student-t kernel density (uniform weights, Silverman bandwidth)."""
    from oracle import models
    from stein_thinning import proxy
    sample, _, logpdf, _ = models.gm_reference_sample(1000)
    w, L, log_norm = proxy.kde_t_factors(sample, df)
    return sample, logpdf(sample), sample @ L, np.log(w), log_norm, L


def ratios(lq, g, r):
    """(worst |log q error| / bound, worst |gradient error| / bound); non-finite results count as inf."""
    el, eg = np.abs(lq - r['logq']), np.abs(g - r['grad'])
    with np.errstate(invalid='ignore', divide='ignore'):
        rl = np.where(el == 0, 0.0, el / r['tol_logq'])        # an exact result meets a zero bound
        rg = np.where(eg == 0, 0.0, eg / r['tol_grad'])
    rl = np.where(np.isfinite(lq), rl, np.inf)
    rg = np.where(np.isfinite(g), rg, np.inf)
    return float(np.max(rl)), float(np.max(rg))


def log_norm_t(L, df):
    """sum(log diag L) + lgamma((nu + d) / 2) - lgamma(nu / 2) - d / 2 log(nu pi)   (float64, as the host)."""
    from scipy.special import gammaln
    d = L.shape[0]
    return float(np.sum(np.log(np.diag(L))) + gammaln(0.5 * (df + d)) - gammaln(0.5 * df) - 0.5 * d * np.log(df * np.pi))


def rw_sample(n=600, d=2, seed=11, accept=0.25):
    """An RW-chain-like sample: a row repeats its predecessor unless a move is accepted (probability
    ``accept``), so about three quarters of the rows are repeats."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, d))
    x[0] = rng.normal(size=d)
    for i in range(1, n):
        x[i] = x[i - 1] + 0.8 * rng.normal(size=d) if rng.random() < accept else x[i - 1]
    return x
