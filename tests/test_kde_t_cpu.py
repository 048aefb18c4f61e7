"""Student-t kernel density proxy, everything that needs no GPU: the long-double reference against scipy's
multivariate_t mixture and central differences, the float64 restatement of the kernel's order inside the
bound derived in tests/kde_t_ref.py, the bound's teeth, the recipe's far third really underflowing without
the shift, the Gaussian limit, the host bookkeeping of collapse_repeats, and the ABI's argument checks."""
import ctypes

import numpy as np
import pytest

from tests import dense_ref
from tests import kde_t_ref as T
from tests import side_ref as S

needs_ld = pytest.mark.skipif(not dense_ref.longdouble_ok(),
                              reason='np.longdouble is no wider than float64 here: no error yardstick')


def _case(n, m, d, df):
    c = S.kde_case(n, m, d)
    assert T.in_domain(c['logw'])
    return c, T.log_norm_t(c['L'], df)


# ------------------------------------------------------------------------------------------ (a)
@needs_ld
def test_reference_is_the_multivariate_t_mixture_and_its_gradient():
    from scipy.special import logsumexp
    from scipy.stats import multivariate_t
    from stein_thinning import proxy
    rng = np.random.default_rng(5)
    n, d, df = 200, 3, 4.0
    a = rng.normal(size=(d, d))
    x = rng.normal(size=(n, d)) @ a.T + 1.0
    y = np.vstack([x[:30], x[30:50] + 0.4 * rng.normal(size=(20, d)), x[:10] + 25.0])
    wts = rng.uniform(0.2, 1.0, size=n)
    for weights in (None, wts):
        w, L, log_norm = proxy.kde_t_factors(x, df, 'silverman', weights)
        assert log_norm == T.log_norm_t(L, df)
        shape = np.linalg.inv(L @ L.T)                      # cov * factor^2
        terms = np.stack([multivariate_t.logpdf(y, loc=x[i], shape=shape, df=df) for i in range(n)], axis=1)
        want = logsumexp(terms + np.log(w)[None, :], axis=1)
        r = T.tkde_ld(x @ L, y @ L, np.log(w), df, log_norm, L)
        # the yardstick's own float64 rounding: shape comes from an inversion and scipy factors it again, so its
        # Mahalanobis form is off by a few cond(shape) u, which h carries into the log (8 h cond u); 64 u on
        # 1 + |log q| for the rest (the d-term sums, log1p, the logsumexp over n terms)
        err = np.abs(r['logq'].astype(np.float64) - want)
        tol = T.U * (64 * (1 + np.abs(want)) + 8 * 0.5 * (df + d) * np.linalg.cond(shape))
        print(f'tkde_ld vs scipy mixture: max error {err.max():.2e}, error / tolerance {np.max(err / tol):.3f}')
        assert np.all(err <= tol)

        def logq(pts):
            return T.tkde_ld(x @ L, pts @ L, np.log(w), df, log_norm, L)['logq']
        eps = 1e-5
        for l in range(d):
            e = np.zeros(d)
            e[l] = eps
            fd = ((logq(y + e) - logq(y - e)) / (2 * eps)).astype(np.float64)
            assert np.max(np.abs(fd - r['grad'][:, l].astype(np.float64))) < 1e-7     # O(eps^2) of a smooth function


def test_factors_reject_bad_df():
    from stein_thinning import proxy
    x = np.random.default_rng(0).normal(size=(10, 2))
    for df in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            proxy.kde_t_factors(x, df)


# ------------------------------------------------------------------------------------------ (b)
@needs_ld
@pytest.mark.parametrize('d', T.TKDE_DIMS_CPU)
@pytest.mark.parametrize('n,m', S.KDE_SHAPES)
def test_restated_kernel_order_within_the_derived_bound(n, m, d):
    for df in T.TKDE_DFS:
        c, log_norm = _case(n, m, d, df)
        r = T.tkde_ld(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        lq, g = T.tkde_emulate(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        rl, rg = T.ratios(lq, g, r)
        print(f'tkde emulate n={n} m={m} d={d} df={df:g}: error / bound = {rl:.3f} (log q), {rg:.3f} (grad)')
        assert rl <= 1.0 and rg <= 1.0, (df, rl, rg)


# ------------------------------------------------------------------------------------------ (c)
@needs_ld
@pytest.mark.parametrize('wrong,df', [('h', 3.0), ('coef', 3.0), ('unshifted', 1e5)])
def test_bound_has_teeth(wrong, df):
    """Each planted mistake must leave the bound on at least one of these cases."""
    outside = False
    for n, m, d in [(257, 255, 4), (513, 300, 9)]:
        c, log_norm = _case(n, m, d, df)
        r = T.tkde_ld(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        lq, g = T.tkde_emulate(c['p'], c['q'], c['logw'], df, log_norm, c['L'], wrong=wrong)
        if wrong == 'unshifted':      # the far third: every term underflows, log q = -inf
            rl, rg = T.ratios(lq[c['far']:], g[c['far']:], {k: v[c['far']:] for k, v in r.items()})
        else:
            rl, rg = T.ratios(lq, g, r)
        print(f'wrong={wrong} n={n} d={d}: error / bound = {rl:.3g} (log q), {rg:.3g} (grad)')
        outside |= (rg > 1.0) if wrong == 'coef' else (rl > 1.0)
    assert outside


# ------------------------------------------------------------------------------------------ dropped rows
@needs_ld
@pytest.mark.parametrize('n,d,zero_weights', T.OFFSET_CASES)
def test_dropped_rows_closer_than_every_weighted_point(n, d, zero_weights):
    """Data around 50 per coordinate, queries at the origin: a zero-weight row (moved to the origin) or a padding
    row of the runtime-d kernel has rho > 1 there, and at df = 1e5 rho^h overflows.  The restatement with the
    clamp stays inside the bound; without it the case really yields 0 * inf = NaN."""
    c = T.offset_case(n, 40, d, zero_weights)
    for df in (1e5, 3.0):
        log_norm = T.log_norm_t(c['L'], df)
        r = T.tkde_ld(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        assert np.all(np.isfinite(r['logq'].astype(np.float64)))
        lq, g = T.tkde_emulate(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        rl, rg = T.ratios(lq, g, r)
        print(f'offset n={n} d={d} df={df:g}: error / bound = {rl:.3f} (log q), {rg:.3f} (grad); log q[0] = {lq[0]:.1f}')
        assert rl <= 1.0 and rg <= 1.0, (df, rl, rg)
    lq, g = T.tkde_emulate(c['p'], c['q'], c['logw'], 1e5, T.log_norm_t(c['L'], 1e5), c['L'], wrong='unclamped')
    assert np.isnan(lq[0]) and np.isnan(lq[1]) and np.all(np.isfinite(lq[2:]))


# ------------------------------------------------------------------------------------------ (d)
@needs_ld
@pytest.mark.parametrize('d', [1, 4, 8, 17])
def test_far_third_underflows_without_the_shift_at_large_df(d):
    c = S.kde_case(257, 255, d)
    e = T.unshifted_exponents(c['p'], c['q'][c['far']:], 1e5)
    assert e.min() > 745.0, e.min()
    assert T.unshifted_exponents(c['p'], c['q'][c['far']:], 3.0).min() < 745.0     # small df never underflows


# ------------------------------------------------------------------------------------------ (e)
@needs_ld
def test_gaussian_limit():
    """df = 1e7 on the near two thirds of kde_case(257, 255, 4) against side_ref.kde_ld.  Per pair
    delta_ij = h log1p(r2 / nu) - r2 / 2 = (d r2 / 2 - r2^2 / 4) / nu + O(r2^3 / nu^2), and the normalisers differ by
    lgamma(h) - lgamma(nu / 2) - d / 2 log(nu / 2) = d (d - 2) / (4 nu) + O(nu^-2) plus the float64 rounding of the
    two lgamma values (~ nu log(nu) 2^-53 each).  With the Gaussian softmax weights s_ij, log q moves by
    -log sum_i s_ij exp(-delta_ij) = sum_i s_ij delta_ij to first order, and the softmax mean of (p - q) by
    sum_i s_ij (|delta_ij| + |mean delta| + |d - r2_ij| / nu) |p_i - q| (the weights' change and the coefficient
    (nu + d) / (nu + r2)).  The bounds are twice those leading terms: the factor covers the next order, which is
    max(delta, r2 / nu) ~ 1e-3 of them here."""
    ld = np.longdouble
    df, (n, m, d) = 1e7, (257, 255, 4)
    c = S.kde_case(n, m, d)
    q = c['q'][:c['far']]
    t = T.tkde_ld(c['p'], q, c['logw'], df, T.log_norm_t(c['L'], df), c['L'])
    g = S.kde_ld(c['p'], q, c['logw'], c['log_norm'], c['L'])
    r2 = T._r2_ld(c['p'], q)
    arg = c['logw'].astype(ld)[None, :] - r2 / 2
    s = np.exp(arg - np.max(arg, axis=1)[:, None])
    s /= np.sum(s, axis=1)[:, None]
    delta = np.abs(d * r2 / 2 - r2 * r2 / 4) / ld(df)
    assert float(np.max(np.where(s >= ld(2.0 ** -53), delta, ld(0)))) < 1e-2          # "next order" is small
    mean_delta = np.sum(s * delta, axis=1)
    norm = abs(d * (d - 2) / (4 * df)) + 2 * df * np.log(df) * 2.0 ** -53
    bound = 2 * (mean_delta + norm)
    err = np.abs(t['logq'] - g['logq'])
    print(f'Gaussian limit df={df:g}: max |d log q| = {float(err.max()):.3e}, bound in [{float(bound.min()):.3e}, '
          f'{float(bound.max()):.3e}]')
    assert np.all(err <= bound)
    assert float(err.max()) > 1e-9          # and the two are not the same function
    rel = delta + mean_delta[:, None] + np.abs(d - r2) / ld(df)
    dv = np.stack([2 * np.sum(s * rel * np.abs(c['p'][None, :, l] - q[:, l, None]), axis=1) for l in range(d)], axis=1)
    gb = dv @ np.abs(c['L']).astype(ld).T + g['tol_grad'] + t['tol_grad']
    gerr = np.abs(t['grad'] - g['grad'])
    print(f'Gaussian limit df={df:g}: max |d grad| = {float(gerr.max()):.3e}, bound up to {float(gb.max()):.3e}')
    assert np.all(gerr <= gb)


# ------------------------------------------------------------------------------------------ (f)
def test_collapse_rows_bookkeeping():
    from stein_thinning import proxy
    rng = np.random.default_rng(9)
    base = rng.normal(size=(40, 3))
    idx = rng.integers(0, 40, size=300)
    idx[:40] = np.arange(40)
    rows = base[idx]
    w = rng.uniform(0.1, 1.0, size=300)
    w /= w.sum()
    uniq, summed, inverse = proxy.collapse_rows(rows, w)
    assert uniq.shape == (40, 3) and inverse.shape == (300,)
    assert np.array_equal(uniq[inverse], rows)                       # the scatter index restores every row
    for k in range(40):                                              # brute force
        same = np.all(rows == uniq[k], axis=1)
        assert same.sum() == np.sum(idx == idx[np.flatnonzero(same)[0]])
        assert abs(summed[k] - w[same].sum()) <= 4 * 2.0 ** -53 * w[same].sum() * same.sum()
    assert len({tuple(r) for r in uniq}) == 40
    assert abs(summed.sum() - 1.0) < 1e-14
    uniq2, none, inv2 = proxy.collapse_rows(rows)
    assert none is None and np.array_equal(uniq2, uniq) and np.array_equal(inv2, inverse)


# ------------------------------------------------------------------------------------------ end to end
@needs_ld
def test_restated_order_and_reference_select_the_same_rows():
    """Precondition of the GPU end-to-end test: with m = 20 and df = 4 (the issue's values, unchanged) the
    float64 restatement's proxy and the long-double proxy rounded to float64 make thin_gf select the same 20
    rows of the fixture, so rounding-level differences of the proxy do not decide the selection."""
    from oracle import stein_numpy as ref
    sample, log_p, p, logw, log_norm, L = T.gm_thin_case()
    r = T.tkde_ld(p, p, logw, 4.0, log_norm, L)
    lq, g = T.tkde_emulate(p, p, logw, 4.0, log_norm, L)
    want = ref.thin_gf(sample, log_p, r['logq'].astype(np.float64), r['grad'].astype(np.float64), 20,
                       range_cap=200, preconditioner='med')
    got = ref.thin_gf(sample, log_p, lq, g, 20, range_cap=200, preconditioner='med')
    assert np.array_equal(got, want), (got, want)
    assert len(set(want.tolist())) > 10


# ------------------------------------------------------------------------------------------ (g)
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_abi_workspace_bytes(lib):
    assert lib.st_abi_version() == 1
    for d in range(1, 9):
        assert lib.st_kde_t_workspace_bytes(1000, d) == 0
    for d in (9, 17, 128):
        assert lib.st_kde_t_workspace_bytes(1000, d) == 8 * 1000 * d
    assert lib.st_kde_t_workspace_bytes(0, 4) == 0
    for m, d in [(-1, 4), (10, 0), (10, -2), (10, 129)]:
        assert lib.st_kde_t_workspace_bytes(m, d) == -1, (m, d)


def test_abi_validation_happens_before_any_hip_call(lib):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    names = ['p', 'ldp', 'n', 'logw', 'logw0', 'q', 'ldq', 'm', 'd', 'df', 'log_norm', 'L', 'log_q', 'grad', 'ws',
             'ws_bytes', 'stream']
    base = [p, 128, 100, None, -4.6, p, 64, 50, 4, 4.0, 0.0, p, p, p, p, 1 << 20, None]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_kde_t_logpdf_grad(*a)

    for name in ('p', 'q', 'L', 'log_q', 'grad'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    assert call(n=0) == inv and call(n=-1) == inv and call(m=-1) == inv
    assert call(ldp=99) == inv and call(ldq=49) == inv
    for df in (0.0, -1.0, float('inf'), float('-inf'), float('nan')):
        assert call(df=df) == inv, df
        assert b'df' in lib.st_last_error()
    assert call(d=0) == uns and call(d=-1) == uns and call(d=129) == uns
    need = lib.st_kde_t_workspace_bytes(50, 9)
    assert need == 8 * 50 * 9
    assert call(d=9, ws_bytes=need - 8) == inv and b'workspace' in lib.st_last_error()
    assert call(d=9, ws=None) == inv
    assert call(m=0) == _native.ST_OK and call(m=0, p=None, df=-1.0) == _native.ST_OK      # m = 0: a no-op
    assert lib.st_tune(24, 1) == 0 and lib.st_tune(24, 2) == 0 and lib.st_tune(24, 0) == 0 and lib.st_tune(24, 3) != 0
