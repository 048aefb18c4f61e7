"""Student-t kernel density proxy (csrc/kde.hip: st_kde_t_logpdf_grad, proxy.kde_t_proxy / kde_t_thin) on the
GPU (``pytest -m gpu``).  Yardstick: tests/kde_t_ref.py's long-double ``tkde_ld`` with the bound derived in its
docstring, on side_ref.kde_case's inputs (coincident / near / far queries, weights over 300 orders of
magnitude, exact zeros, a whole zero-weight staging tile); n on either side of the staging tile, m of the
block, every power path (even and odd integer nu + d, non-integer, nu + d above the chain's limit).
Everything the call has no business reading is NaN: padding rows, outputs and workspace before the call.

Observed on MI355X: worst error / bound 0.354 (log q, d = 9, df = 1e5) and 0.512 (gradient, d = 128); 0.33 / 0.24 for
d <= 8; log q of the far queries about -1800 at df = 1e5 and finite; zero weights drop out bit for bit with their
coordinates set to NaN; the chain and the forced exp-log path both inside the bound."""
import numpy as np
import pytest

from tests import dense_ref
from tests import kde_t_ref as T
from tests import side_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)
if not dense_ref.longdouble_ok():
    pytest.skip('np.longdouble is no wider than float64 here: no error yardstick', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import proxy  # noqa: E402
from stein_thinning.device import padded_ld  # noqa: E402


def _soa(a):
    n, d = a.shape
    ld = padded_ld(n)
    host = np.full((d, ld), np.nan)
    host[:, :n] = a.T
    return torch.from_numpy(host).cuda(), ld


def _tkde(p, q, logw, df, log_norm, L):
    """(log_q (m), grad (m, d)) of st_kde_t_logpdf_grad; logw an (n) array, or a float for the uniform
    form (log_weights = NULL)."""
    n, d = p.shape
    m = q.shape[0]
    lib = nat.lib()
    pt, ldp = _soa(p)
    qt, ldq = _soa(q)
    uniform = np.isscalar(logw)
    lw = None if uniform else torch.from_numpy(np.array(logw, dtype=np.float64)).cuda()
    lt = torch.from_numpy(np.array(L, dtype=np.float64)).cuda()
    log_q = torch.full((m,), np.nan, dtype=torch.float64, device='cuda')
    grad = torch.full((m, d), np.nan, dtype=torch.float64, device='cuda')
    wsb = int(lib.st_kde_t_workspace_bytes(m, d))
    assert wsb == (8 * m * d if d > 8 else 0)
    ws = torch.full((max(wsb // 8, 2),), np.nan, dtype=torch.float64, device='cuda')
    nat.check(lib.st_kde_t_logpdf_grad(nat.ptr(pt), ldp, n, nat.ptr(lw), float(logw) if uniform else 0.0,
                                       nat.ptr(qt), ldq, m, d, float(df), float(log_norm), nat.ptr(lt),
                                       nat.ptr(log_q), nat.ptr(grad), nat.ptr(ws), ws.numel() * 8,
                                       nat.stream_handle()), 'st_kde_t_logpdf_grad')
    return log_q.cpu().numpy(), grad.cpu().numpy()


def _check(tag, lq, g, r):
    assert np.all(np.isfinite(lq)) and np.all(np.isfinite(g)), tag
    rl, rg = T.ratios(lq, g, r)
    print(f'tkde {tag}: error / bound = {rl:.3f} (log q), {rg:.3f} (grad); log q in [{lq.min():.1f}, {lq.max():.1f}]')
    assert rl <= 1.0, (tag, rl)
    assert rg <= 1.0, (tag, rg)


@pytest.mark.parametrize('n,m,d,dfs', [(n, m, d, tuple(T.TKDE_DFS)) for n, m in S.KDE_SHAPES for d in T.TKDE_DIMS_GPU]
                         + [(n, m, d, (3.0,)) for n, m, d in S.KDE_WIDE])
def test_log_q_and_gradient_within_the_derived_bound(n, m, d, dfs):
    c = S.kde_case(n, m, d)
    assert T.in_domain(c['logw'])
    for df in dfs:
        log_norm = T.log_norm_t(c['L'], df)
        r = T.tkde_ld(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        lq, g = _tkde(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        _check(f'n={n} m={m} d={d} df={df:g} path={"chain" if T.integer_path(df, d) else "exp-log"}', lq, g, r)


@pytest.mark.parametrize('n,d,zero_weights', T.OFFSET_CASES)
def test_dropped_rows_closer_than_every_weighted_point(n, d, zero_weights):
    """kde_t_ref.offset_case: data around 50 per coordinate, queries at the origin, where a zero-weight row (moved
    to the origin by the kernel; d <= 8) or a padding row of the runtime-d kernel's last tile (n % 32 != 0) is far
    closer than every weighted point and rho^h would overflow at df = 1e5 without the clamp (0 * inf)."""
    c = T.offset_case(n, 40, d, zero_weights)
    for df in (1e5, 3.0):
        log_norm = T.log_norm_t(c['L'], df)
        r = T.tkde_ld(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        lq, g = _tkde(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
        _check(f'offset n={n} d={d} df={df:g} zero weights={zero_weights}', lq, g, r)
    if zero_weights:                       # and the dropped rows' own coordinates do not matter
        p = c['p'].copy()
        p[c['w'] == 0.0] = np.nan
        lq2, g2 = _tkde(p, c['q'], c['logw'], df, log_norm, c['L'])
        assert np.array_equal(lq, lq2) and np.array_equal(g, g2)


@pytest.mark.parametrize('d', [2, 9])
def test_forced_general_path_agrees(d):
    """st_tune key 24 = 1 sends an integer nu + d down exp(h log rho): the same bound holds."""
    c = S.kde_case(257, 255, d)
    df = 3.0
    log_norm = T.log_norm_t(c['L'], df)
    r = T.tkde_ld(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
    nat.check(nat.lib().st_tune(24, 1), 'st_tune')
    try:
        lq, g = _tkde(c['p'], c['q'], c['logw'], df, log_norm, c['L'])
    finally:
        nat.check(nat.lib().st_tune(24, 0), 'st_tune')
    _check(f'd={d} df=3 forced exp-log', lq, g, r)


@pytest.mark.parametrize('d,df', [(2, 3.0), (8, 2.5), (9, 1.0)])
def test_zero_weights_drop_out_exactly(d, df):
    """-inf log-weights (every fifth point and the whole tile [256, 512)) with their coordinates poisoned by NaN,
    against the same call on the data with those rows removed: bit for bit."""
    c = S.kde_case(513, 300, d)
    log_norm = T.log_norm_t(c['L'], df)
    keep = np.setdiff1d(np.arange(513), c['zero'])
    assert set(range(256, 512)) <= set(c['zero'].tolist())
    p = c['p'].copy()
    p[c['zero']] = np.nan
    lq, g = _tkde(p, c['q'], c['logw'], df, log_norm, c['L'])
    lq2, g2 = _tkde(c['p'][keep], c['q'], c['logw'][keep], df, log_norm, c['L'])
    assert np.all(np.isfinite(lq)) and np.all(np.isfinite(g))
    assert np.array_equal(lq, lq2) and np.array_equal(g, g2)
    logw = c['logw'].copy()                               # zeros in the first and the last position too
    logw[[0, 512]] = -np.inf
    p[[0, 512]] = np.nan
    keep = np.flatnonzero(np.isfinite(logw))
    lq, g = _tkde(p, c['q'], logw, df, log_norm, c['L'])
    lq2, g2 = _tkde(c['p'][keep], c['q'], logw[keep], df, log_norm, c['L'])
    assert np.array_equal(lq, lq2) and np.array_equal(g, g2)


@pytest.mark.parametrize('n,m,d', [(257, 255, 2), (513, 300, 8), (257, 65, 9), (1, 5, 3)])
def test_all_weights_zero_gives_minus_infinity(n, m, d):
    c = S.kde_case(n, m, d)
    log_norm = T.log_norm_t(c['L'], 3.0)
    lq, _ = _tkde(c['p'], c['q'], np.full(n, -np.inf), 3.0, log_norm, c['L'])
    assert np.all(np.isneginf(lq))
    lq, _ = _tkde(c['p'], c['q'], float(-np.inf), 2.5, log_norm, c['L'])
    assert np.all(np.isneginf(lq))


@pytest.mark.parametrize('n,m,d,df', [(257, 255, 4, 4.0), (513, 300, 9, 2.5)])
def test_uniform_form_equals_the_explicit_vector(n, m, d, df):
    c = S.kde_case(n, m, d)
    log_norm = T.log_norm_t(c['L'], df)
    lw0 = float(np.log(1.0 / n))
    lq, g = _tkde(c['p'], c['q'], lw0, df, log_norm, c['L'])
    lq2, g2 = _tkde(c['p'], c['q'], np.full(n, lw0), df, log_norm, c['L'])
    assert np.array_equal(lq, lq2) and np.array_equal(g, g2)
    _check(f'uniform n={n} d={d} df={df:g}', lq, g, T.tkde_ld(c['p'], c['q'], np.full(n, lw0), df, log_norm, c['L']))


def _public_ref(x, y, df, weights):
    w, L, log_norm = proxy.kde_t_factors(x, df, 'silverman', weights)
    return T.tkde_ld(x @ L, y @ L, np.log(w), df, log_norm, L)


def _within(lq, g, r, factor=1):
    assert np.all(np.abs(lq - r['logq']) <= factor * r['tol_logq'])
    assert np.all(np.abs(g - r['grad']) <= factor * r['tol_grad'])


@pytest.mark.parametrize('d', [2, 9])
def test_public_path(d):
    rng = np.random.default_rng(40 + d)
    n = 401
    x = rng.normal(size=(n, d)) * 1.5 + 0.3
    y = np.vstack([x[:40], x[260:300] * 1.1 + 0.05, x[:5] + 30.0])
    for weights in (None, rng.uniform(0.1, 1.0, size=n)):
        lq, g = proxy.kde_t_proxy(x, y, df=4.0, weights=weights)
        r = _public_ref(x, y, 4.0, weights)
        _check(f'kde_t_proxy d={d} weights={weights is not None}', lq, g, r)
    lq, g = proxy.kde_t_proxy(x, df=2.5)                     # points default to the sample
    _check(f'kde_t_proxy d={d} self', lq, g, _public_ref(x, x, 2.5, None))
    lq1, g1 = proxy.kde_t_proxy(x[:, 0], df=4.0)             # 1-D input is a column
    lq2, g2 = proxy.kde_t_proxy(x[:, :1], df=4.0)
    assert g1.shape == (n, 1) and np.array_equal(lq1, lq2) and np.array_equal(g1, g2)
    with pytest.raises(ValueError):
        proxy.kde_t_proxy(x, df=0.0)


@pytest.mark.parametrize('weighted', [False, True])
def test_collapse_repeats_student_t(weighted):
    """A 600-row RW-style sample, about three quarters of the rows repeating their predecessor: the collapsed
    call agrees with the plain one within twice the bound (each within the bound of the same reference)."""
    x = T.rw_sample(600, 2)
    assert 100 < np.unique(x, axis=0).shape[0] < 200
    weights = np.random.default_rng(3).uniform(0.1, 1.0, size=600) if weighted else None
    lq, g = proxy.kde_t_proxy(x, df=4.0, weights=weights)
    lqc, gc = proxy.kde_t_proxy(x, df=4.0, weights=weights, collapse_repeats=True)
    r = _public_ref(x, x, 4.0, weights)
    _within(lq, g, r)
    assert np.all(np.abs(lq - lqc) <= 2 * r['tol_logq']) and np.all(np.abs(g - gc) <= 2 * r['tol_grad'])
    y = np.vstack([x[:50], x[:50], x[100:130] + 0.1])       # separate, repeated queries
    lq, g = proxy.kde_t_proxy(x, y, df=4.0, weights=weights)
    lqc, gc = proxy.kde_t_proxy(x, y, df=4.0, weights=weights, collapse_repeats=True)
    r = _public_ref(x, y, 4.0, weights)
    assert np.all(np.abs(lq - lqc) <= 2 * r['tol_logq']) and np.all(np.abs(g - gc) <= 2 * r['tol_grad'])


@pytest.mark.parametrize('weighted', [False, True])
def test_collapse_repeats_gaussian(weighted):
    """kde_proxy(collapse_repeats=True) against kde_proxy: within twice side_ref's bound for the Gaussian kernel."""
    x = T.rw_sample(600, 2)
    weights = np.random.default_rng(4).uniform(0.1, 1.0, size=600) if weighted else None
    w, L, log_norm = proxy.kde_factors(x, 'silverman', weights)
    r = S.kde_ld(x @ L, x @ L, np.log(w), log_norm, L)
    lq, g = proxy.kde_proxy(x, weights=weights)
    lqc, gc = proxy.kde_proxy(x, weights=weights, collapse_repeats=True)
    _within(lq, g, r)
    assert np.all(np.abs(lq - lqc) <= 2 * r['tol_logq']) and np.all(np.abs(g - gc) <= 2 * r['tol_grad'])


def test_kde_t_thin_end_to_end():
    """kde_t_thin on the Gaussian-mixture fixture selects the rows the NumPy oracle's thin_gf selects from the
    long-double proxy rounded to float64 (m = 20, df = 4; test_kde_t_cpu.py confirms that the float64
    restatement selects the same rows, so the comparison does not hinge on rounding), collapsed or not."""
    from oracle import stein_numpy as ref
    sample, log_p, p, logw, log_norm, L = T.gm_thin_case()
    r = T.tkde_ld(p, p, logw, 4.0, log_norm, L)
    want = ref.thin_gf(sample, log_p, r['logq'].astype(np.float64), r['grad'].astype(np.float64), 20,
                       range_cap=200, preconditioner='med')
    assert np.array_equal(proxy.kde_t_thin(sample, log_p, 20, df=4), want)
    assert np.array_equal(proxy.kde_t_thin(sample, log_p, 20, df=4, collapse_repeats=False), want)
