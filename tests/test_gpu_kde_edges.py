"""KDE proxy kernel (csrc/kde.hip: st_kde_logpdf_grad) at its edges (``pytest -m gpu``), at the ABI's
level: n and m on either side of the tiles, far queries whose every exponent underflows without the
max-shift, weights over 300 orders of magnitude, zero weights (log w = -inf) down to a whole staging
tile of them, the runtime-d kernel up to d = 128, and the all-weights-zero result.

Yardstick: tests/side_ref.py's long-double ``kde_ld`` with the bounds derived in its docstring --
|log q_j - ref_j| <= tau_j + 2^-52 |ref_j|, tau_j = 2^-53 (n + (d + 6) (1 + A_j)), and the gradient
tolerance built from tau_j, the spread of the points that carry weight, and the d-term product with L.
Everything the call has no business reading is NaN: the padding rows of p and q, the outputs and the
workspace before the call.

Observed on MI355X: worst error / bound 0.291 (log q) and 0.030 (gradient) over all shapes, weighted and
uniform; log q of the far queries about -1800 (down to -2186 at d = 128); the n = 1 log q bit-identical to
its closed form; zero weights drop out exactly."""
import warnings

import numpy as np
import pytest

from tests import dense_ref
from tests import side_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)
if not dense_ref.longdouble_ok():
    pytest.skip('np.longdouble is no wider than float64 here: no error yardstick', allow_module_level=True)

from oracle import proxy_numpy as op  # noqa: E402
from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import proxy  # noqa: E402
from stein_thinning.device import padded_ld  # noqa: E402
from tests.test_gpu_proxy import _close  # noqa: E402


def _soa(a):
    n, d = a.shape
    ld = padded_ld(n)
    host = np.full((d, ld), np.nan)
    host[:, :n] = a.T
    return torch.from_numpy(host).cuda(), ld


def _kde(p, q, logw, log_norm, L):
    """(log_q (m), grad (m, d)) of st_kde_logpdf_grad; logw an (n) array, or a float for the uniform
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
    wsb = int(lib.st_kde_workspace_bytes(m, d))
    assert wsb == (8 * m * d if d > 8 else 0)
    ws = torch.full((max(wsb // 8, 2),), np.nan, dtype=torch.float64, device='cuda')
    nat.check(lib.st_kde_logpdf_grad(nat.ptr(pt), ldp, n, nat.ptr(lw), float(logw) if uniform else 0.0,
                                     nat.ptr(qt), ldq, m, d, float(log_norm), nat.ptr(lt), nat.ptr(log_q),
                                     nat.ptr(grad), nat.ptr(ws), ws.numel() * 8, nat.stream_handle()),
              'st_kde_logpdf_grad')
    return log_q.cpu().numpy(), grad.cpu().numpy()


def _ratios(lq, g, r):
    return (float(np.max(np.abs(lq - r['logq']) / r['tol_logq'])), float(np.max(np.abs(g - r['grad']) / r['tol_grad'])))


def _check_single_point(c, logw0, lq, g):
    """n = 1 closed forms: the shift is the only exponent, so log q is the float64 a_0j itself (exp(0) = 1,
    log(1) = 0: bit for bit), v = p_0 - q_j is one rounding and grad its d-term product with L."""
    arg = S.kde_arg_model(c['p'], c['q'], np.array([logw0]), c['log_norm'])[:, 0]
    assert np.array_equal(lq, arg)
    ld = np.longdouble
    v = (c['p'][0][None, :] - c['q']).astype(ld)
    absL = np.abs(c['L']).astype(ld)
    tol = (c['d'] + 1) * ld(S.U) * (np.abs(v) @ absL.T)
    assert np.all(np.abs(g - v @ c['L'].astype(ld).T) <= tol)


@pytest.mark.parametrize('n,m,d', [(n, m, d) for n, m in S.KDE_SHAPES for d in S.KDE_DIMS] + S.KDE_WIDE)
def test_log_q_and_gradient_within_the_derived_bounds(n, m, d):
    c = S.kde_case(n, m, d)
    for name, logw in (('weighted', c['logw']), ('uniform', float(-np.log(n)))):
        lq, g = _kde(c['p'], c['q'], logw, c['log_norm'], c['L'])
        r = S.kde_ld(c['p'], c['q'], np.full(n, logw) if np.isscalar(logw) else logw, c['log_norm'], c['L'])
        assert np.all(np.isfinite(lq)) and np.all(np.isfinite(g))
        assert np.all(lq[c['far']:] < -745.0)
        rl, rg = _ratios(lq, g, r)
        print(f'kde n={n} m={m} d={d} {name}: error / bound = {rl:.3f} (log q), {rg:.3f} (grad); '
              f'log q in [{lq.min():.1f}, {lq.max():.1f}]')
        assert np.all(np.abs(lq - r['logq']) <= r['tol_logq']), int(np.argmax(np.abs(lq - r['logq']) / r['tol_logq']))
        assert np.all(np.abs(g - r['grad']) <= r['tol_grad'])
        if n == 1:
            _check_single_point(c, 0.0 if name == 'weighted' else logw, lq, g)


@pytest.mark.parametrize('d', [2, 8, 9])
def test_zero_weights_drop_out_exactly(d):
    """-inf log-weights on a subset S (every fifth point and the whole tile [256, 512)) against the same
    call on the data with S removed: a zero term adds exactly 0 to s and fma(0, p, sm) = sm, so log q
    and grad are equal by value."""
    c = S.kde_case(513, 300, d)
    keep = np.setdiff1d(np.arange(513), c['zero'])
    assert keep.size == 513 - 256 - 51 and set(range(256, 512)) <= set(c['zero'].tolist())
    lq, g = _kde(c['p'], c['q'], c['logw'], c['log_norm'], c['L'])
    lq2, g2 = _kde(c['p'][keep], c['q'], c['logw'][keep], c['log_norm'], c['L'])
    assert np.array_equal(lq, lq2) and np.array_equal(g, g2)
    # and zeros in the first and the last position of the data
    logw = c['logw'].copy()
    logw[[0, 512]] = -np.inf
    keep = np.flatnonzero(np.isfinite(logw))
    lq, g = _kde(c['p'], c['q'], logw, c['log_norm'], c['L'])
    lq2, g2 = _kde(c['p'][keep], c['q'], logw[keep], c['log_norm'], c['L'])
    assert np.array_equal(lq, lq2) and np.array_equal(g, g2)


@pytest.mark.parametrize('n,m,d', [(257, 255, 2), (513, 300, 8), (257, 65, 9), (1, 5, 3)])
def test_all_weights_zero_gives_minus_infinity(n, m, d):
    """The kernel documents log q = -inf when every weight is zero (the gradient is not pinned)."""
    c = S.kde_case(n, m, d)
    lq, _ = _kde(c['p'], c['q'], np.full(n, -np.inf), c['log_norm'], c['L'])
    assert np.all(np.isneginf(lq))
    lq, _ = _kde(c['p'], c['q'], float(-np.inf), c['log_norm'], c['L'])
    assert np.all(np.isneginf(lq))


@pytest.mark.parametrize('d', [2, 9])
def test_public_path_with_zero_weights(d):
    """proxy.kde_proxy with a third of the weights exactly 0 (a contiguous run among them) against the
    restatement of jax's gaussian_kde (log(0) = -inf there too: divide warnings filtered)."""
    rng = np.random.default_rng(70 + d)
    n = 601
    x = rng.normal(size=(n, d)) * 1.5 + 0.3
    w = rng.uniform(0.1, 1.0, size=n)
    w[100:250] = 0.0                                       # a contiguous run
    w[rng.choice(np.r_[0:100, 250:n], size=n // 3 - 150, replace=False)] = 0.0
    assert np.sum(w == 0.0) == n // 3
    y = np.vstack([x[:40], x[260:300] * 1.1 + 0.05])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        lq, gq = proxy.kde_proxy(x, y, bw_method='silverman', weights=w)
        wl, wg = op.kde_proxy(x, y, bw_method='silverman', weights=w)
    assert np.all(np.isfinite(lq)) and np.all(np.isfinite(gq))
    print(f'kde_proxy d={d}, {int(np.sum(w == 0.0))} zero weights: max |log q - oracle| = {np.max(np.abs(lq - wl)):.2e}, '
          f'max |grad - oracle| = {np.max(np.abs(gq - wg)):.2e}')
    _close(lq, wl)
    _close(gq, wg)
