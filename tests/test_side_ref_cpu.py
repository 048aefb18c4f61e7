"""CPU tier of the energy-distance / KDE edge tests: the references, bounds and recipes of
tests/side_ref.py are themselves right (no GPU).  dist_model against scipy's cdist bit for bit, the
long-double references against the float64 oracles, the float64 restatements of the kernels' operation
order inside the derived bounds on every shape the GPU tests use, and the planted edge values really
there."""
import warnings

import numpy as np
import pytest

from oracle import proxy_numpy as op
from oracle import stein_numpy as o
from tests import dense_ref
from tests import side_ref as S

needs_ld = pytest.mark.skipif(not dense_ref.longdouble_ok(), reason='np.longdouble is no wider than float64 here')


@pytest.mark.parametrize('d', [1, 4, 9])
def test_dist_model_is_scipy_cdist_bit_for_bit(d):
    from scipy.spatial.distance import cdist
    x, y = S.points(300, d, 1), S.points(77, d, 2)
    assert np.array_equal(S.dist_model(x, y), cdist(x, y))
    assert np.array_equal(S.dist_model(x, x), cdist(x, x))


@needs_ld
@pytest.mark.parametrize('d', [1, 4, 9])
def test_colsum_ld_against_the_energy_oracle(d):
    from scipy.spatial.distance import cdist
    x, y = S.points(300, d, 1), S.points(77, d, 2)
    cross, c = S.colsum_ld(x, y, 0, 77, False)
    assert np.all(c == 77)
    np.testing.assert_allclose(float(np.sum(cross)) / (300 * 77), np.mean(cdist(x, y)), rtol=1e-12)
    for z, n in ((x, 300), (y, 77)):
        tri, c = S.colsum_ld(z, z, 0, n, True)
        assert np.array_equal(c, np.arange(n))
        np.testing.assert_allclose(2 * float(np.sum(tri)) / (n * n), np.mean(cdist(z, z)), rtol=1e-12)
    xx, yy = S.colsum_ld(x, x, 0, 300, True)[0], S.colsum_ld(y, y, 0, 77, True)[0]
    ed = 2 * np.sum(cross) / (300 * 77) - 2 * np.sum(xx) / 300 ** 2 - 2 * np.sum(yy) / 77 ** 2
    assert abs(float(ed) - o.energy_distance(x, y)) <= 1e-12 * np.mean(cdist(x, y))
    part, c = S.colsum_ld(x, y, 5, 40, False, cols=[0, 7, 299])     # a sub-range, a column subset
    assert np.all(c == 35)
    np.testing.assert_allclose(part.astype(np.float64), np.sum(cdist(x[[0, 7, 299]], y[5:40]), axis=1), rtol=1e-12)


@needs_ld
@pytest.mark.parametrize('d', S.ENERGY_DIMS)
def test_energy_emulation_inside_the_bound(d):
    worst = 0.0
    for na, nb, b0, b1, tri in S.COLSUM_SHAPES:
        A = S.points(na, d, 11)
        B = A if tri else S.points(nb, d, 12)
        ref, cnt = S.colsum_ld(A, B, b0, b1, tri)
        bound = S.energy_bound(ref, cnt, d)
        for unroll in (1, 2, 4):
            got = S.energy_emulate(A, B, b0, b1, tri, unroll=unroll)
            assert np.all(got[cnt == 0] == 0.0)
            assert np.all(np.abs(got - ref) <= bound), (na, nb, b0, b1, tri, unroll)
            nz = bound > 0
            if nz.any():
                worst = max(worst, float(np.max(np.abs(got[nz] - ref[nz]) / bound[nz])))
    print(f'energy emulation d={d}: worst error / bound = {worst:.3f}')


@needs_ld
@pytest.mark.parametrize('geom', S.CHUNK_GEOMETRIES[:3])
def test_chunked_emulation_inside_the_bound(geom):
    na, nb, b0, b1, tri, units, K, chunk = geom
    assert S.chunk_split(na, b0, b1) == (K, chunk)
    d = 3
    A = S.points(na, d, 11)
    B = A if tri else S.points(nb, d, 12)
    cols = S.check_columns(na)
    ref, cnt = S.colsum_ld(A, B, b0, b1, tri, cols=cols)
    got = S.energy_emulate(A, B, b0, b1, tri, K=K, chunk=chunk, cols=cols)
    assert np.all(np.abs(got - ref) <= S.energy_bound(ref, cnt, d))


def test_chunk_split_restates_the_listed_geometries():
    for na, nb, b0, b1, tri, units, K, chunk in S.CHUNK_GEOMETRIES:
        assert S.chunk_split(na, b0, b1, units or 32768) == (K, chunk)
    na, nb, b0, b1, tri, units, K, chunk = S.CHUNK_GEOMETRIES[0]
    assert b0 + (K - 1) * chunk == b1 - 1                        # the last chunk is one point
    na, nb, b0, b1, tri, units, K, chunk = S.CHUNK_GEOMETRIES[3]
    assert b0 + 12 * chunk < b1 <= b0 + 13 * chunk                # chunks 13-15 are empty
    assert b0 % S.TILE != 0 and S.CHUNK_GEOMETRIES[2][2] % S.TILE != 0


@pytest.mark.parametrize('d', [1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 128])
def test_boundary_points_hold_the_planted_values(d):
    x = S.boundary_points(d)
    assert x.shape == (513, d) and np.all(np.isfinite(x))
    assert np.all(np.isin(x[:256], S.IN_RANGE)) and np.all(S.in_fast_range(x[:256]))
    assert np.any(np.signbit(x[:256]) & (x[:256] == 0.0))          # a -0.0
    out = ~S.in_fast_range(x[256:512])
    assert out[0].any() and out[255].any() and out.sum() >= 5      # rows 256 and 511 are probed as B
    assert np.all(np.isin(np.abs(x[256:512][out]), S.OUT_OF_RANGE))
    ss = S.ss_model(x, x)
    assert not np.any(np.isnan(S.dist_model(x, x)))
    assert ss[1, 0] == 2.0 ** -224 and ss[257, 0] == 2.0 ** -224   # fast and slow column block, B = row 0
    assert ss[254, 255] == d * 2.0 ** 122
    assert ss[2, 0] == 0.0 and ss[253, 255] == 0.0 and ss[258, 0] == 0.0 and ss[3, 4] == 0.0
    pos = ss[:256, :256][ss[:256, :256] > 0]
    assert pos.min() == 2.0 ** -224 and pos.max() == d * 2.0 ** 122   # the fast range's two ends
    assert np.isinf(ss[256:512, 511]).any()                         # overflow to inf is allowed and must match


@pytest.mark.parametrize('n,m,d', [(n, m, d) for n, m in S.KDE_SHAPES for d in (1, 2, 8, 9, 17)] + S.KDE_WIDE)
def test_kde_case_recipe(n, m, d):
    c = S.kde_case(n, m, d)
    assert c['p'].shape == (n, d) and c['q'].shape == (m, d)
    assert np.array_equal(c['L'], np.tril(c['L']))
    assert np.all(np.isneginf(c['logw'][c['zero']])) and np.all(np.isfinite(np.delete(c['logw'], c['zero'])))
    assert np.array_equal(c['zero'][c['zero'] < 256], np.arange(4, min(n, 256), 5))
    if n > 300:
        assert set(range(256, 512)) <= set(c['zero'].tolist())
    assert np.array_equal(c['q'][:m // 3], c['p'][np.arange(m // 3) % n])     # coincident queries
    # the far third: every exponent below exp's underflow (-745.13) unless the maximum is subtracted
    far = S.kde_arg_model(c['p'], c['q'][c['far']:], np.zeros(n), 0.0)
    assert far.shape[0] >= 1 and far.max() < -745.0, far.max()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.all(np.exp(far) == 0.0)


@needs_ld
@pytest.mark.parametrize('d', [1, 3, 9])
@pytest.mark.parametrize('weighted', [False, True])
def test_kde_ld_against_the_kde_oracle(d, weighted):
    """kde_ld on kde_factors' outputs against oracle.proxy_numpy.kde_proxy at test_gpu_proxy's bar."""
    from stein_thinning.proxy import kde_factors
    rng = np.random.default_rng(d)
    x = rng.normal(size=(400, d)) * 1.5 + 0.3
    y = x[:90] * 1.1 + 0.05
    w = np.exp(-0.3 * np.sum(x ** 2, axis=1)) if weighted else None
    wn, L, log_norm = kde_factors(x, 'silverman', w)
    r = S.kde_ld(x @ L, y @ L, np.log(wn), log_norm, L)
    wl, wg = op.kde_proxy(x, y, bw_method='silverman', weights=w)
    for got, want in ((r['logq'], wl), (r['grad'], wg)):
        np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-12, atol=1e-12 * max(np.abs(want).max(), 1.0))


@needs_ld
@pytest.mark.parametrize('n,m,d', [(n, m, d) for n, m in S.KDE_SHAPES for d in S.KDE_DIMS] + S.KDE_WIDE)
def test_kde_emulation_inside_the_bounds(n, m, d):
    c = S.kde_case(n, m, d)
    for logw in (c['logw'], np.full(n, -np.log(n))):
        r = S.kde_ld(c['p'], c['q'], logw, c['log_norm'], c['L'])
        lq, g = S.kde_emulate(c['p'], c['q'], logw, c['log_norm'], c['L'])
        assert np.all(np.isfinite(r['logq'])) and np.all(r['logq'][c['far']:] < -745.0)
        assert np.all(np.abs(lq - r['logq']) <= r['tol_logq'])
        assert np.all(np.abs(g - r['grad']) <= r['tol_grad'])
