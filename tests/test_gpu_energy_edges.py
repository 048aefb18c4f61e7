"""Energy-distance column sums (csrc/pairwise.hip K7: st_distance_colsum[_ws]) at their edges
(``pytest -m gpu``): every kernel variant (st_tune key 13), ranges off the tile boundary, the
block-uniform fast range's two ends and the slow path, the chunk geometries of the workspace
launch, against the bit model and the long-double reference of tests/side_ref.py.

Single distances must equal ``dist_model`` bit for bit (the header's "sqrt of the sequential sum",
fast_dist's "same bits as __builtin_sqrt" -- also at ss = d 2^122, which at d = 8 is 2^125, one binade past
the 2^124 the kernel's comment names); column sums must lie within the derived bound
(c_i + d + 2) 2^-53 ref_i of the long-double sum (side_ref's docstring), zero-pair columns exactly 0.0.
Everything a call has no business reading is NaN: the SoA padding rows of A and B, the B rows outside
[b_begin, b_end) (where B is an array of its own), the workspace and the output before the call.

Observed on MI355X: every single distance bit-identical (d = 1 .. 8 under all six variants, d = 9, 17,
128); worst error / bound 0.192 for the column sums (all variants and d), 0.081 for the chunked sums
against long double, 0.011 of twice the bound between the chunked and the unsplit launch; |ED(x, x)| at
most 0.001 of its bound; the curve with repeated indices within 6.6e-15 relative of the oracle."""
import functools

import numpy as np
import pytest

from oracle import stein_numpy as o
from tests import dense_ref
from tests import side_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)
if not dense_ref.longdouble_ok():
    pytest.skip('np.longdouble is no wider than float64 here: no error yardstick', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import energy as se  # noqa: E402
from stein_thinning.device import padded_ld  # noqa: E402

VARIANTS = [1, 2, 3, 4, 5, 6]     # st_tune key 13: U = 1 / 2 / 4 partial sums, 4 / 8 blocks per CU, SEL


def _soa(points, keep=None):
    """SoA upload as energy._soa, with NaN in the padding rows [n, ld) and in every row outside
    keep = (begin, end)."""
    n, d = points.shape
    ld = padded_ld(n)
    host = np.full((d, ld), np.nan)
    b, e = (0, n) if keep is None else keep
    host[:, b:e] = points[b:e].T
    return torch.from_numpy(host).cuda(), ld


def _colsum(a, lda, na, b, ldb, nb, d, b0, b1, tri, ws):
    """out (na) of st_distance_colsum_ws (ws) or st_distance_colsum; out and workspace NaN before the call."""
    L = nat.lib()
    out = torch.full((na,), np.nan, dtype=torch.float64, device='cuda')
    if ws:
        wsb = int(L.st_distance_workspace_bytes(na, b0, b1))
        assert wsb >= 0
        w = torch.full((max(wsb // 8, 2),), np.nan, dtype=torch.float64, device='cuda')
        nat.check(L.st_distance_colsum_ws(nat.ptr(a), lda, na, nat.ptr(b), ldb, nb, d, b0, b1, tri, nat.ptr(out),
                                          nat.ptr(w), w.numel() * 8, nat.stream_handle()), 'st_distance_colsum_ws')
    else:
        nat.check(L.st_distance_colsum(nat.ptr(a), lda, na, nat.ptr(b), ldb, nb, d, b0, b1, tri, nat.ptr(out),
                                       nat.stream_handle()), 'st_distance_colsum')
    return out.cpu().numpy()


class _tuned:
    """st_tune keys for the block; keys 13 and 14 cannot be read back (st_tune_get: INT32_MIN), so they
    are restored with -1 (automatic)."""

    def __init__(self, **keys):
        self.keys = {int(k[1:]): v for k, v in keys.items() if v is not None}

    def __enter__(self):
        for k, v in self.keys.items():
            nat.check(nat.lib().st_tune(k, v), f'st_tune({k}, {v})')

    def __exit__(self, *exc):
        for k in self.keys:
            nat.check(nat.lib().st_tune(k, -1), f'st_tune({k}, -1)')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize('d,variant', [(d, v) for d in range(1, 9) for v in VARIANTS]
                         + [(9, None), (17, None), (128, None)])
def test_single_distances_bit_for_bit(d, variant):
    """B = one row of the boundary table: out[i] is one distance.  With b = 0 (in range) the block of
    columns 0-255 takes the fast path and the block 256-511 the slow one; with b = 256 (out of range)
    every block takes the slow path: both see the planted pairs (ss = 2^-224, d 2^122, 0, inf)."""
    x = S.boundary_points(d)
    a, lda = _soa(x)
    zeros = infs = 0
    with _tuned(k13=variant):
        for b in (0, 255, 256, 511, 512):
            bt, ldb = _soa(x, keep=(b, b + 1))
            want = S.dist_model(x, x[b:b + 1])[:, 0]
            zeros, infs = zeros + int(np.sum(want == 0.0)), infs + int(np.sum(np.isinf(want)))
            for ws in (False, True):
                got = _colsum(a, lda, 513, bt, ldb, 513, d, b, b + 1, 0, ws)
                bad = np.flatnonzero(_bits(got) != _bits(want))
                assert bad.size == 0, (b, ws, bad[:5], got[bad[:5]], want[bad[:5]])
    print(f'd={d} variant={variant}: 5 x 513 distances bit-identical ({zeros} zeros, {infs} infs among them)')


@functools.lru_cache(maxsize=None)
def _colsum_reference(d, shape):
    na, nb, b0, b1, tri = shape
    A = S.points(na, d, 11)
    B = A if tri else S.points(nb, d, 12)
    ref, cnt = S.colsum_ld(A, B, b0, b1, tri)
    return A, B, ref, cnt, S.energy_bound(ref, cnt, d)


@pytest.mark.parametrize('d,variant', [(d, v) for d in (1, 2, 3, 4, 8) for v in VARIANTS] + [(9, None), (17, None)])
def test_column_sums_within_the_derived_bound(d, variant):
    worst = 0.0
    with _tuned(k13=variant):
        for shape in S.COLSUM_SHAPES:
            na, nb, b0, b1, tri = shape
            A, B, ref, cnt, bound = _colsum_reference(d, shape)
            a, lda = _soa(A)
            b, ldb = (a, lda) if tri else _soa(B, keep=(b0, b1))
            for ws in (False, True):
                got = _colsum(a, lda, na, b, ldb, nb, d, b0, b1, tri, ws)
                again = _colsum(a, lda, na, b, ldb, nb, d, b0, b1, tri, ws)
                assert np.array_equal(_bits(got), _bits(again)), (shape, ws)       # deterministic
                assert np.all(got[cnt == 0] == 0.0) and not np.any(np.signbit(got[cnt == 0])), (shape, ws)
                err = np.abs(got - ref)
                assert np.all(err <= bound), (shape, ws, int(np.argmax(err - bound)))
                nz = bound > 0
                if nz.any():
                    worst = max(worst, float(np.max(err[nz] / bound[nz])))
    print(f'colsum d={d} variant={variant}: worst error / bound = {worst:.3f}')


@pytest.mark.parametrize('geom,d', [(g, d) for g in S.CHUNK_GEOMETRIES[:3] for d in (3, 9)]
                         + [(S.CHUNK_GEOMETRIES[3], 3)])
def test_chunk_geometries(geom, d):
    """The workspace launch's splits: a last chunk of one point, a triangle whose last chunk adds
    nothing, an off-tile start, and (key 14 = 256) trailing empty chunks.  K is asserted through
    st_distance_workspace_bytes, so a changed split rule is noticed here."""
    na, nb, b0, b1, tri, units, K, chunk = geom
    A = S.points(na, d, 11)
    B = A if tri else S.points(nb, d, 12)
    a, lda = _soa(A)
    b, ldb = (a, lda) if tri else _soa(B, keep=(b0, b1))
    with _tuned(k14=units):
        assert int(nat.lib().st_distance_workspace_bytes(na, b0, b1)) == K * na * 8
        assert S.chunk_split(na, b0, b1, units or 32768) == (K, chunk)
        split = _colsum(a, lda, na, b, ldb, nb, d, b0, b1, tri, True)
        assert np.array_equal(_bits(split), _bits(_colsum(a, lda, na, b, ldb, nb, d, b0, b1, tri, True)))
    whole = _colsum(a, lda, na, b, ldb, nb, d, b0, b1, tri, False)
    cols = S.check_columns(na)
    ref, cnt = S.colsum_ld(A, B, b0, b1, tri, cols=cols)
    bound = S.energy_bound(ref, cnt, d)
    err = np.abs(split[cols] - ref)
    assert np.all(err <= bound), int(cols[np.argmax(err - bound)])
    assert np.all(np.abs(whole[cols] - ref) <= bound)
    # every column: both launches are within B_i ref_i of the same ref_i <= whole_i / (1 - B_i)
    count = np.minimum(np.arange(na), b1) - np.minimum(np.arange(na), b0) if tri else np.full(na, b1 - b0)
    B_rel = (count + d + 2) * S.U
    pair_tol = 2 * B_rel * whole / (1 - B_rel)
    assert np.all(split[count == 0] == 0.0) and np.all(whole[count == 0] == 0.0)
    assert np.all(np.abs(split - whole) <= pair_tol), int(np.argmax(np.abs(split - whole) - pair_tol))
    nz = bound > 0
    print(f'chunks na={na} [{b0}, {b1}) tri={tri} d={d} K={K}: worst error / bound = '
          f'{float(np.max(err[nz] / bound[nz])):.3f}; split against whole / (2 x bound) = '
          f'{float(np.max(np.abs(split - whole)[count > 0] / pair_tol[count > 0])):.3f}')


@pytest.mark.parametrize('d', [1, 4, 9])
def test_energy_distance_of_a_sample_with_itself(d):
    """ED(x, x) = 2 E|X - X'| - 2 E|X - X'| cancels exactly in real arithmetic: what is left is the rounding
    of the three terms, each a mean of column sums within (n + d + 2) 2^-53 relative (plus the final
    sums' own rounding): |ED| <= 4 (n + d + 3) 2^-53 (mean pairwise distance)."""
    n = 700
    x = S.points(n, d, 21)
    mean = float(np.sum(S.colsum_ld(x, x, 0, n, False)[0])) / (n * n)
    got = se.energy_distance(x, x)
    tol = 4 * (n + d + 3) * S.U * mean
    print(f'ED(x, x) d={d}: {got:.3e}, bound {tol:.3e}, ratio {abs(got) / tol:.3f}')
    assert abs(got) <= tol


@pytest.mark.parametrize('d', [1, 4, 9])
def test_curve_with_repeated_indices(d):
    """A selection that repeats indices: zero distances inside the selection's triangle."""
    rng = np.random.default_rng(d + 60)
    x = S.points(900, d, 22)
    sample = S.points(400, d, 23) * 1.2
    idx = rng.integers(0, 25, size=300)                     # 300 picks of 25 rows
    idx[:4] = idx[0]
    sizes = np.array([1, 2, 3, 4, 5, 17, 256, 257, 300])
    want = np.array([np.sqrt(o.energy_distance(x, sample[idx[:k]])) for k in sizes])
    got = se.energy_distance_curve(x, sample, idx, sizes)
    print(f'curve d={d}: max relative difference {float(np.max(np.abs(got - want) / want)):.2e}')
    np.testing.assert_allclose(got, want, rtol=1e-10)
