"""Proxy producers (csrc/proxy.hip: st_proxy_logpdf_grad) at their edges (``pytest -m gpu``), at the ABI's
level, every kernel variant (st_tune key 7: 0 auto, 1 VALU, 2 LDS-tiled matrix cores, 3 guarded streaming
form, 4 buffer-instruction form; a mode the dimension does not admit falls back as launch_proxy says).

Yardstick: tests/proxy_ref.py's long-double ``reference`` with the per-element bounds derived in its
docstring -- no global scale: every log q and every gradient element against its own bound; the VALU kernel
against scipy's |dev U|^2 form, the matrix-core kernels against dev . P dev and, with the long-double gap
between the two forms added, against the U form.  Recipes: benign, per-dimension scales over 1e4 (cond up to
1e8), a location 1e6 away, rows exactly at loc, 1e-6 / 1.5 / 1e4 sigma out and a block at 1e140.

Beyond the bounds: exact values at loc, every n around the 16-row and 64-row blocks, no store outside the
outputs (sentinels around 16-byte-aligned views), grid-stride loops run three and four times per wave or
block (n from the CU count), outputs that depend on the row alone (bit for bit across positions, n and
copies), and NaN / inf rows that stay alone.

Observed on MI355X (256 CUs): worst error / bound over all recipes, dims and df -- VALU kernel 0.51 (log q)
and 0.36 (gradient); matrix-core kernels 0.50 (log q, P form), 0.22 (gradient) and, by construction, up to
1.00 against the U form on the scaled recipes (the error there IS the gap between the two forms).  Every
copy of a row was bit-identical in every variant; the deep cases ran at n = 49 157 (streaming), 98 309
(buffer) and 98 341 (LDS-tiled)."""
import numpy as np
import pytest

from tests import dense_ref
from tests import proxy_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)
if not dense_ref.longdouble_ok():
    pytest.skip('np.longdouble is no wider than float64 here: no error yardstick', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import proxy  # noqa: E402

N = 257
MODES = [0, 1, 2, 3, 4]
SENTINEL = 0x7FF8C0FFEE15BAD1                  # a NaN no kernel computes (as int64)
# every mode at the matrix-core dims; below and above their range every mode runs the VALU kernel
MODE_DIMS = [(m, d) for d in R.EDGE_DIMS for m in MODES] + [(m, d) for d in (5, 65) for m in (0, 1)]


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).cuda()      # a writable C-order copy


def _launch(mode, xd, n, d, loc, whiten, precision, df, c_log, log_q, grad):
    """st_proxy_logpdf_grad under st_tune key 7 = mode on device tensors; log_q / grad are written in place."""
    lib = nat.lib()
    ld_, ud, pd = _dev(loc), _dev(whiten), _dev(precision)
    assert lib.st_tune(7, mode) == 0
    try:
        nat.check(lib.st_proxy_logpdf_grad(nat.ptr(xd), n, d, nat.ptr(ld_), nat.ptr(ud), nat.ptr(pd), float(df),
                                           float(c_log), nat.ptr(log_q), nat.ptr(grad), nat.stream_handle()),
                  'st_proxy_logpdf_grad')
        torch.cuda.synchronize()
    finally:
        lib.st_tune(7, 0)


def _run(mode, x, loc, whiten, precision, df, c_log):
    """(log_q (n), grad (n, d)) on the host; the outputs are NaN before the call."""
    n, d = x.shape
    log_q = torch.full((n,), np.nan, dtype=torch.float64, device='cuda')
    grad = torch.full((n, d), np.nan, dtype=torch.float64, device='cuda')
    _launch(mode, _dev(x), n, d, loc, whiten, precision, df, c_log, log_q, grad)
    return log_q.cpu().numpy(), grad.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _inputs(name, d, df, n=N):
    c = R.recipe(name, n, d)
    whiten, precision, c_log = R.factors(name, n, d, df)
    return c['x'], c['loc'], whiten, precision, df, c_log


def _modes_for(d):
    """The modes that reach distinct kernels at dimension d."""
    return MODES if 16 < d <= 64 else [0, 1]


@pytest.mark.parametrize('d', R.MFMA_DIMS + R.VALU_DIMS)
@pytest.mark.parametrize('name', R.RECIPES)
def test_every_element_within_its_bound(name, d):
    """n = 257, every mode the dimension admits, df in {Gaussian, 1e-3, 1, 30.5, 1e6, 1e15}; rows at loc give
    log q = -0.5 c_log (Gaussian) or c_log (Student-t) and a zero gradient exactly."""
    worst = {}
    at = R.at_loc(name, N)
    for df in R.DFS:
        args = _inputs(name, d, df)
        r = R.reference(*args)
        for mode in _modes_for(d):
            lq, g = _run(mode, *args)
            assert np.all(np.isfinite(lq)) and np.all(np.isfinite(g)), (mode, df)
            out = R.check(R.kernel_kind(mode, d), lq, g, r, what=f'{name} d={d} df={df} mode {mode}')
            for k, v in out.items():
                worst[(mode, k)] = max(worst.get((mode, k), 0.0), v)
            assert np.all(lq[at] == (args[5] if df > 0 else -0.5 * args[5])), (mode, df)
            assert np.all(g[at] == 0.0), (mode, df)
    print(f'{name} d={d}: worst error / bound ' + ', '.join(f'mode {m} {k} {v:.3f}' for (m, k), v in sorted(worst.items())))


@pytest.mark.parametrize('d', R.EDGE_DIMS)
@pytest.mark.parametrize('mode', MODES)
def test_tile_and_block_edges(mode, d):
    """n on either side of the 16-row blocks of the streaming forms and of the 64-row tiles."""
    for df in (0.0, 30.5):
        x, *rest = _inputs('benign', d, df, 127)
        r = R.reference(x, *rest)
        for n in R.EDGE_N:
            lq, g = _run(mode, x[:n], *rest)
            assert lq.shape == (n,) and g.shape == (n, d)
            R.check(R.kernel_kind(mode, d), lq, g, r, rows=slice(0, n), what=f'n={n} d={d} df={df} mode {mode}')


@pytest.mark.parametrize('mode,d', MODE_DIMS)
def test_nothing_is_written_outside_the_outputs(mode, d):
    """log_q and grad as 16-byte-aligned views inside sentinel-filled buffers; n % 16 != 0 (and n = 64 + 1:
    one row in the last 64-row tile)."""
    pad = 256
    for n in (1, 17, 65, 127, 261):
        for df in (0.0, 3.5):
            x, *rest = _inputs('benign', d, df, 261)
            lbuf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int64, device='cuda')
            gbuf = torch.full((n * d + 2 * pad,), SENTINEL, dtype=torch.int64, device='cuda')
            log_q = lbuf[pad:pad + n].view(torch.float64)
            grad = gbuf[pad:pad + n * d].view(torch.float64)
            assert log_q.data_ptr() % 16 == 0 and grad.data_ptr() % 16 == 0
            _launch(mode, _dev(x[:n]), n, d, *rest, log_q, grad)
            for buf, m in ((lbuf, n), (gbuf, n * d)):
                assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + m:] == SENTINEL).all()), (n, df)
                assert not bool((buf[pad:pad + m] == SENTINEL).any()), (n, df)     # and every element is written
            r = R.reference(x[:n], *rest)
            R.check(R.kernel_kind(mode, d), log_q.cpu().numpy(), grad.cpu().numpy().reshape(n, d), r,
                    what=f'n={n} d={d} df={df} mode {mode}')


def _stream_passes(n, cus, bpc):
    """(fewest, most) 16-row blocks a wave of the streaming / buffer form handles: grid_for restated
    (two blocks per wave, 4 waves per block, at most cus * bpc blocks)."""
    nsub = (n + 15) // 16
    grid = max(1, min(((nsub + 1) // 2 + 3) // 4, cus * bpc))
    waves = 4 * grid
    return nsub // waves, (nsub + waves - 1) // waves


def _tiled_passes(n):
    """(fewest, most) 64-row tiles a block of the LDS-tiled kernel handles: grid = min(tiles, 512)."""
    tiles = (n + 63) // 64
    grid = min(tiles, 512)
    return tiles // grid, (tiles + grid - 1) // grid


def _deep_n(mode, d):
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if mode == 2:
        n = 64 * 3 * 512 + 37
        passes = _tiled_passes(n)
    else:
        bpc = 2 if mode == 4 and d % 2 == 0 else 1
        n = 16 * 3 * (4 * cus * bpc) + 5
        passes = _stream_passes(n, cus, bpc)
    assert passes == (3, 4), (mode, d, cus, n, passes)     # some wave / block makes 4 passes, the others 3
    assert n * d * 8 <= 64 << 20
    return n


@pytest.mark.parametrize('mode,d', [(2, 17), (2, 18), (2, 63), (2, 64), (3, 17), (3, 18), (3, 63), (3, 64),
                                    (4, 18), (4, 64)])
def test_deep_grid_stride(mode, d):
    """Every wave (block, mode 2) goes three or four times round its loop: the streaming form's shift of its
    in-flight register blocks and guarded third prefetch, the buffer form's empty descriptor past the end
    followed by live ones, the tiled kernel's prefetch of tile + gridDim.  x tiles 509 distinct rows (a prime:
    every lane position sees every row), the first 509 outputs are held to the bounds and every copy of a
    row to the bits of its first copy: a row's outputs depend on the row alone (one variant keeps one
    summation order; the cross-lane adds are commutative pairs)."""
    n = _deep_n(mode, d)
    m = R.TILED_ROWS
    idx = torch.arange(n, device='cuda') % m
    for df in (0.0, 30.5):
        base, *rest = _inputs('scaled', d, df, m)
        r = R.reference(base, *rest)
        xd = _dev(base)[idx].contiguous()
        log_q = torch.full((n,), np.nan, dtype=torch.float64, device='cuda')
        grad = torch.full((n, d), np.nan, dtype=torch.float64, device='cuda')
        _launch(mode, xd, n, d, *rest, log_q, grad)
        R.check('mfma', log_q[:m].cpu().numpy(), grad[:m].cpu().numpy(), r, what=f'n={n} d={d} df={df} mode {mode}')
        lb, gb = log_q.view(torch.int64), grad.view(torch.int64)
        assert torch.equal(lb, lb[:m][idx]), (df, 'log q differs between copies of a row')
        assert torch.equal(gb, gb[:m][idx]), (df, 'grad differs between copies of a row')


@pytest.mark.parametrize('mode,d', MODE_DIMS)
def test_rows_do_not_depend_on_their_position_or_on_n(mode, d):
    for df in (0.0, 3.5):
        x, *rest = _inputs('scaled', d, df)
        lq, g = _run(mode, x, *rest)
        again_l, again_g = _run(mode, x, *rest)
        assert np.array_equal(_bits(again_l), _bits(lq)) and np.array_equal(_bits(again_g), _bits(g))
        perm = np.random.default_rng(5).permutation(N)
        perm_l, perm_g = _run(mode, x[perm], *rest)
        assert np.array_equal(_bits(perm_l), _bits(lq[perm])) and np.array_equal(_bits(perm_g), _bits(g[perm]))
        for n in (100, 37):
            head_l, head_g = _run(mode, x[:n], *rest)
            assert np.array_equal(_bits(head_l), _bits(lq[:n])) and np.array_equal(_bits(head_g), _bits(g[:n]))


@pytest.mark.parametrize('mode,d', MODE_DIMS)
def test_non_finite_rows_stay_alone(mode, d):
    """NaN and +inf in rows 15 and 16 (either side of a 16-row block), in a mid-tile row and in the last row
    of an n with n % 16 == 5 (the streaming form's padding lanes re-read that row), in the first and in the
    last column (next to the k padding): the planted rows' outputs are all non-finite, every other row has
    the bits of the clean run."""
    n = 261
    planted = {15: (d - 1, np.nan), 16: (0, np.inf), 100: (d - 1, np.inf), n - 1: (d - 1, np.nan)}
    for df in (0.0, 3.5):
        x, *rest = _inputs('benign', d, df, n)
        clean_l, clean_g = _run(mode, x, *rest)
        assert np.all(np.isfinite(clean_l)) and np.all(np.isfinite(clean_g))
        bad = x.copy()
        for row, (col, v) in planted.items():
            bad[row, col] = v
        lq, g = _run(mode, bad, *rest)
        good = np.ones(n, dtype=bool)
        good[list(planted)] = False
        assert not np.any(np.isfinite(lq[~good])) and not np.any(np.isfinite(g[~good])), df
        assert np.array_equal(_bits(lq[good]), _bits(clean_l[good])), df
        assert np.array_equal(_bits(g[good]), _bits(clean_g[good])), df


@pytest.mark.parametrize('d', [5, 18, 63])
def test_the_shim_feeds_these_inputs(d):
    """proxy.gaussian_proxy / student_t_proxy on (x, loc, cov) are the ABI call on R.factors' doubles."""
    c = R.recipe('scaled', N, d)
    lq, g = proxy.gaussian_proxy(c['x'], c['loc'], c['cov'])
    wl, wg = _run(0, *_inputs('scaled', d, 0.0))
    assert np.array_equal(_bits(lq), _bits(wl)) and np.array_equal(_bits(g), _bits(wg))
    lq, g = proxy.student_t_proxy(c['x'], c['loc'], c['cov'], 30.5)
    wl, wg = _run(0, *_inputs('scaled', d, 30.5))
    assert np.array_equal(_bits(lq), _bits(wl)) and np.array_equal(_bits(g), _bits(wg))
