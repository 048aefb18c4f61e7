"""st_rank_normalize, st_autocov, st_autocov_plan and st_autocov_workspace_bytes without a GPU: the symbols exist and
every ST_ERR_INVALID condition is reported before any HIP call (the style of tests/test_abi_hmc.py)."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_abi_version_is_unchanged(lib):
    from stein_thinning import _native
    assert lib.st_abi_version() == _native.ABI_VERSION == 1       # additive entry points


def test_workspace_bytes_and_plan(lib):
    # long plan, 10 series x 250 000, 64 lags: one lag tile, the i range split so that ~2048 blocks run
    assert lib.st_autocov_plan(1, 10, 250000, 0, 64, 0) == 1
    assert lib.st_autocov_workspace_bytes(1, 10, 250000, 0, 64, 0) == (10 * 64 * 64 + 64) * 8
    # short plan, many short series: one sum per series and lag, then one per slab of 256 series
    assert lib.st_autocov_plan(4, 131072, 128, 0, 32, 0) == 2
    assert lib.st_autocov_workspace_bytes(4, 131072, 128, 0, 32, 0) == (4 * 131072 * 32 + 4 * 512 * 32) * 8
    assert lib.st_autocov_plan(1, 2, 4, 0, 4, 0) == 1             # few series: the long plan whatever h is
    assert lib.st_autocov_plan(1, 2, 4, 0, 4, 2) == 2             # unless the caller asks
    for bad in ((0, 2, 16, 0, 4, 0), (1, 0, 16, 0, 4, 0), (1, 2, 3, 0, 2, 0), (1, 2, 16, 4, 4, 0),
                (1, 2, 16, 0, 17, 0), (1, 2, 16, -1, 4, 0), (1, 2, 16, 0, 4, 3), (1, 2, 4096, 0, 4, 2)):
        assert lib.st_autocov_workspace_bytes(*bad) == -1, bad
        assert lib.st_autocov_plan(*bad) == -1, bad


def test_validation_happens_before_any_hip_call(lib):
    from stein_thinning import _native
    inv = _native.ST_ERR_INVALID
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    names = ['series', 'groups', 'S', 'h', 'lag0', 'lag1', 'plan', 'acov_mean', 'series_mean', 'series_var0',
             'acov_series', 'workspace', 'workspace_bytes', 'stream']
    base = [p, 1, 2, 16, 0, 8, 0, p, p, p, None, p, 1 << 20, None]
    assert len(names) == len(base) == len(_native.SIGNATURES['st_autocov'][1])

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_autocov(*a)

    for name in ('series', 'acov_mean', 'series_mean', 'series_var0', 'workspace'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('series', 'acov_mean', 'series_mean', 'series_var0', 'workspace', 'acov_series'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    assert call(h=3) == inv and b'h must be' in lib.st_last_error()
    assert call(h=0) == inv and call(h=-4) == inv
    assert call(lag1=17) == inv and b'lag1' in lib.st_last_error()
    assert call(lag0=8) == inv and b'lag0' in lib.st_last_error()      # lag0 == lag1
    assert call(lag0=9) == inv and call(lag0=-1) == inv
    assert call(S=0) == inv and b'S must be' in lib.st_last_error()
    assert call(S=-2) == inv
    assert call(groups=0) == inv and b'groups' in lib.st_last_error()
    assert call(plan=3) == inv and call(plan=-1) == inv
    assert call(workspace_bytes=8) == inv and b'workspace too small' in lib.st_last_error()
    assert call(plan=2, h=4096, lag1=8) == _native.ST_ERR_UNSUPPORTED

    rnames = ['sorted', 'perm', 'vars', 'count', 'p_out', 'z_out', 'stream']
    rbase = [p, p, 1, 16, None, p, None]
    assert len(rnames) == len(rbase) == len(_native.SIGNATURES['st_rank_normalize'][1])

    def rcall(**kw):
        a = list(rbase)
        for k, v in kw.items():
            a[rnames.index(k)] = v
        return lib.st_rank_normalize(*a)

    for name in ('sorted', 'perm', 'z_out'):
        assert rcall(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('sorted', 'perm', 'z_out', 'p_out'):
        assert rcall(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('vars', 'count'):
        for v in (0, -1):
            assert rcall(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
