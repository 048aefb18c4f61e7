"""st_mvt_moments / st_mvt_moments_workspace_bytes: every validation rule precedes any HIP call (no device
needed), and the workspace size is positive for d <= 16 and -1 above."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_workspace_bytes(lib):
    for d in range(1, 17):
        nacc = 2 + d + d * (d + 1) // 2
        assert lib.st_mvt_moments_workspace_bytes(1, d) == nacc * 8
        assert lib.st_mvt_moments_workspace_bytes(65, d) == 2 * nacc * 8
        big = lib.st_mvt_moments_workspace_bytes(10 ** 9, d)
        assert big > 0 and big == lib.st_mvt_moments_workspace_bytes(10 ** 7, d)   # capped by the grid, not by n
    for n, d in [(100, 17), (100, 64), (100, 0), (100, -1), (0, 4), (-5, 4)]:
        assert lib.st_mvt_moments_workspace_bytes(n, d) == -1, (n, d)


def test_validation_happens_before_any_hip_call(lib):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    names = ['x', 'n', 'd', 'loc', 'whiten', 'df', 'want_grad', 'out', 'ws', 'ws_bytes', 'stream']
    base = [p, 100, 4, p, p, 5.0, 1, p, p, 1 << 20, None]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_mvt_moments(*a)

    for name in ('x', 'loc', 'whiten', 'out', 'ws'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    assert call(n=0) == inv and call(n=-1) == inv
    assert call(d=0) == inv and call(d=-3) == inv
    for df in (0.0, -1.0, float('inf'), float('nan')):
        assert call(df=df) == inv, df
        assert b'df' in lib.st_last_error()
    need = lib.st_mvt_moments_workspace_bytes(100, 4)
    assert call(ws_bytes=need - 8) == inv and b'workspace' in lib.st_last_error()
    assert call(ws_bytes=0) == inv
    assert call(d=17) == uns and b'16' in lib.st_last_error()
    assert call(d=64, ws_bytes=1 << 30) == uns
    # invalid arguments win over an unsupported width
    assert call(d=17, n=0) == inv and call(d=17, x=None) == inv and call(d=17, df=0.0) == inv
