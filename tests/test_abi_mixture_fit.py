"""st_mixture_em_stats / st_mixture_em_workspace_bytes: every validation rule precedes any HIP call (no device
needed), and the workspace size is positive for d <= 16, k <= 32, -1 otherwise, and bounded by the grid."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_workspace_bytes(lib):
    size = lib.st_mixture_em_workspace_bytes
    for d in range(1, 17):
        for k in (1, 2, 7, 32):
            rec = (1 + k * (1 + d + d * (d + 1) // 2)) * 8
            assert size(1, d, k) == rec
            assert size(64, d, k) == rec
            assert size(65, d, k) == 2 * rec                      # one record per 64-row tile ...
            big = size(10 ** 9, d, k)
            assert big == size(10 ** 7, d, k) and big % rec == 0   # ... capped by the grid, not by n
            assert 64 <= big // rec <= 1024
    for n, d, k in [(100, 17, 2), (100, 64, 2), (100, 0, 2), (100, -1, 2), (0, 4, 2), (-5, 4, 2), (100, 4, 0),
                    (100, 4, -1), (100, 4, 33), (100, 4, 1024)]:
        assert size(n, d, k) == -1, (n, d, k)


def test_validation_happens_before_any_hip_call(lib):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    names = ['x', 'n', 'd', 'k', 'log_coef', 'means', 'precision', 'row_weights', 'out', 'log_p', 'ws', 'ws_bytes',
             'stream']
    base = [p, 100, 4, 3, p, p, p, p, p, p, p, 1 << 24, None]
    assert len(names) == len(base) == len(_native.SIGNATURES['st_mixture_em_stats'][1])

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_mixture_em_stats(*a)

    for name in ('x', 'log_coef', 'means', 'precision', 'out', 'ws'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('x', 'log_coef', 'means', 'precision', 'row_weights', 'out', 'log_p', 'ws'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    assert call(n=0) == inv and call(n=-1) == inv
    assert call(d=0) == inv and call(d=-3) == inv
    assert call(k=0) == inv and call(k=-3) == inv and b'k must' in lib.st_last_error()
    need = lib.st_mixture_em_workspace_bytes(100, 4, 3)
    assert call(ws_bytes=need - 8) == inv and b'workspace' in lib.st_last_error()
    assert call(ws_bytes=0) == inv
    assert call(d=17) == uns and b'16' in lib.st_last_error()
    assert call(d=64, ws_bytes=1 << 30) == uns
    assert call(k=33) == uns and b'32' in lib.st_last_error()
    # invalid arguments win over an unsupported shape
    assert call(d=17, n=0) == inv and call(d=17, x=None) == inv and call(k=33, out=odd) == inv
