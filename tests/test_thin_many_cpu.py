"""st_chain_stats, st_pdist_many, st_greedy_many without a GPU: the symbols exist, every ST_ERR_INVALID /
ST_ERR_UNSUPPORTED condition is reported before any HIP call (the style of tests/test_abi_mala.py), the engine's
size limit is at least 4096 rows, and on every input of the GPU parity test (tests/test_gpu_thin_many.py) the NumPy
oracle and the C bit model in the exact arithmetic select the same indices -- which makes that test's two
assertions (idx equals the oracle's; idx and the running sums equal the bit model's) consistent."""
import ctypes

import numpy as np
import pytest

from tests import many_ref as R


@pytest.fixture(scope='module')
def lib():
    return R.native_lib()


@pytest.fixture(scope='module')
def ptrs():
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return dict(keep=buf, p=p, odd=ctypes.c_void_p(p.value + 4), byte=ctypes.c_void_p(p.value + 2))


def _caller(lib, fn_name, names, base):
    from stein_thinning import _native
    assert len(names) == len(base) == len(_native.SIGNATURES[fn_name][1])

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return getattr(lib, fn_name)(*a)
    return call


def test_abi_version_is_unchanged(lib):
    from stein_thinning import _native
    assert lib.st_abi_version() == _native.ABI_VERSION == 1       # additive entry points


def test_max_n_and_plan(lib):
    from stein_thinning import _native
    for d in (2, 4):
        for w in (0, 1):
            assert lib.st_greedy_many_max_n(d, w) >= 4096
    for d in (0, 1, 3, 5, 8, -1):
        assert lib.st_greedy_many_max_n(d, 0) == 0
    t, r = ctypes.c_int32(0), ctypes.c_int32(0)
    for d in (2, 4):
        mx = lib.st_greedy_many_max_n(d, 0)
        for n in (1, 2, 64, 65, 1000, mx):
            assert lib.st_greedy_many_plan(n, d, 0, ctypes.byref(t), ctypes.byref(r)) == 0
            assert t.value % 64 == 0 and 64 <= t.value <= 1024 and t.value * r.value >= n    # every row has a slot
        assert lib.st_greedy_many_plan(mx + 1, d, 0, ctypes.byref(t), ctypes.byref(r)) == _native.ST_ERR_UNSUPPORTED
        assert lib.st_greedy_many_plan(0, d, 0, ctypes.byref(t), ctypes.byref(r)) == _native.ST_ERR_INVALID
        assert lib.st_greedy_many_plan(8, d, 0, None, ctypes.byref(r)) == _native.ST_ERR_INVALID
    assert lib.st_greedy_many_plan(8, 3, 0, ctypes.byref(t), ctypes.byref(r)) == _native.ST_ERR_UNSUPPORTED


def test_greedy_many_validation_happens_before_any_hip_call(lib, ptrs):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    p, odd, byte = ptrs['p'], ptrs['odd'], ptrs['byte']
    names = ['x', 'g', 'scl', 'weights', 'linv_scale', 'linv_trace', 'chains', 'n', 'd', 'n_points', 'idx_out',
             'a_out', 'stream']
    call = _caller(lib, 'st_greedy_many', names, [p, p, p, p, p, p, 3, 100, 4, 20, p, p, None])
    for name in ('x', 'g', 'scl', 'linv_scale', 'linv_trace', 'idx_out'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('x', 'g', 'scl', 'weights', 'linv_scale', 'linv_trace', 'a_out'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    assert call(idx_out=byte) == inv and b'aligned' in lib.st_last_error()
    for name in ('chains', 'n', 'd', 'n_points'):
        for v in (0, -1):
            assert call(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
    assert call(chains=1 << 31) == inv
    for d in (1, 3, 5, 8, 128, 129):
        assert call(d=d) == uns, d
    for d in (2, 4):
        assert call(d=d, n=lib.st_greedy_many_max_n(d, 1) + 1) == uns
        assert call(d=d, n=lib.st_greedy_many_max_n(d, 0) + 1, weights=None) == uns
        assert call(d=d, n=1 << 40) == uns


def test_chain_stats_validation_happens_before_any_hip_call(lib, ptrs):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    p, odd, byte = ptrs['p'], ptrs['odd'], ptrs['byte']
    names = ['x', 'g', 'chains', 'n', 'd', 'standardize', 'loc_out', 'scl_out', 'status_out', 'stream']
    call = _caller(lib, 'st_chain_stats', names, [p, p, 3, 100, 4, 1, p, p, p, None])
    for name in ('x', 'g', 'loc_out', 'scl_out', 'status_out'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('x', 'g', 'loc_out', 'scl_out'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    assert call(status_out=byte) == inv and b'aligned' in lib.st_last_error()
    for name in ('chains', 'n', 'd'):
        for v in (0, -1):
            assert call(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
    assert call(chains=1 << 31) == inv
    for d in (1, 9, 128):
        assert call(d=d) == uns, d


def test_pdist_many_validation_happens_before_any_hip_call(lib, ptrs):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    p, odd, byte = ptrs['p'], ptrs['odd'], ptrs['byte']
    names = ['x', 'scl', 'sub_rows', 'chains', 'n', 'd', 'k', 'out', 'stream']
    call = _caller(lib, 'st_pdist_many', names, [p, p, p, 3, 1500, 4, 1000, p, None])
    for name in ('x', 'scl', 'out'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('x', 'scl', 'out'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    assert call(sub_rows=byte) == inv and b'aligned' in lib.st_last_error()
    for name in ('chains', 'n', 'd'):
        for v in (0, -1):
            assert call(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
    for k in (-1, 0, 1, 1501):
        assert call(k=k) == inv, k
    assert call(sub_rows=None) == inv            # all rows means k == n
    assert call(d=129) == uns
    assert call(n=70000, k=65536) == uns
    assert call(chains=1 << 31) == uns           # chains * (k - 1) blocks


def test_max_n_is_zero_for_an_unsupported_width(lib):
    """The host-only query never touches HIP: an unsupported width reports 0 rows."""
    assert lib.st_greedy_many_max_n(-7, 0) == 0 and lib.st_greedy_many_max_n(129, 1) == 0


def test_parity_shapes_cover_every_plan_change():
    for d in R.DIMS:
        ns = R.parity_ns(d)
        assert {2, 63, 64, 65, 256, 257, 1000, 1001, 1500, R.max_n(d) - 1, R.max_n(d)} <= set(ns)
        changes = R.plan_changes(d)
        assert changes, 'the plan changes somewhere between 1 and max_n'
        for n in changes:
            assert R.plan(n, d) != R.plan(n + 1, d) and n in ns and n + 1 in ns


@pytest.mark.parametrize('d,n,precon', R.parity_cases())
def test_numpy_oracle_and_exact_bit_model_select_the_same_rows(d, n, precon):
    x, g, ref = R.parity_reference(d, n, precon)
    for c, (oidx, cidx, cA) in enumerate(ref):
        np.testing.assert_array_equal(oidx, cidx, err_msg=f'chain {c}')
        assert np.all(np.isfinite(cA))
    if n >= 63:                                   # the chains do repeat rows: exact ties at every step
        rep = np.all(x[:, 1:] == x[:, :-1], axis=2).mean()
        assert 0.5 < rep < 0.9
