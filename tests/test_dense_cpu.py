"""Dense preconditioners ('smpcov' and full matrices), the parts that need no device: make_precon,
the validation in SteinIntegrand and at the C ABI, the refusals of the paths that stay isotropic, and the
oracle-side preconditions of tests/test_gpu_dense.py (its greedy cases are decided by margins far above
rounding, so identical indices are a fair demand)."""
import ctypes
import types

import numpy as np
import pytest

from oracle import stein_numpy as o
from tests import dense_ref as R

from stein_thinning import thinning as st
from stein_thinning.kernel import make_precon


def test_smpcov_is_the_symmetrised_inverse_sample_covariance():
    c = R.case(1500, 4)
    L = c['L']
    ci = np.linalg.inv(np.cov(c['xs'], rowvar=False))
    assert np.array_equal(L, (ci + ci.T) / 2)
    assert np.array_equal(L, L.T)
    np.linalg.cholesky(L)


def test_smpcov_one_dimension():
    xs = R.case(300, 1)['xs']
    L = make_precon(xs, 'smpcov')
    assert L.shape == (1, 1)
    assert L[0, 0] == np.linalg.inv(np.atleast_2d(np.cov(xs, rowvar=False)))[0, 0]


def test_smpcov_degenerate_sample_raises():
    x = np.random.default_rng(0).normal(size=(200, 1))
    with pytest.raises(ValueError, match='Too few unique samples in smp.'):
        make_precon(np.hstack([x, 2 * x]), 'smpcov')
    with pytest.raises(ValueError, match='Too few unique samples in smp.'):
        make_precon(np.ones((1, 3)), 'smpcov')
    with pytest.raises(ValueError, match='Incorrect preconditioner type.'):
        make_precon(np.ones((5, 3)), 'nonsense')


def test_integrand_accepts_a_dense_preconditioner():
    c = R.case(300, 4)
    integrand = st.SteinIntegrand(c['xs'], c['gs'], c['L'])
    assert np.array_equal(integrand.linv, c['L'])
    assert np.array_equal(integrand.linv_dense, c['L']) and integrand.linv_dense.flags.c_contiguous
    assert integrand.linv_trace == float(np.trace(c['L']))
    iso = st.SteinIntegrand(c['xs'], c['gs'], 0.37 * np.identity(4))
    assert iso.linv_dense is None and iso.linv_scale == 0.37


def test_integrand_rejects_bad_matrices():
    c = R.case(300, 4)
    skew = c['L'].copy()
    skew[0, 1] += 1e-3
    with pytest.raises(ValueError, match='symmetric'):
        st.SteinIntegrand(c['xs'], c['gs'], skew)
    with pytest.raises(ValueError, match='positive definite'):
        st.SteinIntegrand(c['xs'], c['gs'], -np.identity(4) + 1e-3 * (np.ones((4, 4)) - np.identity(4)))
    with pytest.raises(ValueError):
        st.SteinIntegrand(c['xs'], c['gs'], R.case(300, 3)['L'])   # (3, 3) for a 4-dimensional sample
    c17 = R.raw(100, 17, 7)
    L17 = np.identity(17) + 0.01 * np.ones((17, 17))
    with pytest.raises(NotImplementedError, match='16'):
        st.SteinIntegrand(c17[0], c17[1], L17)


def test_minus_identity_is_rejected():
    """-I is l * I with l < 0: not a positive-definite preconditioner either way."""
    c = R.case(300, 4)
    with pytest.raises(ValueError):
        st.SteinIntegrand(c['xs'], c['gs'], -np.identity(4))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_dense_entry_points_validate_before_any_hip_call(lib):
    from stein_thinning import _native
    inv, uns = _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    buf = (ctypes.c_double * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 8)
    big = 1 << 26
    # st_greedy_dense(x, g, w, n, d, ld, linv, tr, m, idx, a, ws, ws_bytes, stream)
    g = [p, p, None, 10, 4, 16, p, 4.0, 5, p, p, p, big, None]
    calls = {
        'st_greedy_dense': (g, 6, 4, 0),
        # (x, g, w, ld, d, linv, tr, i1, i2, n_pairs, out, stream)
        'st_kernel_pairs_dense': ([p, p, None, 16, 4, p, 4.0, p, p, 3, p, None], 5, 4, 0),
        # (x, g, w, k, ld, d, linv, tr, out, stream)
        'st_kmat_dense': ([p, p, None, 10, 16, 4, p, 4.0, p, None], 6, 5, 0),
        # (x, g, w, n, ld, d, linv, tr, row_begin, row_end, csum, stream)
        'st_ksd_colsum_dense': ([p, p, None, 10, 16, 4, p, 4.0, 0, 10, p, None], 6, 5, 0),
        # (x, g, w, m, ld, d, linv, tr, ks, ws, ws_bytes, stream)
        'st_ksd_cumulative_dense': ([p, p, None, 10, 16, 4, p, 4.0, p, p, big, None], 6, 5, 0),
    }
    for name, (args, k_linv, k_d, k_x) in calls.items():
        fn = getattr(lib, name)
        for k, bad, want in [(k_linv, None, inv), (k_linv, odd, inv), (k_d, 17, uns), (k_d, 0, inv), (k_x, None, inv)]:
            a = list(args)
            a[k] = bad
            assert fn(*a) == want, (name, k, bad)
            assert lib.st_last_error() != b''
    assert b'16' in (lib.st_kmat_dense(*[p, p, None, 10, 16, 17, p, 4.0, p, None]) and lib.st_last_error())
    a = list(g)
    a[9] = None                                   # no index output
    assert lib.st_greedy_dense(*a) == inv
    a = list(g)
    a[12] = 64                                    # workspace too small
    assert lib.st_greedy_dense(*a) == inv
    a = list(g)
    a[8] = 0                                      # n_points
    assert lib.st_greedy_dense(*a) == inv
    assert lib.st_ksd_colsum_dense(p, p, None, 10, 16, 4, p, 4.0, 3, 2, p, None) == inv   # row_end < row_begin


def test_sharded_and_margin_paths_refuse_dense_preconditioners():
    from stein_thinning import diagnostics, distributed
    c = R.case(300, 4, 7, True)
    integrand = st.SteinIntegrand(c['xs'], c['gs'], c['L'])
    with pytest.raises(NotImplementedError, match='dense'):
        distributed.thin_sharded(c['x'], c['g'], 10, preconditioner='smpcov')
    with pytest.raises(NotImplementedError, match='dense'):
        distributed.thin_gf_sharded(c['x'], c['log_p'], c['log_q'], c['g'], 10, preconditioner='smpcov')
    with pytest.raises(NotImplementedError, match='dense'):
        distributed.thin_across_ranks(integrand, 10)
    with pytest.raises(NotImplementedError, match='dense'):
        distributed.ksd_sharded(integrand, 10)
    with pytest.raises(NotImplementedError, match='dense'):
        diagnostics.greedy_margins(types.SimpleNamespace(linv=c['L']), 10)
    with pytest.raises(NotImplementedError, match='dense'):
        diagnostics.thin_margins(c['x'], c['g'], 10, preconditioner='smpcov')


def test_array_preconditioner_to_thin_stays_a_value_error():
    c = R.case(300, 4)
    with pytest.raises(ValueError):
        make_precon(c['xs'], c['L'])


@pytest.mark.parametrize('n,d,seed,gf,m',
                         R.GREEDY_CASES + [(R.PAIR_N, d, 7, gf, 40) for d in R.PAIR_DIMS for gf in (False, True)]
                         + [(1500, 4, s, False, 40) for s in R.CHAIN_SEEDS[1:]]
                         + [(1500, d, 7, gf, 40) for d, gf in R.KSD_CASES if (d, gf) != (4, False) and d != 12])
def test_oracle_preconditions(n, d, seed, gf, m):
    """Every (n, d, seed) of test_gpu_dense.py: L is symmetric positive definite, and the oracle's greedy
    run is decided at every step by a margin far above rounding (>= MARGIN_MIN of the largest sum)."""
    c = R.case(n, d, seed, gf)
    assert np.array_equal(c['L'], c['L'].T)
    np.linalg.cholesky(c['L'])
    idx, sums, margin = R.greedy(n, d, seed, gf, m)
    assert margin >= R.MARGIN_MIN, margin
    assert len(set(idx.tolist())) >= 1 and np.all(np.isfinite(sums))


def test_reference_error_yardstick_is_measurable():
    """rho_ref (the NumPy reference against np.longdouble) is positive and small for every pair-test case."""
    if not R.longdouble_ok():
        pytest.skip('np.longdouble is no wider than float64 here')
    for d in R.PAIR_DIMS:
        c = R.case(R.PAIR_N, d)
        i1, i2 = R.pair_set(R.PAIR_N)
        k, scale = R.pair_ld(c, i1, i2)
        r = R.rho(R.integrand(c)(i1, i2), k, scale)
        assert 0 < r < 1e-9, (d, r)
