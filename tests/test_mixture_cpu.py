"""Gaussian mixture, host side (no GPU): mixture_factors against scipy, its validation, the C entry
point's argument validation (before any HIP call), the import touching no GPU, and the seeded recipe of
tests/mixture_ref.py against the oracle and the long-double restatement."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
from scipy.stats import multivariate_normal

from stein_thinning import mixture
from tests import mixture_ref as R


@pytest.mark.parametrize('d,k', [(1, 1), (2, 3), (4, 2), (9, 7), (33, 3), (64, 2)])
def test_mixture_factors_match_scipy(d, k):
    x, w, means, covs = R.case(2000, d, k)
    log_coef, mu, prec = mixture.mixture_factors(w, means, covs)
    assert log_coef.shape == (k,) and mu.shape == (k, d) and prec.shape == (k, d, d)
    assert log_coef.dtype == mu.dtype == prec.dtype == np.float64
    rows = x[:7]
    for c in range(k):
        dev = rows - means[c]
        q = np.einsum('nj,jk,nk->n', dev, prec[c], dev)
        want = np.log(w[c]) + np.atleast_1d(multivariate_normal.logpdf(rows, means[c], covs[c]))
        np.testing.assert_allclose(log_coef[c] - q / 2, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(prec, np.linalg.inv(covs))


def test_zero_weight_gives_minus_inf_coefficient():
    _, _, means, covs = R.case(2000, 4, 3)
    log_coef, _, _ = mixture.mixture_factors([0.0, 0.4, 0.6], means, covs)
    assert log_coef[0] == -np.inf and np.all(np.isfinite(log_coef[1:]))


def test_mixture_factors_validation():
    _, w, means, covs = R.case(2000, 4, 3)
    f = mixture.mixture_factors
    with pytest.raises(ValueError, match='means must be \\(2, d\\)'):   # one entry per component
        f(w[:2], means, covs)
    with pytest.raises(ValueError, match='weights'):
        f(w[None, :], means, covs)
    with pytest.raises(ValueError, match='means'):
        f(w, means[:2], covs)
    with pytest.raises(ValueError, match='means'):
        f(w, means[0], covs)
    with pytest.raises(ValueError, match='covs'):
        f(w, means, covs[:, :3, :3])
    with pytest.raises(ValueError, match='covs'):
        f(w, means, covs[0])
    with pytest.raises(ValueError, match='non-negative'):
        f([0.5, -0.1, 0.6], means, covs)
    with pytest.raises(ValueError, match='finite'):
        f([0.5, np.nan, 0.5], means, covs)
    with pytest.raises(ValueError, match='finite'):
        f([0.5, np.inf, 0.5], means, covs)
    with pytest.raises(ValueError, match='zero'):
        f([0.0, 0.0, 0.0], means, covs)
    skew = covs.copy()
    skew[1, 0, 1] += 0.1
    with pytest.raises(ValueError, match='symmetric'):
        f(w, means, skew)
    singular = covs.copy()
    singular[2] = np.ones((4, 4))
    with pytest.raises(np.linalg.LinAlgError):   # as gaussian_proxy on a singular covariance
        f(w, means, singular)
    indefinite = covs.copy()
    indefinite[0] = -np.eye(4)
    with pytest.raises(ValueError, match='positive semidefinite'):
        f(w, means, indefinite)


def test_d_above_64_is_not_implemented():
    with pytest.raises(NotImplementedError, match='64'):
        mixture.mixture_factors([1.0], np.zeros((1, 65)), np.eye(65)[None])
    with pytest.raises(NotImplementedError, match='64'):
        mixture.mixture_logpdf_score(np.zeros((3, 65)), [1.0], np.zeros((1, 65)), np.eye(65)[None])


def test_sample_shape_is_checked_and_empty_sample_needs_no_device():
    _, w, means, covs = R.case(2000, 4, 3)
    with pytest.raises(ValueError, match='sample'):
        mixture.mixture_logpdf_score(np.zeros((5, 3)), w, means, covs)
    log_p, score = mixture.mixture_logpdf_score(np.zeros((0, 4)), w, means, covs)
    assert log_p.shape == (0,) and score.shape == (0, 4)
    from stein_thinning import proxy
    assert proxy.mixture_proxy is mixture.mixture_logpdf_score


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_entry_point_validates_before_any_hip_call(lib):
    from stein_thinning import _native
    ok, inv, uns = _native.ST_OK, _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    # (x, n, d, k, log_coef, means, precision, log_p_out, score_out, stream)
    good = [p, 10, 4, 3, p, p, p, p, p, None]
    for pos in (0, 4, 5, 6, 7, 8):
        for bad in (None, odd):
            a = list(good)
            a[pos] = bad
            assert lib.st_mixture_logpdf_score(*a) == inv, (pos, bad)
            assert lib.st_last_error() != b''
    for pos, bad, want in [(1, -1, inv), (2, 0, inv), (2, -3, inv), (3, 0, inv), (2, 65, uns), (2, 128, uns),
                           (3, 1025, uns)]:
        a = list(good)
        a[pos] = bad
        assert lib.st_mixture_logpdf_score(*a) == want, (pos, bad)
    a = list(good)
    a[2] = 65
    assert lib.st_mixture_logpdf_score(*a) == uns and b'64' in lib.st_last_error()
    a = list(good)
    a[3] = 1025
    assert lib.st_mixture_logpdf_score(*a) == uns and b'1024' in lib.st_last_error()
    # n == 0: nothing to do, nothing enqueued (x and the outputs may be NULL); limits still apply
    assert lib.st_mixture_logpdf_score(None, 0, 4, 3, p, p, p, None, None, None) == ok
    assert lib.st_mixture_logpdf_score(None, 0, 65, 3, p, p, p, None, None, None) == uns
    assert lib.st_abi_version() == 1


def test_import_initialises_no_gpu():
    code = ('import sys; sys.path.insert(0, "gradient-free-mcmc-postprocessing_amd"); import torch; '
            'import stein_thinning.mixture, stein_thinning.proxy; '
            'stein_thinning.mixture.mixture_factors([1.0], [[0.0]], [[[1.0]]]); '
            'print(torch.cuda.is_initialized())')
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, check=True, cwd=root)
    assert out.stdout.strip() == 'False'


@pytest.mark.parametrize('d', R.DIMS)
def test_recipe_oracle_is_finite_and_close_to_long_double(d):
    """The ground the GPU tolerance stands on: on the recipe the oracle (sums of densities) is finite and
    within 1e-14 of the long-double log-space restatement, so RTOL = 1e-12 leaves ~100x headroom; the
    float64 restatement is as close; covariance condition numbers stay <= 18."""
    for k in R.COMPONENTS:
        x, w, means, covs = R.case(2000, d, k)
        assert np.linalg.cond(covs).max() <= 18
        wl, ws = R.stable(x, w, means, covs, np.longdouble)
        for got_l, got_s in (R.oracle(2000, d, k), R.stable(x, w, means, covs)):
            assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_s))
            for got, want in ((got_l, wl), (got_s, ws)):
                err = float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1.0))
                assert err <= 1e-14, (d, k, err)


def test_oracle_is_not_finite_in_the_tails_but_the_restatement_is():
    x, w, means, covs = R.case(200, 4, 3)
    x = x.copy()
    x[:50] += 60.0
    from oracle import models
    _, logpdf, score = models.make_mvn_mixture(w, means, covs)
    with np.errstate(all='ignore'):
        assert not np.any(np.isfinite(logpdf(x)[:50])) and not np.any(np.isfinite(score(x)[:50]))
    for dtype in (np.float64, np.longdouble):
        log_p, sc = R.stable(x, w, means, covs, dtype)
        assert np.all(np.isfinite(log_p)) and np.all(np.isfinite(sc))
