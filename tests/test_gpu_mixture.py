"""Gaussian-mixture log density and score on the GPU (csrc/mixture.hpp via st_mixture_logpdf_score) against
the oracle's restatement of the reference (oracle.models.make_mvn_mixture) where that is finite, and
against the log-space restatement (tests/mixture_ref.py) in the tails; both widths (VALU d <= 16, matrix
cores 16 < d <= 64); the downstream selections of thin / thin_gf on the reference's mixture.  Tolerance:
RTOL = 1e-12 as the proxy tests (the oracle is within 1e-14 of long double on these cases:
tests/test_mixture_cpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from oracle import models  # noqa: E402
from oracle import proxy_numpy as op  # noqa: E402
from oracle import stein_numpy as ref  # noqa: E402
from stein_thinning import mixture, proxy  # noqa: E402
from stein_thinning import thinning as st  # noqa: E402
from tests import mixture_ref as R  # noqa: E402

close = R.close


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize('k', R.COMPONENTS)
@pytest.mark.parametrize('d', R.DIMS)
def test_matches_the_oracle_on_every_row(d, k):
    x, w, means, covs = R.case(2000, d, k)
    log_p, score = mixture.mixture_logpdf_score(x, w, means, covs)
    want_l, want_s = R.oracle(2000, d, k)
    assert log_p.shape == (2000,) and score.shape == (2000, d)
    close(log_p, want_l)
    close(score, want_s)


@pytest.mark.parametrize('d', [4, 16, 17, 64])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_tile_edges(n, d):
    x, w, means, covs = R.case(n, d, 3)
    log_p, score = mixture.mixture_logpdf_score(x, w, means, covs)
    want_l, want_s = R.oracle(n, d, 3)
    assert log_p.shape == (n,) and score.shape == (n, d)
    close(log_p, want_l)
    close(score, want_s)


@pytest.mark.parametrize('d', [4, 33])
def test_tails_stay_finite(d):
    """Rows 60 away in every coordinate: every component density underflows (the oracle gives -inf and
    NaN there, d = 4: tests/test_mixture_cpu.py); the log-space evaluation is finite and accurate."""
    x, w, means, covs = R.case(200, d, 3)
    x = x.copy()
    x[:50] += 60.0
    log_p, score = mixture.mixture_logpdf_score(x, w, means, covs)
    want_l, want_s = R.stable(x, w, means, covs)
    assert np.all(np.isfinite(log_p)) and np.all(np.isfinite(score))
    assert want_l[:50].max() < np.log(np.finfo(np.float64).tiny)
    close(log_p, want_l)
    close(score, want_s)


@pytest.mark.parametrize('d', [4, 33])
@pytest.mark.parametrize('weights', [[0.0, 1.0], [1.0, 0.0], [0.0, 0.4, 0.0, 0.6]])
def test_zero_weight_components_contribute_nothing(weights, d):
    weights = np.array(weights)
    rng, _, means, covs = R.parameters(d, len(weights))
    keep = weights > 0
    x = R.rows(rng, 300, weights, means, covs)
    log_p, score = mixture.mixture_logpdf_score(x, weights, means, covs)
    want_l, want_s = mixture.mixture_logpdf_score(x, weights[keep], means[keep], covs[keep])
    assert np.all(np.isfinite(log_p)) and np.all(np.isfinite(score))
    close(log_p, want_l)
    close(score, want_s)
    ref_l, ref_s = R.stable(x, weights[keep], means[keep], covs[keep])
    close(log_p, ref_l)
    close(score, ref_s)


@pytest.mark.parametrize('d', [4, 33])
def test_component_order_does_not_matter(d):
    """Every row sits at the LAST component, far from the others: the running maximum moves at every
    component; the reversed mixture meets the nearest component first."""
    rng, w, means, covs = R.parameters(d, 3)
    means = means + np.array([[-8.0], [4.0], [12.0]])    # well separated, the nearest component last
    x = means[2] + rng.normal(size=(300, d)) @ np.linalg.cholesky(covs[2]).T
    log_p, score = mixture.mixture_logpdf_score(x, w, means, covs)
    rev_l, rev_s = mixture.mixture_logpdf_score(x, w[::-1].copy(), means[::-1].copy(), covs[::-1].copy())
    close(log_p, rev_l)
    close(score, rev_s)
    want_l, want_s = R.stable(x, w, means, covs)
    close(log_p, want_l)
    close(score, want_s)


@pytest.mark.parametrize('d', [1, 4, 16, 17, 50])
def test_one_component_is_the_gaussian_proxy(d):
    x, _, means, covs = R.case(2000, d, 1)
    log_p, score = mixture.mixture_logpdf_score(x, [1.0], means, covs)
    want_l, want_s = proxy.gaussian_proxy(x, means[0], covs[0])
    close(log_p, want_l)
    close(score, want_s)


@pytest.mark.parametrize('d', [4, 33])
def test_identical_components_add_up(d):
    x, _, means, covs = R.case(2000, d, 1)
    log_p, score = mixture.mixture_logpdf_score(x, [0.3, 0.7], np.repeat(means, 2, 0), np.repeat(covs, 2, 0))
    want_l, want_s = mixture.mixture_logpdf_score(x, [1.0], means, covs)
    close(log_p, want_l)
    close(score, want_s)


@pytest.mark.parametrize('d', [4, 33])
def test_rows_do_not_depend_on_their_position(d):
    x, w, means, covs = R.case(257, d, 3)
    log_p, score = mixture.mixture_logpdf_score(x, w, means, covs)
    again_l, again_s = mixture.mixture_logpdf_score(x, w, means, covs)
    np.testing.assert_array_equal(_bits(again_l), _bits(log_p))
    np.testing.assert_array_equal(_bits(again_s), _bits(score))
    perm = np.random.default_rng(5).permutation(257)
    perm_l, perm_s = mixture.mixture_logpdf_score(x[perm], w, means, covs)
    np.testing.assert_array_equal(_bits(perm_l), _bits(log_p[perm]))
    np.testing.assert_array_equal(_bits(perm_s), _bits(score[perm]))
    head_l, head_s = mixture.mixture_logpdf_score(x[:100], w, means, covs)   # nor on n
    np.testing.assert_array_equal(_bits(head_l), _bits(log_p[:100]))
    np.testing.assert_array_equal(_bits(head_s), _bits(score[:100]))


@pytest.mark.parametrize('d', [4, 33])
def test_bad_rows_are_nan_and_alone(d):
    x, w, means, covs = R.case(257, d, 3)
    clean_l, clean_s = mixture.mixture_logpdf_score(x, w, means, covs)
    x = x.copy()
    x[5, d - 1] = np.nan
    x[70, 1] = np.inf
    log_p, score = mixture.mixture_logpdf_score(x, w, means, covs)
    good = np.ones(257, dtype=bool)
    good[[5, 70]] = False
    assert np.all(np.isnan(log_p[~good])) and np.all(np.isnan(score[~good]))
    np.testing.assert_array_equal(_bits(log_p[good]), _bits(clean_l[good]))
    np.testing.assert_array_equal(_bits(score[good]), _bits(clean_s[good]))


def test_device_tensors_stay_on_the_device():
    x, w, means, covs = R.case(2000, 4, 3)
    host_l, host_s = mixture.mixture_logpdf_score(x, w, means, covs)
    x_dev = torch.from_numpy(x.copy()).cuda()
    log_p, score = mixture.mixture_logpdf_score(x_dev, w, means, covs)
    assert torch.is_tensor(log_p) and torch.is_tensor(score)
    assert log_p.device == x_dev.device and score.device == x_dev.device
    assert log_p.shape == (2000,) and score.shape == (2000, 4)
    np.testing.assert_array_equal(_bits(log_p.cpu().numpy()), _bits(host_l))
    np.testing.assert_array_equal(_bits(score.cpu().numpy()), _bits(host_s))
    got = st.thin(x_dev, score, 40, preconditioner='med')
    np.testing.assert_array_equal(got, st.thin(x, host_s, 40, preconditioner='med'))
    e_l, e_s = mixture.mixture_logpdf_score(x_dev[:0], w, means, covs)
    assert e_l.shape == (0,) and e_s.shape == (0, 4) and e_l.device == x_dev.device


def test_one_dimensional_and_empty_samples():
    x, w, means, covs = R.case(2000, 1, 3)
    log_p, score = mixture.mixture_logpdf_score(x[:, 0], w, means, covs)
    want_l, want_s = R.oracle(2000, 1, 3)
    assert log_p.shape == (2000,) and score.shape == (2000, 1)
    close(log_p, want_l)
    close(score, want_s)
    log_p, score = mixture.mixture_logpdf_score(np.zeros((0, 1)), w, means, covs)
    assert log_p.shape == (0,) and score.shape == (0, 1)


def test_thin_on_the_reference_mixture_selects_the_reference_points(gm):
    sample, _, logpdf, score = gm
    _, gpu_score = mixture.make_mvn_mixture(models.GM_WEIGHTS, models.GM_MEANS, models.GM_COVS)
    got = st.thin(sample, gpu_score(sample), 40, preconditioner='med')
    np.testing.assert_array_equal(got, ref.thin(sample, score(sample), 40, preconditioner='med'))


def test_thin_gf_with_the_gpu_log_density_selects_the_reference_points(gm):
    sample, _, logpdf, _ = gm
    gpu_logpdf, _ = mixture.make_mvn_mixture(models.GM_WEIGHTS, models.GM_MEANS, models.GM_COVS)
    mean = np.mean(sample, axis=0)
    cov = np.cov(sample, rowvar=False, ddof=2)
    got = proxy.gaussian_thin(sample, gpu_logpdf(sample), mean, cov, 40)
    want = op.gaussian_thin(sample, logpdf(sample), mean, cov, 40)
    np.testing.assert_array_equal(got, want)


def test_mixture_thin_with_the_target_as_proxy_is_thin(gm):
    """thin_gf(q = p) is thin: the gradient-free operator with log_q == log_p reduces to the Langevin one."""
    sample = gm[0]
    log_p, score = mixture.mixture_logpdf_score(sample, models.GM_WEIGHTS, models.GM_MEANS, models.GM_COVS)
    got = proxy.mixture_thin(sample, log_p, models.GM_WEIGHTS, models.GM_MEANS, models.GM_COVS, 40)
    np.testing.assert_array_equal(got, st.thin(sample, score, 40, preconditioner='med'))


def test_marginal_log_density(gm):
    sample, _, logpdf, _ = gm
    gpu_logpdf, _ = mixture.make_mvn_mixture(models.GM_WEIGHTS, models.GM_MEANS, models.GM_COVS)
    close(gpu_logpdf(sample), logpdf(sample))
    _, marginal, _ = models.make_mvn_mixture(models.GM_WEIGHTS, models.GM_MEANS[:, :1], models.GM_COVS[:, :1, :1])
    close(gpu_logpdf(sample[:, 0], axes=0), marginal(sample[:, :1]))
    close(gpu_logpdf(sample[:, :1], axes=slice(0, 1)), marginal(sample[:, :1]))
    sub = [1, 0]
    _, swapped, _ = models.make_mvn_mixture(models.GM_WEIGHTS, models.GM_MEANS[:, sub],
                                            models.GM_COVS[:, sub][:, :, sub])
    close(gpu_logpdf(sample[:, ::-1], axes=slice(None, None, -1)), swapped(sample[:, ::-1]))


def test_d_above_64_is_not_implemented():
    with pytest.raises(NotImplementedError, match='64'):
        mixture.mixture_logpdf_score(np.zeros((3, 65)), [1.0], np.zeros((1, 65)), np.eye(65)[None])
    from stein_thinning import _native as nat
    p = torch.zeros(65 * 65, dtype=torch.float64, device='cuda')
    rc = nat.lib().st_mixture_logpdf_score(nat.ptr(p), 3, 65, 1, nat.ptr(p), nat.ptr(p), nat.ptr(p), nat.ptr(p),
                                           nat.ptr(p), None)
    with pytest.raises(NotImplementedError, match='64'):
        nat.check(rc, 'st_mixture_logpdf_score')


def _mixture_deep_n():
    """n at which block 0 of mixture_mfma_kernel takes four 64-row tiles and every other block three:
    launch_mixture_mfma's grid is min(tiles, 2 x CUs)."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    n = 64 * 3 * (2 * cus) + 21
    tiles = (n + 63) // 64
    grid = min(tiles, 2 * cus)
    assert (tiles // grid, (tiles + grid - 1) // grid) == (3, 4), (cus, n, tiles, grid)
    return n


@pytest.mark.parametrize('zero', [None, 0, 1, 2])
@pytest.mark.parametrize('d', [17, 64])
def test_persistent_tile_loop_and_cross_tile_prefetch(d, zero):
    """Every block goes three or four times round the matrix-core kernel's tile loop, so the prefetch of
    "the next component" wraps from the last component of one tile to component 0 of the next -- with all
    weights positive and with the first, the middle or the last component at weight 0 (the skip of an
    a_c = -inf component hands the prefetch on).  x tiles 509 distinct rows (a prime: every lane position
    sees every row); the first 509 outputs against the long-double restatement, every copy of a row bit for
    bit its first copy (the header promises position independence)."""
    n, m = _mixture_deep_n(), 509
    base, w, means, covs = R.case(m, d, 3)
    w = w.copy()
    if zero is not None:
        w[zero] = 0.0
    idx = torch.arange(n, device='cuda') % m
    xd = torch.from_numpy(base.copy()).cuda()[idx].contiguous()
    log_p, score = mixture.mixture_logpdf_score(xd, w, means, covs)
    assert log_p.shape == (n,) and score.shape == (n, d)
    want_l, want_s = R.stable(base, w, means, covs, dtype=np.longdouble)
    close(log_p[:m].cpu().numpy(), want_l.astype(np.float64))
    close(score[:m].cpu().numpy(), want_s.astype(np.float64))
    lb, sb = log_p.view(torch.int64), score.view(torch.int64)
    assert torch.equal(lb, lb[:m][idx]), 'log_p differs between copies of a row'
    assert torch.equal(sb, sb[:m][idx]), 'score differs between copies of a row'
