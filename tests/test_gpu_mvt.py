"""The multivariate-t fit on the GPU (csrc/mvt_moments.hpp via st_mvt_moments; stein_thinning.proxy:
StudentTLikelihood, fit_mvt, fit_mvt2).  Every sum against long double within 1e-12 * sum |term|
(tests/mvt_ref.py: the bound the float64 NumPy moments hold, tests/test_mvt_cpu.py), across the tile
edges, both kernel widths (d <= 8 in registers, 8 < d <= 16 split over the waves), several passes per
block, the extremes; bit-reproducibility; the likelihood and gradient against the NumPy restatement; the
fits against the reference's own finite-difference fit within 10 x the spread recorded in mvt_ref.RECORDED;
the downstream selection of thin_gf_t."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import proxy  # noqa: E402
from tests import mvt_ref as R  # noqa: E402


def _record(lik, loc, u, df, grad=True):
    """The raw output record of one evaluation (copy)."""
    return proxy._mvt_moments(lik, np.asarray(loc, dtype=np.float64), np.asarray(u, dtype=np.float64), float(df),
                              grad).copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(x, loc, u, df):
    lik = proxy.StudentTLikelihood(x)
    got = lik.moments(loc, u, df)
    worst = R.check_moments(got, x, loc, u, df)
    assert np.array_equal(got[3], got[3].T)
    s0 = lik.moments(loc, u, df, grad=False)
    assert s0[1:] == (None, None, None)
    assert _bits(s0[0]) == _bits(got[0])          # want_grad = 0: the same S0 bits
    return worst


@pytest.mark.parametrize('d', R.MOMENT_DIMS)
@pytest.mark.parametrize('n', R.MOMENT_ROWS)
def test_every_sum_against_long_double(n, d):
    x, loc, u = R.moment_inputs(d, n)
    for df in R.MOMENT_DFS:
        print(d, n, df, 'worst error / sum |term|', _check(x, loc, u, df))


@pytest.mark.parametrize('d', [4, 8, 9, 16])
def test_several_passes_per_block(d):
    x, loc, u = R.moment_inputs(d, 4097)
    with nat.grid_cap(2):
        print(d, 'grid cap 2: worst', _check(x, loc, u, 5.0))
        lik = proxy.StudentTLikelihood(x)
        capped = _record(lik, loc, u, 5.0)
        np.testing.assert_array_equal(_bits(_record(lik, loc, u, 5.0)), _bits(capped))
    free = _record(lik, loc, u, 5.0)               # another grid: another summation order, the same sums
    scale = np.abs(free).max()
    np.testing.assert_allclose(capped, free, rtol=0, atol=1e-12 * scale)


def test_long_sample_on_the_default_grid():
    x, loc, u = R.moment_inputs(4, 300_001)
    print('n = 300001: worst', _check(x, loc, u, 5.0))


@pytest.mark.parametrize('d', [4, 9])
def test_extremes(d):
    for name, (x, loc, u, df) in R.extreme_inputs(d).items():
        print(d, name, 'worst', _check(x, loc, u, df))
    x, loc, u, df = R.extreme_inputs(d)['all_at_loc']
    s0, s1, sz, szz = proxy.StudentTLikelihood(x).moments(loc, u, df)
    assert s0 == 0.0 and abs(s1 - 65 * (df + d) / df) <= 1e-13 * s1 and not sz.any() and not szz.any()


@pytest.mark.parametrize('d', [4, 16])
def test_reproducible_bits(d):
    x, loc, u = R.moment_inputs(d, 4097)
    lik = proxy.StudentTLikelihood(x)
    first = _record(lik, loc, u, 9.456)
    for _ in range(3):
        np.testing.assert_array_equal(_bits(_record(lik, loc, u, 9.456)), _bits(first))
    other = proxy.StudentTLikelihood(x.copy())       # another upload, workspace and output
    np.testing.assert_array_equal(_bits(_record(other, loc, u, 9.456)), _bits(first))
    x_dev = torch.from_numpy(x.copy()).cuda()
    on_device = proxy.StudentTLikelihood(x_dev)
    np.testing.assert_array_equal(_bits(_record(on_device, loc, u, 9.456)), _bits(first))
    assert on_device._device['x'].data_ptr() == x_dev.data_ptr()      # used in place


def test_tensor_validation():
    with pytest.raises(ValueError):
        proxy.StudentTLikelihood(torch.zeros((5, 4), dtype=torch.float32, device='cuda'))
    bad = torch.zeros((70, 4), dtype=torch.float64, device='cuda')
    bad[66, 2] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        proxy.StudentTLikelihood(bad).moments(np.zeros(4), np.eye(4), 5.0)
    with pytest.raises(ValueError, match='16'):
        proxy.StudentTLikelihood(torch.zeros((5, 17), dtype=torch.float64, device='cuda'))


@pytest.mark.parametrize('d,n,seed', R.FIT_CASES)
def test_nll_and_grad_against_the_numpy_restatement(d, n, seed):
    x = R.case(d, n, seed)[0]
    lik = proxy.StudentTLikelihood(x)
    start = R.start_and_bounds(x)[0]
    for par in (start, start * (1 + 0.05 * np.cos(np.arange(len(start))))):
        value, grad = lik.nll_and_grad(par)
        want_v, want_g = R.nll_grad(x, par)
        print(d, n, 'value', abs(value - want_v) / abs(want_v), 'grad', np.abs(grad - want_g).max() / np.abs(want_g).max())
        assert abs(value - want_v) <= 1e-12 * abs(want_v)
        assert np.abs(grad - want_g).max() <= 1e-12 * np.abs(want_g).max()
        assert _bits(lik.nll(par)) == _bits(value)


def _check_fit(res, want, base, diffs, recorded):
    print('fit: differences', diffs, 'fun rel', (res.fun - want.fun) / abs(want.fun), 'nfev', res.nfev, 'against',
          base.nfev, '(NumPy moments)', want.nfev, '(reference)')
    assert res.success
    assert res.fun <= want.fun + R.FTOL * abs(want.fun)
    for got, rec in zip(diffs, recorded):
        assert got <= R.BOUND_FACTOR * rec
    assert res.nfev < 3 * base.nfev


@pytest.mark.parametrize('d,n,seed', R.FIT_CASES)
def test_fit_mvt_against_the_reference_fit(d, n, seed):
    res = proxy.fit_mvt(R.case(d, n, seed)[0], R.MU_BOUNDS, R.A_BOUNDS, R.DF_BOUNDS)
    want = R.reference_fit(d, n, seed)
    _check_fit(res, want, R.numpy_fit(d, n, seed), R.fit_differences(res, want, d), R.RECORDED[(d, n)])


def test_fit_mvt_with_finite_differences_against_the_reference_fit():
    d, n, seed = R.FIT_CASES[1]
    res = proxy.fit_mvt(R.case(d, n, seed)[0], R.MU_BOUNDS, R.A_BOUNDS, R.DF_BOUNDS, jac=None)
    want = R.reference_fit(d, n, seed)
    _check_fit(res, want, R.numpy_fit(d, n, seed, None), R.fit_differences(res, want, d), R.RECORDED[(d, n)])


def test_fit_mvt2_against_the_reference_fit():
    d, n, seed = R.FIT_CASES[0]
    res = proxy.fit_mvt2(R.case(d, n, seed)[0], R.SCALE_BOUNDS, R.DF_BOUNDS, R.mode_row(d, n, seed))
    want = R.reference_fit2(d, n, seed)
    _check_fit(res, want, R.numpy_fit2(d, n, seed), R.fit2_differences(res, want), R.RECORDED['fit_mvt2'])


def test_fit_accepts_a_device_tensor():
    d, n, seed = R.FIT_CASES[1]
    x = R.case(d, n, seed)[0]
    res = proxy.fit_mvt(torch.from_numpy(x.copy()).cuda(), R.MU_BOUNDS, R.A_BOUNDS, R.DF_BOUNDS)
    host = proxy.fit_mvt(x, R.MU_BOUNDS, R.A_BOUNDS, R.DF_BOUNDS)
    np.testing.assert_array_equal(_bits(res.x), _bits(host.x))
    assert res.nfev == host.nfev


def test_thin_gf_t_with_the_fitted_proxy_selects_the_reference_points():
    """Fit -> proxy -> thin on the (4, 4000) case, the target a seeded Gaussian's log density: the GPU
    fit's parameters select the 20 points the reference fit's parameters select."""
    from scipy import stats
    d, n, seed = R.FIT_CASES[0]
    x, loc, sigma, _ = R.case(d, n, seed)
    rng = np.random.default_rng(77)
    log_p = stats.multivariate_normal.logpdf(x, loc + 0.01 * rng.normal(size=d), 1.5 * sigma)
    got = proxy.thin_gf_t(x, log_p, *proxy.extract_t_params(proxy.fit_mvt(x, R.MU_BOUNDS, R.A_BOUNDS, R.DF_BOUNDS).x, d), 20)
    want = proxy.thin_gf_t(x, log_p, *proxy.extract_t_params(R.reference_fit(d, n, seed).x, d), 20)
    np.testing.assert_array_equal(got, want)
