"""The Gaussian-mixture fit on the GPU (csrc/mixture_fit.hpp via st_mixture_em_stats; stein_thinning.proxy:
MixtureEStep, fit_mixture, mixture_fit_thin).  Every entry of the statistics against the long-double
restatement within the derived bound of tests/mixture_fit_ref.py, across the tile edges, every component
grouping and with row weights; the special rows and components; log_p_out bit for bit the mixture kernel's;
bit-reproducibility; every iterate of a fit on its own; the free-running fit against the float64 restatement
within mixture_fit_ref.ALLOW (10 x the recorded float64 / long-double spread of the restatement itself, 4e-15);
the row-weight behaviours; the fit through to thinning."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import mixture, proxy  # noqa: E402
from tests import mixture_fit_ref as R  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(x, om, weights, means, covs, what='', as_tensor=False):
    """The GPU statistics at (weights, means, covs) checked against the long-double restatement from the same
    float64 factors, log_p_out against the mixture kernel (``as_tensor``: the rows go in as a ROCm tensor, which
    may hold non-finite rows); returns (record, estimator, worst error / bound)."""
    fac = mixture.mixture_factors(weights, means, covs)
    est = proxy.MixtureEStep(torch.from_numpy(x).cuda() if as_tensor else x, om)
    rec = est.record(fac, log_p=True).copy()
    k, d = fac[1].shape
    got = proxy.unpack_em_record(rec, k, d)
    worst = R.check(got, R.stats(x, om, fac), what)
    assert np.array_equal(got[3], got[3].transpose(0, 2, 1))
    finite = np.all(np.isfinite(x), axis=1)
    want_lp = mixture.mixture_logpdf_score(x, weights, means, covs)[0]
    lp = est.log_p.cpu().numpy()
    np.testing.assert_array_equal(_bits(lp[finite]), _bits(want_lp[finite]))
    assert np.all(np.isnan(lp[~finite])) and np.all(np.isnan(want_lp[~finite]))
    return rec, est, worst


@pytest.mark.parametrize('k', R.COMPONENTS)
@pytest.mark.parametrize('d', R.DIMS)
def test_statistics_against_long_double(d, k):
    for n in R.ROWS:
        for weighted in (False, True):
            x, om, w, mu, cv = R.inputs(n, d, k, weighted)
            _, _, worst = _run(x, om, w, mu, cv, (n, d, k, weighted))
            print(n, d, k, weighted, 'worst error / bound', worst)


@pytest.mark.parametrize('d,k', [(4, 3), (8, 7), (16, 2)])
def test_several_tiles_per_block(d, k):
    x, om, w, mu, cv = R.inputs(4099, d, k, True)
    with nat.grid_cap(2):
        capped, est, worst = _run(x, om, w, mu, cv, 'grid cap 2')
        print(d, k, 'grid cap 2: worst error / bound', worst)
        np.testing.assert_array_equal(_bits(est.record(mixture.mixture_factors(w, mu, cv))), _bits(capped))
    free, _, _ = _run(x, om, w, mu, cv)            # another grid: another summation order, the same sums
    np.testing.assert_allclose(free, capped, rtol=0, atol=1e-12 * np.abs(free).max())


def test_zero_weight_component():
    x, om, w, mu, cv = R.inputs(257, 4, 3, True)
    rec3, _, _ = _run(x, om, w, mu, cv)
    # a fourth component of weight 0 in second place: its statistics exactly 0, the others' bits unchanged
    w4 = np.insert(w, 1, 0.0)
    mu4 = np.insert(mu, 1, mu[0] + 1.0, axis=0)
    cv4 = np.insert(cv, 1, cv[0], axis=0)
    rec4, _, _ = _run(x, om, w4, mu4, cv4)
    ll, n_c, s_c, q_c = proxy.unpack_em_record(rec4, 4, 4)
    assert n_c[1] == 0.0 and not s_c[1].any() and not q_c[1].any()
    e = 1 + 4 + 10
    body3, body4 = rec3[1:].reshape(3, e), rec4[1:].reshape(4, e)
    np.testing.assert_array_equal(_bits(body4[[0, 2, 3]]), _bits(body3))
    assert _bits(rec4[0]) == _bits(rec3[0])


def test_rows_of_weight_zero_may_hold_anything():
    x, om, w, mu, cv = R.inputs(257, 4, 3, True)
    zero = np.flatnonzero(om == 0)
    assert zero.size >= 3
    clean, _, _ = _run(x, om, w, mu, cv)
    dirty = x.copy()
    dirty[zero[0], 1] = np.nan
    dirty[zero[1]] = np.inf
    dirty[zero[2]] = 1e300
    got, _, _ = _run(dirty, om, w, mu, cv, as_tensor=True)
    with pytest.raises(ValueError, match='non-finite'):
        proxy.MixtureEStep(dirty, om)                # a NumPy sample is checked on the host
    np.testing.assert_array_equal(_bits(got), _bits(clean))
    # the same rows with a positive weight: LL is NaN, and fit_mixture's tensor path turns that into an error
    om2 = om.copy()
    om2[zero[0]] = 1.0
    rec = proxy.MixtureEStep(torch.from_numpy(dirty).cuda(), om2).record(mixture.mixture_factors(w, mu, cv))
    assert np.isnan(rec[0])
    with pytest.raises(ValueError, match='not finite'):
        proxy.fit_mixture(torch.from_numpy(dirty).cuda(), 3, row_weights=om2, weights_init=w, means_init=mu, covs_init=cv)


def test_far_tail_rows():
    # d = 2 and one row in eight: the bound grows with |l| (the rounding of q alone is |l| 2^-53 in r's exponent)
    # and at d = 4 would pass mixture_fit_ref.VACUOUS for rows this far out
    x, om, w, mu, cv = R.inputs(257, 2, 3, False)
    far = x.copy()
    far[::8] += 120.0                                # every l_ic of these rows is below -1e4
    fac = mixture.mixture_factors(w, mu, cv)
    want = R.stats(far, None, fac)
    l_max = want['log_p'][::8].astype(np.float64)
    assert np.all(l_max < -1e4)
    rec, est, worst = _run(far, None, w, mu, cv, 'far tail')
    print('far tail: worst error / bound', worst)
    assert np.all(np.isfinite(rec))
    n_c = proxy.unpack_em_record(rec, 3, 2)[1]
    assert abs(np.sum(n_c) - 257.0) <= float(np.sum(want['bound']['N']))    # sum_c r_ic stays 1


def test_data_far_from_the_origin():
    x, om, w, mu, cv = R.inputs(257, 4, 3, True, centre=1e4)
    rec, _, worst = _run(x, om, w, mu, cv, 'centre 1e4')
    print('centre 1e4: worst error / bound', worst)
    # the M-step from the centred statistics is the shifted problem's M-step
    x0, _, _, mu0, _ = R.inputs(257, 4, 3, True)
    rec0, _, _ = _run(x0, om, w, mu0, cv)
    a = proxy.mixture_m_step(float(np.sum(om)), mu, *proxy.unpack_em_record(rec, 3, 4)[1:], 1e-6)
    b = proxy.mixture_m_step(float(np.sum(om)), mu0, *proxy.unpack_em_record(rec0, 3, 4)[1:], 1e-6)
    # the shifted rows differ from x0 + 1e4 by the rounding of the shift, 1e4 * 2^-53 ~ 1e-12 per coordinate
    np.testing.assert_allclose(a[2], b[2], rtol=0, atol=1e-10)
    np.testing.assert_allclose(a[1] - 1e4, b[1], rtol=0, atol=1e-10)


@pytest.mark.parametrize('d,k', [(4, 3), (16, 7)])
def test_reproducible_bits_and_total_weight(d, k):
    x, om, w, mu, cv = R.inputs(4099, d, k, True)
    first, est, _ = _run(x, om, w, mu, cv)
    fac = mixture.mixture_factors(w, mu, cv)
    for _ in range(2):
        np.testing.assert_array_equal(_bits(est.record(fac)), _bits(first))
    other = proxy.MixtureEStep(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(om.copy()).cuda())
    np.testing.assert_array_equal(_bits(other.record(fac)), _bits(first))
    assert other._device['x'].data_ptr() == other.sample.data_ptr()           # used in place
    n_c = proxy.unpack_em_record(first, k, d)[1]
    bound = float(np.sum(R.stats(x, om, fac)['bound']['N']))
    assert abs(np.sum(n_c) - np.sum(om)) <= bound + 4 * R.U * np.sum(om)


def test_every_iterate_on_its_own():
    n, d, k = 3000, 4, 3
    x = R.planted(n, d, k)[0]
    run = R.planted_em(n, d, k, 1e-8)
    est = proxy.MixtureEStep(x)
    worst = 0.0
    for weights, means, covs in run['path']:
        fac = mixture.mixture_factors(weights, means, covs)
        got = proxy.unpack_em_record(est.record(fac), k, d)
        worst = max(worst, R.check(got, R.stats(x, None, fac), 'iterate'))
    print(len(run['path']), 'iterates: worst error / bound', worst)


def _same_fit(fit, run, allow=R.ALLOW):
    got = dict(ll=fit.log_likelihood, weights=fit.weights, means=fit.means, covs=fit.covs)
    s = R.spread(got, run)
    print('spread', s, 'allowed', allow)
    assert s <= allow


@pytest.mark.parametrize('tol', R.FIT_TOLS)
@pytest.mark.parametrize('shape', R.FIT_SHAPES)
def test_free_running_fit(shape, tol):
    n, d, k = shape
    x, w0, m0, c0 = R.planted(n, d, k)
    run = R.planted_em(n, d, k, tol)               # asserts that its stopping decision is not marginal
    fit = proxy.fit_mixture(x, k, weights_init=w0, means_init=m0, covs_init=c0, tol=tol, max_iter=200)
    assert fit.converged and fit.n_iter == run['n_iter'] == len(fit.history)
    # measured float64 / long-double spread of the restatement: <= R.RECORDED = 4e-15; allowed: 10 x that
    _same_fit(fit, run)
    np.testing.assert_allclose(fit.history, run['history'], rtol=0, atol=R.ALLOW)
    assert fit.log_likelihood == fit.history[-1]
    # the returned parameters are the ones the returned log likelihood was evaluated at
    ll = proxy.MixtureEStep(x).stats(fit.weights, fit.means, fit.covs)[0] / n
    assert ll == fit.log_likelihood


def test_row_weights_equal_repeated_rows():
    n, d, k = 3000, 4, 3
    x, w0, m0, c0 = R.planted(n, d, k)
    rng = np.random.default_rng(5)
    reps = rng.integers(1, 4, size=1000)
    base = x[:1000]
    repeated = np.repeat(base, reps, axis=0)
    kw = dict(weights_init=w0, means_init=m0, covs_init=c0, tol=1e-8, max_iter=200)
    plain = proxy.fit_mixture(repeated, k, **kw)
    weighted = proxy.fit_mixture(base, k, row_weights=reps.astype(np.float64), **kw)
    run = dict(ll=plain.log_likelihood, weights=plain.weights, means=plain.means, covs=plain.covs)
    assert weighted.n_iter == plain.n_iter and weighted.weight_sum == plain.weight_sum == float(reps.sum())
    _same_fit(weighted, run)
    # an RW chain's repeats, in runs: collapse_repeats sends each distinct row once
    collapsed = proxy.fit_mixture(repeated, k, collapse_repeats=True, **kw)
    assert collapsed.n_iter == plain.n_iter
    _same_fit(collapsed, run)
    assert abs(collapsed.bic - plain.bic) <= 1e-9 * abs(plain.bic)
    # seeded start: the seeding looks at the rows as given, so both start from the same means
    a = proxy.fit_mixture(repeated, k, seed=3)
    b = proxy.fit_mixture(repeated, k, seed=3, collapse_repeats=True)
    assert a.n_iter == b.n_iter
    _same_fit(b, dict(ll=a.log_likelihood, weights=a.weights, means=a.means, covs=a.covs))


def test_tensor_input_gives_the_same_bits():
    n, d, k = 3000, 4, 3
    x, w0, m0, c0 = R.planted(n, d, k)
    xt = torch.from_numpy(x.copy()).cuda()
    for kw in (dict(weights_init=w0, means_init=m0, covs_init=c0), dict(means_init=m0), dict(seed=1)):
        host = proxy.fit_mixture(x, k, **kw)
        dev = proxy.fit_mixture(xt, k, **kw)
        assert dev.n_iter == host.n_iter and dev.converged == host.converged
        if 'covs_init' in kw:                       # the same start: the same bits
            for name in ('weights', 'means', 'covs'):
                np.testing.assert_array_equal(_bits(getattr(dev, name)), _bits(getattr(host, name)))
            assert dev.history == host.history
        else:
            # the rows stay on the device, so the default start covariance is summed there: the two starts differ
            # by rounding and the fits are two free-running float64 runs, held to the same allowance R.ALLOW as
            # every other pair of them (measured: 1.5e-16 and 7.5e-17)
            _same_fit(dev, dict(ll=host.log_likelihood, weights=host.weights, means=host.means, covs=host.covs))
    assert dev.sample is xt
    with pytest.raises(ValueError, match='host sample'):
        proxy.fit_mixture(xt, k, collapse_repeats=True)


def test_through_to_thinning():
    from oracle import models
    sample, _, log_p, _, _ = models.bivariate_reference_sample(1000)
    fit = proxy.fit_mixture(sample, 2, seed=0)
    assert fit.n_parameters == 1 + 4 + 6
    idx = proxy.mixture_fit_thin(sample, log_p, 2, 20, seed=0)
    np.testing.assert_array_equal(idx, proxy.mixture_thin(sample, log_p, fit.weights, fit.means, fit.covs, 20))
    log_q, grad = fit.proxy()
    want = proxy.mixture_proxy(sample, fit.weights, fit.means, fit.covs)
    np.testing.assert_array_equal(_bits(log_q), _bits(want[0]))
    np.testing.assert_array_equal(_bits(grad), _bits(want[1]))
    pts = sample[:7] + 0.5
    np.testing.assert_array_equal(_bits(fit.proxy(pts)[0]), _bits(proxy.mixture_proxy(pts, fit.weights, fit.means, fit.covs)[0]))
