"""The mixture fit without a GPU: the restatement of tests/mixture_fit_ref.py (monotone EM, weighted rows =
repeated rows, shift invariance of the centred M-step, its recorded float64 / long-double spread, scikit-learn
as an outside yardstick), the host pieces of stein_thinning.proxy (seeding, M-step, MixtureFit's criteria) and
every Python validation rule of fit_mixture, all of which fire before any launch."""
import numpy as np
import pytest

from stein_thinning import proxy
from tests import mixture_fit_ref as R


@pytest.mark.parametrize('shape', R.FIT_SHAPES)
def test_restated_em_is_monotone(shape):
    n, d, k = shape
    run = R.planted_em(n, d, k, 1e-8)
    h = np.array(run['history'])
    assert run['n_iter'] >= 5 and np.all(np.diff(h) >= -1e-13)
    # the returned parameters are the ones the last ll was evaluated at
    x = R.planted(n, d, k)[0]
    st = R.stats(x, None, R.factors(run['weights'], run['means'], run['covs']), np.float64, want_bound=False)
    assert float(st['LL'] / n) == run['ll']


@pytest.mark.parametrize('shape', R.FIT_SHAPES)
@pytest.mark.parametrize('tol', R.FIT_TOLS)
def test_recorded_spread(shape, tol):
    n, d, k = shape
    x, w0, m0, c0 = R.planted(n, d, k)
    run = R.planted_em(n, d, k, tol)
    ld = R.em(x, None, w0, m0, c0, tol=tol, max_iter=200, dtype=np.longdouble)
    assert ld['n_iter'] == run['n_iter']
    s = R.spread(run, ld)
    print(shape, tol, 'float64 against long double:', s)
    assert s <= R.RECORDED


def test_bound_is_not_vacuous_and_holds_for_float64_numpy():
    for n, d, k, weighted in [(257, 4, 3, True), (65, 16, 7, False), (63, 1, 32, True)]:
        x, om, w, mu, cv = R.inputs(n, d, k, weighted)
        fac = R.factors(w, mu, cv)
        want = R.stats(x, om, fac)
        got = R.stats(x, om, fac, np.float64, want_bound=False)
        print(n, d, k, 'worst error / bound', R.check((got['LL'], got['N'], got['S'], got['Q']), want))


def test_weighted_rows_equal_repeated_rows():
    x, w0, m0, c0 = R.planted(3000, 4, 3)
    reps = np.random.default_rng(5).integers(1, 4, size=600)
    base = x[:600]
    a = R.em(np.repeat(base, reps, axis=0), None, w0, m0, c0, tol=1e-8)
    b = R.em(base, reps.astype(np.float64), w0, m0, c0, tol=1e-8)
    assert a['n_iter'] == b['n_iter'] and R.spread(a, b) <= R.ALLOW
    # weight 0 removes a row, whatever it holds
    om = np.ones(600)
    om[::7] = 0.0
    dirty = base.copy()
    dirty[::7] = np.nan
    c = R.em(dirty, om, w0, m0, c0, tol=1e-8)
    e = R.em(base[om > 0], None, w0, m0, c0, tol=1e-8)
    assert c['n_iter'] == e['n_iter'] and R.spread(c, e) == 0.0


def test_m_step_is_invariant_to_a_shift():
    x, om, w, mu, cv = R.inputs(257, 4, 3, True)
    shift = 1e4
    xs = x + shift                                       # rounds every coordinate by <= 1e4 * 2^-53 ~ 1e-12
    for step in (R.m_step, proxy.mixture_m_step):
        out = []
        for rows, means in ((x, mu), (xs, mu + shift)):
            st = R.stats(rows, om, (R.factors(w, mu, cv)[0], means, R.factors(w, mu, cv)[2]), np.float64, want_bound=False)
            out.append(step(float(np.sum(om)), means, st['N'], st['S'], st['Q'], 1e-6))
        np.testing.assert_allclose(out[1][0], out[0][0], rtol=0, atol=1e-10)
        np.testing.assert_allclose(out[1][1] - shift, out[0][1], rtol=0, atol=1e-10)
        np.testing.assert_allclose(out[1][2], out[0][2], rtol=0, atol=1e-10)
    # the package's M-step is the restatement's
    st = R.stats(x, om, R.factors(w, mu, cv), np.float64, want_bound=False)
    for a, b in zip(proxy.mixture_m_step(float(np.sum(om)), mu, st['N'], st['S'], st['Q'], 1e-6),
                    R.m_step(float(np.sum(om)), mu, st['N'], st['S'], st['Q'], 1e-6)):
        np.testing.assert_array_equal(a, b)


def test_seeding():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(500, 3))
    a = proxy.kmeanspp_seeds(x, 8, seed=4)
    np.testing.assert_array_equal(a, proxy.kmeanspp_seeds(x.copy(), 8, seed=4))     # deterministic in seed
    assert not np.array_equal(a, proxy.kmeanspp_seeds(x, 8, seed=5))
    for seed in range(20):                                                           # distinct rows: no row twice
        s = proxy.kmeanspp_seeds(x[:12], 12, seed=seed)
        assert sorted(s.tolist()) == list(range(12))
    dup = np.repeat(x[:3], 4, axis=0)                                                # 3 distinct rows among 12
    s = proxy.kmeanspp_seeds(dup, 3, seed=1)
    assert len({tuple(dup[i]) for i in s}) == 3
    assert proxy.kmeanspp_seeds(dup, 5, seed=1).shape == (5,)                        # more seeds than distinct rows
    with pytest.raises(ValueError):
        proxy.kmeanspp_seeds(x, 0)
    with pytest.raises(ValueError):
        proxy.kmeanspp_seeds(x[:3], 4)
    # D^2 sampling finds far clusters: three well separated blobs get one seed each
    blobs = np.concatenate([rng.normal(size=(100, 2)) + c for c in ([0, 0], [50, 0], [0, 50])])
    for seed in range(5):
        s = proxy.kmeanspp_seeds(blobs, 3, seed=seed)
        assert sorted((s // 100).tolist()) == [0, 1, 2]


def test_criteria():
    k, d, n = 3, 4, 1000.0
    fit = proxy.MixtureFit(np.full(k, 1 / 3), np.zeros((k, d)), np.repeat(np.eye(d)[None], k, 0), -5.25, 7, True,
                           (-6.0, -5.25), n)
    assert fit.n_parameters == (k - 1) + k * d + k * d * (d + 1) // 2 == 44
    assert fit.bic == -2 * -5.25 * n + 44 * np.log(n)
    assert fit.aic == -2 * -5.25 * n + 2 * 44
    with pytest.raises(Exception):
        fit.n_iter = 3                                    # frozen
    with pytest.raises(ValueError, match='points'):
        fit.proxy()


def test_criteria_match_scikit_learn():
    mix = pytest.importorskip('sklearn.mixture')
    n, d, k = 3000, 4, 3
    x, w0, m0, c0 = R.planted(n, d, k)
    run = R.planted_em(n, d, k, 1e-8)
    gm = mix.GaussianMixture(k, covariance_type='full')
    gm.weights_, gm.means_, gm.covariances_ = run['weights'], run['means'], run['covs']
    gm.precisions_cholesky_ = np.linalg.cholesky(np.linalg.inv(run['covs']))
    fit = proxy.MixtureFit(run['weights'], run['means'], run['covs'], run['ll'], run['n_iter'], True,
                           tuple(run['history']), float(n))
    assert abs(gm.bic(x) - fit.bic) <= 1e-9 * abs(fit.bic)
    assert abs(gm.aic(x) - fit.aic) <= 1e-9 * abs(fit.aic)


@pytest.mark.parametrize('shape', R.FIT_SHAPES + [(1500, 3, 4)])
def test_iteration_count_of_scikit_learn(shape):
    mix = pytest.importorskip('sklearn.mixture')
    n, d, k = shape
    x, w0, m0, c0 = R.planted(n, d, k)
    run = R.planted_em(n, d, k, 1e-8)
    gm = mix.GaussianMixture(k, covariance_type='full', tol=1e-8, max_iter=200, reg_covar=1e-6, weights_init=w0,
                             means_init=m0, precisions_init=np.linalg.inv(c0)).fit(x)
    print(shape, 'n_iter', run['n_iter'], gm.n_iter_, 'll difference', gm.lower_bound_ - run['ll'])
    assert gm.converged_ and gm.n_iter_ == run['n_iter']
    assert abs(gm.lower_bound_ - run['ll']) <= 1e-12     # two float64 evaluations of a sum of n terms of size <= 30


def test_validation_before_any_launch(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError('validation must not touch the device')
    monkeypatch.setattr(proxy.nat, 'require_device', no_device)
    monkeypatch.setattr(proxy.MixtureEStep, 'record', no_device)
    x = np.random.default_rng(1).normal(size=(40, 3))
    ok = dict(weights_init=np.full(2, 0.5), means_init=x[:2], covs_init=np.repeat(np.eye(3)[None], 2, 0))
    bad = [
        (dict(sample=np.zeros((4, 3, 2)), k=2), ValueError),
        (dict(sample=np.zeros((0, 3)), k=1), ValueError),
        (dict(sample=x, k=0), ValueError),
        (dict(sample=x, k=2.5), ValueError),
        (dict(sample=x[:20], k=21), ValueError),
        (dict(sample=x, k=33), NotImplementedError),
        (dict(sample=np.zeros((40, 17)), k=2), NotImplementedError),
        (dict(sample=np.where(np.arange(120).reshape(40, 3) == 5, np.nan, x), k=2), ValueError),
        (dict(sample=np.where(np.arange(120).reshape(40, 3) == 5, np.inf, x), k=2), ValueError),
        (dict(sample=x, k=2, row_weights=np.ones(39)), ValueError),
        (dict(sample=x, k=2, row_weights=-np.ones(40)), ValueError),
        (dict(sample=x, k=2, row_weights=np.full(40, np.nan)), ValueError),
        (dict(sample=x, k=2, row_weights=np.zeros(40)), ValueError),
        (dict(sample=x, k=2, **{**ok, 'weights_init': np.ones(3)}), ValueError),
        (dict(sample=x, k=2, **{**ok, 'weights_init': np.array([-1.0, 2.0])}), ValueError),
        (dict(sample=x, k=2, **{**ok, 'means_init': x[:3]}), ValueError),
        (dict(sample=x, k=2, **{**ok, 'covs_init': np.eye(3)}), ValueError),
        (dict(sample=x, k=2, **{**ok, 'covs_init': np.repeat(np.array([[1.0, 2, 0], [0, 1, 0], [0, 0, 1]])[None], 2, 0)}),
         ValueError),                                             # not symmetric
        (dict(sample=x, k=2, tol=0.0), ValueError),
        (dict(sample=x, k=2, max_iter=0), ValueError),
        (dict(sample=x, k=2, reg_covar=-1.0), ValueError),
    ]
    for kw, exc in bad:
        kw = dict(kw)
        with pytest.raises(exc):
            proxy.fit_mixture(kw.pop('sample'), kw.pop('k'), **kw)
    with pytest.raises(np.linalg.LinAlgError):                   # a singular covariance raises as mixture_factors does
        proxy.fit_mixture(x, 2, **{**ok, 'covs_init': np.zeros((2, 3, 3))})
    # valid arguments get as far as the first launch
    with pytest.raises(AssertionError, match='device'):
        proxy.fit_mixture(x, 2, **ok)
    with pytest.raises(AssertionError, match='device'):
        proxy.fit_mixture(x, 2, seed=3, row_weights=np.ones(40))
