"""CPU tier of the proxy producers' edge tests: the reference, bounds and recipes of tests/proxy_ref.py are
themselves right (no GPU).  The float64 restatements of every kernel's operation order stay inside the
derived bounds on every recipe, scipy and the oracle sit inside the U-form bound, the restated host factors
are the package's bit for bit, and the gap between the two Mahalanobis forms (|dev U|^2 against dev . P dev)
is below the rounding bound on the benign recipe and above it on the scaled one."""
import numpy as np
import pytest

from oracle import proxy_numpy as op
from tests import dense_ref
from tests import proxy_ref as R

needs_ld = pytest.mark.skipif(not dense_ref.longdouble_ok(), reason='np.longdouble is no wider than float64 here')

N = 257


def _inputs(name, d, df, n=N):
    c = R.recipe(name, n, d)
    whiten, precision, c_log = R.factors(name, n, d, df)
    return c['x'], c['loc'], whiten, precision, df, c_log


@pytest.mark.parametrize('d', [1, 4, 17, 64])
def test_factors_are_the_packages(d):
    """R.factors restates stein_thinning.proxy's host prep: the same doubles reach the kernel either way."""
    from scipy.special import gammaln
    from stein_thinning import proxy
    for name in ('benign', 'scaled'):
        cov = R.recipe(name, N, d)['cov']
        assert np.array_equal(cov, cov.T)
        psd = proxy._psd(cov, allow_singular=False)
        assert psd.rank == d
        whiten, precision, c_log = R.factors(name, N, d, 0.0)
        assert np.array_equal(whiten, psd.U) and np.array_equal(precision, np.linalg.inv(cov))
        assert c_log == psd.rank * proxy._LOG_2PI + psd.log_pdet
        _, _, c_t = R.factors(name, N, d, 30.5)
        t = 0.5 * (30.5 + d)
        assert c_t == float(gammaln(t) - gammaln(0.5 * 30.5) - d / 2. * np.log(30.5 * np.pi) - 0.5 * psd.log_pdet)


@pytest.mark.parametrize('name', R.RECIPES)
def test_recipes_hold_what_they_promise(name):
    d = 64
    c = R.recipe(name, N, d)
    assert c['x'].shape == (N, d) and not c['x'].flags.writeable
    cond = np.linalg.cond(c['cov'])
    if name in ('scaled', 'special_scaled'):
        assert 1e6 < cond < 1e9, cond
    else:
        assert cond < 18.5, cond
    if name == 'shifted':
        assert np.all(c['loc'] > 9e5) and np.max(np.abs(c['x'] - c['loc'])) < 100
    whiten, _, _ = R.factors(name, N, d, 0.0)
    radius = np.sqrt(np.sum(((c['x'] - c['loc']) @ whiten) ** 2, axis=1))
    at = R.at_loc(name, N)
    if name.startswith('special'):
        assert at.size == 61 and np.all(c['x'][at] == c['loc'])
        far = np.arange(*R.FAR_BLOCK)
        assert np.all(radius[far] > 0.99e140) and np.all(radius[far] < 1.01e140)
        rest = np.setdiff1d(np.arange(N), far)
        for k, want in enumerate(R.RADII[1:], start=1):
            got = radius[rest[rest % 4 == k]]
            assert np.all(np.abs(got / want - 1) < 1e-3), (k, got.min(), got.max())
    else:
        assert at.size == 0 and np.all(radius > 0)


@needs_ld
@pytest.mark.parametrize('d', sorted(set(R.MFMA_DIMS + R.VALU_DIMS)))
@pytest.mark.parametrize('name', R.RECIPES)
def test_emulations_inside_the_bounds(name, d):
    worst = {}
    for df in R.DFS:
        args = _inputs(name, d, df)
        r = R.reference(*args)
        assert all(np.all(np.isfinite(v)) for v in r.values())
        for variant in ((1, 2, 3) if 16 < d <= 64 else (1,)):
            lq, g = R.emulate(variant, *args)
            assert np.all(np.isfinite(lq)) and np.all(np.isfinite(g))
            out = R.check('valu' if variant == 1 else 'mfma', lq, g, r, what=f'{name} d={d} df={df} variant {variant}')
            for k, v in out.items():
                worst[k] = max(worst.get(k, 0.0), v)
            at = R.at_loc(name, N)
            assert np.all(lq[at] == (args[5] if df > 0 else -0.5 * args[5])) and np.all(g[at] == 0.0)
    print(f'{name} d={d}: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(worst.items())))


@needs_ld
@pytest.mark.parametrize('d', [3, 17, 50, 64])
@pytest.mark.parametrize('name', ['benign', 'scaled', 'shifted'])
def test_scipy_and_the_oracle_inside_the_u_form_bound(name, d):
    from scipy import stats
    c = R.recipe(name, N, d)
    for df in (0.0, 1.0, 30.5, 1e6):
        args = _inputs(name, d, df)
        r = R.reference(*args)
        if df == 0.0:
            lq = stats.multivariate_normal.logpdf(c['x'], mean=c['loc'], cov=c['cov'])
            wl, wg = op.gaussian_proxy(c['x'], c['loc'], c['cov'])
        else:
            lq = stats.multivariate_t.logpdf(c['x'], loc=c['loc'], shape=c['cov'], df=df)
            wl, wg = op.student_t_proxy(c['x'], c['loc'], c['cov'], df)
        assert np.array_equal(lq, wl)
        R.check('valu', lq, wg, r, what=f'scipy {name} d={d} df={df}')


@needs_ld
@pytest.mark.parametrize('d', R.MFMA_DIMS + [50])
def test_gap_between_the_two_forms_is_below_rounding_on_the_benign_recipe(d):
    """So the 1e-12 comparisons of tests/test_gpu_proxy.py against scipy mean what they say."""
    r = R.reference(*_inputs('benign', d, 0.0))
    assert np.all(r['gap'] <= r['tol_mP'])
    print(f'benign d={d}: largest gap / m = {float(np.max(r["gap"] / r["m_U"])):.2e}, '
          f'largest gap / tol_mP = {float(np.max(r["gap"] / r["tol_mP"])):.3f}')


@needs_ld
def test_gap_exceeds_rounding_on_the_scaled_recipe():
    """The figures of DESIGN.md section 1: the largest |m_P - m_U| / m over the matrix-core dims, per
    spread of the per-dimension scales."""
    for spread in (1.0, 1e2, 1e4):
        worst, cond, over = 0.0, 0.0, 0.0
        for d in R.MFMA_DIMS + [50]:
            c = R.recipe('scaled', N, d, spread)
            whiten, precision, c_log = R.factors('scaled', N, d, 0.0, spread)
            r = R.reference(c['x'], c['loc'], whiten, precision, 0.0, c_log)
            worst = max(worst, float(np.max(r['gap'] / r['m_U'])))
            over = max(over, float(np.max(r['gap'] / r['tol_mP'])))
            cond = max(cond, float(np.linalg.cond(c['cov'])))
        print(f'scaled, spread {spread:g}: cond up to {cond:.1e}, largest gap / m = {worst:.1e}, '
              f'largest gap / tol_mP = {over:.1e}')
        if spread == 1e4:
            assert over > 1.0 and worst > 1e-12
        if spread == 1.0:
            assert over <= 1.0
