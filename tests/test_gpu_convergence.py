"""stein_thinning.convergence on the GPU (csrc/convergence.hip) against the long-double oracle of
tests/convergence_ref.py: ranks and p bit for bit, z within max(4 ulp, 2 E) of mpmath (E: scipy ndtri's own
worst error, convergence_ref.E_NDTRI_ULP), every autocovariance within its derived per-element bound on both
plans, every summary column within the bound propagated through tau, B and W, and the behaviour the host layer
promises (host = device input, repeatable bits, columns independent of their neighbours).

Recorded on MI355X: p equal on every case; worst z error 2-5 ulp (9.06 allowed); worst autocovariance error / bound
0.008-0.18 over the cases on both plans, 0.0009 on the 3 x 9001 series; worst summary column error / bound 0.081, the
largest relative bound 3.4e-11."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import convergence as conv  # noqa: E402
from tests import convergence_ref as R  # noqa: E402

CASE_IDS = [f'{C}x{n}-phi{phi}' for (C, n, phi), _ in R.CASES]
COLS = conv.COLUMNS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _columns():
    """name -> (C, n) column: the shared cases and the tie case."""
    cols = {cid: R.case_column(k) for k, cid in enumerate(CASE_IDS)}
    cols['ties'] = R.ties_column()
    return cols


@pytest.mark.parametrize('name', CASE_IDS + ['ties'])
def test_rank_p_bits_and_z(name):
    sp = R.split(_columns()[name])
    z, p = conv.rank_normalize(_dev(sp.reshape(1, -1)), want_p=True)
    p, z = p.cpu().numpy().reshape(sp.shape), z.cpu().numpy().reshape(sp.shape)
    want_p = R.rank_p(sp)
    np.testing.assert_array_equal(p, want_p)
    want_z = R.z_mp(want_p)
    err = np.abs(z - want_z) / np.spacing(np.abs(want_z))
    print(name, 'worst z error', err.max(), 'ulp; allowed', R.Z_TOL_ULP)
    assert err.max() <= R.Z_TOL_ULP


def _check_autocov(b, lag0, lag1, plan):
    S, h = b.shape
    ac, mu, v0, ser = conv.autocov(_dev(b[None]), lag0, lag1, plan=plan, per_series=True)
    want = R.acov_ld(b, lag0, lag1)
    bound = R.acov_bound(b, lag0, lag1)
    got = ser[0].cpu().numpy().astype(R.LD)
    ratio = float((np.abs(got - want) / bound).max())
    assert ratio <= 1, (ratio, plan, lag0, lag1)
    want_m = want.mean(axis=0)
    r2 = float((np.abs(ac[0].cpu().numpy().astype(R.LD) - want_m) / R.acov_mean_bound(want, bound)).max())
    assert r2 <= 1, (r2, plan)
    r3 = float((np.abs(mu[0].cpu().numpy().astype(R.LD) - b.astype(R.LD).mean(axis=1)) / R.mean_bound(b)).max())
    assert r3 <= 1, r3
    r4 = float((np.abs(v0[0].cpu().numpy().astype(R.LD) - R.acov_ld(b, 0, 1)[:, 0]) / R.acov_bound(b, 0, 1)[:, 0]).max())
    assert r4 <= 1, r4
    return max(ratio, r2, r3, r4)


@pytest.mark.parametrize('plan', [1, 2], ids=['long', 'short'])
@pytest.mark.parametrize('name', CASE_IDS + ['ties'])
def test_autocov_within_derived_bound(name, plan):
    b = R.split(_columns()[name])
    S, h = b.shape
    if plan == 2 and h > 2048:
        with pytest.raises(NotImplementedError):
            conv.autocov(_dev(b[None]), 0, 4, plan=2)
        return
    worst = _check_autocov(b, 0, h, plan)                      # every lag: the block ends at h
    if h >= 8:
        worst = max(worst, _check_autocov(b, h // 3, h, plan))     # lag0 > 0, ends at h
        worst = max(worst, _check_autocov(b, 3, min(h, 300), plan))  # lag0 > 0, past one lag tile where h allows
    print(name, 'plan', plan, 'worst error / bound', worst)


def test_autocov_long_plan_many_chunks_and_splits():
    """A series of several i chunks on the long plan: 3 x 9001, the i range split over blocks."""
    b = R.ar1(3, 9001, 0.95, 31)
    worst = max(_check_autocov(b, 0, 70, 1), _check_autocov(b, 250, 600, 1), _check_autocov(b, 8990, 9001, 1))
    print('worst error / bound', worst)


def test_autocov_auto_plan_and_bits_repeat():
    b = _dev(R.case_column(6).reshape(1, -1, 8))
    lib = conv.nat.lib()
    assert lib.st_autocov_plan(1, b.shape[1], 8, 0, 8, 0) == 2
    one = [t.cpu().numpy() for t in conv.autocov(b, 0, 8)]
    two = [t.cpu().numpy() for t in conv.autocov(b, 0, 8)]
    forced = [t.cpu().numpy() for t in conv.autocov(b, 0, 8, plan=2)]
    for x, y, w in zip(one, two, forced):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, w)


def _check_summary(a, want, label):
    got = conv.summary(_dev(a[:, :, None]))
    worst = 0.0
    for col in COLS:
        g = float(getattr(got, col)[0])
        v, bnd = want[col]
        if np.isnan(v):
            assert np.isnan(g), (label, col, g)
            continue
        assert bnd <= 1e-9 * abs(v), (label, col, v, bnd)
        r = abs(R.LD(g) - R.LD(v)) / bnd if bnd > 0 else (0.0 if g == v else np.inf)
        print(label, col, g, 'error / bound', float(r), 'relative bound', bnd / abs(v))
        assert r <= 1, (label, col, g, v, bnd)
        worst = max(worst, float(r))
    return worst


@pytest.mark.parametrize('k', range(len(R.CASES)), ids=CASE_IDS)
def test_summary_within_propagated_bound(k):
    _check_summary(R.case_column(k), R.case_summary(k), CASE_IDS[k])


def test_summary_ties_and_shifted_chain():
    _check_summary(R.ties_column(), R.summary_column(R.ties_column()), 'ties')
    a = R.shifted_column()
    _check_summary(a, R.summary_column(a), 'shifted')
    assert conv.rhat(a[:, :, None])[0] > 1.1


def test_stack_equals_columns_and_bits_repeat():
    x = R.stack_columns()
    whole = conv.summary(x)
    again = conv.summary(x)
    on_device = conv.summary(_dev(x))
    for col in COLS:
        np.testing.assert_array_equal(getattr(whole, col), getattr(again, col), err_msg=col)
        np.testing.assert_array_equal(getattr(whole, col), getattr(on_device, col), err_msg=col)
        assert getattr(whole, col).shape == (5,)
    for j in range(5):
        one = conv.summary(x[:, :, j:j + 1])
        for col in COLS:
            assert getattr(one, col)[0] == getattr(whole, col)[j], (j, col)
    for j in range(5):
        _check_summary(x[:, :, j], R.summary_column(x[:, :, j]), f'stack[{j}]')


def test_constant_and_nan_columns():
    x = R.stack_columns()[:, :, :3].copy()
    clean = conv.summary(x)
    x2 = x.copy()
    x2[:, :, 1] = 3.25
    s = conv.summary(x2)
    assert s.ess_bulk[1] == s.ess_tail[1] == x2.shape[0] * (x2.shape[1] // 2) * 2
    assert s.mean[1] == 3.25 and s.sd[1] == 0.0
    x3 = x.copy()
    x3[2, 100, 1] = np.nan
    s3 = conv.summary(x3)
    for col in COLS:
        assert np.isnan(getattr(s3, col)[1]), col
        for j in (0, 2):
            assert getattr(s3, col)[j] == getattr(clean, col)[j] == getattr(s, col)[j], (col, j)


def test_single_chain_and_methods():
    a = R.case_column(0)                      # (1, 8): r_hat of the two halves
    s = conv.summary(a[0][:, None])           # (n, d) input
    assert np.isfinite(s.r_hat[0])
    x = R.stack_columns()
    full = conv.summary(x, var_names=list('abcde'))
    np.testing.assert_array_equal(conv.ess(x, 'bulk'), full.ess_bulk)
    np.testing.assert_array_equal(conv.ess(x, 'tail'), full.ess_tail)
    np.testing.assert_array_equal(conv.rhat(x), full.r_hat)
    np.testing.assert_array_equal(conv.mcse(x, 'mean'), full.mcse_mean)
    np.testing.assert_array_equal(conv.mcse(x, 'sd'), full.mcse_sd)
    with pytest.raises(ValueError):
        conv.summary(x, var_names=['a'])


def test_mala_samples_go_straight_in():
    from stein_thinning import lotka_volterra as lv
    data = lv.reference_data()
    rng = np.random.default_rng(5)
    starts = np.log(lv.THETA) + 0.02 * rng.normal(size=(3, 4))
    run = lv.mala_sample(starts, 64, 0.001, seed=5, drift_cap=1.0, data=data, device_out=True)
    assert isinstance(run.samples, torch.Tensor) and run.samples.is_cuda
    s = conv.summary(run.samples)
    for col in COLS:
        v = getattr(s, col)
        assert v.shape == (4,) and np.all(np.isfinite(v)), (col, v)
