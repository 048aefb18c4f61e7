"""stein_thinning.convergence without a GPU: the oracle (tests/convergence_ref.py) behaves as the theory says,
the package's host Geyer routine reproduces the oracle's bit for bit, and every shared case keeps each Geyer
decision at least 100 bounds away from flipping, so the GPU comparison of tests/test_gpu_convergence.py is
between like and like (a condition on the cases, not a tolerance)."""
import numpy as np
import pytest

from stein_thinning import convergence as conv
from tests import convergence_ref as R


def test_oracle_ar1_ess_mean():
    phi = 0.9
    a = R.ar1(4, 20000, phi, 1)
    e = R.ess_of(R.split(a))['ess']
    want = a.size * (1 - phi) / (1 + phi)
    assert abs(e - want) <= 0.15 * want, (e, want)


def test_oracle_iid():
    a = R.ar1(4, 2000, 0.0, 2)
    s = R.summary_column(a)
    assert abs(s['ess_bulk'][0] - a.size) <= 0.2 * a.size, s['ess_bulk']
    assert s['r_hat'][0] < 1.01


def test_oracle_constant_and_nan_rules():
    c = np.full((2, 40), 3.25)
    assert R.ess_of(R.split(c))['ess'] == c.size
    a = R.ar1(2, 40, 0.3, 3)
    a[1, 7] = np.nan
    s = R.summary_column(a)
    assert all(np.isnan(s[k][0]) for k in conv.COLUMNS)


def test_oracle_shifted_chain_is_flagged():
    assert R.summary_column(R.shifted_column())['r_hat'][0] > 1.1


@pytest.mark.parametrize('k', range(len(R.CASES)))
def test_host_geyer_parity(k):
    a = R.case_column(k)
    for name, (b, _) in R.quantity_series(a).items():
        S, h = b.shape
        ac = R.acov_fft64(b).mean(axis=0)
        var_mu = np.var(b.mean(axis=1), ddof=1)
        want = R.geyer(ac, S, h, var_mu)
        got = conv.geyer_ess(ac, S, h, var_mu)
        assert got[0] == want[0] and got[1] == want[1], (name, got, want[:2])
        # fed lag blocks, the routine asks for more until the positive sequence has ended, then agrees
        K = min(h, 64)
        while conv.geyer_ess(ac[:K], S, h, var_mu, full=K >= h) is None:
            K = min(h, 2 * K)
        assert conv.geyer_ess(ac[:K], S, h, var_mu, full=K >= h) == got
        assert K >= min(h, want[1] + 2)


@pytest.mark.parametrize('k', range(len(R.CASES)))
def test_decisions_are_robust(k):
    s = R.case_summary(k)
    print(R.CASES[k], {q: f'{w:.3g}' for q, w in s['worst'].items()}, s['max_t'])
    for q, w in s['worst'].items():
        assert w >= 100, (R.CASES[k], q, w)


def test_decisions_are_robust_further_cases():
    cols = [R.ties_column(), R.shifted_column()] + [c for c in np.moveaxis(R.stack_columns(), 2, 0)]
    for j, a in enumerate(cols):
        s = R.summary_column(a)
        print(j, {q: f'{w:.3g}' for q, w in s['worst'].items()})
        for q, w in s['worst'].items():
            assert w >= 100, (j, q, w)


def test_device_bound_is_meaningful():
    """The acceptance bound of every ESS and R-hat column stays below 1e-9 relative on every shared case."""
    for k in range(len(R.CASES)):
        s = R.case_summary(k)
        for col in ('ess_bulk', 'ess_tail', 'ess_mean', 'ess_sd', 'r_hat', 'mcse_mean', 'mcse_sd', 'sd'):
            v, b = s[col]
            assert b <= 1e-9 * abs(v), (R.CASES[k], col, v, b)


def test_input_validation_needs_no_device():
    with pytest.raises(ValueError):
        conv.summary(np.zeros((2, 7, 3)))
    with pytest.raises(ValueError):
        conv.summary(np.zeros(16))
    with pytest.raises(ValueError):
        conv.summary(np.zeros((2, 2, 16, 3)))
    torch = pytest.importorskip('torch')
    with pytest.raises(ValueError):
        conv.summary(torch.zeros((2, 16, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        conv.ess(np.zeros((2, 16, 3)), method='median')
    import stein_thinning
    assert stein_thinning.summary is conv.summary
