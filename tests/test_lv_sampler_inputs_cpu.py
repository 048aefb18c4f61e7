"""The conditions the GPU edge tests of the LV samplers rely on (tests/test_gpu_lv_sampler_edges.py), checked
without a device on the table of tests/sampler_ref.py -- conditions on the inputs, not tolerances, with nothing left
out: at every row of every host chain (3 x 9 per set and sampler) theta is finite and positive, scipy ends with
status 0, no attempted step is nearer than lv_ref.MARGIN_MIN to a flipped decision (so the kernels' step sequence
is scipy's), the sequential-order solve takes scipy's accepted and rejected counts, |log_p| > 0.1, and no MALA
drift is NaN; across the table some drift components are clipped and some are not.  scipy's own reordering noise
delta is under lv_ref.NOISE_CAP for every pair but those of sampler_ref.LOG_P_EXCEPTIONS, which really are over it.
A GPU failure on these inputs is then the kernels', not the inputs'."""
import numpy as np
import pytest

from tests import lv_ref as R
from tests import sampler_ref as S

PAIRS = [(kind, name) for kind in ('rw', 'mala') for name in S.SETS[kind]]


def test_the_table_is_the_one_the_gpu_tests_were_set():
    assert S.RW_SETS[:-1] == S.MALA_SETS[:-1] and S.RW_SETS[-1] == 'grid_outside' and S.MALA_SETS[-1] == 'mala_outside'
    assert set(S.RW_SETS) <= set(R.input_sets()) and 'loose' not in S.RW_SETS and 'cov_asym' not in S.RW_SETS
    for kind in ('rw', 'mala'):
        assert list(S.RECORDED[kind]) == S.SETS[kind]
    assert {k for k, _ in S.LOG_P_EXCEPTIONS} == {'rw'} and all(n in S.RW_SETS for _, n in S.LOG_P_EXCEPTIONS)
    x0, z, log_u = S.noise()
    assert x0.shape == (3, 4) and z.shape == (3, 8, 4) and log_u.shape == (3, 8) and np.all(np.isneginf(log_u))
    assert len(set(S.STEP4)) == 4 and len(set(S.EPS4)) >= 3          # a wrongly indexed step is visible
    s = S.input_set('mala_outside')
    np.testing.assert_array_equal(s.data.t, np.linspace(-0.1, 25.1, 90))
    assert (s.rtol, s.atol, tuple(s.data.t_span), tuple(s.data.u_init)) == (1e-3, 1e-6, (0.0, 25.0), (1.0, 1.0))
    # what the sampler suites hold fixed and these sets move
    I = S.input_set
    for name in ('cov_pos', 'cov_neg'):
        cov = I(name).data.cov
        assert abs(cov[0, 1]) > 0.01 and np.array_equal(cov, cov.T) and np.all(np.linalg.eigvalsh(cov) > 0)
    assert (I('tol5').rtol, I('tol5').atol) == (1e-5, 1e-8) and (I('tol7_sparse').rtol, I('tol7_sparse').atol) == (1e-7, 1e-10)
    assert tuple(I('span').data.t_span) == (1.0, 9.5) and tuple(I('span').data.u_init) == (0.8, 1.7)
    assert [I(f'grid_{n}').data.t.size for n in (1, 2, 3, 63, 64, 65, 129)] == [1, 2, 3, 63, 64, 65, 129]
    assert np.any(np.diff(I('grid_repeats').data.t) == 0)
    for name in ('grid_outside', 'mala_outside'):
        assert I(name).data.t[0] < 0.0 and I(name).data.t[-1] > 25.0


@pytest.mark.parametrize('kind,name', PAIRS)
def test_conditions_on_every_row_and_the_noise_cap(kind, name):
    seq = R.sequential_available()
    r = S.host_chain(kind, name, seq)
    theta = np.exp(r.samples)
    assert np.all(np.isfinite(theta)) and np.all(theta > 0)
    assert r.status.shape == (S.CHAINS * S.ROWS,) and not r.status.any()
    assert r.margin >= R.MARGIN_MIN, r.margin
    assert np.all(np.isfinite(r.log_p)) and np.abs(r.log_p).min() > 0.1, np.abs(r.log_p).min()
    if kind == 'mala':
        eps, h, _, c = S.mala_ref.constants(S.EPS4, S.CAP)
        assert not np.isnan(S.mala_ref.drift(r.grad, h, c)).any()
    rec = S.RECORDED[kind][name]
    assert r.margin >= rec[2] / R.DRIFT_FACTOR
    if not seq:
        print(f"        '{name}': (-, -, {r.margin:.1e}),   # this scipy lacks the sequential-order solver")
        return
    assert r.same_counts
    dl, dg = S.deltas(kind, name)
    print(f"        '{name}': ({dl:.1e}, {dg:.1e}, {r.margin:.1e}),   # smallest |log_p| {np.abs(r.log_p).min():.3g}"
          + (f', clipped {int(r.clipped.sum())} of {r.clipped.size}' if kind == 'mala' else ''))
    assert dg <= R.NOISE_CAP
    assert dl <= R.DRIFT_FACTOR * rec[0] and dg <= R.DRIFT_FACTOR * rec[1]
    if (kind, name) in S.LOG_P_EXCEPTIONS:
        # no exception outlives its reason
        assert R.NOISE_CAP < dl <= R.DRIFT_FACTOR * S.LOG_P_EXCEPTIONS[(kind, name)]
    else:
        assert dl <= R.NOISE_CAP


def test_some_drift_components_are_clipped_and_some_are_not():
    clipped = np.stack([S.host_chain('mala', name).clipped for name in S.MALA_SETS])
    print('clipped drift components per set:', dict(zip(S.MALA_SETS, clipped.reshape(len(S.MALA_SETS), -1).sum(axis=1).tolist())),
          'of', clipped[0].size)
    assert clipped.any() and not clipped.all()


def test_the_host_chains_are_the_recursions():
    """Row k+1 from row k alone, in NumPy's operation order -- what the GPU test compares bit for bit."""
    x0, z, _ = S.noise()
    rw = S.host_chain('rw', 'grid_2')
    np.testing.assert_array_equal(rw.samples[:, 0], x0)
    np.testing.assert_array_equal(rw.samples[:, 1:], rw.samples[:, :-1] + S.STEP4 * z)
    m = S.host_chain('mala', 'grid_2')
    eps, h, _, c = S.mala_ref.constants(S.EPS4, S.CAP)
    np.testing.assert_array_equal(m.samples[:, 1:], (m.samples[:, :-1] + np.clip(h * m.grad[:, :-1], -c, c)) + eps * z)
    # the 10-state evaluation is mala_ref.evaluate's when that is given the set's tolerances
    s = S.input_set('tol5')
    lp, g, _ = S.evaluate(x0[0], s)
    want = S.mala_ref.evaluate(x0[0], s.data, s.rtol, s.atol)
    assert lp == want[0] and np.array_equal(g, want[1])
    assert lp != S.mala_ref.evaluate(x0[0], s.data)[0]
