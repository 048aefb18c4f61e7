"""Dense preconditioners on the HIP engine (``pytest -m gpu``): pair values, greedy runs, ties, the
drop-in entry points with 'smpcov', KSD and the Gram matrix (data and CPU references: tests/dense_ref.py).

Error yardstick: the reference formula evaluated in np.longdouble gives, per pair, the value and
scale = |t1| + |t2| + |t3|; rho_ref = max |oracle (NumPy float64) - long double| / scale over a pair set is
the reference's own error there, and the GPU must stay within FACTOR = 8 x rho_ref on the same pairs: both
sides are d-term dot products with the same first-order bound, they differ in summation order and fma use,
the GPU's t1 avoids the reference's L.L product, and the maximum of a rounding statistic over a few
thousand pairs moves by about 2x.  Greedy runs must select the oracle's indices (its margins are asserted
first: decided far above rounding) with running sums within 2 m 8 rho_ref max(scale)."""
import warnings

import numpy as np
import pytest

from oracle import stein_numpy as o
from tests import dense_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)
if not R.longdouble_ok():
    pytest.skip('np.longdouble is no wider than float64 here: no error yardstick', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import stein as ss  # noqa: E402
from stein_thinning import thinning as st  # noqa: E402
from stein_thinning.device import DeviceProblem  # noqa: E402


def _problem(c, L=None):
    L = c['L'] if L is None else L
    return DeviceProblem(c['xs'], c['gs'], c['w'], 0.0, float(np.trace(L)), linv=L)


def _within(got, k_ld, scale, rho_ref, what):
    r = R.rho(got, k_ld, scale)
    print(f'{what}: rho_gpu = {r:.3e}, rho_ref = {rho_ref:.3e}, ratio = {r / rho_ref:.2f}')
    assert r <= R.FACTOR * rho_ref, (what, r, rho_ref)


@pytest.mark.parametrize('gf', [False, True])
@pytest.mark.parametrize('d', R.PAIR_DIMS)
def test_pairs_within_the_reference_error(d, gf):
    c = R.case(R.PAIR_N, d, 7, gf)
    i1, i2 = R.pair_set(R.PAIR_N)
    k_ld, scale = R.pair_ld(c, i1, i2)
    rho_ref = R.rho(R.integrand(c)(i1, i2), k_ld, scale)
    prob = _problem(c)
    got = prob.pairs(i1, i2)
    _within(got, k_ld, scale, rho_ref, f'pairs d={d} gf={gf}')
    if not gf:   # k(i, j) == k(j, i) bit for bit; the weights multiply in argument order, (k w_i) w_j, as the
        assert np.array_equal(got, prob.pairs(i2, i1))   # reference's do, so only the kernel value is symmetric


@pytest.mark.parametrize('d', [4, 12])
def test_dense_scaled_identity_agrees_with_the_isotropic_kernel(d):
    c = dict(R.case(R.PAIR_N, d, 7, True))
    c['L'] = 0.37 * np.identity(d)
    i1, i2 = R.pair_set(R.PAIR_N)
    k_ld, scale = R.pair_ld(c, i1, i2)
    rho_ref = R.rho(R.integrand(c)(i1, i2), k_ld, scale)
    dense = _problem(c).pairs(i1, i2)
    iso = DeviceProblem(c['xs'], c['gs'], c['w'], 0.37, float(np.trace(c['L']))).pairs(i1, i2)
    _within(dense, k_ld, scale, rho_ref, f'0.37 I dense d={d}')
    assert np.max(np.abs(dense - iso) / scale.astype(np.float64)) <= R.FACTOR * rho_ref


def _greedy_reference(n, d, seed, gf, m):
    """(indices, sums, tolerance of the sums) of the oracle, the margin precondition asserted first."""
    idx, sums, margin = R.greedy(n, d, seed, gf, m)
    assert margin >= R.MARGIN_MIN, margin
    c = R.case(n, d, seed, gf)
    rows = np.arange(n)
    rho_ref, smax = 0.0, 0.0
    for j in idx.astype(np.int64):               # every pair the run evaluates: all rows against each winner
        i2 = np.full(n, j)
        k_ld, scale = R.pair_ld(c, rows, i2)
        rho_ref = max(rho_ref, R.rho(R.integrand(c)(rows, i2), k_ld, scale))
        smax = max(smax, float(np.max(scale)))
    return idx, sums, 2 * m * R.FACTOR * rho_ref * smax


@pytest.mark.parametrize('n,d,seed,gf,m', R.GREEDY_CASES)
def test_greedy_selects_the_oracle_indices(n, d, seed, gf, m):
    idx, sums, tol = _greedy_reference(n, d, seed, gf, m)
    prob = _problem(R.case(n, d, seed, gf))
    L = nat.lib()
    prev = int(L.st_tune_get(0))
    try:
        if n > 10000:                             # few blocks: grid-stride looping, many rows per record
            nat.check(L.st_tune(0, 8), 'st_tune')
        got, a = prob.greedy(m, return_sums=True)
    finally:
        nat.check(L.st_tune(0, prev), 'st_tune')
    assert np.array_equal(got, idx)
    print(f'greedy n={n} d={d} gf={gf}: max |sum - oracle| = {np.max(np.abs(a - sums)):.3e}, tol = {tol:.3e}')
    assert np.max(np.abs(a - sums)) <= tol
    assert prob.near_tie is None and prob.fallback is None


def test_ties_go_to_the_lower_index_across_blocks():
    n, d, m = 1500, 4, 40
    c = R.case(n, d)
    idx = R.greedy(n, d, 7, False, m)[0]
    xs2, gs2 = np.vstack([c['xs'], c['xs'][:50]]), np.vstack([c['gs'], c['gs'][:50]])
    prob = DeviceProblem(xs2, gs2, None, 0.0, c['tr'], linv=c['L'])
    L = nat.lib()
    prev = int(L.st_tune_get(0))
    try:
        nat.check(L.st_tune(0, 3), 'st_tune')     # rows 0 .. 49 and their copies fall in different blocks
        got = prob.greedy(m)
    finally:
        nat.check(L.st_tune(0, prev), 'st_tune')
    assert np.array_equal(got, idx) and int(got.max()) < n
    assert np.array_equal(_problem(c).greedy(m), idx)


def test_thin_smpcov_end_to_end():
    n, d, m = 1500, 4, 40
    c = R.case(n, d)
    idx = R.greedy(n, d, 7, False, m)[0]
    assert np.array_equal(st.thin(c['x'], c['g'], m, preconditioner='smpcov'), idx)
    xt, gt = torch.from_numpy(c['x']).cuda(), torch.from_numpy(c['g']).cuda()
    assert np.array_equal(st.thin(xt, gt, m, preconditioner='smpcov'), idx)


def test_thin_gf_smpcov_end_to_end():
    n, d, m = 1500, 4, 40
    c = R.case(n, d, 7, True)
    idx = R.greedy(n, d, 7, True, m)[0]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = st.thin_gf(c['x'], c['log_p'], c['log_q'], c['g'], m, preconditioner='smpcov')
    assert np.array_equal(got, idx)


def test_dedup_gives_the_same_indices():
    m = 40
    c = R.case(1500, 4)
    x, g = np.repeat(c['x'][:500], 3, axis=0), np.repeat(c['g'][:500], 3, axis=0)
    try:
        st.set_dedup(False)
        want = st.thin(x, g, m, preconditioner='smpcov')
        st.set_dedup(True)
        assert np.array_equal(st.thin(x, g, m, preconditioner='smpcov'), want)
    finally:
        st.set_dedup(None)
    prob = st._make_stein_integrand(x, g, True, 'smpcov').device_problem()
    got, sums = prob.greedy(m, return_sums=True, dedup='always')
    assert prob.dedup_used and prob.dedup_view().problem.linv is not None
    assert np.array_equal(got, want)
    assert np.array_equal(sums, prob.greedy(m, return_sums=True)[1])


def test_thin_chains_equals_the_loop():
    m = 40
    xs = [R.case(1500, 4, s)['x'] for s in R.CHAIN_SEEDS]
    gs = [R.case(1500, 4, s)['g'] for s in R.CHAIN_SEEDS]
    want = [R.greedy(1500, 4, s, False, m)[0] for s in R.CHAIN_SEEDS]
    got = st.thin_chains(xs, gs, m, preconditioner='smpcov')
    loop = [st.thin(x, g, m, preconditioner='smpcov') for x, g in zip(xs, gs)]
    for a, b, w in zip(got, loop, want):
        assert np.array_equal(a, b) and np.array_equal(a, w)


def test_dense_runs_are_unguarded():
    c = R.case(1500, 4)
    integrand = st._make_stein_integrand(c['x'], c['g'], True, 'smpcov')
    st._greedy_search(40, integrand)
    prob = integrand.device_problem()
    assert prob.linv is not None and prob.guard_mode(True) is None and prob.near_tie is None
    idx, a, ws = prob.greedy_buffers(40)
    prob.greedy_launch(40, idx, a, ws)
    assert nat.near_tie_step(ws) == -2


def _integrands(d, gf):
    c = R.case(1500, d, 7, gf)
    if gf:
        dev = st._make_stein_gf_integrand(c['x'], c['log_p'], c['log_q'], c['g'], preconditioner='smpcov')
    else:
        dev = st._make_stein_integrand(c['x'], c['g'], preconditioner='smpcov')
    assert np.array_equal(dev.linv, c['L'])
    return c, dev, R.integrand(c)


@pytest.mark.parametrize('d,gf', R.KSD_CASES)
def test_kmat_is_symmetric_and_within_the_reference_error(d, gf):
    c, dev, ref = _integrands(d, gf)
    k = 200
    got = ss.kmat(dev, k)
    assert np.array_equal(got, got.T)
    a, b = np.meshgrid(np.arange(k), np.arange(k), indexing='ij')
    k_ld, scale = R.pair_ld(c, a.reshape(-1), b.reshape(-1))
    rho_ref = R.rho(o.kmat(ref, k).reshape(-1), k_ld, scale)
    _within(got.reshape(-1), k_ld, scale, rho_ref, f'kmat d={d} gf={gf}')


@pytest.mark.parametrize('d,gf', R.KSD_CASES)
def test_ksd_within_the_reference_error(d, gf):
    """The same 8 x rho rule on the KSD values themselves, against a long-double cumulative sum."""
    c, dev, ref = _integrands(d, gf)
    idx = R.greedy(1500, 4, 7, False, 40)[0].astype(np.int64)
    for rows, got in [(np.arange(1000), ss.ksd(dev, 1000)), (idx, ss.ksd(dev.reindex(idx), 40))]:
        m = rows.shape[0]
        want_ld = R.ksd_ld(c, rows)
        want = o.ksd(lambda a, b: ref(rows[a], rows[b]), m)
        rho_ref = float(np.max(np.abs(want.astype(np.longdouble) - want_ld) / want_ld))
        r = float(np.max(np.abs(got.astype(np.longdouble) - want_ld) / want_ld))
        print(f'ksd d={d} gf={gf} m={m}: rho_gpu = {r:.3e}, rho_ref = {rho_ref:.3e}')
        assert r <= R.FACTOR * rho_ref, (m, r, rho_ref)


def test_vfk0_imq_and_make_imq_take_a_dense_matrix():
    from stein_thinning import kernel as sk
    c = R.case(R.PAIR_N, 5)
    i1, i2 = R.pair_set(R.PAIR_N, 500)
    k_ld, scale = R.pair_ld(c, i1, i2)
    rho_ref = R.rho(R.integrand(c)(i1, i2), k_ld, scale)
    got = sk.vfk0_imq(c['xs'][i1], c['xs'][i2], c['gs'][i1], c['gs'][i2], c['L'])
    _within(got, k_ld, scale, rho_ref, 'vfk0_imq d=5')
    vfk0 = sk.make_imq(c['xs'], 'smpcov')
    assert np.array_equal(vfk0.linv, c['L'])
    assert np.array_equal(vfk0(c['xs'][i1], c['xs'][i2], c['gs'][i1], c['gs'][i2]), got)
    one = sk.vfk0_imq(c['xs'], c['xs'][[3]], c['gs'], c['gs'][[3]], c['L'])   # all rows against one
    assert np.array_equal(one, _problem(c).pairs(np.arange(R.PAIR_N), np.full(R.PAIR_N, 3)))


def test_seventeen_dimensions_are_refused():
    x, g, _ = R.raw(400, 17, 7)
    with pytest.raises(NotImplementedError, match='16'):
        st.thin(x, g, 10, preconditioner='smpcov')
