"""Set-batched KSD and energy distance on the GPU (``pytest -m gpu``): one resident problem, many
arbitrary index sets, one result per set (st_ksd_sets / st_distance_sets) -- the reference's
naive-thinning curves.

Bars.  Column sums: bit-identical to st_ksd_colsum on each set's compact subset (same pair functions,
same sequential order per column).  KSD per set: 1e-12 relative of the NumPy oracle, the project's KSD
bar (tests/test_gpu_ksd.py).  Energy distance per set: 1e-10 of the oracle, the bar of the curve tests
(tests/test_gpu_energy.py); the sets' own triangles within 1e-13 of the existing triangle kernel's sums.
Golden: the reference figure's naive curves (tests/golden/gm_comparison_curves.json) within
test_gpu_energy.CURVE_RTOL = 1.5e-8 -- the oracle itself is 1.39e-8 ('ed/naive') and 1.12e-8
('ksd/naive', which carries the same naive energy-distance series) from them.
"""
import warnings

import numpy as np
import pytest

from oracle import stein_numpy as o

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import energy as se  # noqa: E402
from stein_thinning import naive  # noqa: E402
from stein_thinning import stein as ss  # noqa: E402
from stein_thinning import thinning as st  # noqa: E402
from tests import dense_ref, oracle_c  # noqa: E402
from tests.test_gpu_ksd import _problem  # noqa: E402

SIZES = [1, 2, 5, 63, 64, 65, 255, 256, 257, 513, 1, 700]
SIZES_D50 = [1, 31, 32, 33, 300]
CURVE_RTOL = 1.5e-8
N = 3000


def _sets(n, sizes, seed=17):
    """Random permutation slices; one set repeats a row, one row is shared by several sets."""
    rng = np.random.default_rng(seed)
    sets = [rng.permutation(n)[:m].astype(np.int64) for m in sizes]
    big = [k for k, m in enumerate(sizes) if m >= 5]
    sets[big[1]][3] = sets[big[1]][1]           # a repeated row inside one set
    for k in big[::2]:
        sets[k][0] = n // 2                     # one row in several sets
    return sets


def _offsets(sets):
    return np.concatenate([[0], np.cumsum([s.shape[0] for s in sets])]).astype(np.int64)


def _subset_colsum(prob, rows):
    """st_ksd_colsum over all rows of the compact subset (the existing path)."""
    sub = prob.subset(rows)
    m = rows.shape[0]
    cs = torch.zeros(sub.ld, dtype=torch.float64, device=sub.device)
    nat.check(nat.lib().st_ksd_colsum(nat.ptr(sub.x), nat.ptr(sub.g), nat.ptr(sub.w), m, sub.ld, sub.d, sub.l,
                                      sub.tr, 0, m, nat.ptr(cs), nat.stream_handle()), 'st_ksd_colsum')
    return cs[:m].cpu().numpy()


def _check_same_bits(dev, sets):
    prob = dev.device_problem()
    off = _offsets(sets)
    for mode in ('compact', 'exact'):
        with nat.arithmetic_override(mode):
            ks, cs = prob.ksd_sets(np.concatenate(sets), off, return_colsums=True)
            ks2, cs2 = prob.ksd_sets(np.concatenate(sets), off, return_colsums=True)
            assert np.array_equal(ks, ks2) and np.array_equal(cs, cs2)      # two runs: the same bits
            for k, rows in enumerate(sets):
                np.testing.assert_array_equal(cs[off[k]:off[k + 1]], _subset_colsum(prob, rows),
                                              err_msg=f'{mode}, set {k} (m = {rows.shape[0]})')


CASES = [(1, False, SIZES), (2, False, SIZES), (4, False, SIZES), (8, False, SIZES), (4, True, SIZES),
         (9, False, SIZES), (50, True, SIZES_D50)]


@pytest.fixture(scope='module')
def problems():
    cache = {}

    def get(d, gf):
        if (d, gf) not in cache:
            cache[d, gf] = _problem(N, d, gf)
        return cache[d, gf]
    return get


@pytest.mark.parametrize('d,gf,sizes', CASES, ids=[f'd{d}-{"gf" if gf else "langevin"}' for d, gf, _ in CASES])
def test_colsums_same_bits_as_compact_subset(problems, d, gf, sizes):
    dev, _ = problems(d, gf)
    _check_same_bits(dev, _sets(N, sizes))


@pytest.mark.parametrize('gf', [False, True])
def test_colsums_same_bits_with_rows_out_of_the_fast_range(gf):
    """A few rows with a coordinate below 2^-60: the per-pair rule decides (stein_math.hpp
    pair_value_sel), in the batched kernel as in st_ksd_colsum."""
    n, d = N, 4
    rng = np.random.default_rng(21)
    x = rng.normal(size=(n, d))
    g = -x + 0.1 * rng.normal(size=(n, d))
    sets = _sets(n, SIZES)
    for k in (3, 6, 9, 11):                      # rows that the sets use
        g[sets[k][2], 1] = 1e-25
        g[sets[k][sets[k].shape[0] // 2], 2] = 1e-25
    if gf:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            dev = st._make_stein_gf_integrand(x, -0.5 * np.sum(x * x, 1), -0.45 * np.sum(x * x, 1), g,
                                              preconditioner='med')
    else:
        dev = st._make_stein_integrand(x, g, preconditioner='med')
    r = int(sets[3][2])
    assert not oracle_c.compact_ok(dev.sample[[r]], dev.gradient[[r]], dev.linv_scale, dev.linv_trace)
    _check_same_bits(dev, sets)


@pytest.mark.parametrize('d,gf,sizes', CASES, ids=[f'd{d}-{"gf" if gf else "langevin"}' for d, gf, _ in CASES])
def test_ksd_sets_matches_oracle(problems, d, gf, sizes):
    dev, ref = problems(d, gf)
    sets = _sets(N, sizes)
    got = ss.ksd_sets(dev, sets)
    want = np.array([o.ksd(o.reindex_integrand(ref, s), s.shape[0])[-1] for s in sets])
    for k in range(len(sets)):
        print(f'set {k} m = {sizes[k]}: rel err {abs(got[k] - want[k]) / abs(want[k]):.3e}')
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # the forms ksd resolves: a reindex view and the harness's closure give the same batch
    perm = np.random.default_rng(2).permutation(N)
    inv = np.argsort(perm)
    assert np.array_equal(ss.ksd_sets(dev.reindex(perm), [inv[s] for s in sets]), got)
    assert np.array_equal(ss.ksd_sets(o.reindex_integrand(dev, perm), [inv[s] for s in sets]), got)


@pytest.mark.parametrize('d', [1, 2, 4, 9])
def test_energy_distance_sets(d):
    rng = np.random.default_rng(d)
    x = rng.normal(size=(1500, d))
    y = rng.normal(size=(333, d)) * 1.3 + 0.2
    sets = _sets(1500, SIZES)
    got = se.energy_distance_sets(y, x, sets)
    want = np.array([np.sqrt(o.energy_distance(y, x[s])) for s in sets])
    for k in range(len(sets)):
        print(f'set {k} m = {SIZES[k]}: rel err {abs(got[k] - want[k]) / abs(want[k]):.3e}')
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    assert np.array_equal(got, se.energy_distance_sets(y, x, sets))          # two runs: the same bits
    # the sets' own triangles against the existing triangle kernel on each subset
    dev = nat.require_device()
    soa, n, _, ld = se._soa(x, dev)
    rows = torch.from_numpy(np.concatenate(sets)).to(dev)
    self_sums, seg = se.distance_sets(soa, n, d, ld, rows, _offsets(sets))
    assert seg is None
    self_sums = self_sums.cpu().numpy()
    for k, s in enumerate(sets):
        sub, m, _, lds = se._soa(x[s], dev)
        tri = float(se._colsum(sub, m, lds, sub, m, lds, d, 0, m, True, dev, host=False).sum().item())
        assert abs(self_sums[k] - tri) <= 1e-13 * abs(tri), (k, self_sums[k], tri)


def test_golden_naive_energy_curves(gm, curves):
    sample, sample2, _, _ = gm
    c = np.array(curves['ed/naive'])
    M = c[:, 0].astype(int)
    got = se.energy_distance_sets(sample2, sample, [naive.naive_idx(1000, int(m)) for m in M])
    print(f"max rel err vs ed/naive: {np.max(np.abs(got - c[:, 1]) / c[:, 1]):.3e}")
    np.testing.assert_allclose(got, c[:, 1], rtol=CURVE_RTOL)
    assert np.array_equal(got, naive.naive_energy_curve(sample2, sample, M))
    # the figure's right panel carries the same naive series
    k = np.array(curves['ksd/naive'])
    assert np.array_equal(k[:, 0].astype(int), M)
    print(f"max rel err vs ksd/naive: {np.max(np.abs(got - k[:, 1]) / k[:, 1]):.3e}")
    np.testing.assert_allclose(got, k[:, 1], rtol=CURVE_RTOL)


def test_calculate_ksd_sets_against_oracle(gm):
    sample, _, _, score = gm
    gradient = score(sample)
    sizes = [1, 2, 5, 64, 65, 256, 257, 700, 1000]
    got = naive.naive_ksd_curve(sample, gradient, sizes)
    want = np.array([o.calculate_ksd(sample, gradient, naive.naive_idx(1000, m))[-1] for m in sizes])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert np.array_equal(got, naive.calculate_ksd_sets(sample, gradient, [naive.naive_idx(1000, m) for m in sizes]))


def test_many_small_sets(problems):
    dev, ref = problems(2, False)
    rng = np.random.default_rng(8)
    sets = [rng.integers(0, N, size=1 + k % 3) for k in range(5000)]
    got = ss.ksd_sets(dev, sets)
    want = np.array([o.ksd(o.reindex_integrand(ref, s), s.shape[0])[-1] for s in sets])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert np.array_equal(got, ss.ksd_sets(dev, sets))


def test_fallback_loop_empty_and_errors(problems):
    dev, _ = problems(4, False)
    assert ss.ksd_sets(dev, []).shape == (0,)
    with pytest.raises(ValueError):
        ss.ksd_sets(dev, [np.array([1, 2]), np.array([], dtype=int)])
    with pytest.raises(IndexError):
        ss.ksd_sets(dev, [np.array([0, N])])
    neg = ss.ksd_sets(dev, [np.array([-1, 5, -N])])
    assert np.array_equal(neg, ss.ksd_sets(dev, [np.array([N - 1, 5, 0])]))
    with pytest.raises(ValueError):
        se.energy_distance_sets(np.zeros((5, 2)), np.ones((9, 2)), [np.array([], dtype=int)])
    assert se.energy_distance_sets(np.zeros((5, 2)), np.ones((9, 2)), []).shape == (0,)
    sets = _sets(300, [1, 2, 40, 77])
    # a dense preconditioner and a wrapper that transforms the values: exactly the per-set loop
    c = dense_ref.case(300, 4)
    dense = st._make_stein_integrand(c['x'], c['g'], True, 'smpcov')
    assert dense.linv_dense is not None
    loop = np.array([ss.ksd(dense.reindex(s), s.shape[0])[-1] for s in sets])
    assert np.array_equal(ss.ksd_sets(dense, sets), loop)
    small = st._make_stein_integrand(c['x'], c['g'], True, 'med')

    def doubled(i1, i2):
        return 2.0 * small(i1, i2)
    loop = np.array([ss.ksd(o.reindex_integrand(doubled, s), s.shape[0])[-1] for s in sets])
    assert np.array_equal(ss.ksd_sets(doubled, sets), loop)
