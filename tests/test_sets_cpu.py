"""Set-batched KSD / energy distance, the parts that need no GPU: the notebooks' naive index sets, the
protocol-loop form of ``stein.ksd_sets``, the host work-item table of the batched kernels
(``st_sets_work_items``) and the argument validation of ``st_ksd_sets`` / ``st_distance_sets``, every
case of which returns before any HIP call."""
import numpy as np
import pytest

from oracle import stein_numpy as o

COL_BLOCK = 256   # columns per work item (csrc/pairwise.hip kColBlock)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


@pytest.mark.parametrize('n,m', [(1000, 1), (1000, 40), (1000, 1000), (7, 20)])
def test_naive_idx_is_the_notebooks_expression(n, m):
    from stein_thinning import naive_idx
    got = naive_idx(n, m)
    want = np.linspace(0, n - 1, m).astype(int)
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_ksd_sets_protocol_loop_bit_for_bit():
    """A plain matrix-lookup integrand reaches no SteinIntegrand: ksd_sets is the loop of per-set
    ksd(...)[-1], the reference's own calls."""
    from stein_thinning import stein
    rng = np.random.default_rng(5)
    a = rng.normal(size=(40, 40))
    K = a @ a.T

    def integrand(i1, i2):
        return K[i1, i2]
    sets = [np.array([3]), np.array([1, 2, 5]), rng.permutation(40)[:17], np.array([7, 7, 3, -1]), np.arange(40)]
    got = stein.ksd_sets(integrand, sets)
    want = np.array([o.ksd(o.reindex_integrand(integrand, s), s.shape[0])[-1] for s in sets])
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert stein.ksd_sets(integrand, []).shape == (0,)
    with pytest.raises(ValueError):
        stein.ksd_sets(integrand, [np.array([1, 2]), np.array([], dtype=int)])
    with pytest.raises(IndexError):
        stein.ksd_sets(integrand, [np.array([1, 40])])


def _items(lib, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_sets = len(sizes)
    count = lib.st_sets_work_items(off.ctypes.data, n_sets, None, 0)
    assert count == sum((m + COL_BLOCK - 1) // COL_BLOCK for m in sizes)
    items = np.full((count, 2), -1, dtype=np.int32)
    assert lib.st_sets_work_items(off.ctypes.data, n_sets, items.ctypes.data, count) == count
    assert lib.st_sets_work_items(off.ctypes.data, n_sets, items.ctypes.data, count - 1) == -1
    return items


def _work(m, cb):
    c0, c1 = cb * COL_BLOCK, min((cb + 1) * COL_BLOCK, m)
    return sum(range(c0, c1))   # pairs a < j of the block's columns j


@pytest.mark.parametrize('sizes', [[1, 2, 255, 256, 257, 700], [1 + k % 3 for k in range(5000)]],
                         ids=['edges', '5000-small'])
def test_work_item_table(lib, sizes):
    items = _items(lib, sizes)
    want = {(s, cb) for s, m in enumerate(sizes) for cb in range((m + COL_BLOCK - 1) // COL_BLOCK)}
    got = [tuple(int(v) for v in it) for it in items]
    assert len(got) == len(set(got)) and set(got) == want          # every (set, column block) exactly once
    for s, cb in got:                                              # a block lies inside ONE set
        assert 0 <= cb * COL_BLOCK < sizes[s]
    work = [_work(sizes[s], cb) for s, cb in got]
    assert all(a >= b for a, b in zip(work, work[1:]))             # heaviest first


def test_work_item_table_rejects_bad_offsets(lib):
    for off in ([1, 2], [0, 3, 2], [0, 2, 2]):
        a = np.array(off, dtype=np.int64)
        assert lib.st_sets_work_items(a.ctypes.data, len(off) - 1, None, 0) == -1
    assert lib.st_sets_work_items(np.zeros(1, dtype=np.int64).ctypes.data, 0, None, 0) == 0
    assert lib.st_sets_work_items(None, 1, None, 0) == -1


def test_abi_validation_before_any_hip_call(lib):
    """Fake (never dereferenced) device addresses: every rejected call returns from the host-side checks;
    an accepted one would have to touch the device, which this host does not have."""
    from stein_thinning import _native as nat
    assert lib.st_abi_version() == 1
    dev, dev_odd, dev8 = 0x10000, 0x10004, 0x10008
    off = np.array([0, 3, 5], dtype=np.int64)
    op = off.ctypes.data
    big = 1 << 20

    def ksd(x=dev, g=dev, w=None, n=10, ld=16, d=4, rows=dev8, offsets=op, n_sets=2, ks=dev8, cs=None,
            ws=dev, wsb=big):
        return lib.st_ksd_sets(x, g, w, n, ld, d, 1.0, 4.0, rows, offsets, n_sets, ks, cs, ws, wsb, None)

    def dist(p=dev, ldp=16, n=10, d=4, rows=dev8, offsets=op, n_sets=2, so=dev8, rv=None, seg=None, ws=dev,
             wsb=big):
        return lib.st_distance_sets(p, ldp, n, d, rows, offsets, n_sets, so, rv, seg, ws, wsb, None)

    invalid = [
        ksd(x=None), ksd(g=None), ksd(rows=None), ksd(offsets=None), ksd(ks=None), ksd(ws=None),
        ksd(x=dev8), ksd(w=dev8), ksd(rows=dev_odd), ksd(ks=dev_odd), ksd(cs=dev_odd), ksd(ws=dev8),
        ksd(n_sets=-1), ksd(n=0), ksd(ld=12), ksd(d=0),
        ksd(wsb=lib.st_ksd_sets_workspace_bytes(5, 2, 4) - 1),
        dist(p=None), dist(rows=None), dist(offsets=None), dist(so=None), dist(ws=None),
        dist(p=dev8), dist(rows=dev_odd), dist(so=dev_odd), dist(ws=dev8), dist(rv=dev8), dist(seg=dev8),
        dist(n_sets=-1), dist(n=0), dist(ldp=12), dist(d=0),
        dist(wsb=lib.st_distance_sets_workspace_bytes(5, 2, 4) - 1),
    ]
    for a in ([1, 3, 5], [0, 3, 2], [0, 3, 3], [0, 0, 5]):   # not from 0, decreasing, empty sets
        keep = np.array(a, dtype=np.int64)
        invalid += [ksd(offsets=keep.ctypes.data), dist(offsets=keep.ctypes.data)]
    for k, rc in enumerate(invalid):
        assert rc == nat.ST_ERR_INVALID, k
    assert ksd(ks=None) == nat.ST_ERR_INVALID and b'NULL' in lib.st_last_error()
    empty = np.array([0, 3, 3], dtype=np.int64)
    assert ksd(offsets=empty.ctypes.data) == nat.ST_ERR_INVALID and b'empty' in lib.st_last_error()
    assert ksd(wsb=8) == nat.ST_ERR_INVALID and b'workspace' in lib.st_last_error()
    assert ksd(d=129) == nat.ST_ERR_UNSUPPORTED and b'129' in lib.st_last_error()
    assert dist(d=129) == nat.ST_ERR_UNSUPPORTED and b'129' in lib.st_last_error()
    # no sets: nothing to do, whatever else is passed
    assert ksd(n_sets=0, x=None, ws=None) == nat.ST_OK
    assert dist(n_sets=0, p=None, ws=None) == nat.ST_OK
    # workspace sizes: host only
    assert lib.st_ksd_sets_workspace_bytes(5, 2, 4) > 0 and lib.st_distance_sets_workspace_bytes(5, 2, 4) > 0
    assert lib.st_ksd_sets_workspace_bytes(5, 2, 129) == -1 and lib.st_ksd_sets_workspace_bytes(-1, 2, 4) == -1
    assert lib.st_distance_sets_workspace_bytes(5, -1, 4) == -1
