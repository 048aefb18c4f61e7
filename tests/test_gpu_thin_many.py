"""thin_many / thin_gf_many on the GPU (csrc/many.hip: one workgroup per chain) against the NumPy oracle and,
bit for bit, against the C bit model in the exact arithmetic (oracle/stein_ref.c sr_greedy), on the shared inputs
of tests/many_ref.py; st_chain_stats against NumPy and st_pdist_many's median against kernel.make_precon, both
bitwise; errors, fallback and the sampler-to-thin pipeline."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from oracle import stein_numpy as o  # noqa: E402
from stein_thinning import kernel, thinning as st  # noqa: E402
from stein_thinning.device import isotropic_scale  # noqa: E402
from tests import many_ref as R, oracle_c  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _loop(x, g, m, **kw):
    return np.stack([o.thin(x[c], g[c], m, **kw) for c in range(x.shape[0])])


@pytest.mark.parametrize('d,n,precon', R.parity_cases())
def test_parity_with_the_oracle_and_the_exact_bit_model(d, n, precon):
    x, g, ref = R.parity_reference(d, n, precon)
    idx, sums = st._thin_many_engine(x, g, R.M, True, precon, want_sums=True)
    assert idx.dtype == np.uint32 and idx.shape == (x.shape[0], R.M)
    np.testing.assert_array_equal(st.thin_many(x, g, R.M, preconditioner=precon), idx)
    assert st.last_engine == 'many'
    sums = sums.cpu().numpy()
    for c, (oidx, cidx, cA) in enumerate(ref):
        np.testing.assert_array_equal(idx[c], oidx, err_msg=f'chain {c}: NumPy oracle')
        np.testing.assert_array_equal(idx[c], cidx, err_msg=f'chain {c}: C bit model')
        np.testing.assert_array_equal(_bits(sums[c]), _bits(cA), err_msg=f'chain {c}: running sums')


@pytest.mark.parametrize('d', R.DIMS)
def test_a_single_row_is_selected_every_time(d):
    x, g = R.rw_chains(4, 1, d)
    idx = st.thin_many(x, g, 7, standardize=False)
    assert st.last_engine == 'many'
    np.testing.assert_array_equal(idx, np.zeros((4, 7), dtype=np.uint32))


@pytest.mark.parametrize('d', R.DIMS)
def test_more_points_than_rows(d):
    x, g = R.rw_chains(4, 5, d, accept=1.0)
    idx, sums = st._thin_many_engine(x, g, 17, True, 'id', want_sums=True)
    np.testing.assert_array_equal(idx, _loop(x, g, 17))
    for c in range(4):
        s, gs = o._validate_and_standardize(x[c], g[c], True)
        cidx, cA = oracle_c.greedy(s, gs, None, 1.0, float(d), 17, arith='exact')
        np.testing.assert_array_equal(idx[c], cidx)
        np.testing.assert_array_equal(_bits(sums[c].cpu().numpy()), _bits(cA))


def test_chains_are_independent_and_runs_repeat():
    C, n, d = 600, 64, 4                          # more blocks than are resident at once
    x, g = R.rw_chains(C, n, d)
    idx, sums = st._thin_many_engine(x, g, R.M, True, 'id', want_sums=True)
    again, sums2 = st._thin_many_engine(x, g, R.M, True, 'id', want_sums=True)
    np.testing.assert_array_equal(idx, again)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    for c in (0, 1, 255, 256, 511, 599):
        np.testing.assert_array_equal(st.thin_many(x[c:c + 1], g[c:c + 1], R.M), idx[c:c + 1])
    for c in (0, 313, 599):
        np.testing.assert_array_equal(idx[c], o.thin(x[c], g[c], R.M))


@pytest.mark.filterwarnings('ignore:log_q differs from log_p')
@pytest.mark.parametrize('d,n', [(2, 65), (4, 257), (4, 1500)])
@pytest.mark.parametrize('range_cap', [None, 0.25])
def test_gradient_free(d, n, range_cap):
    x, _ = R.rw_chains(3, n, d)
    log_p, log_q, gq = R.gf_inputs(x)
    for precon in ('id', 'med'):
        idx = st.thin_gf_many(x, log_p, log_q, gq, R.M, range_cap=range_cap, preconditioner=precon)
        assert st.last_engine == 'many'
        for c in range(3):
            want = o.thin_gf(x[c], log_p[c], log_q[c], gq[c], R.M, range_cap=range_cap, preconditioner=precon)
            np.testing.assert_array_equal(idx[c], want, err_msg=f'{precon} chain {c}')
    # the bit model with weights: thin_gf's weights on the oracle's standardised rows
    idx, sums = st._thin_many_engine(x, gq, R.M, True, 'id', gf=(log_p, log_q, range_cap), want_sums=True)
    for c in range(3):
        s, gs = o._validate_and_standardize(x[c], gq[c], True)
        w = np.exp(o._log_weights(log_p[c], log_q[c], range_cap))
        cidx, cA = oracle_c.greedy(s, gs, w, 1.0, float(d), R.M, arith='exact')
        np.testing.assert_array_equal(idx[c], cidx)
        np.testing.assert_array_equal(_bits(sums[c].cpu().numpy()), _bits(cA))


def test_gradient_free_with_equal_densities_is_thin_many():
    x, g = R.rw_chains(4, 300, 4)
    log_p = R.gf_inputs(x)[0]
    np.testing.assert_array_equal(st.thin_gf_many(x, log_p, log_p, g, R.M, preconditioner='med'),
                                  st.thin_many(x, g, R.M, preconditioner='med'))


def test_the_log_ratio_warning_is_raised_once_and_names_the_first_chain():
    x, g = R.rw_chains(4, 100, 2)
    log_p = R.gf_inputs(x)[0]
    log_q = log_p.copy()
    log_q[2, 5] += 30.0
    log_q[3, 7] += 40.0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        st.thin_gf_many(x, log_p, log_q, g, 5)
    msgs = [str(r.message) for r in rec if issubclass(r.category, UserWarning)]
    assert len(msgs) == 1 and msgs[0].startswith('log_q differs from log_p by more than 10') \
        and msgs[0].endswith('(chain 2)')


@pytest.mark.parametrize('precon', ['id', 'med'])
def test_rocm_tensors_give_the_host_result_and_stay_unchanged(precon):
    x, g = R.rw_chains(5, 700, 4)
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    x0, g0 = xt.clone(), gt.clone()
    idx = st.thin_many(xt, gt, R.M, preconditioner=precon)
    np.testing.assert_array_equal(idx, st.thin_many(x, g, R.M, preconditioner=precon))
    np.testing.assert_array_equal(idx, _loop(x, g, R.M, preconditioner=precon))
    assert torch.equal(xt.view(torch.int64), x0.view(torch.int64))
    assert torch.equal(gt.view(torch.int64), g0.view(torch.int64))


def test_chain_stats_are_numpys_bit_for_bit():
    C, n, d = 8, 4096, 4
    rng = np.random.default_rng(R.SEED)
    mag = np.array([1e-3, 1.0, 1e3, 1e6])                     # the summation order shows in the last bits
    x = rng.normal(size=(C, n, d)) * mag + rng.normal(size=(C, 1, d)) * mag * 3
    g = rng.normal(size=(C, n, d))
    x[1, 100, 2] = np.nan
    x[1, 200, 0] = np.inf                                      # NaN is reported before inf
    g[3, 4000, 1] = -np.inf
    x[5, :, 3] = 7.25                                          # a constant column: zero scale
    g[6, 17, 0] = np.nan
    loc, scl, status = (a.cpu().numpy() for a in
                        st._many_stats(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), True))
    assert status.tolist() == [0, 1, 0, 2, 0, 3, 1, 0]
    for c in np.flatnonzero(status == 0):
        want_loc = np.mean(x[c], axis=0)
        want_scl = np.mean(np.abs(x[c] - want_loc), axis=0)
        np.testing.assert_array_equal(_bits(loc[c]), _bits(want_loc), err_msg=f'loc, chain {c}')
        np.testing.assert_array_equal(_bits(scl[c]), _bits(want_scl), err_msg=f'scl, chain {c}')
    assert scl[5, 3] == 0.0
    # the order does show on this input: a pairwise sum of the same column differs in some chain
    assert any(np.mean(np.ascontiguousarray(x[c, :, k])) != np.mean(x[c], axis=0)[k] for c in (0, 2, 4, 7)
               for k in range(d))
    # standardize = False: unit scales, finiteness only (a constant column is no error)
    _, scl1, status1 = (a.cpu().numpy() for a in
                        st._many_stats(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), False))
    assert status1.tolist() == [0, 1, 0, 2, 0, 0, 1, 0] and np.all(scl1 == 1.0)


@pytest.mark.parametrize('d', R.DIMS)
@pytest.mark.parametrize('n', [1000, 1500])
def test_median_scales_are_make_precons_bit_for_bit(n, d):
    x, g = R.rw_chains(3, n, d)
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    _, scl, _ = st._many_stats(xt, gt, True)
    med = st._many_medians(xt, scl)
    for precon in ('med', 'sclmed'):
        l, tr, zero = st._many_precon_scales(n, d, precon, med)
        assert zero is None
        for c in range(3):
            s, _ = o._validate_and_standardize(x[c], g[c], True)
            wl, wtr = isotropic_scale(kernel.make_precon(s, precon))
            assert _bits(l[c]) == _bits(wl) and _bits(tr[c]) == _bits(wtr), (precon, c)
    np.testing.assert_array_equal(st.thin_many(x, g, R.M, preconditioner='sclmed'),
                                  _loop(x, g, R.M, preconditioner='sclmed'))


def test_errors_name_the_lowest_failing_chain():
    x, g = R.rw_chains(8, 200, 4)
    bad_x = x.copy()
    bad_x[5] = [1.5, -2.25, 0.5, 3.0]                          # an all-equal chain (its column means are exact)
    with pytest.raises(ValueError, match='Too few unique samples'):
        o.thin(bad_x[5], g[5], 5)
    with pytest.raises(ValueError) as e:
        st.thin_many(bad_x, g, 5)
    assert str(e.value) == 'Too few unique samples in smp. (chain 5)'
    bad_g = g.copy()
    bad_g[3, 17, 1] = np.nan
    with pytest.raises(ValueError) as e:
        st.thin_many(bad_x, bad_g, 5)
    assert str(e.value) == 'sample or gradient contains NaNs. (chain 3)'
    inf_x = x.copy()
    inf_x[6, 0, 0] = np.inf
    with pytest.raises(ValueError) as e:
        st.thin_many(inf_x, g, 5, preconditioner='med')
    assert str(e.value) == 'sample or gradient contains infs. (chain 6)'
    # a zero median: more than half of the pairs coincide, the scales do not vanish
    med0 = x.copy()
    med0[2, 40:] = med0[2, 39]
    with pytest.raises(ValueError) as e:
        st.thin_many(med0, g, 5, preconditioner='med')
    assert str(e.value) == 'Too few unique samples in smp. (chain 2)'
    with pytest.raises(ValueError):
        o.thin(med0[2], g[2], 5, preconditioner='med')
    # n_points as the loop checks it: after chain 0's input, before the other chains'
    with pytest.raises(ValueError, match='negative dimensions'):
        st.thin_many(bad_x, g, -1)
    with pytest.raises(IndexError):
        st.thin_many(x, g, 0)
    first = x.copy()
    first[0, 3, 1] = np.nan
    with pytest.raises(ValueError, match=r'NaNs\. \(chain 0\)'):
        st.thin_many(first, g, 0)
    with pytest.raises(ValueError, match='not two-dimensional'):
        st.thin_many(x[0], g[0], 5)
    with pytest.raises(ValueError, match='inconsistent'):
        st.thin_many(x, g[:, :-1], 5)


@pytest.mark.filterwarnings('ignore:log_q differs from log_p')
def test_fallback_to_the_chain_loop():
    x3, g3 = R.rw_chains(2, 90, 3)
    np.testing.assert_array_equal(st.thin_many(x3, g3, 10), _loop(x3, g3, 10))
    assert st.last_engine == 'chains'
    x, g = R.rw_chains(2, R.max_n(4) + 1, 4)
    np.testing.assert_array_equal(st.thin_many(x, g, 10), _loop(x, g, 10))
    assert st.last_engine == 'chains'
    np.testing.assert_array_equal(st.thin_many(x[:, :300], g[:, :300], 10), _loop(x[:, :300], g[:, :300], 10))
    assert st.last_engine == 'many'
    idx = st.thin_many(x[:, :300], g[:, :300], 10, preconditioner='smpcov')
    assert st.last_engine == 'chains'
    np.testing.assert_array_equal(idx, np.stack([st.thin(x[c, :300], g[c, :300], 10, preconditioner='smpcov')
                                                 for c in range(2)]))
    log_p, log_q, gq = R.gf_inputs(x3)
    want = np.stack([o.thin_gf(x3[c], log_p[c], log_q[c], gq[c], 10) for c in range(2)])
    np.testing.assert_array_equal(st.thin_gf_many(x3, log_p, log_q, gq, 10), want)
    assert st.last_engine == 'chains'


def test_sampler_to_thin_pipeline_stays_on_the_device():
    from stein_thinning import lotka_volterra as lv
    data = lv.reference_data()
    data = lv.LvData(t=data.t[:65], y=data.y[:65], cov=data.cov, t_span=data.t_span, u_init=data.u_init)
    starts = np.log(lv.THETA) + 0.02 * np.random.default_rng(42).normal(size=(64, 4))
    run = lv.mala_sample(starts, 64, 0.003, seed=20261021, drift_cap=2.0, data=data, device_out=True)
    assert run.samples.is_cuda and run.grad.is_cuda and tuple(run.samples.shape) == (64, 64, 4)
    # a chain that hardly moved has no scale or no median (thin raises for it): keep the chains whose longest run
    # of repeated rows is under half the chain
    same = np.all(np.diff(run.samples.cpu().numpy(), axis=1) == 0, axis=2)
    longest = [max(len(r) for r in ''.join('x' if s else ' ' for s in row).split(' ')) + 1 for row in same]
    keep = [c for c in range(64) if longest[c] < 32]
    assert len(keep) >= 8
    keep = torch.tensor(keep, device=run.samples.device)
    xs, gs = run.samples[keep], run.grad[keep]
    idx = st.thin_many(xs, gs, 10, preconditioner='med')
    assert st.last_engine == 'many'
    hx, hg = xs.cpu().numpy(), gs.cpu().numpy()
    np.testing.assert_array_equal(idx, np.stack([st.thin(hx[c], hg[c], 10, preconditioner='med')
                                                 for c in range(hx.shape[0])]))
