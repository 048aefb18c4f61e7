"""The LV samplers (csrc/lv_mcmc.hip: lv_rwmh_kernel, lv_rwmh_wave_kernel, lv_mala_wave_kernel, and their host
driver in lotka_volterra.py / capi.hip) on every input the sampler suites hold fixed: dense covariances (the
off-diagonal entries of the whitening factor and of cov_inv), other tolerances, span and start (the six doubles of
span_u0_tol), short / repeated / out-of-span observation grids, a vector random-walk step, Philox keys with
non-zero high words, tensor noise, the hand-off of a chain between the entry points and the rows a launch writes.

Reference: scipy through the host chains of tests/sampler_ref.py, on the sets of tests/lv_ref.py; log_u = -inf
accepts every proposal that has a density, so rows are compared bit for bit and values within RTOL = 1e-8 of
tests/test_gpu_lv.py (log_p: relative; grad: max|got - want| / max|want| per row).
tests/test_lv_sampler_inputs_cpu.py holds the conditions on the inputs: scipy's own reordering noise is under 1e-9
for every pair but the random walk on 'grid_2' and 'grid_3' (sampler_ref.LOG_P_EXCEPTIONS: 1.9e-9 and 2.4e-9),
which are held to 10 x their recorded noise.  MALA's device rows are not bit-equal to the host chain's (g differs
by rounding), so the host is evaluated at the device's rows, as tests/test_gpu_lv_mala.py does.

Recorded on MI355X (the tests print the figures; bound 1e-8 unless stated).  Random walk, log_p against scipy /
against log_target_density, the same in both layouts to the digits shown:
  cov_pos 5.9e-10 / 8.3e-10, cov_neg 5.0e-10 / 7.1e-10, tol5 3.4e-13 / 3.4e-13, tol7_sparse 3.7e-14 / 2.2e-14,
  span 5.5e-15 / 2.5e-15, grid_1 7.3e-15 / 1.0e-14, grid_2 2.6e-10 (bound 1.9e-8) / 6.6e-11, grid_3 3.3e-10 (bound
  2.4e-8) / 7.9e-11, grid_63 2.6e-10 / 3.6e-10, grid_64 5.9e-11 / 8.3e-11, grid_65 1.2e-10 / 1.7e-10, grid_129
  2.3e-10 / 3.2e-10, grid_repeats 2.9e-10 / 4.0e-10, grid_outside 1.9e-10 / 2.7e-10.
Wave against thread, |log_p difference| / max(|log_p|, 1): at most 2.6e-15 (tol5), 0 on grid_1 and grid_2.
MALA, log_p against scipy / grad against scipy / grad against grad_log_posterior:
  cov_pos 1.1e-11 / 2.8e-12 / 3.6e-13, cov_neg 5.6e-11 / 3.4e-12 / 7.3e-14, tol5 2.0e-14 / 9.0e-14 / 1.4e-13,
  tol7_sparse 1.6e-14 / 9.6e-15 / 8.9e-15, span 1.2e-10 / 7.1e-11 / 1.9e-11, grid_1 6.6e-16 / 4.0e-15 / 7.2e-16,
  grid_2 6.3e-14 / 6.1e-13 / 1.2e-13, grid_3 2.4e-13 / 3.5e-13 / 1.1e-13, grid_63 2.1e-13 / 5.3e-13 / 2.0e-13,
  grid_64 1.2e-13 / 8.4e-13 / 4.8e-14, grid_65 7.4e-14 / 5.6e-13 / 2.2e-13, grid_129 1.4e-13 / 2.3e-12 / 4.9e-14,
  grid_repeats 5.2e-14 / 3.9e-13 / 6.5e-14, mala_outside 4.2e-11 / 4.8e-12 / 9.8e-13;
  clipped drift components 80, 83, 80, 0, 96 of 96 on the first five sets, 4 on grid_129, 0 elsewhere.
Device noise with 64-bit keys: z within 2.3e-16 of the host restatement, log_u equal.
Each test was seen to fail once: with U transposed in lv_loglik_term the random-walk and MALA tests on cov_pos and
cov_neg (log_p off by 0.3 to 14 relative); with two STEP4 entries swapped on the host side every random-walk test;
with the high word of the seed dropped in the call both Philox tests.
"""
import functools
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import mcmc_ref as M  # noqa: E402
from tests import sampler_ref as S  # noqa: E402
from tests.test_gpu_lv import RTOL  # noqa: E402
from tests.test_gpu_lv_mcmc import NOISE_ATOL  # noqa: E402
from tests.test_gpu_lv_mcmc_wave import LP_RTOL  # noqa: E402

RW_NAMES = ('samples', 'log_p', 'accepted', 'n_failed')
MALA_NAMES = ('samples', 'log_p', 'grad', 'accepted', 'n_failed')
FULL = [S.ROWS - 1] * S.CHAINS


def _quiet(f, *args, **kw):
    """f(...) with the status warning an error."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        return f(*args, **kw)


def _same(a, b, names):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def _grad_err(got, want):
    return np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)


@functools.lru_cache(maxsize=None)
def _rw(name, layout):
    s = S.input_set(name)
    x0, z, log_u = S.noise()
    return lv.rw_sample(x0, S.ROWS, S.STEP4, noise=(z, log_u), data=s.data, rtol=s.rtol, atol=s.atol, layout=layout)


@functools.lru_cache(maxsize=None)
def _mala(name):
    s = S.input_set(name)
    x0, z, log_u = S.noise()
    return lv.mala_sample(x0, S.ROWS, S.EPS4, noise=(z, log_u), drift_cap=S.CAP, data=s.data, rtol=s.rtol, atol=s.atol)


# ---- a. random walk, every set, both layouts

@pytest.mark.parametrize('layout', ['thread', 'wave'])
@pytest.mark.parametrize('name', S.RW_SETS)
def test_random_walk_on_every_set(name, layout):
    s = S.input_set(name)
    x0, z, _ = S.noise()
    want = S.host_chain('rw', name)
    r = _rw(name, layout)
    assert r.accepted.tolist() == FULL and r.n_failed.tolist() == [0] * S.CHAINS
    np.testing.assert_array_equal(r.samples[:, 0], x0)
    np.testing.assert_array_equal(r.samples[:, 1:], r.samples[:, :-1] + S.STEP4 * z)
    np.testing.assert_array_equal(r.samples, want.samples)
    err = np.abs(r.log_p - want.log_p) / np.abs(want.log_p)
    dens = _quiet(lv.log_target_density, r.samples.reshape(-1, 4), s.data, rtol=s.rtol, atol=s.atol).reshape(r.log_p.shape)
    err_d = np.abs(r.log_p - dens) / np.abs(dens)
    bound = S.log_p_bound('rw', name, RTOL)
    print(f'{name} {layout}: log_p against scipy {err.max():.2e} (bound {bound:g}), against log_target_density '
          f'{err_d.max():.2e} (bound {RTOL:g})')
    assert err.max() < bound, (np.unravel_index(err.argmax(), err.shape), err.max())
    assert err_d.max() < RTOL, (np.unravel_index(err_d.argmax(), err_d.shape), err_d.max())


@pytest.mark.parametrize('name', S.RW_SETS)
def test_random_walk_wave_against_thread(name):
    wave, thread = _rw(name, 'wave'), _rw(name, 'thread')
    _same(wave, thread, ('samples', 'accepted', 'n_failed'))
    diff = np.abs(wave.log_p - thread.log_p)
    print(f'{name}: max |log_p wave - thread| / max(|log_p|, 1) {(diff / np.maximum(np.abs(thread.log_p), 1.0)).max():.2e}')
    assert np.all(diff <= LP_RTOL * np.maximum(np.abs(thread.log_p), 1.0)), diff.max()
    if S.input_set(name).data.t.size <= 2:                 # the two summation orders coincide
        np.testing.assert_array_equal(wave.log_p, thread.log_p)


# ---- b. MALA, every set

@pytest.mark.parametrize('name', S.MALA_SETS)
def test_mala_on_every_set(name):
    s = S.input_set(name)
    x0, z, _ = S.noise()
    eps, h, _, c = S.mala_ref.constants(S.EPS4, S.CAP)
    r = _mala(name)
    assert r.accepted.tolist() == FULL and r.n_failed.tolist() == [0] * S.CHAINS
    np.testing.assert_array_equal(r.samples[:, 0], x0)
    drift = h * r.grad[:, :-1]
    np.testing.assert_array_equal(r.samples[:, 1:], (r.samples[:, :-1] + np.minimum(np.maximum(drift, -c), c)) + eps * z)
    rows = r.samples.reshape(-1, 4)
    host = [S.evaluate(x, s) for x in rows]
    want_lp = np.array([v[0] for v in host]).reshape(r.log_p.shape)
    want_g = np.array([v[1] for v in host]).reshape(r.grad.shape)
    theta = np.exp(rows)
    kern_g = (theta * _quiet(lv.grad_log_posterior, theta, s.data, rtol=s.rtol, atol=s.atol)).reshape(r.grad.shape)
    e_lp = np.abs(r.log_p - want_lp) / np.abs(want_lp)
    e_g, e_k = _grad_err(r.grad, want_g), _grad_err(r.grad, kern_g)
    print(f'{name}: log_p against scipy {e_lp.max():.2e}, grad against scipy {e_g.max():.2e}, against '
          f'grad_log_posterior {e_k.max():.2e} (bound {RTOL:g}); clipped {int((np.abs(drift) > c).sum())} of {drift.size}')
    assert e_lp.max() < RTOL, (np.unravel_index(e_lp.argmax(), e_lp.shape), e_lp.max())
    assert e_g.max() < RTOL, (np.unravel_index(e_g.argmax(), e_g.shape), e_g.max())
    assert e_k.max() < RTOL, (np.unravel_index(e_k.argmax(), e_k.shape), e_k.max())


# ---- c. Philox keys with non-zero high words

def _three_kernels(x0, rows, data, **kw):
    return (lv.rw_sample(x0, rows, S.STEP4, data=data, layout='thread', **kw),
            lv.rw_sample(x0, rows, S.STEP4, data=data, layout='wave', **kw),
            lv.mala_sample(x0, rows, S.EPS4, drift_cap=S.CAP, data=data, **kw))


@pytest.mark.parametrize('seed,first_chain', [(2 ** 64 - 1, 2 ** 40 + 3), (987654321987654321, 129)])
def test_philox_keys_use_all_64_bits(seed, first_chain):
    data = S.input_set('grid_2').data
    x0 = S.noise()[0]
    z, log_u = M.device_noise(seed, S.CHAINS, 4, first_chain=first_chain)
    assert np.all(np.isfinite(log_u))
    # the low words alone give other noise: a dropped high word cannot pass
    z_lo = M.device_noise(seed & 0xFFFFFFFF, S.CHAINS, 4, first_chain=first_chain & 0xFFFFFFFF)[0]
    assert np.abs(z - M.device_noise(seed & 0xFFFFFFFF, S.CHAINS, 4, first_chain=first_chain)[0]).min() > 1e-6
    assert np.abs(z - z_lo).min() > 1e-6
    runs = _three_kernels(x0, 5, data, seed=seed, first_chain=first_chain, return_noise=True)
    for r in runs:
        print('max abs err z', np.abs(r.z - z).max(), 'log_u', np.abs(r.log_u - log_u).max())
        assert np.abs(r.z - z).max() < NOISE_ATOL and np.abs(r.log_u - log_u).max() < NOISE_ATOL
        np.testing.assert_array_equal(r.z, runs[0].z)
        np.testing.assert_array_equal(r.log_u, runs[0].log_u)
    plain = _three_kernels(x0, 5, data, seed=seed, first_chain=first_chain)
    for r, p, names in zip(runs, plain, (RW_NAMES, RW_NAMES, MALA_NAMES)):
        _same(p, r, names)
        assert p.z is None and p.log_u is None
    assert sum(int(r.accepted.sum()) for r in runs) > 0


# ---- d. noise as ROCm tensors

@pytest.mark.parametrize('view', ['contiguous', 'strided'])
def test_tensor_noise_is_the_numpy_path(view):
    data = S.input_set('grid_65').data
    x0, z, _ = S.noise()
    log_u = np.log(np.random.default_rng(12).random((S.CHAINS, S.ROWS - 1)))
    dev = nat.require_device()
    if view == 'contiguous':
        zt, lt = torch.from_numpy(np.array(z)).to(dev), torch.from_numpy(log_u).to(dev)
        assert zt.is_contiguous() and lt.is_contiguous()
    else:                                                    # slices of larger tensors: no stride is the packed one
        big_z = torch.full((S.CHAINS + 1, S.ROWS + 2, 6), float('nan'), dtype=torch.float64, device=dev)
        big_l = torch.full((S.CHAINS + 1, 2 * S.ROWS), float('nan'), dtype=torch.float64, device=dev)
        zt, lt = big_z[1:, 2:-1, 1:5], big_l[:-1, 1:2 * (S.ROWS - 1):2]
        zt.copy_(torch.from_numpy(np.array(z)))
        lt.copy_(torch.from_numpy(log_u))
        assert not zt.is_contiguous() and not lt.is_contiguous()
    assert zt.is_cuda and zt.dtype == torch.float64 and tuple(zt.shape) == z.shape and tuple(lt.shape) == log_u.shape
    got = _three_kernels(x0, S.ROWS, data, noise=(zt, lt))
    want = _three_kernels(x0, S.ROWS, data, noise=(z, log_u))
    for g, w, names in zip(got, want, (RW_NAMES, RW_NAMES, MALA_NAMES)):
        _same(g, w, names)
    assert 0 < want[0].accepted.sum() < S.CHAINS * (S.ROWS - 1)


# ---- e. hand-off between the entry points and the rows a launch writes, through the C ABI

CANARY = -777.25
STEPS, OUT_LD, NOISE_LD = 7, 8 + 3, 7 + 2
SPLIT = ((1, 3, 1, 0, 1), (4, 4, 4, 3, 0))      # (first_step, steps, out_row0, noise_row0, init) of the two launches
ABI_SEED = 2 ** 63 + 12345


def _problem():
    """The posterior on 'grid_2' as the entry points take it: device t, y and the host settings."""
    s = S.input_set('grid_2')
    _, t, y, sp, U, c_log, norm_logc = lv._chain_problem(s.data, s.rtol, s.atol)
    dev = nat.require_device()
    td, yd = (torch.from_numpy(a).to(dev) for a in (t, y))
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(s.data.cov, dtype=np.float64)))
    return s, dev, td, yd, sp, U, c_log, norm_logc, cinv


def _canaries(dev, *shapes):
    return [torch.full(shape, CANARY, dtype=torch.float64, device=dev) for shape in shapes]


def _state(dev, x0, words):
    """The state record: x, then zeros (lp, the counts: int64 zero is 0.0's bits), the spare words a canary."""
    st = torch.zeros((S.CHAINS, words), dtype=torch.float64, device=dev)
    st[:, :4] = torch.from_numpy(np.array(x0)).to(dev)
    st[:, 7] = CANARY
    if words == 16:
        st[:, 12:] = CANARY
    return st


def _abi_noise():
    rng = np.random.default_rng(13)
    return rng.standard_normal((S.CHAINS, STEPS, 4)), np.log(rng.random((S.CHAINS, STEPS)))


def _rw_launches(entries, mode, zd, lud, seed):
    """Two launches (SPLIT) of the named entry points on one state record; returns state, samples, log_p."""
    s, dev, td, yd, sp, U, c_log, norm_logc, _ = _problem()
    L = nat.lib()
    state = _state(dev, S.noise()[0], 8)
    samples, log_p = _canaries(dev, (S.CHAINS, OUT_LD, 4), (S.CHAINS, OUT_LD))
    for entry, (first_step, steps, out_row0, noise_row0, init) in zip(entries, SPLIT):
        nat.check(getattr(L, entry)(
            nat.ptr(state), S.CHAINS, 0, first_step, steps, init, S.STEP4.ctypes.data, mode, seed, nat.ptr(zd),
            nat.ptr(lud), NOISE_LD, noise_row0, nat.ptr(td), td.numel(), nat.ptr(yd), sp.ctypes.data, U.ctypes.data,
            c_log, norm_logc, lv.MAX_STEPS, nat.ptr(samples), nat.ptr(log_p), OUT_LD, out_row0,
            nat.stream_handle()), entry)
    torch.cuda.synchronize()
    return state.cpu().numpy(), samples.cpu().numpy(), log_p.cpu().numpy()


def _check_rows_and_canaries(state, want, **arrays):
    """Rows 0 .. 7 of every output are the driver's run, every other cell and the spare state words the canary."""
    for name, a in arrays.items():
        np.testing.assert_array_equal(a[:, :STEPS + 1], getattr(want, name), err_msg=name)
        assert np.all(a[:, STEPS + 1:] == CANARY), name
    np.testing.assert_array_equal(state[:, :4], want.samples[:, -1])
    np.testing.assert_array_equal(state[:, 4], want.log_p[:, -1])
    counts = np.ascontiguousarray(state).view(np.int64)
    np.testing.assert_array_equal(counts[:, 5], want.accepted)
    np.testing.assert_array_equal(counts[:, 6], want.n_failed)
    assert np.all(state[:, 7] == CANARY)
    if state.shape[1] == 16:
        np.testing.assert_array_equal(state[:, 8:12], want.grad[:, -1])
        assert np.all(state[:, 12:] == CANARY)


@pytest.mark.parametrize('entries', [('st_lv_rwmh', 'st_lv_rwmh_wave'), ('st_lv_rwmh_wave', 'st_lv_rwmh')])
def test_either_entry_point_continues_the_others_chain(entries):
    """Supplied noise in rows 0 .. 6 of arrays with NOISE_LD = 9 rows (the spare rows NaN: read, they would fail a
    proposal), real log uniforms, so both decisions occur; with two observation times thread and wave log_p have
    the same bits and the handed-over chain is the thread layout's, bit for bit."""
    s, dev = _problem()[:2]
    z, log_u = _abi_noise()
    zd = torch.full((S.CHAINS, NOISE_LD, 4), float('nan'), dtype=torch.float64, device=dev)
    lud = torch.full((S.CHAINS, NOISE_LD), float('nan'), dtype=torch.float64, device=dev)
    zd[:, :STEPS], lud[:, :STEPS] = torch.from_numpy(z).to(dev), torch.from_numpy(log_u).to(dev)
    want = lv.rw_sample(S.noise()[0], STEPS + 1, S.STEP4, noise=(z, log_u), data=s.data, layout='thread')
    assert 0 < want.accepted.sum() < S.CHAINS * STEPS and want.n_failed.sum() == 0
    state, samples, log_p = _rw_launches(entries, 0, zd, lud, 0)
    _check_rows_and_canaries(state, want, samples=samples, log_p=log_p)
    np.testing.assert_array_equal(zd[:, :STEPS].cpu().numpy(), z)        # supplied noise is only read


@pytest.mark.parametrize('entries', [('st_lv_rwmh', 'st_lv_rwmh_wave'), ('st_lv_rwmh_wave', 'st_lv_rwmh')])
def test_recorded_noise_lands_in_its_own_rows(entries):
    """Record mode with device noise: each launch writes its steps' noise rows and nothing else."""
    s, dev = _problem()[:2]
    zd, lud = _canaries(dev, (S.CHAINS, NOISE_LD, 4), (S.CHAINS, NOISE_LD))
    want = lv.rw_sample(S.noise()[0], STEPS + 1, S.STEP4, seed=ABI_SEED, data=s.data, layout='thread',
                        return_noise=True)
    state, samples, log_p = _rw_launches(entries, 2, zd, lud, ABI_SEED)
    _check_rows_and_canaries(state, want, samples=samples, log_p=log_p)
    zh, lh = zd.cpu().numpy(), lud.cpu().numpy()
    np.testing.assert_array_equal(zh[:, :STEPS], want.z)
    np.testing.assert_array_equal(lh[:, :STEPS], want.log_u)
    assert np.all(zh[:, STEPS:] == CANARY) and np.all(lh[:, STEPS:] == CANARY)


def test_mala_launches_continue_a_chain_and_write_only_their_rows():
    s, dev, td, yd, sp, U, c_log, norm_logc, cinv = _problem()
    L = nat.lib()
    eps, h, w, c = S.mala_ref.constants(S.EPS4, S.CAP)
    ehw = np.ascontiguousarray(np.concatenate([eps, h, w]))
    clip = np.ascontiguousarray(c)
    want = lv.mala_sample(S.noise()[0], STEPS + 1, S.EPS4, seed=ABI_SEED, drift_cap=S.CAP, data=s.data,
                          return_noise=True)
    assert want.n_failed.sum() == 0
    state = _state(dev, S.noise()[0], 16)
    samples, grad, log_p, zd, lud = _canaries(dev, (S.CHAINS, OUT_LD, 4), (S.CHAINS, OUT_LD, 4), (S.CHAINS, OUT_LD),
                                              (S.CHAINS, NOISE_LD, 4), (S.CHAINS, NOISE_LD))
    for first_step, steps, out_row0, noise_row0, init in SPLIT:
        nat.check(L.st_lv_mala_wave(
            nat.ptr(state), S.CHAINS, 0, first_step, steps, init, ehw.ctypes.data, clip.ctypes.data, 2, ABI_SEED,
            nat.ptr(zd), nat.ptr(lud), NOISE_LD, noise_row0, nat.ptr(td), td.numel(), nat.ptr(yd), sp.ctypes.data,
            U.ctypes.data, c_log, norm_logc, cinv.ctypes.data, lv.MAX_STEPS, nat.ptr(samples), nat.ptr(log_p),
            nat.ptr(grad), OUT_LD, out_row0, nat.stream_handle()), 'st_lv_mala_wave')
    torch.cuda.synchronize()
    _check_rows_and_canaries(state.cpu().numpy(), want, samples=samples.cpu().numpy(), grad=grad.cpu().numpy(),
                             log_p=log_p.cpu().numpy())
    zh, lh = zd.cpu().numpy(), lud.cpu().numpy()
    np.testing.assert_array_equal(zh[:, :STEPS], want.z)
    np.testing.assert_array_equal(lh[:, :STEPS], want.log_u)
    assert np.all(zh[:, STEPS:] == CANARY) and np.all(lh[:, STEPS:] == CANARY)
