"""st_lv_nuts_wave and st_lv_nuts_workspace_bytes, without a GPU: the symbols exist and every ST_ERR_INVALID condition is
reported before any HIP call (the table of tests/test_abi_hmc_metric.py, with this sampler's own arguments: max_depth in
n_leapfrog's place, three further per-step outputs, and no supplied-noise form)."""
import ctypes
import math

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_workspace_bytes(lib):
    assert lib.st_lv_nuts_workspace_bytes(1) == 192           # 24 words per chain
    assert lib.st_lv_nuts_workspace_bytes(130) == 130 * 192
    assert lib.st_lv_nuts_workspace_bytes(0) == -1 and lib.st_lv_nuts_workspace_bytes(-3) == -1


def test_abi_version_is_unchanged(lib):
    from stein_thinning import _native
    assert lib.st_abi_version() == _native.ABI_VERSION == 1       # an additive entry point


def test_validation_happens_before_any_hip_call(lib):
    from stein_thinning import _native
    inv = _native.ST_ERR_INVALID
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    half = ctypes.c_void_p(p.value + 8)            # 8-byte aligned only

    def host(vals):
        arr = (ctypes.c_double * len(vals))(*vals)
        return ctypes.cast(arr, ctypes.c_void_p), arr      # (the array is kept alive by the caller)

    clip, _k2 = host([0.01, 0.01, math.inf, math.inf])
    settings, _k3 = host([0.0, 25.0, 1.0, 1.0, 1e-3, 1e-6])
    whiten, _k4 = host([5.0, 0.0, 0.0, 5.0])
    cinv, _k5 = host([25.0, 0.0, 0.0, 25.0])
    names = ['state', 'chains', 'first_chain', 'first_step', 'steps', 'init', 'eps_chain', 'metric_chol', 'kick_clip',
             'max_depth', 'adapt', 'delta', 'noise_mode', 'seed', 'z', 'log_u', 'noise_ld', 'noise_row0', 't_eval',
             't_n', 'y_obs', 'span_u0_tol', 'whiten', 'c_log', 'norm_logc', 'cov_inv', 'max_steps', 'samples', 'log_p',
             'grad', 'accept_stat', 'step_size', 'tree_depth', 'n_leapfrog', 'divergent', 'out_ld', 'out_row0',
             'stream']
    base = [p, 4, 0, 1, 8, 1, p, p, clip, 3, 1, 0.8, 2, 0, p, p, 8, 0, p, 16, p, settings, whiten, 0.0, 0.9, cinv, 1000,
            p, p, p, p, p, p, p, p, 9, 1, None]
    assert len(names) == len(base) == len(_native.SIGNATURES['st_lv_nuts_wave'][1])
    # st_lv_hmc_metric_wave's arguments with tree_depth, n_leapfrog, divergent after step_size (max_depth has
    # n_leapfrog's type and place)
    metric = list(_native.SIGNATURES['st_lv_hmc_metric_wave'][1])
    ptr = metric[0]
    assert _native.SIGNATURES['st_lv_nuts_wave'][1] == metric[:32] + [ptr, ptr, ptr] + metric[32:]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_lv_nuts_wave(*a)

    for name in ('state', 'samples', 'log_p', 'grad', 't_eval', 'y_obs', 'kick_clip', 'span_u0_tol', 'whiten',
                 'cov_inv', 'eps_chain', 'metric_chol', 'accept_stat', 'step_size', 'tree_depth', 'n_leapfrog',
                 'divergent'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('state', 'samples', 'log_p', 'grad', 't_eval', 'y_obs', 'z', 'log_u', 'eps_chain', 'metric_chol',
                 'accept_stat', 'step_size', 'tree_depth', 'n_leapfrog', 'divergent'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('state', 'samples', 'grad', 'z'):     # the arrays written / read as 16-byte pairs
        assert call(**{name: half}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('chains', 'steps', 't_n', 'max_depth'):
        for v in (0, -1):
            assert call(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
    for v in (11, 12, 2 ** 31 - 1):                   # the checkpoint slots end at depth 10
        assert call(max_depth=v) == inv and b'max_depth' in lib.st_last_error()
    assert call(first_step=0) == inv and b'first_step' in lib.st_last_error()
    assert call(first_step=-5) == inv
    assert call(first_chain=-1) == inv
    assert call(first_step=2) == inv and b'init' in lib.st_last_error()     # init continues nothing
    assert call(init=2) == inv
    assert call(max_steps=0) == inv
    # adapt: 0 or 1;  delta: inside (0, 1), also when nothing adapts
    for bad in (2, -1):
        assert call(adapt=bad) == inv and b'adapt' in lib.st_last_error()
    for adapt in (0, 1):
        for bad in (0.0, 1.0, -0.2, 1.5, math.inf, math.nan):
            assert call(adapt=adapt, delta=bad) == inv, (adapt, bad)
            assert b'delta' in lib.st_last_error()
    # the kick clip: > 0 and not NaN; +inf is allowed (the base call has two such components)
    for bad in (0.0, -1.0, -math.inf, math.nan):
        for j in range(4):
            v = [0.01, 0.01, math.inf, math.inf]
            v[j] = bad
            ptr_, _keep = host(v)
            assert call(kick_clip=ptr_) == inv, (bad, j)
            assert b'kick clip' in lib.st_last_error()
    # there is no supplied-noise form (0), with or without the arrays; recorded noise (2) needs the arrays, log_u
    # included although it is not written
    assert call(noise_mode=0) == inv and b'noise_mode' in lib.st_last_error()
    assert call(noise_mode=0, z=None) == inv
    for mode in (0, 2):
        assert call(noise_mode=mode, z=None) == inv and b'noise' in lib.st_last_error()
        assert call(noise_mode=mode, log_u=None) == inv and b'noise' in lib.st_last_error()
        assert call(noise_mode=mode, noise_ld=7) == inv and b'noise rows' in lib.st_last_error()
        assert call(noise_mode=mode, noise_row0=1) == inv
        assert call(noise_mode=mode, noise_row0=-1) == inv
    assert call(noise_mode=3) == inv and call(noise_mode=-1) == inv
    # output rows: init writes row out_row0 - 1, the steps rows out_row0 .. out_row0 + steps - 1
    assert call(out_row0=0) == inv and b'output rows' in lib.st_last_error()
    assert call(out_ld=8) == inv and b'output rows' in lib.st_last_error()
    assert call(out_row0=2) == inv
    bad_span, _k6 = host([25.0, 0.0, 1.0, 1.0, 1e-3, 1e-6])
    assert call(span_u0_tol=bad_span) == inv
    bad_tol, _k7 = host([0.0, 25.0, 1.0, 1.0, 0.0, 1e-6])
    assert call(span_u0_tol=bad_tol) == inv
