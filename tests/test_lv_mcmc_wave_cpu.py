"""Wave-per-chain layout of the random-walk Metropolis sampler, CPU tier: rw_sample's ``layout`` keyword is
checked before the device is asked for, and st_lv_rwmh_wave holds st_lv_rwmh's validation rules, all before
any HIP call (the table of tests/test_lv_mcmc_cpu.py::test_validation_happens_before_any_hip_call)."""
import ctypes

import numpy as np
import pytest

from tests import mcmc_ref as M


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from stein_thinning import _native
    ge.build()
    return _native.load_library(ge.HIP_LIB)


def test_layout_is_checked_before_the_device():
    from stein_thinning import lotka_volterra as lv
    x0 = np.log(M.THETA_INITS)
    for bad in ('bogus', 'Wave', '', None, 1):
        with pytest.raises(ValueError, match='layout'):
            lv.rw_sample(x0, 10, seed=1, layout=bad)
    assert lv.LAYOUTS == ('thread', 'wave', 'auto')
    assert isinstance(lv.WAVE_MAX_CHAINS, int) and lv.WAVE_MAX_CHAINS >= 0
    assert isinstance(lv.STEPS_PER_LAUNCH_WAVE, int) and lv.STEPS_PER_LAUNCH_WAVE >= 1


def test_valid_layouts_pass_up_to_the_device(monkeypatch):
    """The three valid values get through every argument check; the next thing rw_sample does is ask for the
    device, which is replaced here by a marker, so the test is the same with and without a GPU."""
    from stein_thinning import _native
    from stein_thinning import lotka_volterra as lv

    class DeviceAsked(Exception):
        pass

    def asked():
        raise DeviceAsked

    monkeypatch.setattr(_native, 'require_device', asked)
    x0 = np.log(M.THETA_INITS)
    data = lv.LvData(t=np.linspace(0.0, 25.0, 8), y=np.ones((8, 2)))
    for layout in ('thread', 'wave', 'auto'):
        with pytest.raises(DeviceAsked):
            lv.rw_sample(x0, 10, seed=1, data=data, layout=layout)
        # the other argument checks still come first in every layout
        with pytest.raises(ValueError, match='steps_per_launch'):
            lv.rw_sample(x0, 10, seed=1, data=data, layout=layout, steps_per_launch=0)
    with pytest.raises(DeviceAsked):
        lv.rw_sample(x0, 10, seed=1, data=data)                     # the default: 'thread'


def test_wave_entry_point_validates_before_any_hip_call(lib):
    from stein_thinning import _native
    inv = _native.ST_ERR_INVALID
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    half = ctypes.c_void_p(p.value + 8)            # 8-byte aligned only
    step = (ctypes.c_double * 4)(0.0025, 0.0025, 0.0025, 0.0025)
    settings = (ctypes.c_double * 6)(0.0, 25.0, 1.0, 1.0, 1e-3, 1e-6)
    whiten = (ctypes.c_double * 4)(5.0, 0.0, 0.0, 5.0)
    names = ['state', 'chains', 'first_chain', 'first_step', 'steps', 'init', 'step_size', 'noise_mode', 'seed', 'z',
             'log_u', 'noise_ld', 'noise_row0', 't_eval', 't_n', 'y_obs', 'span_u0_tol', 'whiten', 'c_log',
             'norm_logc', 'max_steps', 'samples', 'log_p', 'out_ld', 'out_row0', 'stream']
    base = [p, 4, 0, 1, 8, 1, ctypes.cast(step, ctypes.c_void_p), 0, 0, p, p, 8, 0, p, 16, p,
            ctypes.cast(settings, ctypes.c_void_p), ctypes.cast(whiten, ctypes.c_void_p), 0.0, 0.9, 1000, p, p, 9, 1,
            None]
    assert len(names) == len(base)
    assert _native.SIGNATURES['st_lv_rwmh_wave'] == _native.SIGNATURES['st_lv_rwmh']

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.st_lv_rwmh_wave(*a)

    for name in ('state', 'samples', 'log_p', 't_eval', 'y_obs', 'step_size', 'span_u0_tol', 'whiten'):
        assert call(**{name: None}) == inv, name
        assert b'NULL' in lib.st_last_error()
    for name in ('state', 'samples', 'log_p', 't_eval', 'y_obs', 'z', 'log_u'):
        assert call(**{name: odd}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('state', 'samples', 'z'):           # the arrays written / read as 16-byte pairs
        assert call(**{name: half}) == inv, name
        assert b'aligned' in lib.st_last_error()
    for name in ('chains', 'steps', 't_n'):
        for v in (0, -1):
            assert call(**{name: v}) == inv, (name, v)
            assert name.encode() in lib.st_last_error()
    assert call(first_step=0) == inv and b'first_step' in lib.st_last_error()
    assert call(first_step=-5) == inv
    assert call(first_chain=-1) == inv
    assert call(first_step=2) == inv and b'init' in lib.st_last_error()     # init continues nothing
    assert call(max_steps=0) == inv
    for bad in (0.0, -0.0025, float('inf'), float('nan')):
        for j in range(4):
            s = (ctypes.c_double * 4)(0.0025, 0.0025, 0.0025, 0.0025)
            s[j] = bad
            assert call(step_size=ctypes.cast(s, ctypes.c_void_p)) == inv, (bad, j)
            assert b'step size' in lib.st_last_error()
    # supplied noise (0) and recorded noise (2) need the arrays; device noise (1) does not ask for them
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
    bad_span = (ctypes.c_double * 6)(25.0, 0.0, 1.0, 1.0, 1e-3, 1e-6)
    assert call(span_u0_tol=ctypes.cast(bad_span, ctypes.c_void_p)) == inv
    bad_tol = (ctypes.c_double * 6)(0.0, 25.0, 1.0, 1.0, 0.0, 1e-6)
    assert call(span_u0_tol=ctypes.cast(bad_tol, ctypes.c_void_p)) == inv
