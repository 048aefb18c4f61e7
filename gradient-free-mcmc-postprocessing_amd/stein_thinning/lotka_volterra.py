"""Lotka-Volterra posterior inputs on the GPU, batched over parameter points.

The reference's LV experiments feed Stein thinning with, for every MCMC sample theta,
* the gradient of the log posterior from the forward sensitivity equations
  (``Sensitivity_analysis.ipynb`` cells 16, 40, 46: ``solve_ivp(lotka_volterra_sensitivity, ...,
  dense_output=True)``, the likelihood gradient sum_k J_k^T C^-1 (y_k - u_k), minus log(theta)/theta),
  evaluated for the unique samples of each chain (``parallelise_for_unique``,
  ``code/src/utils/parallel.py``; 18 minutes for 113 143 points on the reference's machine,
  ``Dask_AWS.ipynb``), and
* the log target density ``lotka_volterra.log_target_density(log_theta)``
  (``code/src/lotka_volterra.py``) for the gradient-free operator's log p.

Each parameter point is one thread of ``csrc/lv.hip`` running scipy's RK45 algorithm step for step
(same tableau, initial step, step-size control and dense output), so the values agree with scipy to
rounding.  The observation data ``y`` and times ``t`` are inputs (the reference reads them from its
S3 bucket; ``reference_data()`` rebuilds them with the module's own recipe).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence

import numpy as np

from . import _native as nat

T_SPAN = (0.0, 25.0)                  # code/src/lotka_volterra.py: t_span
T_N = 2400                            # t_n
THETA = np.array([0.67, 1.33, 1., 1.])  # theta (data-generating parameters)
U_INIT = (1.0, 1.0)                   # u_init
MEANS = np.array([0., 0.])
C = np.diag([0.2 ** 2, 0.2 ** 2])     # observation noise covariance
RTOL, ATOL = 1e-3, 1e-6               # scipy.integrate.solve_ivp defaults (the reference passes none)
MAX_STEPS = 1_000_000
# code/src/lotka_volterra.py: theta_inits (the starting points of the reference's five chains)
THETA_INITS = np.array([[0.55, 1., 0.8, 0.8], [1.5, 1., 0.8, 0.8], [1.3, 1.33, 0.5, 0.8], [0.55, 3., 3., 0.8],
                        [0.55, 1., 1.5, 1.5]])


@dataclass
class LvData:
    t: np.ndarray                     # (t_n,) ascending observation times
    y: np.ndarray                     # (t_n, 2) observations
    cov: np.ndarray = field(default_factory=lambda: C.copy())
    t_span: Sequence[float] = T_SPAN
    u_init: Sequence[float] = U_INIT


def reference_data() -> LvData:
    """The observations ``code/src/lotka_volterra.py`` builds at import: the RK45 solution at the
    true theta on np.linspace(0, 25, 2400) plus N(0, C) noise from default_rng(12345)."""
    from scipy import stats
    from scipy.integrate import solve_ivp

    def rhs(t, u, theta):
        theta1, theta2, theta3, theta4 = theta
        u1, u2 = u
        return [theta1 * u1 - theta2 * u1 * u2, theta4 * u1 * u2 - theta3 * u2]
    sol = solve_ivp(rhs, T_SPAN, list(U_INIT), args=(list(THETA),), dense_output=True)
    t = np.linspace(T_SPAN[0], T_SPAN[1], T_N)
    u = sol.sol(t).T
    eps = stats.multivariate_normal.rvs(mean=MEANS, cov=C, size=len(u), random_state=np.random.default_rng(12345))
    return LvData(t=t, y=u + eps)


def _points(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f'parameter points must be (n, 4) (or (4,)), got {a.shape}')
    return a


def _settings(data: LvData, rtol: float, atol: float):
    t = np.ascontiguousarray(data.t, dtype=np.float64)
    y = np.ascontiguousarray(data.y, dtype=np.float64)
    if t.ndim != 1 or y.shape != (t.size, 2):
        raise ValueError(f'need t (t_n,) and y (t_n, 2), got {t.shape} and {y.shape}')
    if t.size and np.any(np.diff(t) < 0):
        raise ValueError('observation times must be ascending')
    s = np.array([data.t_span[0], data.t_span[1], data.u_init[0], data.u_init[1], rtol, atol], dtype=np.float64)
    return t, y, s


def _density_constants(data: LvData):
    """(U, c_log, norm_logc) of the log target density: scipy's whitening factor of ``data.cov`` (``_PSD.U``),
    rank * log(2 pi) + log_pdet, and ``scipy.stats._continuous_distns._norm_pdf_logC``."""
    from .proxy import PsdFactor
    psd = PsdFactor(np.asarray(data.cov, dtype=np.float64), allow_singular=False)
    c_log = psd.rank * float(np.log(2 * np.pi)) + psd.log_pdet
    return np.ascontiguousarray(psd.U, dtype=np.float64), c_log, float(np.log(np.sqrt(2 * np.pi)))


def _status_check(status: np.ndarray, what: str):
    bad = np.flatnonzero(status)
    if bad.size:
        import warnings
        warnings.warn(f'{what}: the RK45 integration failed for {bad.size} parameter point(s) '
                      f'(first: {bad[0]}, status {status[bad[0]]}); their values are NaN', RuntimeWarning)


def grad_log_posterior(theta, data: Optional[LvData] = None, rtol: float = RTOL, atol: float = ATOL,
                       max_steps: int = MAX_STEPS, chunk: int = 1 << 16) -> np.ndarray:
    """``grad_log_posterior`` of Sensitivity_analysis.ipynb cell 46 for every row of ``theta``
    ((n, 4) or (4,)): returns (n, 4).  Two-phase kernels (``st_lv_grad_log_posterior_ws``), at most
    ``chunk`` points per launch (the step table is ~29 KB per point; fewer when device memory is
    short).  A point whose integration takes more than 64 accepted steps is recomputed by the
    single-phase kernel, whose sum over the observation times runs in time order instead of in
    pieces: the two forms agree to rounding (1e-11 relative, tests/test_gpu_lv.py), both within the
    1e-8 tolerance against scipy."""
    import torch
    data = reference_data() if data is None else data
    th = _points(theta)
    t, y, s = _settings(data, rtol, atol)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(data.cov, dtype=np.float64)))
    dev = nat.require_device()
    n = th.shape[0]
    out = torch.empty((max(n, 1), 4), dtype=torch.float64, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    if n:
        L = nat.lib()
        thd, td, yd = (torch.from_numpy(a).to(dev) for a in (th, t, y))
        # the step table is ~29 KB per point: cap a launch's points at a quarter of the free device
        # memory (torch's caching allocator keeps the block for the next call)
        per_point = int(L.st_lv_grad_workspace_bytes(1, t.size))
        free, _ = torch.cuda.mem_get_info(dev)
        chunk = min(int(chunk), max(1024, free // 4 // per_point))
        m = min(n, chunk)
        wb = int(L.st_lv_grad_workspace_bytes(m, t.size))
        work = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            nat.check(L.st_lv_grad_log_posterior_ws(
                nat.ptr(thd[c0:c1]), c1 - c0, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data, cinv.ctypes.data,
                int(max_steps), nat.ptr(out[c0:c1]), nat.ptr(status[c0:c1]), nat.ptr(work), wb,
                nat.stream_handle()), 'st_lv_grad_log_posterior_ws')
    res, st = out[:n].cpu().numpy(), status[:n].cpu().numpy()
    _status_check(st, 'grad_log_posterior')
    return res


def log_target_density(log_theta, data: Optional[LvData] = None, rtol: float = RTOL, atol: float = ATOL,
                       max_steps: int = MAX_STEPS, chunk: int = 1 << 16) -> np.ndarray:
    """``lotka_volterra.log_target_density`` for every row of ``log_theta`` ((n, 4) or (4,)):
    returns (n,)."""
    import torch
    data = reference_data() if data is None else data
    lth = _points(log_theta)
    th = np.exp(lth)                                   # as the reference: np.exp(log_theta)
    t, y, s = _settings(data, rtol, atol)
    U, c_log, norm_logc = _density_constants(data)
    dev = nat.require_device()
    L = nat.lib()
    n = th.shape[0]
    res = np.empty(n)
    st = np.zeros(n, dtype=np.int32)
    td, yd = (torch.from_numpy(a).to(dev) for a in (t, y))
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        m = c1 - c0
        ltd = torch.from_numpy(lth[c0:c1]).to(dev)
        thd = torch.from_numpy(th[c0:c1]).to(dev)
        out = torch.empty(m, dtype=torch.float64, device=dev)
        status = torch.zeros(m, dtype=torch.int32, device=dev)
        wb = int(L.st_lv_log_density_workspace_bytes(m, t.size))
        work = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev)
        nat.check(L.st_lv_log_target_density(
            nat.ptr(ltd), nat.ptr(thd), m, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data, U.ctypes.data,
            c_log, norm_logc, int(max_steps), nat.ptr(out), nat.ptr(status), nat.ptr(work), wb,
            nat.stream_handle()), 'st_lv_log_target_density')
        res[c0:c1] = out.cpu().numpy()
        st[c0:c1] = status.cpu().numpy()
    _status_check(st, 'log_target_density')
    return res


def for_unique(func: Callable[[np.ndarray], np.ndarray], sample: np.ndarray) -> np.ndarray:
    """``parallelise_for_unique`` (code/src/utils/parallel.py) with a batched ``func``: evaluate the
    unique rows once, in one batch, and scatter back."""
    unique_samples, inverse_index = np.unique(sample, axis=0, return_inverse=True)
    return func(unique_samples)[inverse_index.reshape(-1)]


# Metropolis steps per launch of rw_sample: a long run is a sequence of launches that hand the chain state
# on, so that no kernel occupies the device for long.  Measured on MI355X (tools/lv_mcmc_bench.py,
# profiles/lv_mcmc_bench.json): one launch of 256 steps takes 0.180 s at 65 536 chains (0.70 ms per step, device
# noise), 0.170 s at 4096 and 0.140 s at 5 -- under the quarter of a second a launch is meant to stay below.
STEPS_PER_LAUNCH = 256
# layout='wave' (one wave per chain, st_lv_rwmh_wave).  layout='auto' takes it for at most WAVE_MAX_CHAINS chains:
# the largest chain count of the sweep 5, 64, 256, 1024, 4096 at which the wave layout is faster than the thread
# layout by more than the spread of the windows.  Measured on MI355X (tools/lv_mcmc_bench.py,
# profiles/lv_mcmc_wave_bench.json, 256 steps, supplied noise): wave / thread time 0.109 at 5 chains (0.056 against
# 0.510 ms per step), 0.094, 0.093, 0.092 at 64, 256, 1024 and still 0.254 at 4096 (0.160 against 0.629 ms per
# step), where the windows of either layout spread by 1 % (12 % for the thread layout at 5 chains).  More than 4096
# chains were not measured in the wave layout: every wave repeats the integrator, so its time grows with the
# chain count from 2048 waves on (two per SIMD) while the thread layout's stays flat up to 65 536 chains.
# STEPS_PER_LAUNCH_WAVE: one launch of 256 steps at 4096 chains takes 0.044 s (device noise; 0.015 s at 5 chains),
# under the quarter of a second with room for chains whose steps take twice as long (seen: 0.104 against 0.057 ms
# per step for one of the reference's five starts); launches queue, so longer ones were not expected to gain.
# Results do not depend on it.
WAVE_MAX_CHAINS = 4096
STEPS_PER_LAUNCH_WAVE = 256
LAYOUTS = ('thread', 'wave', 'auto')


@dataclass
class RwSample:
    """Result of ``rw_sample`` (NumPy arrays, or ROCm tensors with ``device_out=True``)."""
    samples: object                   # (chains, n_samples, 4) log theta; row 0 is the start
    log_p: object                     # (chains, n_samples) log target density of every row
    accepted: object                  # (chains,) int64: accepted proposals
    n_failed: object                  # (chains,) int64: proposals rejected without a density (theta out of
    #                                   range, or an RK45 integration that failed)
    z: object = None                  # (chains, n_samples - 1, 4): the normal noise used (return_noise)
    log_u: object = None              # (chains, n_samples - 1): the log uniforms used (return_noise)


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith('torch')


def _chain_start(log_theta_init, n_samples, step_size):
    """Checked arguments every sampler starts from: the (chains, 4) starts, n_samples as an int, the (4,) step."""
    x0 = _points(log_theta_init)
    if x0.shape[0] < 1:
        raise ValueError('need at least one chain')
    if not np.all(np.isfinite(x0)):
        raise ValueError('log_theta_init must be finite')
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or n_samples < 1:
        raise ValueError(f'n_samples must be an integer >= 1, got {n_samples!r}')
    step = np.asarray(step_size, dtype=np.float64)
    if step.ndim == 0:
        step = np.full(4, float(step))
    if step.shape != (4,):
        raise ValueError(f'step_size must be a scalar or (4,), got {step.shape}')
    if not np.all(np.isfinite(step)) or np.any(step <= 0):
        raise ValueError(f'step_size must be finite and > 0, got {step_size!r}')
    return x0, int(n_samples), np.ascontiguousarray(step)


def _chain_noise(chains, steps, seed, noise, first_chain, steps_per_launch, default_spl, max_steps):
    """The samplers' remaining common checks: (seed as an int or None, noise as a pair (z, log_u) or None, steps
    per launch)."""
    if noise is None and seed is None:
        raise ValueError('give seed= (device noise) or noise=(z, log_u)')
    if noise is not None and seed is not None:
        raise ValueError('give either seed= or noise=(z, log_u), not both')
    if noise is not None:
        if not isinstance(noise, (tuple, list)) or len(noise) != 2:
            raise ValueError('noise must be a pair (z, log_u)')
        noise = z_in, lu_in = [a if _is_tensor(a) else np.asarray(a, dtype=np.float64) for a in noise]
        if tuple(z_in.shape) != (chains, steps, 4) or tuple(lu_in.shape) != (chains, steps):
            raise ValueError(f'noise must be z ({chains}, {steps}, 4) and log_u ({chains}, {steps}), got '
                             f'{tuple(z_in.shape)} and {tuple(lu_in.shape)}')
    else:
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f'seed must be an integer in [0, 2**64), got {seed!r}')
        seed = int(seed)
    if isinstance(first_chain, bool) or int(first_chain) != first_chain or first_chain < 0:
        raise ValueError(f'first_chain must be an integer >= 0, got {first_chain!r}')
    spl = default_spl if steps_per_launch is None else steps_per_launch
    if isinstance(spl, bool) or int(spl) != spl or spl < 1:
        raise ValueError(f'steps_per_launch must be an integer >= 1, got {steps_per_launch!r}')
    if max_steps < 1:
        raise ValueError('max_steps must be >= 1')
    return seed, noise, int(spl)


def _chain_problem(data, rtol, atol):
    """The posterior as the samplers' entry points take it: (data, t, y, s, U, c_log, norm_logc), host values."""
    data = reference_data() if data is None else data
    t, y, s = _settings(data, rtol, atol)
    if t.size < 1:
        raise ValueError('need at least one observation')
    return (data, t, y, s) + _density_constants(data)


def _check_start(failed_start, log_p):
    """Raise for chains whose start row has no density (its log_p is NaN)."""
    import torch
    bad = torch.isnan(log_p[:, 0])
    if bool(bad.any()):
        first = int(torch.nonzero(bad)[0, 0])
        raise ValueError(f'{failed_start} of {int(bad.sum())} starting point(s) failed '
                         f'(first: chain {first}): theta out of range or the RK45 integration did not finish')


def _run_chains(*, failed_start, x0, n_samples, seed, noise, first_chain, spl, max_steps, problem, return_noise,
                device_out, state_words, n_extra, launch, n_extra_rows=0, drive=None):
    """Run checked chains (``_chain_start``, ``_chain_noise``, ``_chain_problem``) on the device: returns samples,
    log_p, ``n_extra`` further (chains, n_samples, 4) per-row outputs, ``n_extra_rows`` further (chains, n_samples)
    ones, accepted, n_failed, z, log_u.  The state
    record has ``state_words`` words per chain.  ``launch(L, head=, mid=, rows=, extra=, tail=)`` makes one
    entry-point call from the argument groups that every sampler's entry point has, in this order, between its own
    (head: state .. init; mid: noise_mode .. norm_logc; rows: max_steps, samples, log_p; tail: out_ld ..).
    ``drive(advance, state, samples, log_p)`` replaces the plain run of all steps: it calls ``advance(k0, k1)`` for
    consecutive step ranges (launches never cross a range's end; ``each=`` is called after every launch) and may read
    and write the state record and whatever device arrays ``launch`` hands over in between."""
    import torch
    _, t, y, s, U, c_log, norm_logc = problem
    chains, steps = x0.shape[0], n_samples - 1
    dev = nat.require_device()
    L = nat.lib()
    td, yd = (torch.from_numpy(a).to(dev) for a in (t, y))
    state = torch.zeros((chains, state_words), dtype=torch.float64, device=dev)   # counts: int64 zero = float 0.0 bits
    state[:, :4] = torch.from_numpy(np.array(x0)).to(dev)          # (a copy: the caller's array may be read-only)
    # n_samples = 1: the kernel runs at least one step; that step goes to a spare row and is dropped
    ld = max(n_samples, 2)
    samples, *extra = (torch.empty((chains, ld, 4), dtype=torch.float64, device=dev) for _ in range(1 + n_extra))
    log_p = torch.empty((chains, ld), dtype=torch.float64, device=dev)
    extra += [torch.empty((chains, ld), dtype=torch.float64, device=dev) for _ in range(n_extra_rows)]
    mode, zd, lud = 1, None, None
    if steps >= 1 and noise is not None:
        mode = 0
        zd, lud = (a.to(device=dev, dtype=torch.float64).contiguous() if _is_tensor(a)
                   else torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(dev) for a in noise)
    elif steps >= 1 and return_noise:
        mode = 2
        zd = torch.empty((chains, steps, 4), dtype=torch.float64, device=dev)
        lud = torch.empty((chains, steps), dtype=torch.float64, device=dev)
    run = max(steps, 1)

    def advance(first, last, each=None):
        for k0 in range(first, last, spl):
            k = min(spl, last - k0)
            launch(L, head=(nat.ptr(state), chains, int(first_chain), k0 + 1, k, 1 if k0 == 0 else 0),
                   mid=(mode, seed if noise is None else 0, nat.ptr(zd), nat.ptr(lud), run, k0, nat.ptr(td), t.size,
                        nat.ptr(yd), s.ctypes.data, U.ctypes.data, c_log, norm_logc),
                   rows=(int(max_steps), nat.ptr(samples), nat.ptr(log_p)), extra=[nat.ptr(e) for e in extra],
                   tail=(ld, k0 + 1, nat.stream_handle()))
            if each is not None:
                each()
    if drive is None:
        advance(0, run)
    else:
        drive(advance, state, samples, log_p)
    _check_start(failed_start, log_p)
    counts = state.view(torch.int64)[:, 5:7]
    if steps == 0:
        counts = torch.zeros_like(counts)
        samples, log_p, extra = samples[:, :1], log_p[:, :1], [e[:, :1] for e in extra]
        if return_noise or noise is not None:
            zd = torch.empty((chains, 0, 4), dtype=torch.float64, device=dev)
            lud = torch.empty((chains, 0), dtype=torch.float64, device=dev)
    if not return_noise:
        zd = lud = None
    res = (samples, log_p, *extra, counts[:, 0].clone(), counts[:, 1].clone(), zd, lud)
    return res if device_out else tuple(None if a is None else a.cpu().numpy() for a in res)


def rw_sample(log_theta_init, n_samples, step_size=0.0025, *, seed=None, noise=None,
              data: Optional[LvData] = None, rtol: float = RTOL, atol: float = ATOL, max_steps: int = MAX_STEPS,
              first_chain: int = 0, steps_per_launch: Optional[int] = None, return_noise: bool = False,
              device_out: bool = False, layout: str = 'thread') -> RwSample:
    """Random-walk Metropolis chains on the LV log posterior, one chain per GPU thread (``st_lv_rwmh``) or per
    wave (``st_lv_rwmh_wave``; csrc/lv_mcmc.hip): the sampling stage of the reference's ``Sampling.ipynb``
    (5 chains of 500 000 rows, proposal step 0.0025, acceptance ~0.23), for as many chains as are given.

    ``log_theta_init`` is (chains, 4) or (4,): the chains' starting rows (log theta).  Every chain gets
    ``n_samples`` rows, row 0 being its start.  The proposal is ``x + step_size * N(0, I)`` (``step_size`` a
    scalar or a (4,) vector) and is accepted exactly when ``log_u < log_p(proposal) - log_p(x)``.  This is the
    project's own definition of the sampler: the reference's loop lives in a package (``toy_mcmc``) that is not
    part of its tree.  ``log_p`` is ``log_target_density`` of every row, computed by the sampler itself (the
    reference recomputes ``rw_log_p`` in a separate job); its sum over the observation times runs in time
    order, ~1e-13 relative from ``log_target_density``'s pairwise order.

    Noise: ``noise=(z, log_u)`` with z (chains, n_samples - 1, 4) standard normals and log_u
    (chains, n_samples - 1) log uniforms (NumPy arrays or ROCm tensors) reproduces a host generator exactly;
    otherwise ``seed`` (0 <= seed < 2**64) is required and chain c draws from NumPy's Philox with key
    ``(seed, first_chain + c)``: step t uses ``np.random.Philox(key=[seed, c], counter=[0, 0, 0, 0])
    .random_raw(8 * t)[8 * (t - 1):]`` = r0 .. r7 as u_k = ((r_k >> 11) + 1) 2^-53, (z0, z1) =
    sqrt(-2 ln u0) (cos, sin)(2 pi u1), (z2, z3) from u2, u3, log_u = log((r4 >> 11) 2^-53).  The noise depends
    on (seed, chain id, t) only, never on the number of chains or on ``steps_per_launch``; ``first_chain``
    offsets the chain ids, so a run may be split over calls or devices.  ``return_noise=True`` also returns
    the noise used.

    A proposal whose theta = exp(log theta) has a zero or non-finite component, or whose integration fails,
    is rejected and counted in ``n_failed``; a START whose own density fails raises ValueError.
    ``device_out=True`` returns ROCm tensors (for ``thin_chains`` / ``thin_gf`` without a host round trip).
    ``steps_per_launch`` (default ``STEPS_PER_LAUNCH``, ``STEPS_PER_LAUNCH_WAVE`` in the wave layout) splits the
    run into launches; the result does not depend on it.

    ``layout``: ``'thread'`` (default) runs one chain per GPU thread, the shape for thousands of chains.
    ``'wave'`` runs one chain per wave of 64 lanes, the shape for a few long chains such as the reference's five:
    every lane repeats the chain's proposal and RK45 integration and the observation points are split over the
    lanes (point k goes to lane k mod 64).  ``'auto'`` takes ``'wave'`` for at most ``WAVE_MAX_CHAINS`` chains and
    ``'thread'`` otherwise.  Everything above holds in both layouts.  Between the two, proposals and device
    noise are bit-identical, and so is every per-point term of ``log_p``; only the order of their sum differs
    (wave: each lane adds its points in increasing k, then the 64 partial sums are combined by an xor butterfly
    with offsets 32 .. 1; an order that depends on t_n only), so ``log_p`` agrees to ~1e-13 relative (bit for bit
    with at most 2 observation times) and the chains are equal row for row as long as no accept / reject
    decision is closer than that.  A wave-layout chain is bit-identical to itself under any launch split, any
    ``first_chain`` offset, with or without ``return_noise``, and when re-run from its recorded noise."""
    if layout not in LAYOUTS:
        raise ValueError(f'layout must be one of {LAYOUTS}, got {layout!r}')
    x0, n_samples, step = _chain_start(log_theta_init, n_samples, step_size)
    wave = layout == 'wave' or (layout == 'auto' and x0.shape[0] <= WAVE_MAX_CHAINS)
    seed, noise, spl = _chain_noise(x0.shape[0], n_samples - 1, seed, noise, first_chain, steps_per_launch,
                                    STEPS_PER_LAUNCH_WAVE if wave else STEPS_PER_LAUNCH, max_steps)
    name = 'st_lv_rwmh_wave' if wave else 'st_lv_rwmh'

    def launch(L, head, mid, rows, extra, tail):
        nat.check(getattr(L, name)(*head, step.ctypes.data, *mid, *rows, *tail), name)
    return RwSample(*_run_chains(
        failed_start='rw_sample: the log target density', x0=x0, n_samples=n_samples, seed=seed, noise=noise,
        first_chain=first_chain, spl=spl, max_steps=max_steps, problem=_chain_problem(data, rtol, atol),
        return_noise=return_noise, device_out=device_out, state_words=8, n_extra=0, launch=launch))


# Metropolis steps per launch of mala_sample.  Measured on MI355X (tools/lv_mala_bench.py, profiles/lv_mala_bench.json:
# 256 steps as four launches of 64, device noise, eps 0.003, drift cap 1, starts near the mode): a launch of 64 steps
# takes 0.046 s at 4096 chains, the largest count swept (0.72 ms per step), and 0.011-0.012 s at 5 to 1024 chains
# (0.18 ms per step).  256 steps in one launch would take 0.185 s at 4096 chains -- under the quarter of a second a
# launch is meant to stay below, but without room for chains whose integrations take twice the steps (seen in
# rw_sample from one of the reference's starts), so 64 stays.  Launches queue behind one another; a different split
# was not timed.  Results do not depend on it.
STEPS_PER_LAUNCH_MALA = 64


@dataclass
class MalaSample:
    """Result of ``mala_sample`` (NumPy arrays, or ROCm tensors with ``device_out=True``)."""
    samples: object                   # (chains, n_samples, 4) log theta; row 0 is the start
    log_p: object                     # (chains, n_samples) log target density of every row (10-state solution)
    grad: object                      # (chains, n_samples, 4) gradient of log p with respect to log theta
    accepted: object                  # (chains,) int64: accepted proposals
    n_failed: object                  # (chains,) int64: proposals rejected without a density
    z: object = None                  # (chains, n_samples - 1, 4): the normal noise used (return_noise)
    log_u: object = None              # (chains, n_samples - 1): the log uniforms used (return_noise)


def mala_sample(log_theta_init, n_samples, step_size, *, seed=None, noise=None, drift_cap: float = math.inf,
                data: Optional[LvData] = None, rtol: float = RTOL, atol: float = ATOL, max_steps: int = MAX_STEPS,
                first_chain: int = 0, steps_per_launch: Optional[int] = None, return_noise: bool = False,
                device_out: bool = False) -> MalaSample:
    """Metropolis-adjusted Langevin (MALA) chains on the LV log posterior, one chain per GPU wave
    (``st_lv_mala_wave``, csrc/lv_mcmc.hip): the gradient-based stage of the reference's ``Sampling.ipynb``.  The
    reference uses Stan's HMC there, which is not part of its tree, so the sampler is this project's own
    definition.  Every row leaves with ``log_p`` and with ``grad`` = the gradient of log p with respect to
    log theta -- the ``exp(samples) * grads`` the reference hands to ``thin`` -- so no separate
    ``grad_log_posterior`` pass is needed: ``thin_chains(list(run.samples), list(run.grad), m)``.

    Definition.  The chain runs in x = log theta; ``step_size`` is eps, a scalar or a (4,) vector (no default:
    nothing in the reference fixes one; measured with the reference data, 5 chains of 256 steps from starts 0.02
    off log(THETA) with ``drift_cap=1``: acceptance 0.98 at eps 0.0005, 0.73 at 0.001, 0.30 at 0.002, 0.15 at
    0.003, 0.08 at 0.004 -- eps between 0.001 and 0.002 is usable, profiles/lv_mala_bench.json).  The host computes h = 0.5 eps eps, w = 0.5 / (eps eps) and
    c = drift_cap eps once.  One 10-state RK45 integration at theta = exp(x) gives lp(x) (the terms of
    ``log_target_density``) and g(x) = theta * sum_k J_k^T C^-1 (y_k - u_k) - x, which equals
    ``exp(x) * grad_log_posterior(exp(x))`` to rounding.  A step proposes
    ``p = (x + clip(h * g(x), -c, c)) + eps * z`` and accepts exactly when
    ``log_u < (lp(p) - lp(x)) + (qf - qr)`` with qf = sum_j w_j rf_j rf_j, rf = (p - x) - d(x), and qr likewise
    from rr = (x - p) - d(p); the comparison is strict and a NaN anywhere rejects.  ``drift_cap`` (> 0, default
    inf: none) bounds every drift component at ``drift_cap * eps``; far from the mode the gradient is large and
    an uncapped drift throws proposals to theta where the integration takes very long.

    ``log_p`` comes from the 10-state solution, whose RK45 step sequence is not the 2-state one of
    ``log_target_density`` / ``rw_sample``: the two differ by the integrator's tolerance (rtol 1e-3), not by
    rounding (DESIGN.md section 17 has the figures).

    Noise, ``seed``, ``noise=(z, log_u)``, ``first_chain``, ``return_noise``, ``device_out`` and the treatment of
    failed proposals (``n_failed``) are ``rw_sample``'s: for one seed and chain id the noise is the same, bit for
    bit.  A START whose own evaluation fails raises ValueError.  ``steps_per_launch`` (default
    ``STEPS_PER_LAUNCH_MALA``) splits the run into launches; the result does not depend on it.  Lane l of a
    chain's wave adds the observation points k = l (mod 64) in increasing k and the 64 partial sums are combined
    by an xor butterfly (offsets 32 .. 1), for the density and for each gradient component; a chain is
    bit-identical to itself under any launch split, any ``first_chain`` offset, with or without
    ``return_noise``, and when re-run from its recorded noise."""
    x0, n_samples, eps = _chain_start(log_theta_init, n_samples, step_size)
    with np.errstate(over='ignore', divide='ignore'):
        ehw = np.ascontiguousarray(np.concatenate([eps, 0.5 * eps * eps, 0.5 / (eps * eps)]))
    if not np.all(np.isfinite(ehw)) or np.any(ehw <= 0):
        raise ValueError(f'step_size {step_size!r}: 0.5 eps^2 and 0.5 / eps^2 must be finite and > 0')
    try:
        cap = float(drift_cap)
    except (TypeError, ValueError):
        raise ValueError(f'drift_cap must be a number > 0, got {drift_cap!r}') from None
    if isinstance(drift_cap, bool) or not cap > 0:
        raise ValueError(f'drift_cap must be > 0 (inf: no cap), got {drift_cap!r}')
    clip = np.ascontiguousarray(cap * eps)
    seed, noise, spl = _chain_noise(x0.shape[0], n_samples - 1, seed, noise, first_chain, steps_per_launch,
                                    STEPS_PER_LAUNCH_MALA, max_steps)
    problem = _chain_problem(data, rtol, atol)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(problem[0].cov, dtype=np.float64)))

    def launch(L, head, mid, rows, extra, tail):
        nat.check(L.st_lv_mala_wave(*head, ehw.ctypes.data, clip.ctypes.data, *mid, cinv.ctypes.data, *rows, *extra,
                                    *tail), 'st_lv_mala_wave')
    return MalaSample(*_run_chains(
        failed_start='mala_sample: the evaluation', x0=x0, n_samples=n_samples, seed=seed, noise=noise,
        first_chain=first_chain, spl=spl, max_steps=max_steps, problem=problem, return_noise=return_noise,
        device_out=device_out, state_words=16, n_extra=1, launch=launch))


def STEPS_PER_LAUNCH_HMC(n_leapfrog: int) -> int:
    """Metropolis steps per launch of ``hmc_sample`` for trajectories of ``n_leapfrog`` stages."""
    # 64 leapfrog stages per launch, first an estimate from MALA's 0.18 ms per gradient evaluation, then MEASURED on
    # MI355X (tools/lv_hmc_bench.py, profiles/lv_hmc_bench.json: eps 0.001, kick cap 0.5, starts near the mode, L = 1,
    # 4 and 16): a launch of 64 stages takes 0.012-0.013 s at 5 to 1024 chains (0.18-0.20 ms per stage) and 0.048-0.049 s
    # at 4096 (0.73-0.75 ms), as MALA's 64 steps do, and 0.025 s from the reference's far starts -- far below the
    # quarter of a second, with room for integrations that take several times the steps.  A trajectory longer than
    # 64 stages is one launch per step.  Other splits were not timed.  Results do not depend on it.
    return max(1, 64 // int(n_leapfrog))


NUTS_MAX_DEPTH = 10                  # the kernel's checkpoint slots: a step is at most 2**10 - 1 = 1023 stages


def STEPS_PER_LAUNCH_NUTS(max_depth: int) -> int:
    """Steps per launch of ``nuts_sample`` for trees of at most ``max_depth`` doublings."""
    # STEPS_PER_LAUNCH_HMC's launch of 64 stages, taken at the worst case of 2**max_depth - 1 stages per step.  From
    # depth 6 on it is one step per launch, and one step at depth 10 can be 1023 stages.  MEASURED on MI355X
    # (tools/lv_nuts_bench.py, profiles/lv_nuts_bench.json): a stage takes 0.189-0.195 ms at 5 to 1024 chains and
    # 0.77 ms at 4096; the worst case, a launch in which a chain runs all 1023 stages, 0.194 s at 64 chains, 0.195 s
    # at 1024 and 0.769 s at 4096 -- above the quarter of a second a launch is meant to stay below: with thousands of
    # chains max_depth 8 (255 stages) keeps to it.  The reference-shaped run's longest step was 103 stages (0.02 s).
    # Other splits were not timed.  Results do not depend on it.
    return max(1, 64 // (2 ** int(max_depth) - 1))


@dataclass
class HmcSample:
    """Result of ``hmc_sample`` (NumPy arrays, or ROCm tensors with ``device_out=True``)."""
    samples: object                   # (chains, n_samples, 4) log theta; row 0 is the start
    log_p: object                     # (chains, n_samples) log target density of every row (10-state solution)
    grad: object                      # (chains, n_samples, 4) gradient of log p with respect to log theta
    accepted: object                  # (chains,) int64: accepted trajectories
    n_failed: object                  # (chains,) int64: trajectories rejected because a stage had no density
    z: object = None                  # (chains, n_samples - 1, 4): the normal noise used (return_noise)
    log_u: object = None              # (chains, n_samples - 1): the log uniforms used (return_noise)


def hmc_sample(log_theta_init, n_samples, step_size, n_leapfrog, *, seed=None, noise=None,
               kick_cap: float = math.inf, data: Optional[LvData] = None, rtol: float = RTOL, atol: float = ATOL,
               max_steps: int = MAX_STEPS, first_chain: int = 0, steps_per_launch: Optional[int] = None,
               return_noise: bool = False, device_out: bool = False) -> HmcSample:
    """Hamiltonian Monte Carlo (HMC) chains on the LV log posterior, one chain per GPU wave (``st_lv_hmc_wave``,
    csrc/lv_mcmc.hip): the gradient-based stage of the reference's ``Sampling.ipynb``, which uses Stan's HMC.  Stan
    is not part of the reference's tree, so the sampler is this project's own definition: a fixed trajectory
    length and a fixed step size, no adaptation.  As with ``mala_sample`` every row leaves with ``log_p`` and
    ``grad``, so ``thin_chains(list(run.samples), list(run.grad), m)`` needs no further pass.

    Definition.  The chain runs in x = log theta with unit-variance momenta; ``step_size`` is eps, a scalar or a
    (4,) vector (a vector eps is a diagonal mass matrix), ``n_leapfrog`` = L >= 1 the stages of a trajectory and
    ``kick_cap`` > 0 (default inf: none) the bound c on every component of eps * g.  lp(x) and g(x) are
    ``mala_sample``'s: one 10-state RK45 integration at theta = exp(x).  With hk(q) = 0.5 * clip(eps * g(q), -c, c)
    and K(r) = 0.5 * sum_j r_j r_j, one step draws r^0 = z (the step's four normals), runs from (q^0, r^0) = (x, z)
    the stages ``r' = r + hk(q); q = q + eps * r'; r = r' + hk(q)`` (one multiply and one add per component, an
    interior kick as two half-kick additions) and accepts q^L exactly when
    ``log_u < (lp(q^L) - lp(x)) + (K(r^0) - K(r^L))``; the comparison is strict and a NaN anywhere rejects.  A
    trajectory of L stages is therefore, bit for bit, L one-stage trajectories chained through (q, r).  With
    L = 1 the proposal is MALA's up to rounding.  The capped force depends on q alone, so every stage stays a
    shear: the map is reversible and volume-preserving, and with the true lp in the ratio the chain still targets
    the posterior.  ``kick_cap`` plays ``drift_cap``'s role: from far starts eps * g is ~1e2 and an uncapped
    trajectory is thrown to theta where integrations take very long.  Nothing in the reference fixes eps or L;
    measured with the reference data (5 chains of 128 steps from starts 0.02 off log(THETA), ``kick_cap=0.5``,
    profiles/lv_hmc_bench.json): acceptance 0.68 / 0.59 / 0.46 for L = 1 / 4 / 16 at eps 0.001, 0.83 / 0.83 / 0.76 at
    0.0005, 0.42 / 0.29 / 0.11 at 0.002.

    A stage whose theta has a zero or non-finite component, or whose integration fails, fails its whole
    trajectory: it is rejected and counted once in ``n_failed``, and its later stages run no integration.  A START
    whose own evaluation fails raises ValueError.

    Noise, ``seed``, ``noise=(z, log_u)``, ``first_chain``, ``return_noise`` and ``device_out`` are ``rw_sample``'s:
    for one seed and chain id the noise is the same, bit for bit (one set of four normals and one log uniform
    per step, whatever L is).  ``steps_per_launch`` (default ``STEPS_PER_LAUNCH_HMC(n_leapfrog)``) splits the run
    into launches; the result does not depend on it.  The summation order is ``mala_sample``'s; a chain is
    bit-identical to itself under any launch split, any ``first_chain`` offset, with or without ``return_noise``,
    and when re-run from its recorded noise."""
    x0, n_samples, eps = _chain_start(log_theta_init, n_samples, step_size)
    if isinstance(n_leapfrog, bool) or not isinstance(n_leapfrog, (int, np.integer)) or not 1 <= n_leapfrog < 2 ** 31:
        raise ValueError(f'n_leapfrog must be an integer >= 1, got {n_leapfrog!r}')
    n_leapfrog = int(n_leapfrog)
    try:
        cap = float(kick_cap)
    except (TypeError, ValueError):
        raise ValueError(f'kick_cap must be a number > 0, got {kick_cap!r}') from None
    if isinstance(kick_cap, bool) or not cap > 0:
        raise ValueError(f'kick_cap must be > 0 (inf: no cap), got {kick_cap!r}')
    clip = np.full(4, cap)
    seed, noise, spl = _chain_noise(x0.shape[0], n_samples - 1, seed, noise, first_chain, steps_per_launch,
                                    STEPS_PER_LAUNCH_HMC(n_leapfrog), max_steps)
    problem = _chain_problem(data, rtol, atol)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(problem[0].cov, dtype=np.float64)))

    def launch(L, head, mid, rows, extra, tail):
        nat.check(L.st_lv_hmc_wave(*head, eps.ctypes.data, clip.ctypes.data, n_leapfrog, *mid, cinv.ctypes.data, *rows,
                                   *extra, *tail), 'st_lv_hmc_wave')
    return HmcSample(*_run_chains(
        failed_start='hmc_sample: the evaluation', x0=x0, n_samples=n_samples, seed=seed, noise=noise,
        first_chain=first_chain, spl=spl, max_steps=max_steps, problem=problem, return_noise=return_noise,
        device_out=device_out, state_words=16, n_extra=1, launch=launch))


# ---- HMC with a per-chain step size and dense metric, and its warm-up ----
# words 16 .. 20 of st_lv_hmc_metric_wave's state record: eps, m, sbar, xbar, mu
_DA_WORDS = slice(16, 21)
DA_GAMMA, DA_T0, DA_KAPPA = 0.05, 10.0, 0.75        # the kernel's constants (Stan's defaults)
WARMUP_INIT_BUFFER, WARMUP_TERM_BUFFER, WARMUP_BASE_WINDOW = 75, 50, 25
METRIC_REG = 1e-3                                    # Stan's regulariser: Sigma = n/(n+5) S + 1e-3 * 5/(n+5) I


@dataclass
class HmcMetricSample:
    """Result of ``hmc_metric_sample``: ``HmcSample``'s fields, then the per-step outputs."""
    samples: object
    log_p: object
    grad: object
    accepted: object
    n_failed: object
    z: object = None
    log_u: object = None
    accept_stat: object = None        # (chains, n_samples - 1): min(1, exp(a)) of the step that wrote row t + 1
    step_size: object = None          # (chains, n_samples - 1): the eps that step used
    adapt_state: object = None        # (chains, 5) eps, m, sbar, xbar, mu after the last step (target_accept given)
    adapt_trace: object = None        # (launches, chains, 5): the same after every launch (return_adapt_trace)


@dataclass
class NutsSample:
    """Result of ``nuts_sample``: ``HmcMetricSample``'s fields (``log_u`` stays None: the sampler has no accept
    draw), then the tree's per-step outputs."""
    samples: object
    log_p: object
    grad: object
    accepted: object                  # (chains,) int64: steps whose row was replaced at least once
    n_failed: object                  # (chains,) int64: divergent steps
    z: object = None
    log_u: object = None
    accept_stat: object = None        # (chains, n_samples - 1): the mean of min(1, exp(a)) over the step's stages
    step_size: object = None
    adapt_state: object = None
    adapt_trace: object = None
    tree_depth: object = None         # (chains, n_samples - 1) int32: doublings started
    n_leapfrog: object = None         # (chains, n_samples - 1) int32: stages done
    divergent: object = None          # (chains, n_samples - 1) bool


@dataclass
class HmcWindow:
    """One slow window of ``hmc_warmup``: steps [start, stop), the dual-averaging xbar (chains,) at its end, and the
    step size (chains,) and metric factor (chains, 4, 4) the chains went on with."""
    start: int
    stop: int
    xbar: object
    step_size: object
    metric_chol: object


@dataclass
class HmcAdaptation:
    """Result of ``hmc_warmup`` (NumPy arrays, or ROCm tensors with ``device_out=True`` for the per-row fields)."""
    step_size: object                 # (chains,) the adapted eps = exp(xbar)
    metric_chol: object               # (chains, 4, 4) Lam, lower triangular, M^-1 = Lam Lam^T
    last_row: object                  # (chains, 4) the last warm-up row: the start of the sampling run
    samples: object                   # (chains, n_warmup + 1, 4); row 0 is the start
    log_p: object
    grad: object
    accept_stat: object               # (chains, n_warmup)
    step_sizes: object                # (chains, n_warmup): the eps every warm-up step used
    windows: object                   # list of HmcWindow
    accepted: object = None
    n_failed: object = None


def _libm(fn, a, *args):
    """``fn`` (a ``math`` function) of every element of ``a``, one C-library call per value.  The warm-up's few host
    scalars go this way, not through NumPy's exp / log / power, whose SIMD variants differ by an ulp between CPUs: the
    chains are chaotic, and the schedule should give the same step sizes wherever it runs."""
    a = np.asarray(a, dtype=np.float64)

    def one(v):
        try:
            return fn(v, *args)
        except OverflowError:
            return math.inf
    return np.array([one(float(v)) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def hmc_warmup_windows(n_warmup: int):
    """The slow windows [(start, stop), ...] of Stan's warm-up schedule for ``n_warmup`` steps: an initial buffer of
    75 steps, a final one of 50 and a first window of 25 -- or, where these do not fit, 15 % / 10 % of ``n_warmup``
    (rounded down) and the rest as one window; every window is twice as long as the one before, and a window is
    stretched to the end of the slow region when the next one would not fit.  Steps before the first window and
    after the last adapt the step size only."""
    if isinstance(n_warmup, bool) or int(n_warmup) != n_warmup or n_warmup < 20:
        raise ValueError(f'n_warmup must be an integer >= 20, got {n_warmup!r}')
    n = int(n_warmup)
    init, term, size = WARMUP_INIT_BUFFER, WARMUP_TERM_BUFFER, WARMUP_BASE_WINDOW
    if init + size + term > n:
        init, term = int(0.15 * n), int(0.1 * n)
        size = n - init - term
    slow_end = n - term
    windows, start = [], init
    while start < slow_end:
        stop = start + size
        if stop + 2 * size > slow_end:
            stop = slow_end
        windows.append((start, stop))
        start, size = stop, 2 * size
    return windows


def hmc_window_metric(rows):
    """Lam (chains, 4, 4) from a window's rows (chains, n, 4), n >= 2: S the sample covariance (n - 1 divisor),
    Sigma = n / (n + 5) S + 1e-3 * 5 / (n + 5) I (Stan's regularisation), Lam = chol(Sigma), lower triangular.  torch,
    batched over the chains, on the rows' device; NumPy in, NumPy out."""
    import torch
    r = rows if _is_tensor(rows) else torch.from_numpy(np.asarray(rows, dtype=np.float64))
    if r.ndim != 3 or r.shape[2] != 4 or r.shape[1] < 2:
        raise ValueError(f'rows must be (chains, n >= 2, 4), got {tuple(r.shape)}')
    n = r.shape[1]
    d = r - r.mean(dim=1, keepdim=True)
    cov = d.transpose(1, 2) @ d / (n - 1)
    sigma = (n / (n + 5.0)) * cov + (METRIC_REG * 5.0 / (n + 5.0)) * torch.eye(4, dtype=r.dtype, device=r.device)
    lam = torch.linalg.cholesky(sigma)
    return lam if _is_tensor(rows) else lam.numpy()


def hmc_rescale_step(step_size, chol_old, chol_new):
    """The step size after a change of metric: eps * (det Lam_old / det Lam_new) ** (1 / 4), per chain -- the
    project's own rule, which keeps the mean physical step eps * det(Lam) ** (1 / 4) across the change."""
    old, new = (np.asarray(a.cpu().numpy() if _is_tensor(a) else a, dtype=np.float64) for a in (chol_old, chol_new))
    det_old, det_new = (((a[..., 0, 0] * a[..., 1, 1]) * a[..., 2, 2]) * a[..., 3, 3] for a in (old, new))
    return np.asarray(step_size, dtype=np.float64) * _libm(math.pow, det_old / det_new, 0.25)


def hmc_adapt_restart(step_size):
    """The dual-averaging state (chains, 5) = eps, m, sbar, xbar, mu that starts an adaptation at eps: m = sbar =
    xbar = 0, mu = log(10 eps)."""
    eps = np.atleast_1d(np.asarray(step_size, dtype=np.float64))
    da = np.zeros((eps.size, 5))
    da[:, 0] = eps
    da[:, 4] = _libm(math.log, 10.0 * eps)
    return da


def hmc_warmup_schedule(run_segment, n_warmup, step_size, metric_chol, window_metric=None):
    """The host side of ``hmc_warmup``, without a device: ``run_segment(start, stop, metric_chol, da)`` runs steps
    [start, stop) of all chains with the metric factors (chains, 4, 4) from the dual-averaging state ``da`` (chains, 5)
    = eps, m, sbar, xbar, mu, adapting eps after every step, and returns (the rows these steps wrote (chains,
    stop - start, 4), the state after them).  Segments are the initial buffer, every slow window of
    ``hmc_warmup_windows`` and the final buffer.  At a slow window's end, per chain: Lam_new =
    ``hmc_window_metric(rows)``, eps = ``hmc_rescale_step(exp(xbar), Lam_old, Lam_new)`` and the adaptation restarts
    (``hmc_adapt_restart``).  At the end eps = exp(xbar).  ``window_metric`` replaces ``hmc_window_metric`` (a test double's
    own, bit-reproducible statement of it).  Returns (eps (chains,), Lam (chains, 4, 4), [HmcWindow])."""
    windows = hmc_warmup_windows(n_warmup)
    chol = np.array(metric_chol, dtype=np.float64)
    da = hmc_adapt_restart(np.broadcast_to(np.asarray(step_size, dtype=np.float64), chol.shape[:1]))
    segments =[(0, windows[0][0], False)] + [(a, b, True) for a, b in windows] + [(windows[-1][1], int(n_warmup), False)]
    trace = []
    for start, stop, slow in segments:
        if stop == start:
            continue
        rows, da = run_segment(start, stop, chol, da)
        da = np.array(da, dtype=np.float64)
        if slow:
            new = (window_metric or hmc_window_metric)(rows)
            new = np.array(new.cpu().numpy() if _is_tensor(new) else new, dtype=np.float64)
            eps = hmc_rescale_step(_libm(math.exp, da[:, 3]), chol, new)
            trace.append(HmcWindow(start, stop, da[:, 3].copy(), eps, new))
            chol, da = new, hmc_adapt_restart(eps)
    return _libm(math.exp, da[:, 3]), chol, trace


def _metric_chol(metric_chol, chains):
    """Checked (chains, 4, 4) lower-triangular factors with a positive diagonal."""
    lam = np.array(metric_chol.cpu().numpy() if _is_tensor(metric_chol) else metric_chol, dtype=np.float64)
    if lam.shape == (4, 4):
        lam = np.tile(lam, (chains, 1, 1))
    if lam.shape != (chains, 4, 4):
        raise ValueError(f'metric_chol must be (4, 4) or ({chains}, 4, 4), got {lam.shape}')
    if not np.all(np.isfinite(lam)):
        raise ValueError('metric_chol must be finite')
    if np.any(np.triu(lam, 1) != 0.0):
        raise ValueError('metric_chol must be lower triangular')
    if np.any(np.diagonal(lam, axis1=1, axis2=2) <= 0.0):
        raise ValueError('metric_chol must have a positive diagonal')
    return lam


_TRIL = np.tril_indices(4)            # row-major order of the lower triangle: the kernel's packing


def _hmc_metric_run(who, log_theta_init, n_samples, step_size, metric_chol, n_leapfrog, *, seed, noise, kick_cap, data,
                    rtol, atol, max_steps, first_chain, steps_per_launch, return_noise, device_out, delta, drive_with,
                    max_depth=None, nuts=False):
    """The checks and the launch closure ``hmc_metric_sample``, ``hmc_warmup``, ``nuts_sample`` and ``nuts_warmup``
    share.  ``drive_with(eps_d, chol_d, eps, lam)`` returns ``_run_chains``' drive (or None) given the device arrays
    the launches read.  ``nuts`` runs the NUTS kernel with ``max_depth`` (``n_leapfrog`` is not used) and returns
    ``NutsSample``."""
    import torch
    x0, n_samples, _ = _chain_start(log_theta_init, n_samples, 1.0)
    chains = x0.shape[0]
    eps = np.asarray(step_size.cpu().numpy() if _is_tensor(step_size) else step_size, dtype=np.float64)
    if eps.ndim == 0:
        eps = np.full(chains, float(eps))
    if eps.shape != (chains,):
        raise ValueError(f'step_size must be a scalar or ({chains},), one per chain, got {eps.shape}')
    if not np.all(np.isfinite(eps)) or np.any(eps <= 0):
        raise ValueError(f'step_size must be finite and > 0, got {step_size!r}')
    lam = _metric_chol(metric_chol, chains)
    if nuts:
        if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or \
                not 1 <= max_depth <= NUTS_MAX_DEPTH:
            raise ValueError(f'max_depth must be an integer from 1 to {NUTS_MAX_DEPTH}, got {max_depth!r}')
        length, default_spl = int(max_depth), STEPS_PER_LAUNCH_NUTS(int(max_depth))
    else:
        if isinstance(n_leapfrog, bool) or not isinstance(n_leapfrog, (int, np.integer)) or \
                not 1 <= n_leapfrog < 2 ** 31:
            raise ValueError(f'n_leapfrog must be an integer >= 1, got {n_leapfrog!r}')
        length, default_spl = int(n_leapfrog), STEPS_PER_LAUNCH_HMC(int(n_leapfrog))
    try:
        cap = float(kick_cap)
    except (TypeError, ValueError):
        raise ValueError(f'kick_cap must be a number > 0, got {kick_cap!r}') from None
    if isinstance(kick_cap, bool) or not cap > 0:
        raise ValueError(f'kick_cap must be > 0 (inf: no cap), got {kick_cap!r}')
    adapt = delta is not None
    if adapt and not 0.0 < float(delta) < 1.0:
        raise ValueError(f'target_accept must lie in (0, 1), got {delta!r}')
    clip = np.full(4, cap)
    seed, noise, spl = _chain_noise(chains, n_samples - 1, seed, noise, first_chain, steps_per_launch,
                                    default_spl, max_steps)
    problem = _chain_problem(data, rtol, atol)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(problem[0].cov, dtype=np.float64)))
    dev = nat.require_device()
    eps_d = torch.from_numpy(np.ascontiguousarray(eps)).to(dev)
    chol_d = torch.from_numpy(np.ascontiguousarray(lam[:, _TRIL[0], _TRIL[1]])).to(dev)
    name = 'st_lv_nuts_wave' if nuts else 'st_lv_hmc_metric_wave'

    def launch(L, head, mid, rows, extra, tail):
        nat.check(getattr(L, name)(*head, nat.ptr(eps_d), nat.ptr(chol_d), clip.ctypes.data, length,
                                   1 if adapt else 0, float(delta) if adapt else 0.5, *mid, cinv.ctypes.data,
                                   *rows, *extra, *tail), name)
    res = _run_chains(
        failed_start=f'{who}: the evaluation', x0=x0, n_samples=n_samples, seed=seed, noise=noise,
        first_chain=first_chain, spl=spl, max_steps=max_steps, problem=problem, return_noise=return_noise,
        device_out=device_out, state_words=24, n_extra=1, launch=launch, n_extra_rows=5 if nuts else 2,
        drive=drive_with(eps_d, chol_d, eps, lam))
    if not nuts:
        samples, log_p, grad, alpha, eps_used, accepted, n_failed, z, log_u = res
        return HmcMetricSample(samples, log_p, grad, accepted, n_failed, z, log_u, alpha[:, 1:], eps_used[:, 1:])
    samples, log_p, grad, alpha, eps_used, depth, stages, div, accepted, n_failed, z, _ = res
    if device_out:
        depth, stages, div = depth[:, 1:].to(torch.int32), stages[:, 1:].to(torch.int32), div[:, 1:] != 0
    else:
        depth, stages, div = depth[:, 1:].astype(np.int32), stages[:, 1:].astype(np.int32), div[:, 1:] != 0
    # the kernel neither reads nor writes log_u
    return NutsSample(samples, log_p, grad, accepted, n_failed, z, None, alpha[:, 1:], eps_used[:, 1:],
                      tree_depth=depth, n_leapfrog=stages, divergent=div)


def _adapt_drive_with(out, n_samples, target_accept, adapt_state, return_adapt_trace):
    """``_hmc_metric_run``'s ``drive_with`` for a sampling run: with ``target_accept`` the dual-averaging state is put
    into the state record before the first launch and read back into ``out`` ('state', 'trace') after the last."""
    import torch

    def drive_with(eps_d, chol_d, eps, lam):
        if target_accept is None:
            if adapt_state is not None or return_adapt_trace:
                raise ValueError('adapt_state and return_adapt_trace need target_accept')
            return None
        da0 = hmc_adapt_restart(eps) if adapt_state is None else np.array(adapt_state, dtype=np.float64)
        if da0.shape != (eps.size, 5) or not np.all(np.isfinite(da0)) or np.any(da0[:, 0] <= 0) or np.any(da0[:, 1] < 0):
            raise ValueError(f'adapt_state must be ({eps.size}, 5) finite values eps > 0, m >= 0, sbar, xbar, mu')

        def drive(advance, state, samples, log_p):
            state[:, _DA_WORDS] = torch.from_numpy(da0).to(state.device)
            trace = []
            advance(0, samples.shape[1] - 1,
                    each=(lambda: trace.append(state[:, _DA_WORDS].clone())) if return_adapt_trace else None)
            out['state'] = state[:, _DA_WORDS].clone()
            if samples.shape[1] - 1 > int(n_samples) - 1:       # a one-row run: its spare step is dropped
                out['state'], trace = torch.from_numpy(da0).to(state.device), trace[:0]
            out['trace'] = (torch.stack(trace) if trace else state.new_empty((0, eps.size, 5))) \
                if return_adapt_trace else None
        return drive
    return drive_with


def _adapt_result(run, out, target_accept, device_out):
    """``run`` with the dual-averaging state and trace that ``_adapt_drive_with`` left in ``out``."""
    if target_accept is not None:
        run.adapt_state = out['state'] if device_out else out['state'].cpu().numpy()
        if out['trace'] is not None:
            run.adapt_trace = out['trace'] if device_out else out['trace'].cpu().numpy()
    return run


def _warmup_drive_with(out, who, n_warmup):
    """``_hmc_metric_run``'s ``drive_with`` for a warm-up: ``hmc_warmup_schedule`` with a ``run_segment`` that sets the
    dual-averaging state and the metric and launches the segment's steps; eps, Lam and the windows go to ``out``."""
    import torch

    def drive_with(eps_d, chol_d, eps, lam):
        def drive(advance, state, samples, log_p):
            def run_segment(start, stop, chol, da):
                state[:, _DA_WORDS] = torch.from_numpy(np.ascontiguousarray(da)).to(state.device)
                chol_d.copy_(torch.from_numpy(np.ascontiguousarray(chol[:, _TRIL[0], _TRIL[1]])))
                advance(start, stop)
                if start == 0:
                    _check_start(f'{who}: the evaluation', log_p)
                return samples[:, start + 1:stop + 1], state[:, _DA_WORDS].cpu().numpy()
            out['eps'], out['chol'], out['windows'] = hmc_warmup_schedule(run_segment, n_warmup, eps, lam)
        return drive
    return drive_with


def _warmup_result(run, out, device_out):
    last = run.samples[:, -1].clone() if device_out else run.samples[:, -1].copy()
    return HmcAdaptation(out['eps'], out['chol'], last, run.samples, run.log_p, run.grad, run.accept_stat,
                         run.step_size, out['windows'], run.accepted, run.n_failed)


def hmc_metric_sample(log_theta_init, n_samples, step_size, metric_chol, n_leapfrog, *, seed=None, noise=None,
                      kick_cap: float = math.inf, target_accept: Optional[float] = None, adapt_state=None,
                      return_adapt_trace: bool = False, data: Optional[LvData] = None, rtol: float = RTOL,
                      atol: float = ATOL, max_steps: int = MAX_STEPS, first_chain: int = 0,
                      steps_per_launch: Optional[int] = None, return_noise: bool = False,
                      device_out: bool = False) -> HmcMetricSample:
    """HMC chains on the LV log posterior with a step size per chain and a dense metric per chain, one chain per GPU
    wave (``st_lv_hmc_metric_wave``, csrc/lv_mcmc.hip): ``hmc_sample`` as Stan's adapted sampler would run it after
    ``hmc_warmup``.  This is the project's own definition; Stan's bits are not claimed.  The trajectory length is
    fixed (no jitter); ``nuts_sample`` chooses it per step.

    Definition.  ``step_size`` is eps, a scalar or (chains,) -- one per CHAIN, not per component as in ``hmc_sample``;
    ``metric_chol`` is Lam, (4, 4) or (chains, 4, 4), lower triangular with a positive diagonal (anything else raises
    ValueError), the inverse metric being M^-1 = Lam Lam^T.  The momentum stays r ~ N(0, I), so the noise is
    ``rw_sample``'s bit for bit and K(r) = 0.5 * sum_j r_j r_j.  With f_j(q) = Lam_jj g_j(q) + sum_{k > j} Lam_kj g_k(q)
    (the first term alone, then k ascending), hk(q) = 0.5 * clip(eps * f(q), -c, c) and v_j = sum_{k <= j} Lam_jk r'_k
    (from the k = 0 term, k ascending) a stage is ``r' = r + hk(q); q = q + eps * v; r = r' + hk(q)``: unit-mass HMC in
    y = Lam^-1 x.  The capped force depends on q alone, so every stage stays a shear and the chain still targets the
    posterior.  Accept, failure and NaN rules, ``n_leapfrog``, ``kick_cap`` and every other keyword are
    ``hmc_sample``'s.  With Lam = I and a scalar eps the result is ``hmc_sample``'s bit for bit.

    Two per-step outputs: ``accept_stat`` = min(1, exp(a)) with a = (lp(q^L) - lp(x)) + (K(r^0) - K(r^L)), 0 when a is
    NaN, and ``step_size`` = the eps the step used; entry t belongs to the step that wrote row t + 1.

    ``target_accept`` = delta in (0, 1) turns on the kernel's dual averaging of eps (Hoffman & Gelman; Stan's
    constants gamma 0.05, t0 10, kappa 0.75): after every step m += 1; eta = 1 / (m + 10); sbar = (1 - eta) sbar +
    eta (delta - alpha); ell = mu - sbar sqrt(m) / gamma; w = m ** -0.75; xbar = (1 - w) xbar + w ell; eps = exp(ell).
    ``adapt_state`` (chains, 5) = eps, m, sbar, xbar, mu is the state it starts from (default:
    ``hmc_adapt_restart(step_size)``, i.e. mu = log(10 eps)); the result's ``adapt_state`` is the state after the last
    step and, with ``return_adapt_trace``, ``adapt_trace`` the state after every launch.  The state lives in the
    chain's state record, so the result does not depend on ``steps_per_launch`` (default
    ``STEPS_PER_LAUNCH_HMC(n_leapfrog)``); a chain is bit-identical to itself under any launch split, any
    ``first_chain`` offset, with or without ``return_noise``, and when re-run from its recorded noise."""
    out = {}
    run = _hmc_metric_run('hmc_metric_sample', log_theta_init, n_samples, step_size, metric_chol, n_leapfrog, seed=seed,
                          noise=noise, kick_cap=kick_cap, data=data, rtol=rtol, atol=atol, max_steps=max_steps,
                          first_chain=first_chain, steps_per_launch=steps_per_launch, return_noise=return_noise,
                          device_out=device_out, delta=target_accept,
                          drive_with=_adapt_drive_with(out, n_samples, target_accept, adapt_state, return_adapt_trace))
    return _adapt_result(run, out, target_accept, device_out)


def hmc_warmup(log_theta_init, n_warmup, step_size, n_leapfrog, *, target_accept: float = 0.8, metric_chol=None,
               seed=None, noise=None, kick_cap: float = math.inf, data: Optional[LvData] = None, rtol: float = RTOL,
               atol: float = ATOL, max_steps: int = MAX_STEPS, first_chain: int = 0,
               steps_per_launch: Optional[int] = None, device_out: bool = False) -> HmcAdaptation:
    """Warm-up for ``hmc_metric_sample``: ``n_warmup`` HMC steps per chain during which the step size is tuned to the
    acceptance ``target_accept`` by dual averaging inside the kernel and a dense metric is learned from the draws in
    windows.  It follows Stan's warm-up -- Hoffman & Gelman's dual averaging, Stan's windows and its regularisation of
    the covariance -- but these are this project's own definitions and Stan's bits are not claimed; jittered
    trajectory lengths and Stan's search for a first step size are out of scope.  ``nuts_warmup`` is the same
    warm-up with the trajectory length chosen by the no-U-turn rule, for ``nuts_sample``.

    Schedule (``hmc_warmup_windows``): 75 steps that adapt eps only, slow windows of 25, 50, 100, ... steps (the last
    stretched to the end of the slow region), 50 final steps that adapt eps only; 15 % / 10 % / one window where
    these do not fit; ``n_warmup`` < 20 raises ValueError.  The chains start from ``step_size`` (a scalar or
    (chains,)) and ``metric_chol`` (default: the identity) with mu = log(10 eps), m = sbar = xbar = 0.  At each slow
    window's end, per chain: S = the sample covariance of the window's rows (n - 1 divisor), Sigma = n / (n + 5) S +
    1e-3 * 5 / (n + 5) I, Lam_new = chol(Sigma) (torch on the device, batched over the chains), eps = exp(xbar) *
    (det Lam_old / det Lam_new) ** (1 / 4) -- the project's own rule, which keeps the mean physical step across the
    change of coordinates -- and dual averaging restarts with mu = log(10 eps), m = sbar = xbar = 0.  At the end
    eps = exp(xbar).  Launch boundaries fall on window ends; within a window the kernel adapts on its own for
    ``steps_per_launch`` (default ``STEPS_PER_LAUNCH_HMC(n_leapfrog)``) steps per launch, and the result does not depend
    on that number.

    Returns ``HmcAdaptation``: ``step_size`` (chains,), ``metric_chol`` (chains, 4, 4) and ``last_row`` (chains, 4) to
    go on with -- ``hmc_metric_sample(a.last_row, n, a.step_size, a.metric_chol, n_leapfrog, seed=another_seed)`` --
    then every warm-up row with ``log_p`` and ``grad`` (row 0 is the start), ``accept_stat`` and ``step_sizes``
    (chains, n_warmup), the list ``windows`` of ``HmcWindow`` and the counts.  The noise of warm-up step t is
    ``hmc_sample``'s for (seed, chain, t): sample with another seed.  A START that cannot be evaluated raises
    ValueError."""
    hmc_warmup_windows(n_warmup)                    # (its check of n_warmup, before anything runs)
    out = {}
    lam0 = np.eye(4) if metric_chol is None else metric_chol
    run = _hmc_metric_run('hmc_warmup', log_theta_init, int(n_warmup) + 1, step_size, lam0, n_leapfrog, seed=seed,
                          noise=noise, kick_cap=kick_cap, data=data, rtol=rtol, atol=atol, max_steps=max_steps,
                          first_chain=first_chain, steps_per_launch=steps_per_launch, return_noise=False,
                          device_out=device_out, delta=target_accept,
                          drive_with=_warmup_drive_with(out, 'hmc_warmup', n_warmup))
    return _warmup_result(run, out, device_out)


def nuts_sample(log_theta_init, n_samples, step_size, metric_chol=None, *, max_depth: int = NUTS_MAX_DEPTH, seed=None,
                kick_cap: float = math.inf, target_accept: Optional[float] = None, adapt_state=None,
                return_adapt_trace: bool = False, data: Optional[LvData] = None, rtol: float = RTOL,
                atol: float = ATOL, max_steps: int = MAX_STEPS, first_chain: int = 0,
                steps_per_launch: Optional[int] = None, return_noise: bool = False,
                device_out: bool = False) -> NutsSample:
    """No-U-turn sampler (NUTS) chains on the LV log posterior, one chain per GPU wave (``st_lv_nuts_wave``,
    csrc/lv_mcmc.hip): ``hmc_metric_sample`` with the trajectory length chosen per step, the counterpart of the Stan
    stage of the reference's ``Sampling.ipynb``.  It follows Hoffman & Gelman's NUTS in Betancourt's multinomial form,
    built iteratively with checkpoints; it is the project's own definition, Stan's bits and its
    further cross-sub-tree U-turn checks are not claimed.

    ``step_size`` (a scalar or (chains,)), ``metric_chol`` (default: the identity), ``kick_cap``, the stage, and
    ``target_accept`` / ``adapt_state`` / ``return_adapt_trace`` are ``hmc_metric_sample``'s; a stage in direction
    v = -1 is the stage with -eps.  One step from the row (x, lp, g) with momentum z (``hmc_sample``'s z for the same
    seed, chain and step): for j = 0 .. max_depth - 1 a direction v is drawn and 2^j stages extend the trajectory from
    its end on side v.  Leaf n = (q, r) has a_n = (lp(q) - lp) + (K(z) - K(r)) and weight exp(a_n); a NaN a_n (a stage
    without a density) or a_n < -1000 makes the step *divergent*: the sub-tree is dropped and the step ends.  Inside
    the sub-tree leaf n > 0 replaces the sub-tree's proposal when log u < a_n - W' (W' the log of the weights so
    far); every aligned block of 2^k leaves is tested for a U-turn -- NOT (rho . r_first > 0 AND rho . r_last > 0),
    rho the block's momentum sum -- and a turn drops the sub-tree and ends the step.  A complete sub-tree's proposal
    replaces the tree's when log u_T < W' - W; the step ends when the whole tree turns or after ``max_depth``
    (1 .. 10) doublings.  The next row is the proposal.  Each stage is a volume-preserving map whose inverse is the
    stage with -eps, also under the cap, so a trajectory is an orbit and the selection with the true H keeps the
    target.

    Noise is the device's Philox only (``seed`` is required, ``noise=`` is not accepted): stage l = 1, 2, ... of step
    t draws ``np.random.Philox(key=[seed, chain], counter=[t - 1, l, 0, 0]).random_raw(4)``.  ``return_noise`` returns
    z; ``log_u`` stays None.

    Returns ``NutsSample``: ``accept_stat`` is the mean of min(1, exp(a_n)) over the step's stages (what dual
    averaging is fed), ``tree_depth`` the doublings started, ``n_leapfrog`` the stages done, ``divergent`` the flag;
    ``accepted`` counts the steps whose row was replaced, ``n_failed`` the divergent steps.  ``steps_per_launch``
    (default ``STEPS_PER_LAUNCH_NUTS(max_depth)``) splits the run into launches; a chain is bit-identical to itself
    under any launch split, any ``first_chain`` offset and with or without ``return_noise``."""
    out = {}
    run = _hmc_metric_run('nuts_sample', log_theta_init, n_samples, step_size,
                          np.eye(4) if metric_chol is None else metric_chol, None, seed=seed, noise=None,
                          kick_cap=kick_cap, data=data, rtol=rtol, atol=atol, max_steps=max_steps,
                          first_chain=first_chain, steps_per_launch=steps_per_launch, return_noise=return_noise,
                          device_out=device_out, delta=target_accept, max_depth=max_depth, nuts=True,
                          drive_with=_adapt_drive_with(out, n_samples, target_accept, adapt_state, return_adapt_trace))
    return _adapt_result(run, out, target_accept, device_out)


def nuts_warmup(log_theta_init, n_warmup, step_size, *, max_depth: int = NUTS_MAX_DEPTH, target_accept: float = 0.8,
                metric_chol=None, seed=None, kick_cap: float = math.inf, data: Optional[LvData] = None,
                rtol: float = RTOL, atol: float = ATOL, max_steps: int = MAX_STEPS, first_chain: int = 0,
                steps_per_launch: Optional[int] = None, device_out: bool = False) -> HmcAdaptation:
    """Warm-up for ``nuts_sample``: ``hmc_warmup``'s schedule (``hmc_warmup_schedule``: dual averaging of the step
    size inside the kernel, the metric learned in windows) with NUTS steps of at most ``max_depth`` doublings, fed
    with the tree's ``accept_stat``.  Returns ``HmcAdaptation``; go on with
    ``nuts_sample(a.last_row, n, a.step_size, a.metric_chol, seed=another_seed)``."""
    hmc_warmup_windows(n_warmup)                    # (its check of n_warmup, before anything runs)
    out = {}
    run = _hmc_metric_run('nuts_warmup', log_theta_init, int(n_warmup) + 1, step_size,
                          np.eye(4) if metric_chol is None else metric_chol, None, seed=seed, noise=None,
                          kick_cap=kick_cap, data=data, rtol=rtol, atol=atol, max_steps=max_steps,
                          first_chain=first_chain, steps_per_launch=steps_per_launch, return_noise=False,
                          device_out=device_out, delta=target_accept, max_depth=max_depth, nuts=True,
                          drive_with=_warmup_drive_with(out, 'nuts_warmup', n_warmup))
    return _warmup_result(run, out, device_out)
