"""The no-U-turn sampler on the GPU (csrc/lv_mcmc.hip: lv_nuts_wave_kernel; lotka_volterra.nuts_sample, nuts_warmup;
DESIGN.md section 22) against its host restatement (tests/nuts_ref.py) rebuilt from one-stage calls of the existing
kernel (hmc_metric_sample with L = 1, momentum v r and log_u = -inf), and against itself.

What is compared how.  The restatement's stage is a device call, so q', lp(q'), g(q') are the device's bits; r' and a_n
are formed on the host from the same values by the same IEEE operations in the same order, so they are the kernel's
bits too.  Only exp and log1p differ between host and device, by ulps; they enter (1) the selection decisions, through
W' and W -- a decision can flip only if its margin |log u - (a_n - W')| or |log u_T - (W' - W)| is within rounding, so
the test ASSERTS every margin > 1e-9 (W is O(1..10) here and ulps of it are ~1e-15; a condition on the inputs: a seed
that fails it is replaced, the figure is never loosened) -- and (2) accept_stat.  Everything else -- the new row,
log_p, grad, tree_depth, n_leapfrog, divergent, accepted, n_failed -- is compared bit for bit.

accept_stat bound, u = 2^-52: alpha_n = min(1, exp(a_n)) with the same a_n on both sides and exp within 1 ulp on
either side: |d alpha_n| <= 2 u alpha_n.  The sum of n non-negative terms in order rounds n - 1 times on either side,
each by at most u times a partial sum <= the sum: 2 (n - 1) u sum.  The division rounds once on either side: 2 u.
Together |d accept_stat| <= (2 n + 2) u accept_stat (+ 1e-300 for terms in exp's subnormal range)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

from stein_thinning import lotka_volterra as lv  # noqa: E402
from tests import hmc_adapt_ref as A  # noqa: E402
from tests import hmc_ref as R  # noqa: E402
from tests import nuts_ref as N  # noqa: E402

U = 2.0 ** -52
SEED = 20261021
T_NS = [1, 2, 63, 65, 130]
CAP = 0.2
DELTA = 0.8
MARGIN = 1e-9
ROWS = ('samples', 'log_p', 'grad', 'accepted', 'n_failed', 'accept_stat', 'step_size', 'tree_depth', 'n_leapfrog',
        'divergent')
# tests/test_gpu_lv_hmc_metric.py's dense factor and per-chain step sizes; the last chain's is far too large for the
# ~0.02-wide posterior of the first 130 observations: its steps diverge
LAM = np.array([[1.0, 0.0, 0.0, 0.0],
                [0.3, 0.9, 0.0, 0.0],
                [-0.2, 0.25, 1.1, 0.0],
                [0.15, -0.35, 0.2, 0.8]])
EPS5 = np.array([0.012, 0.014, 0.016, 0.018, 0.5])


def _eps(n):
    return 0.012 + 0.002 * np.arange(n)


@functools.lru_cache(maxsize=None)
def _data(t_n=130):
    d = lv.reference_data()
    return lv.LvData(t=d.t[:t_n], y=d.y[:t_n], cov=d.cov, t_span=d.t_span, u_init=d.u_init)


def _starts(n):
    rng = np.random.default_rng(42)
    return np.log(lv.THETA) + 0.02 * rng.normal(size=(n, 4))


def _same(a, b, names=ROWS, rows=slice(None)):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name)[rows], err_msg=name)


def _stages(q, g, r, v, eps, cap, max_steps):
    """One stage in direction v for a batch, from the existing kernel: (q', lp', g', r'); NaN where it has no density."""
    n = q.shape[0]
    lam, c = np.tile(LAM, (n, 1, 1)), np.full(4, cap)
    rv = v[:, None] * r
    kw = {} if max_steps is None else dict(max_steps=max_steps)
    one = lv.hmc_metric_sample(q, 2, eps, lam, 1, noise=(rv[:, None, :], np.full((n, 1), -np.inf)), kick_cap=cap,
                               data=_data(), **kw)
    np.testing.assert_array_equal(one.samples[:, 0], q)
    np.testing.assert_array_equal(one.grad[:, 0], g)
    bad = one.accepted != 1
    with np.errstate(invalid='ignore'):
        r2 = v[:, None] * ((rv + A.half_kick(g, eps, lam, c)) + A.half_kick(one.grad[:, 1], eps, lam, c))
    q2, lp2, g2 = one.samples[:, 1].copy(), one.log_p[:, 1].copy(), one.grad[:, 1].copy()
    lp2[bad], g2[bad], r2[bad] = np.nan, np.nan, np.nan
    return q2, lp2, g2, r2


@functools.lru_cache(maxsize=None)
def _rebuilt(max_depth, cap, failing=False):
    """A 5-chain, 13-row device run and the restatement of each of its 60 steps, driven in lock-step per stage ordinal
    (a finished step repeats its last request).  Computed once; the tests below share it and leave it unchanged."""
    if failing:         # tests/hmc_ref.failing_input()'s scheme: integrations run out of steps away from log(THETA)
        x0, eps5, max_steps = np.tile(np.log(lv.THETA), (5, 1)), np.full(5, R.FAIL_EPS), R.failing_max_steps()
    else:
        x0, eps5, max_steps = R.fixed_input()[0], EPS5, None
    kw = {} if max_steps is None else dict(max_steps=max_steps)
    run = lv.nuts_sample(x0, 13, eps5, LAM, max_depth=max_depth, seed=SEED, kick_cap=cap, data=_data(),
                         return_noise=True, **kw)
    C, S = 5, 12
    eps = np.repeat(eps5, S)
    x, g, lp = (getattr(run, name)[:, :-1].reshape(C * S, -1) for name in ('samples', 'grad', 'log_p'))
    z = run.z.reshape(C * S, 4)
    gens = [N.step_gen(x[i], lp[i, 0], g[i], z[i], eps[i], max_depth, N.tree_draws(SEED, i // S, i % S + 1))
            for i in range(C * S)]
    req = [next(gen) for gen in gens]
    done = [None] * (C * S)
    calls = 0
    while any(d is None for d in done):
        q, gq, r = (np.stack([rq[k] for rq in req]) for k in range(3))
        v = np.array([float(rq[3]) for rq in req])
        q2, lp2, g2, r2 = _stages(q, gq, r, v, eps, cap, max_steps)
        calls += 1
        for i, gen in enumerate(gens):
            if done[i] is None:
                try:
                    req[i] = gen.send((q2[i], lp2[i], g2[i], r2[i]))
                except StopIteration as stop:
                    done[i] = stop.value
    return run, done, calls


def _reasons(steps):
    out = {}
    for s in steps:
        key = s.reason + ('-nan' if s.nan else '') + ('-smaller' if s.reason == 'inner' and s.block < s.subtree else '')
        out[key] = out.get(key, 0) + 1
    return out


@pytest.mark.parametrize('cap', [CAP, np.inf])
@pytest.mark.parametrize('max_depth', [1, 3, 5])
def test_every_step_is_the_restatements(max_depth, cap):
    run, steps, calls = _rebuilt(max_depth, cap)
    C, S = 5, 12
    for name, want in (('samples', np.stack([s.x for s in steps])), ('log_p', np.array([s.lp for s in steps])[:, None]),
                       ('grad', np.stack([s.g for s in steps]))):
        np.testing.assert_array_equal(getattr(run, name)[:, 1:].reshape(C * S, -1), want, err_msg=name)
    for name in ('tree_depth', 'n_leapfrog', 'divergent'):
        np.testing.assert_array_equal(getattr(run, name).reshape(C * S), [getattr(s, name) for s in steps], err_msg=name)
    assert run.tree_depth.dtype == run.n_leapfrog.dtype == np.int32 and run.divergent.dtype == np.bool_
    np.testing.assert_array_equal(run.accepted, np.array([s.replaced for s in steps]).reshape(C, S).sum(axis=1))
    np.testing.assert_array_equal(run.n_failed, np.array([s.divergent for s in steps]).reshape(C, S).sum(axis=1))
    np.testing.assert_array_equal(run.step_size, np.repeat(EPS5[:, None], S, axis=1))
    assert run.log_u is None
    want = np.array([s.accept_stat for s in steps])
    n = np.array([s.n_leapfrog for s in steps])
    bound = (2 * n + 2) * U * want + 1e-300
    ratio = np.abs(run.accept_stat.reshape(C * S) - want) / bound
    margins = [m for s in steps for m in s.margins]
    print('max_depth', max_depth, 'cap', cap, 'device calls', calls, 'stages', int(n.sum()), 'reasons', _reasons(steps),
          'accepted', run.accepted.tolist(), 'n_failed', run.n_failed.tolist(), 'accept_stat: worst error / bound',
          ratio.max(), 'range', want.min(), '..', want.max(), 'smallest decision margin', min(margins),
          'of', len(margins))
    assert n.max() <= 2 ** max_depth - 1 and calls <= 2 ** max_depth - 1
    assert min(margins) > MARGIN
    assert ratio.max() <= 1.0
    assert run.accepted.sum() > 0


def test_a_stage_without_a_density_ends_the_step_as_divergent():
    run, steps, calls = _rebuilt(3, R.FAIL_CAP, failing=True)
    nan = np.array([s.nan for s in steps]).reshape(5, 12)
    print('failing input: device calls', calls, 'reasons', _reasons(steps), 'n_failed', run.n_failed.tolist())
    assert nan.any()
    np.testing.assert_array_equal(run.divergent, np.array([s.divergent for s in steps]).reshape(5, 12))
    np.testing.assert_array_equal(run.n_leapfrog, np.array([s.n_leapfrog for s in steps]).reshape(5, 12))
    np.testing.assert_array_equal(run.samples[:, 1:].reshape(60, 4), np.stack([s.x for s in steps]))
    np.testing.assert_array_equal(run.n_failed, run.divergent.sum(axis=1))
    assert np.all(run.divergent[nan]) and np.all(np.isfinite(run.log_p)) and np.all(np.isfinite(run.grad))
    margins = [m for s in steps for m in s.margins]
    assert not margins or min(margins) > MARGIN


def test_the_coverage_claimed_is_there():
    """From the restatement's reason codes over the runs above: every way a step can end, and both directions."""
    steps = [s for d in (1, 3, 5) for cap in (CAP, np.inf) for s in _rebuilt(d, cap)[1]]
    reasons = _reasons(steps)
    failing = _reasons(_rebuilt(3, R.FAIL_CAP, failing=True)[1])
    print('reasons', reasons, 'failing input', failing)
    assert reasons.get('inner-smaller', 0) > 0          # an inner U-turn of a block smaller than its sub-tree
    assert reasons.get('whole', 0) > 0
    assert reasons.get('max_depth', 0) > 0
    assert reasons.get('divergent', 0) > 0              # a < -1000 with a density: the chain with eps = 0.5
    assert failing.get('divergent-nan', 0) > 0          # a stage without a density
    assert {v for s in steps for v in s.directions} == {1, -1}
    assert any(len(set(s.directions)) == 2 for s in steps)


def test_dual_averaging_transitions_are_numpys_within_the_bound():
    """tests/test_gpu_lv_hmc_metric.py's test for this kernel: steps_per_launch = 1, every transition from the device's
    state with the device's accept_stat against tests/hmc_adapt_ref.da_update within DESIGN.md section 21's bounds."""
    x0, eps = _starts(5), _eps(5)
    run = lv.nuts_sample(x0, 13, eps, LAM, max_depth=3, seed=SEED, kick_cap=CAP, data=_data(), target_accept=DELTA,
                         steps_per_launch=1, return_adapt_trace=True)
    assert run.adapt_trace.shape == (12, 5, 5)
    states = np.concatenate([lv.hmc_adapt_restart(eps)[None], run.adapt_trace])
    np.testing.assert_array_equal(run.adapt_state, states[-1])
    worst = np.zeros(2)
    for t in range(12):
        prev, nxt, alpha = states[t], states[t + 1], run.accept_stat[:, t]
        np.testing.assert_array_equal(run.step_size[:, t], prev[:, 0])
        want = A.da_update(prev, alpha, DELTA)
        m, sbar, mu = want[:, 1], want[:, 2], want[:, 4]
        np.testing.assert_array_equal(nxt[:, 1], m)
        np.testing.assert_array_equal(nxt[:, 1], t + 1.0)
        np.testing.assert_array_equal(nxt[:, 2], sbar)
        np.testing.assert_array_equal(nxt[:, 4], mu)
        tt = (sbar * np.sqrt(m)) / A.GAMMA
        ell = mu - tt
        e_ell = 3 * U * np.abs(tt) + U * np.abs(ell)
        w = A.elementwise(math.pow, m, -A.KAPPA)
        e_x = (2 * U * w + 2 * U) * np.abs(prev[:, 3]) + 3 * U * np.abs(w * ell) + w * e_ell + U * np.abs(want[:, 3])
        e_eps = want[:, 0] * (3 * U + e_ell)
        worst = np.maximum(worst, [(np.abs(nxt[:, 3] - want[:, 3]) / e_x).max(),
                                   (np.abs(nxt[:, 0] - want[:, 0]) / e_eps).max()])
    print('dual averaging: worst error / bound: xbar', worst[0], 'eps', worst[1], 'eps range', states[:, :, 0].min(),
          '..', states[:, :, 0].max(), 'stages', run.n_leapfrog.sum(axis=1).tolist())
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert np.unique(states[1:, :, 0]).size > 12             # eps moves


@pytest.mark.parametrize('t_n', T_NS)
def test_launch_geometry_does_not_matter_while_adapting(t_n):
    sub = _data(t_n)
    x0, eps = _starts(9), _eps(9)                    # 9 chains: two full blocks of 4 waves and one wave
    names = ROWS + ('z', 'adapt_state')
    kw = dict(max_depth=3, seed=SEED, kick_cap=CAP, data=sub, target_accept=DELTA)
    assert lv.STEPS_PER_LAUNCH_NUTS(3) == 9
    r = lv.nuts_sample(x0, 13, eps, LAM, return_noise=True, **kw)
    assert np.all(np.isfinite(r.log_p)) and np.all(np.isfinite(r.grad))
    assert r.accepted.sum() > 0 and np.all(r.adapt_state[:, 1] == 12.0)
    assert np.all((r.n_leapfrog >= 1) & (r.n_leapfrog <= 7)) and np.all((r.tree_depth >= 1) & (r.tree_depth <= 3))
    for spl in (1, 5):                               # 12 steps: 12 launches; 5 + 5 + 2 (the default: 9 + 3)
        _same(lv.nuts_sample(x0, 13, eps, LAM, return_noise=True, steps_per_launch=spl, **kw), r, names)
    _same(lv.nuts_sample(x0[4:], 13, eps[4:], LAM, return_noise=True, first_chain=4, **kw), r, names, slice(4, None))
    _same(lv.nuts_sample(x0, 13, eps, LAM, **kw), r, ROWS + ('adapt_state',))      # records nothing
    for n in (1, 4, 5):                              # one wave of four, a full block, a full block and one wave
        _same(lv.nuts_sample(x0[:n], 13, eps[:n], LAM, return_noise=True, **kw), r, names, slice(0, n))
    if t_n == 130:                                   # the momenta are hmc_sample's for the same (seed, chain, step)
        h = lv.hmc_sample(x0, 13, 0.001, 1, seed=SEED, kick_cap=CAP, data=sub, return_noise=True)
        np.testing.assert_array_equal(r.z, h.z)


def test_warmup_does_not_depend_on_the_launch_split():
    x0 = _starts(5)
    kw = dict(max_depth=4, seed=SEED, kick_cap=0.5, data=_data())
    ad = lv.nuts_warmup(x0, 40, 0.01, **kw)
    assert [(w.start, w.stop) for w in ad.windows] == [(6, 36)]
    assert ad.samples.shape == (5, 41, 4) and ad.step_sizes.shape == ad.accept_stat.shape == (5, 40)
    np.testing.assert_array_equal(ad.step_sizes[:, 0], 0.01)
    np.testing.assert_array_equal(ad.step_sizes[:, 36], ad.windows[0].step_size)
    np.testing.assert_array_equal(ad.last_row, ad.samples[:, -1])
    np.testing.assert_array_equal(ad.metric_chol, ad.windows[0].metric_chol)
    assert np.all(np.isfinite(ad.step_size)) and np.all(ad.step_size > 0)
    again = lv.nuts_warmup(x0, 40, 0.01, steps_per_launch=7, **kw)
    for name in ('step_size', 'metric_chol', 'samples', 'log_p', 'grad', 'accept_stat', 'step_sizes', 'accepted',
                 'n_failed'):
        np.testing.assert_array_equal(getattr(again, name), getattr(ad, name), err_msg=name)
    run = lv.nuts_sample(ad.last_row, 5, ad.step_size, ad.metric_chol, max_depth=4, seed=SEED + 1, kick_cap=0.5,
                         data=_data())
    np.testing.assert_array_equal(run.samples[:, 0], ad.last_row)
    np.testing.assert_array_equal(run.log_p[:, 0], ad.log_p[:, -1])
    print('nuts_warmup: final eps', ad.step_size.tolist(), 'mean accept_stat', ad.accept_stat.mean(axis=1).tolist(),
          'n_failed', ad.n_failed.tolist())


def test_bad_input_and_one_row():
    sub = _data(63)
    with pytest.raises(ValueError, match='starting point'):
        lv.nuts_sample(np.array([800.0, 0.0, 0.0, 0.0]), 3, 0.003, seed=1, data=sub)
    with pytest.raises(ValueError, match='starting point'):
        lv.nuts_warmup(np.array([800.0, 0.0, 0.0, 0.0]), 20, 0.003, seed=1, data=sub)
    with pytest.raises(ValueError, match='adapt_state'):
        lv.nuts_sample(np.log(lv.THETA), 3, 0.003, seed=1, data=sub, adapt_state=np.zeros((1, 5)))
    one = lv.nuts_sample(np.log(lv.THETA), 1, 0.003, max_depth=2, seed=1, data=sub, target_accept=DELTA,
                         return_adapt_trace=True, return_noise=True)
    assert one.samples.shape == (1, 1, 4) and one.accept_stat.shape == one.tree_depth.shape == (1, 0)
    assert one.n_leapfrog.shape == one.divergent.shape == (1, 0) and one.z.shape == (1, 0, 4)
    np.testing.assert_array_equal(one.adapt_state, lv.hmc_adapt_restart([0.003]))
    assert one.adapt_trace.shape == (0, 1, 5) and one.accepted.tolist() == [0] and one.n_failed.tolist() == [0]
    dev = lv.nuts_sample(np.log(lv.THETA), 4, 0.003, max_depth=2, seed=1, data=sub, device_out=True)
    assert dev.tree_depth.dtype == torch.int32 and dev.divergent.dtype == torch.bool and dev.samples.is_cuda
