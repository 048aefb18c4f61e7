"""Near-tie guard, every row class of every guarded plan (csrc/persistent_kernel.hpp rescan_regs /
rescan_rest): constructed pairs (tests/planted_ref.py planted: near-tie twins, bitwise copies, repeats of the
predecessor row, an exact tie between different rows) are placed in register, LDS and streamed rows of a block
of the 512-thread kernels -- at the edges of the LDS repeat-bit words, at the first and past the 32nd streamed
visit, across class and block boundaries, in another block than the winner -- and the kernel's indices, first
flagged step and final guard state must equal the bit model's (oracle/stein_ref.c sr_greedy_mt_ties) bit for
bit, the drop-in thin NumPy's indices.  The grid is capped (st_tune key 5) so that 24 000 .. 98 000 rows reach
the plans a 2e6-row thin takes; each case reads the plan the library made (_native.last_plan) and computes
the positions from it, so a pair is where the test says it is.  tests/test_near_tie_cpu.py proves the
constructions through the models alone."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import stein_ref_c as oc
from tests import planted_ref as pl
from tests.test_near_tie_cpu import model_thresholds

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no HIP device', allow_module_level=True)

import stein_thinning  # noqa: E402
from stein_thinning import _native as nat  # noqa: E402
from stein_thinning import thinning as st  # noqa: E402
from tests.test_gpu_near_tie import _compact_run  # noqa: E402


@contextlib.contextmanager
def _tuned(key5, key15):
    L = nat.lib()
    prev = [(k, int(L.st_tune_get(k))) for k in (5, 15)]
    try:
        nat.check(L.st_tune(5, key5), 'st_tune 5')
        nat.check(L.st_tune(15, key15), 'st_tune 15')
        yield
    finally:
        for k, v in prev:
            L.st_tune(k, v)


@functools.lru_cache(maxsize=4)
def _base_problem(n, d, mirror, gf):
    """The device problem of the base sample of n rows (what the pairs are planted into)."""
    if mirror:
        X = np.random.default_rng(pl.OTHER_SEED).normal(size=(n, 2)) + 2.0
        return st._make_stein_integrand(X, -X, standardize=False).device_problem()
    X, G, _ = pl.planted_base(d, n, pl.OTHER_SEED)
    if gf:   # a weight per row: fewer LDS rows fit
        return st._make_stein_gf_integrand(X, *pl.planted_log_densities(X), G).device_problem()
    return st._make_stein_integrand(X, G).device_problem()


def _layout(plan, d, key15, mirror=False, gf=False):
    """One guarded step on the base sample under the current knobs: (the plan the library made, its row-class
    boundaries).  The plan must be the intended one: the GUARD kernels, the compact-only kernel first with the
    expected register rows and stream_a_lds, and the LDS rows the constructions were proved at."""
    p = pl.PLANS[plan]
    _, step, _ = _compact_run(_base_problem(p['n'], d, mirror, gf), 1)
    lp = nat.last_plan()
    assert step == -1
    assert (lp.blocks, lp.rows_per_block, lp.guarded, lp.compact_first, lp.threads, lp.reg_rows) == \
        (p['key5'], p['R'], 1, 1, 512, p['rt']), lp
    assert lp.stream_a_lds == (p['sal'] if key15 == -1 else 0), lp
    assert lp.lds_rows == (pl.GF_LDS_ROWS if gf else p['RL'][d, key15]), lp
    layout = pl.block_layout(lp.rows_per_block, lp.reg_rows, lp.lds_rows, lp.threads)
    assert 0 < layout[0] < layout[1] < layout[2]   # no class is empty
    return lp, layout


def _state(case):
    it = case.integrand
    thr_all, Q, E = model_thresholds(it.gradient, it.weights, it.linv_scale, it.linv_trace, case.idx, case.wv)
    return list(oc.tie_bounds(it.gradient, it.weights)) + [Q, E, thr_all[-1]]


def _check(case, lp, layout, classes, blocks):
    """Every assertion of one case under the current knobs (bitwise throughout)."""
    case.check_preconditions()
    got_classes = (pl.row_class(layout, case.winner_at), pl.row_class(layout, case.other_at))
    assert (got_classes[0][1], got_classes[1][1]) == classes and (got_classes[0][0], got_classes[1][0]) == blocks
    integrand = case.make_integrand()
    prob = integrand.device_problem()
    idx, step, state = _compact_run(prob, case.m)
    assert nat.last_plan() == lp   # the planted sample took the plan the positions were computed from
    np.testing.assert_array_equal(idx, case.idx)
    assert step == case.first
    np.testing.assert_array_equal(state, _state(case))
    np.testing.assert_array_equal(st._greedy_search(case.m, integrand), case.want)
    assert prob.dedup_used is False          # the raw rows ran, not their run starts
    assert prob.near_tie == case.first       # -1: guarded and no exact re-run; else the flagged step
    if case.gf:
        got = stein_thinning.thin_gf(case.x, case.log_p, case.log_q, case.g, case.m)
    else:
        got = stein_thinning.thin(case.x, case.g, case.m, **case.kw)
    np.testing.assert_array_equal(got, case.want)
    if case.kind == 'repeat':
        # dedup='always' keeps the raw rows here (one repeat is far below the share of repeats dedup_view asks
        # for), so the run starts are thinned through the view itself, as greedy() does when it has one: the
        # planted repeat is the one row dropped, the indices map back to NumPy's, nothing is flagged
        np.testing.assert_array_equal(prob.greedy(case.m, dedup='always', guard=True), case.want)
        assert prob.dedup_used is False and prob.near_tie == -1
        view = prob.dedup_view(any_repeat=True)
        assert view is not None and view.n_unique == case.n - 1
        kept = view.rows_host
        assert case.other_at not in kept and kept[case.winner_at] == case.winner_at
        out, _ = view.problem._greedy_run(case.m, prob.guard_mode(True))
        assert view.problem.near_tie == -1 and view.problem.fallback is None
        np.testing.assert_array_equal(view.to_rows(out), case.want)
    if case.kind in ('twin', 'mirror'):
        assert case.first == case.step
    elif not case.gf:
        assert case.first == -1


def _blocks(kind, position):
    if kind == 'repeat':
        return (0, 1) if position == 'block_to_block' else (1, 1)
    return (1, 2) if position.startswith('xblock') else (1, 1)


@pytest.mark.parametrize('d,position', pl.large_twin_cases())
def test_twin_every_position_large_plan(d, position):
    """The plan of every 2e6-row guarded thin (compact-only kernel, 8 register rows, LDS rows, streamed rows
    with their sums in LDS or -- st_tune key 15 = 0 -- in HBM): a twin at every position flags exactly at step 8."""
    for key15 in (-1, 0):
        with _tuned(pl.PLANS['large']['key5'], key15):
            lp, layout = _layout('large', d, key15)
            case = pl.planted_case('large', 'twin', d, position, layout)
            _check(case, lp, layout, pl.CLASSES[position], _blocks('twin', position))


@pytest.mark.parametrize('plan,kind,d,position', pl.reduced_cases())
def test_every_kind_every_plan(plan, kind, d, position):
    """Copies, repeats and the exact tie between different rows on the large plan; every kind on the mid-size
    plan (4 register rows), on the long-stream plan (streamed visits past the 32 of a thread's bit mask) and on
    the plan whose streamed sums no longer fit in LDS (read from HBM although st_tune key 15 = -1)."""
    with _tuned(pl.PLANS[plan]['key5'], -1):
        lp, layout = _layout(plan, d, -1, kind == 'mirror')
        case = pl.planted_case(plan, kind, d, position, layout)
        if plan in ('long', 'hbm') and position == 'block_last':
            assert case.other_at % layout[2] - layout[1] >= 32 * 448
        _check(case, lp, layout, (pl.REPEAT_CLASSES if kind == 'repeat' else pl.CLASSES)[position],
               _blocks(kind, position))


@pytest.mark.parametrize('position', pl.MIRROR_REPEATS)
def test_exact_tie_among_repeats_large_plan(position):
    """The exact tie between different rows while every other LDS row of the block repeats its predecessor: all
    repeat bits around the other row's are set, so one filed under a wrong word or bit would hide the tie."""
    with _tuned(pl.PLANS['large']['key5'], -1):
        lp, layout = _layout('large', 2, -1, True)
        case = pl.mirror_repeats_case(position, layout)
        _check(case, lp, layout, pl.CLASSES[position], (1, 1))


@pytest.mark.parametrize('kind,position,seed,weight_ulp', pl.GF_CASES)
def test_gradient_free_large_plan(kind, position, seed, weight_ulp):
    """The gradient-free operator on the large plan: the weights enter the bound and the duplicate test -- a
    twin in an LDS and in a streamed row, a bitwise copy, and a copy whose weight differs by one ulp (not a
    duplicate: the model decides whether it flags)."""
    with _tuned(pl.PLANS['large']['key5'], -1):
        lp, layout = _layout('large', 2, -1, gf=True)
        case = pl.planted_gf_case(kind, position, seed, weight_ulp, layout)
        w = case.integrand.weights
        if kind == 'copy':
            assert (w[case.winner_at] != w[case.other_at]) == weight_ulp
        _check(case, lp, layout, pl.CLASSES[position], _blocks(kind, position))
