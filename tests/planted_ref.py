"""Near-tie pairs planted at chosen absolute rows (test infrastructure): planted / PlantedCase put one
constructed pair -- a near-tie twin, a bitwise copy, a repeat of the predecessor row, an exact tie between
different rows -- where a test wants it, so that it falls in a chosen row class (register, LDS, streamed) of a
chosen block of the persistent kernel's guarded plans.  Below them the registry the CPU tests
(tests/test_near_tie_cpu.py) and the GPU tests (tests/test_gpu_near_tie_plans.py, tests/test_gpu_multiprocess.py)
share: the plans and their nominal layouts (PLANS), the positions (pair_positions, repeat_positions, CLASSES),
the fixed seeds (TWIN_SEEDS) and the case lists."""
import functools

import numpy as np


MIRROR_ROW = (0.125, -0.25)   # planted('mirror'): this row and its negation tie exactly at step 0


def planted_base(d: int, n: int, seed: int):
    """The sample planted() plants into: n rows of a centred d-dimensional Gaussian with score -inv(cov) x
    (d = 2: near_tie_twins' covariance; other d: a random SPD one).  Returns (x, g, cov)."""
    rng = np.random.default_rng(seed)
    if d == 2:
        cov = np.array([[1, .8], [.8, 1]])
    else:
        a = rng.normal(size=(d, d))
        cov = a @ a.T / d + 0.5 * np.eye(d)
    x = rng.multivariate_normal(np.zeros(d), cov, size=n)
    return x, -np.linalg.solve(cov, x.T).T, cov


def planted_log_densities(x):
    """(log_p, log_q) of a d = 2 planted sample for thin_gf: the target's log density up to a constant and a
    proxy close enough that the weights' spread stays under the warning (the recipe of
    test_dropin_thin_gf_equals_numpy_on_near_ties); the score passed as gradient_q stays the target's."""
    cov = np.array([[1, .8], [.8, 1]])
    log_p = -0.5 * np.sum(x * np.linalg.solve(cov, x.T).T, axis=1)
    return log_p, 0.9 * log_p


def _model_pick(x, g, step, gf):
    """The row the bit model (compact arithmetic) selects at `step` on thin(x, g)'s integrand (gf: thin_gf's,
    with planted_log_densities)."""
    from oracle import stein_ref_c as oc
    from stein_thinning import thinning as st
    integrand = st._make_stein_gf_integrand(x, *planted_log_densities(x), g) if gf else st._make_stein_integrand(x, g)
    return int(oc.greedy_ties(integrand.sample, integrand.gradient, integrand.weights, integrand.linv_scale,
                              integrand.linv_trace, step + 1)[0][step])


def planted(kind: str, d: int, n: int, seed: int, winner_at: int, other_at: int = None, step: int = 8,
            nudge: int = 4, gf: bool = False, repeats=None):
    """(x, g) with one constructed pair of rows at chosen absolute positions (so that a test can put them in
    chosen row classes of chosen blocks of the persistent kernel), in planted_base(d, n, seed):
    'twin'   -- the row P the NumPy path selects at `step` goes to `winner_at` (swapped with the row there)
                and `other_at` is overwritten with P, x[:, 0] moved by `nudge` ulps, same score: a near-tie
                at `step`.  The bit model decides which of the pair is selected on the final arrays; if it
                is the row at `other_at`, the pair's positions are exchanged;
    'copy'   -- `other_at` is overwritten with P bit for bit (not adjacent to `winner_at`): an exact tie
                between duplicates at `step`, which must not flag;
    'repeat' -- P bit for bit at `winner_at` + 1 (`other_at` is implied): a row repeating its predecessor;
    'mirror' -- d = 2, for thin(x, -x, standardize=False): every row has |x|^2 > 0.5 but MIRROR_ROW at
                `winner_at` and its negation at `other_at`, which tie exactly at step 0 without being
                duplicates (test_exact_tie_between_different_rows_flags).
    gf (d = 2): P is the row thin_gf's NumPy path selects at `step`, with planted_log_densities.
    repeats = (lo, hi), 'mirror' only: every row of [lo + 1, hi) but the pair and the rows after them repeats
    its predecessor bit for bit, so every repeat bit around the other row is set and that row's alone is not:
    a repeat bit filed under a wrong word or bit index lands on it and the tie goes unseen.
    Nothing is promised: planting changes the sample, so the callers assert what the models say about the
    final arrays (tests/test_near_tie_cpu.py does for the layouts the GPU tests use)."""
    from oracle import stein_numpy as o
    if kind == 'mirror':
        assert d == 2 and other_at is not None and other_at != winner_at
        rng = np.random.default_rng(seed)
        x = rng.normal(size=(2 * n + 64, 2))
        x = x[np.sum(x * x, axis=1) > 0.5][:n].copy()
        assert x.shape[0] == n
        x[winner_at] = MIRROR_ROW
        x[other_at] = -x[winner_at]
        if repeats:
            for r in range(repeats[0] + 1, repeats[1]):
                if r not in (winner_at, winner_at + 1, other_at, other_at + 1):
                    x[r] = x[r - 1]
        return x, -x
    x, g, _ = planted_base(d, n, seed)
    if gf:
        assert d == 2
        pick = int(o.thin_gf(x, *planted_log_densities(x), g, step + 1)[step])
    else:
        pick = int(o.thin(x, g, step + 1)[step])
    for a in (x, g):
        a[[pick, winner_at]] = a[[winner_at, pick]]
    if kind == 'repeat':
        assert other_at in (None, winner_at + 1)
        other_at = winner_at + 1
    assert other_at is not None and other_at != winner_at and 0 <= other_at < n
    assert kind == 'repeat' or abs(other_at - winner_at) > 1
    x[other_at], g[other_at] = x[winner_at], g[winner_at]
    if kind == 'twin':
        for _ in range(nudge):
            x[other_at, 0] = np.nextafter(x[other_at, 0], np.inf)
        if _model_pick(x, g, step, gf) == other_at:   # the model selects the nudged row: exchange the pair
            for a in (x, g):
                a[[other_at, winner_at]] = a[[winner_at, other_at]]
    else:
        assert kind in ('copy', 'repeat'), kind
    return x, g


def block_layout(rows_per_block: int, reg_rows: int, lds_rows: int, threads: int = 512):
    """Row-class boundaries of one persistent-kernel block, as offsets from the block's first row:
    (end of the register rows = start of the LDS rows, end of the LDS rows = start of the streamed rows,
    rows per block)."""
    reg = min(reg_rows * threads, rows_per_block)
    return reg, min(reg + lds_rows, rows_per_block), rows_per_block


# The guarded plans the near-tie plan tests use (tests/test_gpu_near_tie_plans.py): st_tune key 5, n, and what
# csrc/persistent.hip plans on an MI355X (160 KB of LDS per block) -- rows per block, register rows per thread
# of the kernel that runs first, its LDS rows for d = 2 / d = 4, streamed sums in LDS.  The GPU tests read the
# plan the library made (stein_thinning._native.last_plan) and compute their positions from that; the CPU
# tests prove the constructions at these nominal layouts.  The GPU tests also assert that the plan read back
# equals the nominal one: a tripwire on purpose -- if the planning constants (or the device's LDS) change, these
# tests fail until the table and the seeds are derived again, they do not adapt silently.
PLANS = {   # RL[d, st_tune key 15]; sal: stream_a_lds under key 15 = -1 (0 under key 15 = 0)
    'mid': dict(key5=8, n=24_000, R=3000, rt=4, sal=1,
                RL={(2, -1): 896, (4, -1): 896, (2, 0): 896, (4, 0): 896}),
    'large': dict(key5=8, n=72_000, R=9000, rt=8, sal=1,
                  RL={(2, -1): 3712, (4, -1): 1856, (2, 0): 3968, (4, 0): 2176}),
    # ~18 000 streamed sums in LDS leave room for a few chunks of LDS rows: streamed visits >= 32 exist
    'long': dict(key5=4, n=92_000, R=23_000, rt=8, sal=1,
                 RL={(2, -1): 256, (4, -1): 128, (2, 0): 3968, (4, 0): 2176}),
    # the streamed sums no longer fit in LDS: they stay in HBM although key 15 = -1
    'hbm': dict(key5=4, n=98_000, R=24_500, rt=8, sal=0,
                RL={(2, -1): 3968, (4, -1): 2176, (2, 0): 3968, (4, 0): 2176}),
}


def nominal_layout(plan: str, d: int, key15: int = -1):
    p = PLANS[plan]
    return block_layout(p['R'], p['rt'], p['RL'][d, key15])


def pair_positions(layout, block: int = 1, other_block: int = 2):
    """name -> (winner_at, other_at), absolute rows, for a pair planted in block `block` (not block 0) of a
    512-thread kernel with the row classes `layout` (block_layout): the winner in a register row (row 1 of
    thread 70, wave 1) unless the name says otherwise.  LDS offsets 0, 31, 32, 63, 64 and the last one are
    the edges of the 32-bit words of the LDS rows' repeat bits; the rescan of the streamed rows deals them
    384 (or 448) to a visit, so 'str_visit0' is a first visit and -- with more than 14 336 streamed rows --
    'block_last' a visit past the 32 a thread keeps in its bit mask."""
    reg, lds_end, R = layout
    assert reg >= 4 * 512 and reg + 65 <= lds_end < R - 1, layout
    b, c = block * R, other_block * R
    w, p = b + 512 + 70, b + 3 * 512 + 200
    pos = {
        'reg_wave0': (w, b + 2 * 512 + 5),       # wave 0's register rows: rescanned by wave 0, reduced by wave 1
        'reg': (w, p),
        'lds0': (w, b + reg), 'lds31': (w, b + reg + 31), 'lds32': (w, b + reg + 32),
        'lds63': (w, b + reg + 63), 'lds64': (w, b + reg + 64), 'lds_last': (w, b + lds_end - 1),
        'str_first': (w, b + lds_end),
        'str_visit0': (w, b + lds_end + min(200, (R - lds_end) // 2)),
        'block_last': (w, b + R - 1),
        'winner_wave0': (b + 7, b + reg + 100),   # the roles exchanged: the winner outside wave 1 .. 7's registers
        'winner_lds': (b + reg + 40, p),
        'winner_str': (b + lds_end + (R - lds_end) // 2, p),
        'winner_last': (b + R - 1, b + reg + 33),
        'xblock_reg': (w, c + 512 + 300),         # the partner is (or nearly is) another block's own minimum
        'xblock_lds': (w, c + reg + 33),
        'xblock_str': (w, c + R - 2),
    }
    return pos


def repeat_positions(layout, block: int = 1):
    """name -> winner_at for planted('repeat'): the repeat sits at winner_at + 1, whose predecessor the kernel
    reads from global memory -- inside each row class and across every class and block boundary."""
    reg, lds_end, R = layout
    b = block * R
    return {
        'reg': b + 3 * 512 + 200, 'reg_to_lds': b + reg - 1,
        'lds': b + reg + 31, 'lds_to_str': b + lds_end - 1,
        'str': b + lds_end + (R - lds_end) // 2, 'block_last': b + R - 2,
        'block_to_block': b - 1,
    }


class PlantedCase:
    """A planted sample with everything the models say about it, computed once: x, g (and log_p, log_q when
    gf), the integrand thin() / thin_gf() would build, the bit model's indices / flags / winner sums over m
    steps (oracle/stein_ref.c sr_greedy_mt_ties, compact arithmetic), `first` = its first flagged step or
    -1, and `want` = the NumPy path's indices."""

    def __init__(self, kind, d, n, seed, winner_at, other_at=None, m=None, gf=False, weight_ulp=False,
                 repeats=None):
        from oracle import stein_numpy as o
        from oracle import stein_ref_c as oc
        self.kind, self.d, self.n, self.gf = kind, d, n, gf
        self.winner_at = winner_at
        self.other_at = winner_at + 1 if kind == 'repeat' else other_at
        self.m = m = m or (3 if kind == 'mirror' else 20)
        self.step = 0 if kind == 'mirror' else 8
        self.x, self.g = planted(kind, d, n, seed, winner_at, other_at, gf=gf, repeats=repeats)
        self.kw = dict(standardize=False) if kind == 'mirror' else {}
        if gf:
            self.log_p, self.log_q = planted_log_densities(self.x)
            if weight_ulp:   # a copy whose weight differs by one ulp: not a duplicate of the winner
                assert kind == 'copy'
                for _ in range(64):
                    self.log_p[self.other_at] = np.nextafter(self.log_p[self.other_at], -np.inf)
                    w = self.make_integrand().weights
                    if w[self.other_at] != w[winner_at]:
                        break
            self.want = o.thin_gf(self.x, self.log_p, self.log_q, self.g, m)
        else:
            self.want = o.thin(self.x, self.g, m, **self.kw)
        it = self.integrand = self.make_integrand()
        self.idx, _, self.gap, self.thr, self.flagged, self.wv = oc.greedy_ties(
            it.sample, it.gradient, it.weights, it.linv_scale, it.linv_trace, m, winner_sums=True)
        self.first = int(np.flatnonzero(self.flagged)[0]) if self.flagged.any() else -1

    def make_integrand(self):
        from stein_thinning import thinning as st
        if self.gf:
            return st._make_stein_gf_integrand(self.x, self.log_p, self.log_q, self.g)
        return st._make_stein_integrand(self.x, self.g, **self.kw)

    def runner_up(self, t):
        """The row with the smallest running sum at step t other than the selected one (lowest index on a
        tie), from the bit model's sums of that step."""
        from oracle import stein_ref_c as oc
        it = self.integrand
        idx, A = oc.greedy_mt(it.sample, it.gradient, it.weights, it.linv_scale, it.linv_trace, t + 1)
        assert idx[t] == self.idx[t]
        A = A.copy()
        A[idx[t]] = np.inf
        return int(np.argmin(A))

    def check_preconditions(self):
        """What the construction is meant to be, asserted on the final arrays through the models."""
        w, oth, t = self.winner_at, self.other_at, self.step
        it = self.integrand
        same = np.array_equal(it.sample[w], it.sample[oth]) and np.array_equal(it.gradient[w], it.gradient[oth])
        if self.kind == 'twin':
            # first flag exactly at the planted step, the pair at the planted rows: the selected row at
            # winner_at and the runner-up (every other row is far away: the base sample flags nothing) at other_at
            assert self.first == t and self.idx[t] == w, (self.first, self.idx[t], w, oth)
            assert not same and oth not in self.idx[:t + 1]
            assert self.runner_up(t) == oth   # the row whose sum comes next at the planted step
        elif self.kind == 'mirror':
            assert self.first == 0 and self.gap[0] == 0.0 and self.idx[0] == min(w, oth) and not same
            assert self.runner_up(0) == max(w, oth)
        else:
            assert same
            if self.gf and self.integrand.weights[w] != self.integrand.weights[oth]:
                wt = self.integrand.weights   # one ulp apart: the model decides (no promise either way)
                assert abs(wt[w] - wt[oth]) == np.spacing(min(wt[w], wt[oth]))
                assert self.idx[t] in (w, oth)
            else:
                assert self.idx[t] == min(w, oth), (self.idx[t], w, oth)
                assert self.first == -1, self.first


# twin seeds per (plan, d): (default, {position: seed}) -- fixed where the preconditions hold at the nominal
# layouts (tests/test_near_tie_cpu.py asserts them); the overrides also take seeds whose compact-arithmetic
# indices differ from NumPy's, so the exact re-run of the flagged thin is needed.  (A seed is also passed over
# when the NumPy path itself departs from the exact bit model on the pair: NumPy's ** 1.5 / ** 2.5 is not
# always the correctly rounded power the exact arithmetic computes, and between twins one ulp decides.)
TWIN_SEEDS = {
    ('large', 2): (8, {'lds31': 3, 'lds32': 3, 'str_first': 3, 'winner_str': 3, 'reg_wave0': 4, 'lds0': 4,
                       'lds_last': 4, 'xblock_reg': 4, 'xblock_lds': 5, 'lds64': 5, 'str_visit0': 6,
                       'xblock_str': 6}),
    ('large', 4): (5, {'winner_str': 14, 'winner_last': 8, 'lds63': 7, 'lds0': 7, 'str_visit0': 7,
                       'block_last': 7, 'reg': 8, 'xblock_lds': 8, 'winner_wave0': 3, 'winner_lds': 6}),
    ('mid', 2): (3, {'reg': 4}), ('long', 2): (3, {}), ('long', 4): (3, {}), ('hbm', 2): (3, {}), ('hbm', 4): (3, {}),
}
OTHER_SEED = 3   # copy, repeat, mirror


def twin_seed(plan, d, position):
    default, special = TWIN_SEEDS[plan, d]
    return special.get(position, default)


# the reduced cover of the plans other than 'large' (and of the kinds other than 'twin' on 'large'): every kind
# reaches the register, LDS and streamed rows, the other block, and the exchanged roles
REDUCED = {
    'twin': ['reg', 'lds32', 'lds_last', 'str_first', 'block_last', 'winner_str', 'xblock_lds'],
    'copy': ['reg_wave0', 'lds63', 'str_visit0', 'block_last', 'winner_lds', 'xblock_str'],
    'mirror': ['reg', 'lds0', 'str_first', 'block_last', 'xblock_reg'],
}


def large_twin_cases():
    """[(d, position)]: 'twin' at every position of the large plan, d = 2 and 4."""
    names = list(pair_positions(nominal_layout('large', 2)))
    return [(d, name) for d in (2, 4) for name in names]


def reduced_cases():
    """[(plan, kind, d, position)]: every other kind on the large plan and every kind on the other plans."""
    out = []
    for plan in PLANS:
        reps = list(repeat_positions(nominal_layout(plan, 2)))
        if plan == 'large':
            for d in (2, 4):
                out += [(plan, 'copy', d, name) for name in REDUCED['copy']]
                out += [(plan, 'repeat', d, name) for name in reps]
        else:
            d_alt = {'mid': 2, 'long': 4, 'hbm': 2}[plan]   # the other d somewhere on every plan
            out += [(plan, 'twin', 2, name) for name in REDUCED['twin']]
            if plan != 'mid':
                out += [(plan, 'twin', 4, name) for name in ('lds_last', 'block_last')]
            out += [(plan, 'copy', d_alt, name) for name in REDUCED['copy']]
            out += [(plan, 'repeat', 6 - d_alt, name) for name in reps]
        out += [(plan, 'mirror', 2, name) for name in REDUCED['mirror']]
    return out


def planted_case(plan, kind, d, position, layout=None, key15=-1):
    """The PlantedCase of one (plan, kind, d, position), at `layout` (block_layout of the plan the library made)
    or at the plan's nominal layout."""
    layout = layout or nominal_layout(plan, d, key15)
    n = PLANS[plan]['n']
    if kind == 'repeat':
        return _planted_case(kind, d, n, OTHER_SEED, repeat_positions(layout)[position], None)
    seed = twin_seed(plan, d, position) if kind == 'twin' else OTHER_SEED
    return _planted_case(kind, d, n, seed, *pair_positions(layout)[position])


@functools.lru_cache(maxsize=2)   # the knob settings of one test share a sample
def _planted_case(kind, d, n, seed, winner_at, other_at):
    return PlantedCase(kind, d, n, seed, winner_at, other_at)


# the row classes (of the winner, of the other row) each position is meant to reach
CLASSES = {
    'reg_wave0': ('reg', 'reg'), 'reg': ('reg', 'reg'), 'lds0': ('reg', 'lds'), 'lds31': ('reg', 'lds'),
    'lds32': ('reg', 'lds'), 'lds63': ('reg', 'lds'), 'lds64': ('reg', 'lds'), 'lds_last': ('reg', 'lds'),
    'str_first': ('reg', 'str'), 'str_visit0': ('reg', 'str'), 'block_last': ('reg', 'str'),
    'winner_wave0': ('reg', 'lds'), 'winner_lds': ('lds', 'reg'), 'winner_str': ('str', 'reg'),
    'winner_last': ('str', 'lds'), 'xblock_reg': ('reg', 'reg'), 'xblock_lds': ('reg', 'lds'),
    'xblock_str': ('reg', 'str'),
}
REPEAT_CLASSES = {
    'reg': ('reg', 'reg'), 'reg_to_lds': ('reg', 'lds'), 'lds': ('lds', 'lds'), 'lds_to_str': ('lds', 'str'),
    'str': ('str', 'str'), 'block_last': ('str', 'str'), 'block_to_block': ('str', 'reg'),
}


def row_class(layout, row: int):
    """(block, 'reg' | 'lds' | 'str') of an absolute row under block_layout `layout`."""
    reg, lds_end, R = layout
    off = row % R
    return row // R, 'reg' if off < reg else ('lds' if off < lds_end else 'str')


# 'mirror' on the large plan with every other LDS row of the block a repeat (planted's `repeats`): the other
# row at the edges of the repeat-bit words
MIRROR_REPEATS = ['lds0', 'lds31', 'lds32', 'lds63', 'lds64', 'lds_last']


@functools.lru_cache(maxsize=2)
def mirror_repeats_case(position, layout=None):
    layout = layout or nominal_layout('large', 2)
    w, oth = pair_positions(layout)[position]
    b = row_class(layout, oth)[0] * layout[2]
    return PlantedCase('mirror', 2, PLANS['large']['n'], OTHER_SEED, w, oth,
                       repeats=(b + layout[0], b + layout[1]))


# gradient-free cases on the large plan, d = 2: (kind, position, seed, the copy's weight moved by one ulp)
GF_CASES = [('twin', 'lds32', 3, False), ('twin', 'str_visit0', 3, False), ('copy', 'lds63', 3, True),
            ('copy', 'str_first', 3, False)]


GF_LDS_ROWS = 3008   # the large plan's LDS rows at d = 2 with a weight per row


@functools.lru_cache(maxsize=2)
def planted_gf_case(kind, position, seed, weight_ulp, layout=None):
    layout = layout or block_layout(PLANS['large']['R'], PLANS['large']['rt'], GF_LDS_ROWS)
    return PlantedCase(kind, 2, PLANS['large']['n'], seed, *pair_positions(layout)[position], gf=True,
                       weight_ulp=weight_ulp)


# Two ranks of 36 000 rows, 4 blocks each (st_tune key 5 = 4): every rank runs the guarded general kernel of
# 512 threads and 4 register rows on 9 000 rows per block (the plan of a multi-rank 2e6-row thin)
RANK_N, RANK_KEY5, RANK_LAYOUT = 72_000, 4, block_layout(9000, 4, 3200)
RANK_CASES = {   # name -> (kind, position, seed, block of the winner, block of the other row); blocks 4 .. 7: rank 1
    'twin_lds': ('twin', 'lds32', 8, 5, 5),
    'twin_str': ('twin', 'block_last', 8, 5, 5),
    'copy_other_rank': ('copy', 'xblock_str', 3, 5, 1),
}


@functools.lru_cache(maxsize=4)
def rank_case(name, layout=RANK_LAYOUT):
    kind, position, seed, blk, oblk = RANK_CASES[name]
    return PlantedCase(kind, 2, RANK_N, seed, *pair_positions(layout, blk, oblk)[position])
