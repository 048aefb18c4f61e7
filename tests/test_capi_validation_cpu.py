"""Every argument check of csrc/capi.hip that fails before the first HIP call, as one table: entry point, full
argument list, expected return code, a substring of st_last_error().  No GPU: the "device" pointers are
addresses inside a host buffer and no row is a valid call.  Twins (diagonal / dense, Gaussian / Student-t, the
seven greedy entry points, ...) get the same mutations, so a check lost from one of them shows up; two-violation
rows pin the ORDER of the checks, which is part of the ABI (the first violated check decides the code)."""
import ctypes
import math
import threading

import pytest

INT32_MIN = -2 ** 31
OK, INV, UNS = 0, -1, -2


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    from stein_thinning import _native
    assert (_native.ST_OK, _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED) == (OK, INV, UNS)
    return _native.load_library(ge.HIP_LIB)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _addr(a):
    return ctypes.cast(a, ctypes.c_void_p).value


def _table(lib):
    """[(entry point, argument list, code, message substring)]"""
    keep = []                                    # host arrays the rows point into
    buf = (ctypes.c_double * 64)()
    keep.append(buf)
    P = (_addr(buf) + 15) & ~15                  # a 16-byte aligned fake device pointer
    Q = P + 16                                   # another one
    P8, P4 = P + 8, P + 4                        # misaligned by 8 (still 8-byte aligned), by 4

    def host(ctype, vals):
        a = _arr(ctype, vals)
        keep.append(a)
        return _addr(a)

    f64, i64, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_void_p
    WS = lib.st_greedy_workspace_bytes(10, 4, 1)
    assert WS > 0
    rows = []
    bases = {}

    def base(entry, **kw):
        bases[entry] = kw

    def row(entry, code, msg, **kw):
        a = dict(bases[entry])
        for k, v in kw.items():
            assert k in a, (entry, k)
            a[k] = v
        rows.append((entry, list(a.values()), code, msg))

    def both(entries, code, msg, **kw):
        for e in entries:
            row(e, code, msg, **kw)

    # ---- the greedy entry points -----------------------------------------------------------------------
    prob = dict(x=P, g=P, w=None, n=10, d=4, ld=16, l=1.0, tr=4.0)
    out = dict(idx_out=P, a_work=P, workspace=P, workspace_bytes=WS, stream=None)
    TP = host(vp, [P, P, 0, 0, 0, 0, 0, 0])     # peer mailbox table of two ranks
    base('st_greedy_steps', **prob, t_begin=0, t_end=5, n_points=5, **out)
    base('st_greedy', **prob, n_points=5, **out)
    base('st_greedy_dense', **{**prob, 'l': P}, n_points=5, **out)
    base('st_greedy_sharded', **prob, row_begin=0, row_end=10, rank=0, nranks=2, peers=TP, seq_base=0, n_points=5,
         **out)
    base('st_greedy_step', **prob, row_offset=0, t=1, nranks=2, cands_in=P, cand_out=P, **out)
    base('st_greedy_step_exchange', **prob, row_offset=0, t=1, rank=0, nranks=2, peers=TP, cands=P, idx_out=P,
         a_work=P, workspace=P, workspace_bytes=WS, status=P, stream=None)
    P2 = host(vp, [P, P])
    base('st_greedy_batch', count=2, x=P2, g=P2, w=None, n=host(i64, [10, 10]), d=4, ld=host(i64, [16, 16]),
         l=host(f64, [1.0, 1.0]), tr=host(f64, [4.0, 4.0]), n_points=5, idx_out=P2, a_work=P2, workspace=P2,
         workspace_bytes=host(i64, [WS, WS]), stream=None)
    single = ['st_greedy_steps', 'st_greedy', 'st_greedy_dense', 'st_greedy_sharded']
    steps = ['st_greedy_step', 'st_greedy_step_exchange']
    short = 'workspace too small (%d < %d)' % (WS - 1, WS)
    # outputs and workspace: the same four mutations (and two more) on all seven
    both(single + steps, INV, 'NULL output/workspace', a_work=None)
    both(single + steps, INV, 'NULL output/workspace', workspace=None)
    both(single + steps, INV, 'a_work/workspace must be 16-byte aligned', a_work=P8)
    both(single + steps, INV, 'a_work/workspace must be 16-byte aligned', workspace=P8)
    both(single, INV, short, workspace_bytes=WS - 1)
    row('st_greedy_step', INV, short, workspace_bytes=WS - 1)            # NEW; the parent: "workspace too small"
    row('st_greedy_step_exchange', INV, short, workspace_bytes=WS - 1)   # NEW; the parent: "workspace too small"
    both(single, INV, 'NULL output/workspace', idx_out=None)
    both(steps, INV, 'idx_out is NULL', idx_out=None)
    row('st_greedy_batch', INV, 'problem 1: NULL output/workspace', a_work=host(vp, [P, 0]))
    row('st_greedy_batch', INV, 'problem 1: NULL output/workspace', workspace=host(vp, [P, 0]))
    row('st_greedy_batch', INV, 'problem 1: NULL output/workspace', idx_out=host(vp, [P, 0]))
    row('st_greedy_batch', INV, 'problem 1: a_work/workspace must be 16-byte aligned', a_work=host(vp, [P, P8]))
    row('st_greedy_batch', INV, 'problem 1: a_work/workspace must be 16-byte aligned', workspace=host(vp, [P, P8]))
    row('st_greedy_batch', INV, 'problem 1: ' + short, workspace_bytes=host(i64, [WS, WS - 1]))
    row('st_greedy_batch', INV, 'problem 0: ' + short, workspace_bytes=host(i64, [WS - 1, WS]))
    # the problem itself (check_problem): every site once, then two of them through every caller
    e = 'st_greedy_steps'
    row(e, INV, 'sample/gradient pointer is NULL', x=None)
    row(e, INV, 'sample/gradient pointer is NULL', g=None)
    row(e, INV, 'n must be >= 1 (got 0)', n=0)
    row(e, INV, 'd must be >= 1 (got 0)', d=0)
    row(e, UNS, 'd = 129 exceeds the supported maximum 128', d=129)
    row(e, INV, 'ld must be a multiple of 8 and >= n (n=10, ld=8)', ld=8)
    row(e, INV, 'ld must be a multiple of 8 and >= n (n=10, ld=12)', ld=12)
    row(e, INV, 'device arrays must be 16-byte aligned', x=P8)
    row(e, INV, 'device arrays must be 16-byte aligned', g=P8)
    row(e, INV, 'device arrays must be 16-byte aligned', w=P8)
    row('st_greedy_batch', INV, 'sample/gradient pointer is NULL', x=host(vp, [P, 0]))
    row('st_greedy_batch', UNS, 'exceeds the supported maximum', d=129)
    row('st_greedy_batch', INV, 'ld must be a multiple of 8', ld=host(i64, [16, 12]))
    # run length and step range
    both(single, INV, 'n_points must be >= 1', n_points=0)
    row('st_greedy_batch', INV, 'n_points must be >= 1', n_points=0)
    row('st_greedy_steps', INV, 'need 0 <= t_begin <= t_end <= n_points', t_begin=-1)
    row('st_greedy_steps', INV, 'need 0 <= t_begin <= t_end <= n_points', t_begin=3, t_end=2)
    row('st_greedy_steps', INV, 'need 0 <= t_begin <= t_end <= n_points', t_end=6)
    # order: n_points before the problem everywhere but in st_greedy_steps
    both(['st_greedy', 'st_greedy_dense', 'st_greedy_sharded'], INV, 'n_points must be >= 1', n_points=0, x=None)
    row('st_greedy_batch', INV, 'n_points must be >= 1', n_points=0, x=host(vp, [0, 0]))
    row('st_greedy_steps', INV, 'sample/gradient pointer is NULL', n_points=0, x=None)
    row('st_greedy_steps', UNS, 'exceeds the supported maximum', n_points=0, d=129)
    # the batch's own checks
    row('st_greedy_batch', INV, 'count must be in [1, 8]', count=0)
    row('st_greedy_batch', INV, 'count must be in [1, 8]', count=9)
    for name in ('x', 'g', 'n', 'ld', 'l', 'tr', 'idx_out', 'a_work', 'workspace', 'workspace_bytes'):
        row('st_greedy_batch', INV, 'NULL argument array', **{name: None})
    row('st_greedy_batch', INV, 'problem 1: weights must be given for every problem or none', w=host(vp, [P, 0]))
    row('st_greedy_batch', INV, 'problem 1: weights must be given for every problem or none', w=host(vp, [0, P]))
    # peers (check_peers) through its three callers
    base('st_mailbox_handshake', peers=TP, nranks=2, rank=0, token=1, ok=P, stream=None)
    peered = ['st_mailbox_handshake', 'st_greedy_sharded', 'st_greedy_step_exchange']
    both(peered, INV, 'nranks must be in [2, 8]', nranks=1)
    both(peered, INV, 'nranks must be in [2, 8]', nranks=9)
    both(peered, INV, 'rank out of range', rank=-1)
    both(peered, INV, 'rank out of range', rank=2)
    both(peered, INV, 'NULL peer mailbox table', peers=None)
    both(peered, INV, 'peer mailbox 1 is NULL or misaligned', peers=host(vp, [P, 0]))
    both(peered, INV, 'peer mailbox 1 is NULL or misaligned', peers=host(vp, [P, P8]))
    both(peered, INV, 'peer mailbox 0 is NULL or misaligned', peers=host(vp, [P8, P]))
    row('st_mailbox_handshake', INV, 'NULL ok flag', ok=None)
    row('st_mailbox_handshake', INV, 'token must be < 2^63', token=1 << 63)
    # row ranges
    base('st_greedy_sharded_supported', n=10, d=4, has_weights=0, row_begin=0, row_end=10, rank=0, nranks=2,
         n_points=5)
    for e in ('st_greedy_sharded', 'st_greedy_sharded_supported'):
        row(e, INV, 'need 0 <= row_begin < row_end <= n', row_begin=-1)
        row(e, INV, 'need 0 <= row_begin < row_end <= n', row_begin=4, row_end=4)
        row(e, INV, 'need 0 <= row_begin < row_end <= n', row_end=11)
    e = 'st_greedy_sharded_supported'
    row(e, INV, 'bad problem (n = 10, d = 0)', d=0)
    row(e, INV, 'bad problem (n = 10, d = 129)', d=129)
    row(e, INV, 'bad problem (n = 0, d = 4)', n=0)
    row(e, INV, 'bad problem (n = 10, d = 4)', n_points=0)
    row(e, INV, 'bad rank 0 of 1', nranks=1)
    row(e, INV, 'bad rank 0 of 9', nranks=9)
    row(e, INV, 'bad rank -1 of 2', rank=-1)
    row(e, INV, 'bad rank 2 of 2', rank=2)
    # one distributed step
    both(steps, INV, 't must be >= 0', t=-1)
    both(steps, INV, 'row_offset must be >= 0', row_offset=-1)
    both(steps, INV, 'sample/gradient pointer is NULL', x=None)
    both(steps, UNS, 'exceeds the supported maximum', d=129)
    row('st_greedy_step', INV, 'nranks must be in [1, 64]', nranks=0)
    row('st_greedy_step', INV, 'nranks must be in [1, 64]', nranks=65)
    row('st_greedy_step', INV, 'cands_in is NULL for t > 0', cands_in=None)
    row('st_greedy_step', INV, 'NULL output/workspace', cand_out=None)
    row('st_greedy_step_exchange', INV, 'NULL output/workspace', cands=None)
    row('st_greedy_step_exchange', INV, 'NULL output/workspace', status=None)
    # order within a step: NULL buffers, idx_out, row_offset, alignment, size
    both(steps, INV, 'NULL output/workspace', a_work=None, idx_out=None)
    both(steps, INV, 'idx_out is NULL', idx_out=None, row_offset=-1)
    both(steps, INV, 'row_offset must be >= 0', row_offset=-1, a_work=P8)
    both(steps, INV, '16-byte aligned', workspace=P8, workspace_bytes=0)
    # near-tie read-back, finalize
    step_out = host(i64, [0])
    base('st_greedy_near_tie', workspace=P, workspace_bytes=1 << 20,
         step_out=ctypes.cast(step_out, ctypes.POINTER(i64)), stream=None)
    row('st_greedy_near_tie', INV, 'NULL workspace/output', workspace=None)
    row('st_greedy_near_tie', INV, 'NULL workspace/output', step_out=None)
    row('st_greedy_near_tie', INV, 'workspace too small', workspace_bytes=64)
    base('st_greedy_finalize', cands_in=P, nranks=2, d=4, idx_out=P, t=1, stream=None)
    e = 'st_greedy_finalize'
    row(e, INV, 'NULL pointer', cands_in=None)
    row(e, INV, 'NULL pointer', idx_out=None)
    row(e, INV, 'nranks must be in [1, 64]', nranks=0)
    row(e, INV, 'nranks must be in [1, 64]', nranks=65)
    row(e, UNS, 'unsupported d', d=0)
    row(e, UNS, 'unsupported d', d=129)
    row(e, INV, 't must be >= 0', t=-1)

    # ---- mailbox and IPC -------------------------------------------------------------------------------
    box = host(vp, [0])
    boxp = ctypes.cast(box, ctypes.POINTER(vp))
    base('st_mailbox_alloc', bytes=lib.st_mailbox_bytes(2), mailbox=boxp)
    row('st_mailbox_alloc', INV, 'bad mailbox request', mailbox=None)
    row('st_mailbox_alloc', INV, 'bad mailbox request', bytes=lib.st_mailbox_bytes(2) - 1)
    base('st_ipc_get_handle', dev_ptr=P, handle_out=P)
    row('st_ipc_get_handle', INV, 'NULL pointer', dev_ptr=None)
    row('st_ipc_get_handle', INV, 'NULL pointer', handle_out=None)
    base('st_ipc_open_handle', handle=P, dev_ptr=boxp)
    row('st_ipc_open_handle', INV, 'NULL pointer', handle=None)
    row('st_ipc_open_handle', INV, 'NULL pointer', dev_ptr=None)

    # ---- diagonal / dense twins ------------------------------------------------------------------------
    kp = dict(x=P, g=P, w=None, ld=16, d=4, l=1.0, tr=4.0, i1=P, i2=P, n_pairs=3, out=P, stream=None)
    base('st_kernel_pairs', **kp)
    base('st_kernel_pairs_dense', **{**kp, 'l': P})
    pm = dict(x=P, g=P, w=None, n=10, ld=16, d=4, l=1.0, tr=4.0)
    base('st_kmat', **pm, kmat_out=P, stream=None)
    base('st_kmat_dense', **{**pm, 'l': P}, kmat_out=P, stream=None)
    base('st_ksd_colsum', **pm, row_begin=0, row_end=10, csum_out=P, stream=None)
    base('st_ksd_colsum_dense', **{**pm, 'l': P}, row_begin=0, row_end=10, csum_out=P, stream=None)
    base('st_ksd_cumulative', **pm, ks_out=P, workspace=P, workspace_bytes=128, stream=None)
    base('st_ksd_cumulative_dense', **{**pm, 'l': P}, ks_out=P, workspace=P, workspace_bytes=128, stream=None)
    base('st_ksd_finish', **pm, csum=P, ks_out=P, stream=None)
    dense = ['st_greedy_dense', 'st_kernel_pairs_dense', 'st_kmat_dense', 'st_ksd_colsum_dense',
             'st_ksd_cumulative_dense']
    both(dense, UNS, 'd = 17 exceeds the dense-preconditioner maximum 16', d=17)
    both(dense, INV, 'linv pointer is NULL', l=None)
    both(dense, INV, 'linv must be 16-byte aligned', l=P8)
    problem_first = ['st_kmat', 'st_kmat_dense', 'st_ksd_colsum', 'st_ksd_colsum_dense', 'st_ksd_cumulative',
                     'st_ksd_cumulative_dense', 'st_ksd_finish']
    both(problem_first, INV, 'sample/gradient pointer is NULL', x=None)
    both(problem_first, INV, 'n must be >= 1', n=0)
    both(problem_first, UNS, 'exceeds the supported maximum', d=129)
    both(problem_first, INV, 'ld must be a multiple of 8', ld=12)
    both(problem_first, INV, 'device arrays must be 16-byte aligned', w=P8)
    # order: the problem before the preconditioner, the preconditioner before the outputs
    both(dense[:1] + dense[2:], INV, 'sample/gradient pointer is NULL', x=None, l=None)
    both(['st_kmat_dense'], INV, 'linv pointer is NULL', l=None, kmat_out=None)
    both(['st_ksd_colsum_dense'], INV, 'linv pointer is NULL', l=None, csum_out=None)
    both(['st_ksd_cumulative_dense'], INV, 'linv pointer is NULL', l=None, ks_out=None)
    both(['st_greedy_dense'], INV, 'linv pointer is NULL', l=None, a_work=None)
    k_big = 65536 * 64
    both(['st_kmat', 'st_kmat_dense'], INV, 'NULL output', kmat_out=None)
    both(['st_kmat', 'st_kmat_dense'], UNS, 'k too large for the tiled grid', n=k_big, ld=k_big)
    both(['st_kmat', 'st_kmat_dense'], INV, 'NULL output', kmat_out=None, n=k_big, ld=k_big)
    cs = ['st_ksd_colsum', 'st_ksd_colsum_dense']
    both(cs, INV, 'NULL output', csum_out=None)
    both(cs, INV, 'need 0 <= row_begin <= row_end <= n', row_begin=-1)
    both(cs, INV, 'need 0 <= row_begin <= row_end <= n', row_begin=3, row_end=2)
    both(cs, INV, 'need 0 <= row_begin <= row_end <= n', row_end=11)
    cu = ['st_ksd_cumulative', 'st_ksd_cumulative_dense']
    both(cu, INV, 'NULL output/workspace', ks_out=None)
    both(cu, INV, 'NULL output/workspace', workspace=None)
    both(cu, INV, 'workspace too small', workspace_bytes=127)
    row('st_ksd_finish', INV, 'NULL pointer', csum=None)
    row('st_ksd_finish', INV, 'NULL pointer', ks_out=None)
    pairs = ['st_kernel_pairs', 'st_kernel_pairs_dense']
    both(pairs, INV, 'sample/gradient pointer is NULL', x=None)
    both(pairs, INV, 'sample/gradient pointer is NULL', g=None)
    both(pairs, INV, 'ld must be >= 1', ld=0)
    for name in ('i1', 'i2', 'out'):
        both(pairs, INV, 'bad pair list', **{name: None})
    both(pairs, INV, 'bad pair list', n_pairs=-1)
    both(pairs, OK, '', n_pairs=0, x=None, g=None, i1=None, i2=None, out=None, d=0, ld=0)
    row('st_kernel_pairs_dense', OK, '', n_pairs=0, l=None)
    row('st_kernel_pairs', UNS, 'unsupported d = 0', d=0)
    row('st_kernel_pairs', UNS, 'unsupported d = 129', d=129)
    row('st_kernel_pairs_dense', INV, 'd must be >= 1 (got 0)', d=0)
    # order: NULL, then d, then ld; the dense form: NULL, d < 1, the preconditioner, ld
    row('st_kernel_pairs', INV, 'sample/gradient pointer is NULL', x=None, g=None, i1=None, i2=None, out=None, d=200)
    row('st_kernel_pairs', UNS, 'unsupported d = 200', d=200, ld=0)
    row('st_kernel_pairs', INV, 'ld must be >= 1', ld=0, out=None)
    row('st_kernel_pairs_dense', INV, 'sample/gradient pointer is NULL', x=None, d=0)
    row('st_kernel_pairs_dense', INV, 'd must be >= 1', d=0, l=None)
    row('st_kernel_pairs_dense', UNS, 'dense-preconditioner maximum', d=17, ld=0)
    row('st_kernel_pairs_dense', INV, 'linv pointer is NULL', l=None, ld=0)
    row('st_kernel_pairs_dense', INV, 'ld must be >= 1', ld=0, out=None)

    # ---- kernel densities ------------------------------------------------------------------------------
    kde = dict(p=P, ldp=64, n=10, logw=None, logw0=-2.3, q=P, ldq=64, m=7, d=4)
    tail = dict(log_norm=0.5, whiten=P, log_q=P, grad=P, ws=None, ws_bytes=0, stream=None)
    base('st_kde_logpdf_grad', **kde, **tail)
    base('st_kde_t_logpdf_grad', **kde, df=3.0, **tail)
    kdes = ['st_kde_logpdf_grad', 'st_kde_t_logpdf_grad']
    both(kdes, OK, '', m=0, p=None, q=None, whiten=None, log_q=None, grad=None, d=0, n=0)
    for name in ('p', 'q', 'whiten', 'log_q', 'grad'):
        both(kdes, INV, 'NULL pointer', **{name: None})
    both(kdes, UNS, 'unsupported d = 0', d=0)
    both(kdes, UNS, 'unsupported d = 129', d=129)
    for kw in (dict(n=0), dict(m=-1), dict(ldp=9), dict(ldq=6)):
        both(kdes, INV, 'bad sizes (need n >= 1, ld >= count)', **kw)
    both(kdes, UNS, 'm too large', m=1 << 40, ldq=1 << 40)
    both(kdes, INV, 'workspace too small (0 < 504)', d=9)
    both(kdes, INV, 'workspace too small (503 < 504)', d=9, ws=P, ws_bytes=503)
    both(kdes, INV, 'workspace too small (504 < 504)', d=9, ws=None, ws_bytes=504)
    for df in (0.0, -1.0, math.inf, math.nan):
        row('st_kde_t_logpdf_grad', INV, 'df must be finite and > 0', df=df)
    # order: the Gaussian form tests d before the sizes; the Student-t form the sizes, then df, then d
    both(kdes, INV, 'NULL pointer', p=None, d=129, n=0)
    row('st_kde_logpdf_grad', UNS, 'unsupported d = 129', d=129, n=0)
    row('st_kde_t_logpdf_grad', INV, 'bad sizes', d=129, n=0)
    row('st_kde_t_logpdf_grad', INV, 'bad sizes', df=0.0, n=0)
    row('st_kde_t_logpdf_grad', INV, 'df must be finite and > 0', df=0.0, d=129)
    both(kdes, UNS, 'unsupported d = 129', d=129, m=1 << 40, ldq=1 << 40)

    # ---- parametric proxies ----------------------------------------------------------------------------
    base('st_proxy_logpdf_grad', x=P, n=5, d=4, loc=P, whiten=P, precision=P, df=0.0, c_log=0.0, log_q=P, grad=P,
         stream=None)
    e = 'st_proxy_logpdf_grad'
    row(e, INV, 'n must be >= 0', n=-1)
    row(e, INV, 'd must be >= 1', d=0)
    row(e, UNS, 'd = 129 exceeds 128', d=129)
    for df in (-1.0, math.inf, math.nan):
        row(e, INV, 'df must be 0 (Gaussian) or finite > 0', df=df)
    for name in ('x', 'loc', 'whiten', 'precision', 'log_q', 'grad'):
        row(e, INV, 'NULL pointer', **{name: None})
    row(e, INV, 'd must be >= 1', n=0, d=0)                          # the checks before the n = 0 return
    row(e, INV, 'df must be 0', n=0, df=-1.0)
    row(e, OK, '', n=0, x=None, loc=None, whiten=None, precision=None, log_q=None, grad=None)
    base('st_mixture_logpdf_score', x=P, n=5, d=4, k=3, log_coef=P, means=P, precision=P, log_p=P, score=P,
         stream=None)
    e = 'st_mixture_logpdf_score'
    row(e, INV, 'n must be >= 0 (got -1)', n=-1)
    row(e, INV, 'd must be >= 1 (got 0)', d=0)
    row(e, INV, 'k must be >= 1 (got 0)', k=0)
    for name in ('x', 'log_coef', 'means', 'precision', 'log_p', 'score'):
        row(e, INV, 'NULL pointer', **{name: None})
        row(e, INV, 'device arrays must be 8-byte aligned', **{name: P4})
    row(e, UNS, "d = 65 exceeds the mixture kernels' maximum 64", d=65)
    row(e, UNS, 'k = 1025 components exceed the maximum 1024', k=1025)
    row(e, INV, 'device arrays must be 8-byte aligned', d=65, x=P4)  # order: alignment before the widths
    row(e, UNS, 'exceeds the mixture', d=65, k=1025)
    row(e, INV, 'NULL pointer', n=0, means=None)                     # the parameters even for n = 0
    row(e, UNS, 'components exceed', n=0, k=1025)
    row(e, OK, '', n=0, x=None, log_p=None, score=None)
    mv_ws = lib.st_mvt_moments_workspace_bytes(5, 4)
    assert mv_ws > 0
    base('st_mvt_moments', x=P, n=5, d=4, loc=P, whiten=P, df=3.0, want_grad=1, out=P, workspace=P,
         workspace_bytes=mv_ws, stream=None)
    e = 'st_mvt_moments'
    row(e, INV, 'n must be >= 1 (got 0)', n=0)
    row(e, INV, 'd must be >= 1 (got 0)', d=0)
    for df in (0.0, -1.0, math.inf, math.nan):
        row(e, INV, 'df must be finite and > 0', df=df)
    for name in ('x', 'loc', 'whiten', 'out', 'workspace'):
        row(e, INV, 'NULL pointer', **{name: None})
        row(e, INV, 'device arrays must be 8-byte aligned', **{name: P4})
    row(e, UNS, "d = 17 exceeds the moment kernels' maximum 16", d=17)
    row(e, INV, 'workspace too small (%d < %d)' % (mv_ws - 1, mv_ws), workspace_bytes=mv_ws - 1)
    row(e, INV, 'device arrays must be 8-byte aligned', d=17, x=P4)

    # ---- Lotka-Volterra --------------------------------------------------------------------------------
    def span(t0=0.0, t1=25.0, rtol=1e-6, atol=1e-8):
        return host(f64, [t0, t1, 1.0, 1.0, rtol, atol])
    W4 = host(f64, [1.0, 0.0, 0.0, 1.0])
    lvp = dict(theta=P, n=5, t_eval=P, t_n=3, y_obs=P, span=span(), cov_inv=W4, max_steps=100, grad_out=P, status=P)
    lv_ws = lib.st_lv_grad_workspace_bytes(5, 3)
    assert lv_ws > 0
    base('st_lv_grad_log_posterior', **lvp, stream=None)
    base('st_lv_grad_log_posterior_ws', **lvp, workspace=P, workspace_bytes=lv_ws, stream=None)
    base('st_lv_log_target_density', log_theta=P, theta=P, n=5, t_eval=P, t_n=3, y_obs=P, span=span(), whiten=W4,
         c_log=0.0, norm_logc=0.9, max_steps=100, grad_out=P, status=P, workspace=P, workspace_bytes=5 * 3 * 8,
         stream=None)
    grads = ['st_lv_grad_log_posterior', 'st_lv_grad_log_posterior_ws']
    lvs = grads + ['st_lv_log_target_density']
    both(lvs, INV, 'n must be >= 0', n=-1)
    both(lvs, INV, 't_n must be >= 1', t_n=0)
    both(lvs, INV, 'NULL solver settings', span=None)
    both(lvs, INV, 'max_steps must be >= 1', max_steps=0)
    for name in ('t_eval', 'y_obs', 'theta', 'grad_out', 'status'):
        both(lvs, INV, 'NULL pointer', **{name: None})
    both(lvs, INV, 'need t1 > t0 (forward integration)', span=span(t0=25.0))
    both(lvs, INV, 'need t1 > t0 (forward integration)', span=span(t1=math.nan))
    both(lvs, INV, 'rtol and atol must be > 0', span=span(rtol=0.0))
    both(lvs, INV, 'rtol and atol must be > 0', span=span(atol=0.0))
    both(grads, INV, 'NULL cov_inv', cov_inv=None)
    both(grads, INV, 'NULL cov_inv', cov_inv=None, n=0)
    both(grads, OK, '', n=0, theta=None, t_eval=None, y_obs=None, grad_out=None, status=None)
    both(grads, INV, 'NULL pointer', theta=None, cov_inv=None)       # order: the shared part first
    row('st_lv_grad_log_posterior_ws', INV, 'NULL workspace', workspace=None)
    row('st_lv_grad_log_posterior_ws', INV, 'workspace too small', workspace_bytes=lv_ws - 1)
    row('st_lv_grad_log_posterior_ws', INV, 'NULL cov_inv', cov_inv=None, workspace=None)
    row('st_lv_grad_log_posterior_ws', INV, 'workspace too small', n=0, workspace_bytes=-1)
    e = 'st_lv_log_target_density'
    row(e, INV, 'NULL whiten', whiten=None)
    row(e, INV, 'NULL log_theta / workspace', log_theta=None)
    row(e, INV, 'NULL log_theta / workspace', workspace=None)
    row(e, INV, 'workspace too small', workspace_bytes=5 * 3 * 8 - 1)
    row(e, OK, '', n=0, log_theta=None, theta=None, t_eval=None, y_obs=None, grad_out=None, status=None,
        workspace=None, workspace_bytes=0)
    # the samplers
    S4 = host(f64, [0.1, 0.1, 0.1, 0.1])
    common = dict(state=P, chains=2, first_chain=0, first_step=1, steps=4, init=0)
    noise = dict(noise_mode=0, seed=1, z=P, log_u=P, noise_ld=8, noise_row0=0, t_eval=P, t_n=3, y_obs=P,
                 span=span(), whiten=W4, c_log=0.0, norm_logc=0.9)
    rw = dict(**common, step=S4, **noise, max_steps=100, samples=P, log_p=P, out_ld=8, out_row0=0, stream=None)
    base('st_lv_rwmh', **rw)
    base('st_lv_rwmh_wave', **rw)
    E12 = host(f64, [0.1] * 4 + [0.005] * 4 + [50.0] * 4)
    C4 = host(f64, [1.0, 1.0, math.inf, 1.0])
    base('st_lv_mala_wave', **common, step=E12, drift_clip=C4, **noise, cov_inv=W4, max_steps=100, samples=P,
         log_p=P, grad=P, out_ld=8, out_row0=0, stream=None)
    samplers = ['st_lv_rwmh', 'st_lv_rwmh_wave', 'st_lv_mala_wave']
    both(samplers, INV, 'chains must be >= 1 (got 0)', chains=0)
    both(samplers, INV, 'steps must be >= 1 (got 0)', steps=0)
    both(samplers, INV, 't_n must be >= 1', t_n=0)
    both(samplers, INV, 'NULL solver settings', span=None)
    both(samplers, INV, 'max_steps must be >= 1', max_steps=0)
    both(samplers, INV, 'NULL pointer', t_eval=None)
    both(samplers, INV, 'NULL pointer', y_obs=None)
    both(samplers, INV, 'need t1 > t0', span=span(t1=0.0))
    both(samplers, INV, 'rtol and atol must be > 0', span=span(rtol=-1.0))
    both(samplers, INV, 'first_step must be >= 1 (got 0)', first_step=0)
    both(samplers, INV, 'first_chain must be >= 0', first_chain=-1)
    both(samplers, INV, 'init must be 0 or 1', init=2)
    both(samplers, INV, 'noise_mode must be 0, 1 or 2', noise_mode=3)
    both(samplers, INV, 'noise_mode must be 0, 1 or 2', noise_mode=-1)
    for name in ('state', 'samples', 'log_p'):
        both(samplers, INV, 'NULL pointer', **{name: None})
    both(samplers, INV, 'NULL host settings', step=None)
    both(samplers, INV, 'NULL host settings', whiten=None)
    for mode in (0, 2):
        both(samplers, INV, 'NULL noise arrays (z, log_u): noise_mode %d needs them' % mode, noise_mode=mode, z=None)
        both(samplers, INV, 'NULL noise arrays (z, log_u): noise_mode %d needs them' % mode, noise_mode=mode,
             log_u=None)
    both(samplers, INV, "noise rows [-1, 3) outside the noise arrays' 8 rows", noise_row0=-1)
    both(samplers, INV, "noise rows [0, 4) outside the noise arrays' 0 rows", noise_ld=0)
    both(samplers, INV, "noise rows [5, 9) outside the noise arrays' 8 rows", noise_row0=5)
    both(samplers, INV, 'noise arrays must be aligned (z: 16 bytes, log_u: 8)', z=P8)
    both(samplers, INV, 'noise arrays must be aligned (z: 16 bytes, log_u: 8)', log_u=P4)
    both(samplers, INV, 'state and samples must be 16-byte aligned', state=P8)
    both(samplers, INV, 'state and samples must be 16-byte aligned', samples=P8)
    for name in ('log_p', 't_eval', 'y_obs'):
        both(samplers, INV, 'log_p, t_eval and y_obs must be 8-byte aligned', **{name: P4})
    both(samplers, INV, "output rows [0, 4) outside the output arrays' 0 rows", out_ld=0)
    both(samplers, INV, "output rows [5, 9) outside the output arrays' 8 rows", out_row0=5)
    both(samplers, INV, "output rows [-1, 4) outside the output arrays' 8 rows", init=1)
    both(samplers, INV, 'init needs first_step = 1', init=1, out_row0=1, first_step=2)
    for j, bad in ((0, 0.0), (1, math.inf), (2, math.nan), (3, -0.1)):
        v = [0.1] * 4 + [0.005] * 4 + [50.0] * 4
        v[j] = bad
        both(samplers[:2], INV, 'step size %d must be finite and > 0' % j, step=host(f64, v[:4]))
        row('st_lv_mala_wave', INV, 'step size %d must be finite and > 0' % j, step=host(f64, v))
    # order: device noise needs no arrays; the noise checks before the other alignments
    both(samplers, INV, 'state and samples must be 16-byte aligned', noise_mode=1, z=None, log_u=None, state=P8)
    both(samplers, INV, 'noise arrays must be aligned', z=P8, state=P8)
    both(samplers, INV, 'chains must be >= 1', chains=0, t_n=0)
    both(samplers, INV, 't_n must be >= 1', t_n=0, first_step=0)
    e = 'st_lv_mala_wave'
    for name in ('grad', 'drift_clip', 'cov_inv'):
        row(e, INV, 'NULL pointer (grad, drift_clip, cov_inv)', **{name: None})
    row(e, INV, 'grad must be 16-byte aligned', grad=P8)
    row(e, INV, 'h and w of component 1 must be finite and > 0',
        step=host(f64, [0.1] * 4 + [.005, 0, .005, .005] + [50.0] * 4))
    row(e, INV, 'h and w of component 2 must be finite and > 0',
        step=host(f64, [0.1] * 4 + [.005] * 4 + [50, 50, math.inf, 50]))
    row(e, INV, 'drift clip 0 must be > 0', drift_clip=host(f64, [0.0, 1.0, 1.0, 1.0]))
    row(e, INV, 'drift clip 3 must be > 0', drift_clip=host(f64, [1.0, 1.0, 1.0, math.nan]))
    row(e, INV, 'step size 0 must be finite', step=host(f64, [0.0] * 12), grad=None)   # the shared checks first

    # ---- energy distance and the set-batched forms -----------------------------------------------------
    dc = dict(a=P, lda=16, na=10, b=P, ldb=16, nb=10, d=4, b_begin=0, b_end=10, triangle=0, out=P)
    base('st_distance_colsum', **dc, stream=None)
    base('st_distance_colsum_ws', **dc, workspace=None, workspace_bytes=0, stream=None)
    dcs = ['st_distance_colsum', 'st_distance_colsum_ws']
    both(dcs, OK, '', na=0, a=None, b=None, out=None, d=0)
    for name in ('a', 'b', 'out'):
        both(dcs, INV, 'NULL pointer', **{name: None})
    both(dcs, UNS, 'unsupported d = 0', d=0)
    both(dcs, UNS, 'unsupported d = 129', d=129)
    for kw in (dict(na=-1), dict(nb=-1, b_end=0), dict(lda=8), dict(ldb=8), dict(lda=12), dict(ldb=12)):
        both(dcs, INV, 'bad sizes (ld must be a multiple of 8 and >= the row count)', **kw)
    both(dcs, INV, 'need 0 <= b_begin <= b_end <= nb', b_begin=-1)
    both(dcs, INV, 'need 0 <= b_begin <= b_end <= nb', b_begin=3, b_end=2)
    both(dcs, INV, 'need 0 <= b_begin <= b_end <= nb', b_end=11)
    both(dcs, INV, 'triangle=1 needs A and B to be the same array', triangle=1, b=Q)
    both(dcs, INV, 'triangle=1 needs A and B to be the same array', triangle=1, lda=24)
    both(dcs, UNS, 'na too large', na=1 << 40, lda=1 << 40)
    row('st_distance_colsum_ws', INV, 'workspace must be 16-byte aligned', workspace=P8, workspace_bytes=1 << 20)
    both(dcs, UNS, 'unsupported d = 129', d=129, na=-1)              # order: d before the sizes
    OFF = host(i64, [0, 3, 5])
    ks_ws = lib.st_ksd_sets_workspace_bytes(5, 2, 4)
    ds_ws = lib.st_distance_sets_workspace_bytes(5, 2, 4)
    assert ks_ws > 0 and ds_ws > 0
    base('st_ksd_sets', **pm, rows=P, set_offsets=OFF, n_sets=2, ks_out=P, csum_out=P, workspace=P,
         workspace_bytes=ks_ws, stream=None)
    base('st_distance_sets', p=P, ldp=16, n=10, d=4, rows=P, set_offsets=OFF, n_sets=2, self_out=P, row_values=None,
         segsum_out=None, workspace=P, workspace_bytes=ds_ws, stream=None)
    sets = ['st_ksd_sets', 'st_distance_sets']
    both(sets, INV, 'n_sets must be >= 0 (got -1)', n_sets=-1)
    both(sets, INV, 'rows/set_offsets pointer is NULL', rows=None)
    both(sets, INV, 'rows/set_offsets pointer is NULL', set_offsets=None)
    both(sets, INV, 'rows/set_offsets must be 8-byte aligned', rows=P4)
    both(sets, INV, 'rows/set_offsets must be 8-byte aligned', set_offsets=P4)
    both(sets, INV, 'set_offsets[0] must be 0 (got 1)', set_offsets=host(i64, [1, 3, 5]))
    both(sets, INV, 'set_offsets must not decrease', set_offsets=host(i64, [0, 3, 2]))
    both(sets, INV, 'empty index set', set_offsets=host(i64, [0, 3, 3]))
    both(sets, UNS, 'too many sets / column blocks for one grid', n_sets=1, set_offsets=host(i64, [0, 1 << 50]))
    both(sets, INV, 'NULL output/workspace', workspace=None)
    both(sets, INV, 'workspace 16-byte aligned', workspace=P8)
    row('st_ksd_sets', OK, '', n_sets=0, x=None, g=None, rows=None, set_offsets=None, ks_out=None, workspace=None)
    row('st_ksd_sets', INV, 'sample/gradient pointer is NULL', x=None)
    row('st_ksd_sets', UNS, 'exceeds the supported maximum', d=129)
    row('st_ksd_sets', INV, 'NULL output/workspace', ks_out=None)
    row('st_ksd_sets', INV, 'outputs must be 8-byte and the workspace 16-byte aligned', ks_out=P4)
    row('st_ksd_sets', INV, 'outputs must be 8-byte and the workspace 16-byte aligned', csum_out=P4)
    row('st_ksd_sets', INV, 'workspace too small', workspace_bytes=ks_ws - 1)
    row('st_ksd_sets', INV, 'sample/gradient pointer is NULL', x=None, rows=None)   # order: problem, sets, outputs
    row('st_ksd_sets', INV, 'rows/set_offsets pointer is NULL', rows=None, ks_out=None)
    e = 'st_distance_sets'
    row(e, OK, '', n_sets=0, p=None, rows=None, set_offsets=None, self_out=None, workspace=None, d=0)
    row(e, INV, 'point pointer is NULL', p=None)
    row(e, INV, 'd must be >= 1 (got 0)', d=0)
    row(e, UNS, 'd = 129 exceeds the supported maximum 128', d=129)
    for kw in (dict(n=0), dict(ldp=8), dict(ldp=12)):
        row(e, INV, 'bad sizes (ld must be a multiple of 8 and >= the row count)', **kw)
    row(e, INV, 'device arrays must be 16-byte aligned', p=P8)
    row(e, INV, 'NULL output/workspace', self_out=None)
    row(e, INV, 'row_values and segsum_out go together (both or neither)', row_values=P)
    row(e, INV, 'row_values and segsum_out go together (both or neither)', segsum_out=P)
    row(e, INV, 'arrays must be 8-byte and the workspace 16-byte aligned', self_out=P4)
    row(e, INV, 'arrays must be 8-byte and the workspace 16-byte aligned', row_values=P4, segsum_out=P)
    row(e, INV, 'arrays must be 8-byte and the workspace 16-byte aligned', row_values=P, segsum_out=P4)
    row(e, INV, 'workspace too small', workspace_bytes=ds_ws - 1)
    row(e, INV, 'point pointer is NULL', p=None, rows=None)

    # ---- layout, distances, repeated rows --------------------------------------------------------------
    base('st_layout_soa', rowmajor=P, n=10, d=4, ld=16, soa=P, stream=None)
    base('st_layout_soa_scaled', rowmajor=P, n=10, d=4, ld=16, scale=P, divide=1, soa=P, stream=None)
    lay = ['st_layout_soa', 'st_layout_soa_scaled']
    both(lay, INV, 'NULL pointer', rowmajor=None)
    both(lay, INV, 'NULL pointer', soa=None)
    row('st_layout_soa_scaled', INV, 'NULL pointer', scale=None)
    for kw in (dict(n=0), dict(d=0), dict(ld=9)):
        both(lay, INV, 'bad sizes', **kw)
    base('st_pdist', rows=P, k=10, d=4, out=P, stream=None)
    row('st_pdist', INV, 'NULL pointer', rows=None)
    row('st_pdist', INV, 'NULL pointer', out=None)
    for kw in (dict(k=1), dict(k=65536), dict(d=0), dict(d=129)):
        row('st_pdist', INV, 'need 2 <= k <= 65535 rows and 1 <= d <= 128', **kw)
    run_ws = lib.st_run_workspace_bytes(10)
    rp = dict(x=P, g=P, w=None, n=10, d=4, ld=16)
    base('st_run_starts', **rp, starts_out=P, workspace=P, workspace_bytes=run_ws, stream=None)
    base('st_run_compact', **rp, starts=P, workspace=P, count=5, ld_out=8, x_out=P, g_out=P, w_out=None, rows_out=P,
         stream=None)
    runs = ['st_run_starts', 'st_run_compact']
    both(runs, INV, 'sample/gradient pointer is NULL', g=None)
    both(runs, UNS, 'exceeds the supported maximum', d=129)
    both(runs, UNS, 'n >= 2^31 rows', n=1 << 31, ld=1 << 31)
    row('st_run_starts', INV, 'NULL output/workspace', starts_out=None)
    row('st_run_starts', INV, 'NULL output/workspace', workspace=None)
    row('st_run_starts', INV, 'workspace must be 16-byte aligned', workspace=P8)
    row('st_run_starts', INV, 'workspace too small (%d < %d)' % (run_ws - 1, run_ws), workspace_bytes=run_ws - 1)
    for name in ('starts', 'workspace', 'x_out', 'g_out', 'rows_out'):
        row('st_run_compact', INV, 'NULL input/output', **{name: None})
    row('st_run_compact', INV, 'NULL input/output', w=P)              # weights without w_out
    for kw in (dict(count=0), dict(count=11), dict(ld_out=4), dict(ld_out=12)):
        row('st_run_compact', INV, 'need 1 <= count <= n and ld_out >= count, a multiple of 8', **kw)
    return rows, keep


def test_every_check_before_the_first_hip_call(lib):
    """Two rows (st_greedy_step / st_greedy_step_exchange, 'workspace too small') expect the two sizes that the
    other five greedy entry points always printed; every other row is what the entry points returned before
    their checks were shared."""
    rows, keep = _table(lib)
    bad = []
    for entry, args, code, msg in rows:
        got = getattr(lib, entry)(*args)
        err = lib.st_last_error().decode()
        if got != code or msg not in err:
            bad.append((entry, args, 'expected', code, msg, 'got', got, err))
    assert not bad, '%d of %d rows:\n%s' % (len(bad), len(rows), '\n'.join(map(repr, bad)))
    del keep


# st_tune keys by owner; two values each accepts (the test writes one that differs from the current value)
PERSISTENT = {3: (4, 8), 4: (512, 256), 5: (7, 9), 9: (256, 512), 10: (2, 4), 12: (8, 9), 15: (1, 0), 16: (5, 6),
              19: (0, 1), 23: (7, 9)}
GREEDY = {0: (128, 64), 1: (2, 4), 2: (1, 0), 6: (512, 64), 11: (0, 1), 20: (0, 1), 22: (0, 1)}
# key -> the value that restores its default; 8: the persistent engine's, accepted (1 / -1) and not kept
WRITE_ONLY = {7: 0, 8: -1, 13: -1, 14: -1, 17: -1, 18: -1, 24: -1}
READ_ONLY = range(100, 111)
UNKNOWN = (-1, 21, 25, 99, 111, 999)


def test_tune_keys_reach_their_owner(lib):
    """Every key st_tune / st_tune_get know: the readable ones round-trip, the last-plan keys are read-only
    (-1 on a thread that has planned nothing), the write-only ones read INT32_MIN, anything else is refused."""
    readable = {**PERSISTENT, **GREEDY}
    before = {k: lib.st_tune_get(k) for k in readable}
    assert INT32_MIN not in before.values()
    try:
        for k, (v, other) in readable.items():
            v = other if v == before[k] else v
            assert lib.st_tune(k, v) == OK, (k, v)
            assert lib.st_tune_get(k) == v, k
        for k, v in WRITE_ONLY.items():
            assert lib.st_tune(k, v) == OK, k
            assert lib.st_tune_get(k) == INT32_MIN, k
        assert lib.st_tune(8, 1) == OK and lib.st_tune(8, 2) == INV
        for k in READ_ONLY:
            assert lib.st_tune(k, 1) == INV and lib.st_tune(k, -1) == INV, k
            assert ('bad tuning key/value %d=-1' % k).encode() in lib.st_last_error()
        fresh = {}
        th = threading.Thread(target=lambda: fresh.update({k: lib.st_tune_get(k) for k in READ_ONLY}))
        th.start()
        th.join()
        assert fresh == {k: -1 for k in READ_ONLY}
        for k in UNKNOWN:
            assert lib.st_tune(k, 1) == INV and lib.st_tune(k, -1) == INV, k
            assert ('bad tuning key/value %d=-1' % k).encode() in lib.st_last_error()
            assert lib.st_tune_get(k) == INT32_MIN, k
    finally:
        # -1 restores a key's default; the two grid caps (keys 0, 6) have no -1 and take their old value back
        for k, v in WRITE_ONLY.items():
            assert lib.st_tune(k, v) == OK, k
        for k in readable:
            assert lib.st_tune(k, -1) == OK or k in (0, 6), k
            if lib.st_tune_get(k) != before[k]:
                assert lib.st_tune(k, before[k]) == OK, k
    assert {k: lib.st_tune_get(k) for k in readable} == before
