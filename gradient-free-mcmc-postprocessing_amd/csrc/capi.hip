// C ABI (include/stein_thinning_hip.h): argument validation, workspace carving, launch sequencing.
// No allocation, no synchronisation: every entry point only enqueues work on the caller's stream.
// Helpers (checks, argument builders, launch sequences, the bodies twin entry points share) come first, in the
// anonymous namespace; extern "C" holds the entry points alone.  The ORDER of an entry point's checks is part of
// the ABI: a call that violates two gets the first one's code.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../include/stein_thinning_hip.h"
#include "stein_internal.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return ST_OK;
    return fail(ST_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

namespace st {
// st_last_error text for entry points defined in other translation units (prep_upload.cpp)
int report_error(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace st

namespace {

// st_tune: who keeps a key's value: the greedy engine, the persistent engine, or a write-only setter of one key.
// Every key number is named here and nowhere else in this file
struct TuneKey {
    enum { kGreedy, kPersistent, kSetter } owner;
    int (*set)(int);   // kSetter only
    bool read_only;
};

TuneKey tune_key(int32_t key) {
    switch (key) {
        case 7: return {TuneKey::kSetter, st::proxy_tune, false};
        case 13: return {TuneKey::kSetter, st::dist_tune, false};
        case 14: return {TuneKey::kSetter, st::dist_units_tune, false};
        case 17: return {TuneKey::kSetter, st::lv_tune, false};
        case 18: return {TuneKey::kSetter, st::lv_pieces_tune, false};
        case 24: return {TuneKey::kSetter, st::kde_t_tune, false};
        case 3: case 4: case 5: case 8: case 9: case 10: case 12: case 15: case 16: case 19: case 23:
            return {TuneKey::kPersistent, nullptr, false};
        default: {   // 100 .. 110: the calling thread's last plan; any other key is the greedy engine's to judge
            const bool plan = key >= 100 && key <= 110;
            return {plan ? TuneKey::kPersistent : TuneKey::kGreedy, nullptr, plan};
        }
    }
}

int check_problem(const double* x, const double* g, const double* w, int64_t n, int32_t d,
                  int64_t ld) {
    if (!x || !g) return fail(ST_ERR_INVALID, "sample/gradient pointer is NULL");
    if (n < 1) return fail(ST_ERR_INVALID, "n must be >= 1 (got %lld)", (long long)n);
    if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1 (got %d)", d);
    if (d > st::kMaxDim)
        return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds the supported maximum %d", d, st::kMaxDim);
    if (ld < n || (ld & 7))
        return fail(ST_ERR_INVALID, "ld must be a multiple of 8 and >= n (n=%lld, ld=%lld)",
                    (long long)n, (long long)ld);
    if (!aligned16(x) || !aligned16(g) || (w && !aligned16(w)))
        return fail(ST_ERR_INVALID, "device arrays must be 16-byte aligned");
    return ST_OK;
}

// dense preconditioner: after check_problem -- d within the dense kernels' widths, the (d, d) array given
int check_dense(const double* linv, int32_t d) {
    if (d > st::kMaxDenseDim)
        return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds the dense-preconditioner maximum %d", d, st::kMaxDenseDim);
    if (!linv) return fail(ST_ERR_INVALID, "linv pointer is NULL");
    if (!aligned16(linv)) return fail(ST_ERR_INVALID, "linv must be 16-byte aligned");
    return ST_OK;
}

// workspace layout: [control block (persistent kernel counters/status)][two ping-pong banks of
// per-block candidate records, kMaxBlocks x stride doubles each]
int64_t greedy_ws_bytes(int32_t d) {
    const int64_t steps = st::kWsControlBytes + 2 * (int64_t)st::kMaxBlocks * st::cand_stride(d) * 8;
    const int64_t persist = st::persistent_ws_max_bytes();
    return steps > persist ? steps : persist;
}

// output and workspace of a greedy entry point (d: checked before).  out: idx_out, or the candidate array of a
// single-step entry point (which needs idx_out for t > 0 only and tests it itself); who: "" or
// st_greedy_batch's "problem q: "
int check_greedy_buffers(const char* who, const void* out, const double* a_work, const void* workspace,
                         int64_t workspace_bytes, int32_t d) {
    if (!out || !a_work || !workspace) return fail(ST_ERR_INVALID, "%sNULL output/workspace", who);
    if (!aligned16(a_work) || !aligned16(workspace))
        return fail(ST_ERR_INVALID, "%sa_work/workspace must be 16-byte aligned", who);
    if (workspace_bytes < greedy_ws_bytes(d))
        return fail(ST_ERR_INVALID, "%sworkspace too small (%lld < %lld)", who, (long long)workspace_bytes,
                    (long long)greedy_ws_bytes(d));
    return ST_OK;
}

int check_peers(void* const* peer_mailboxes, int32_t nranks, int32_t rank) {
    if (nranks < 2 || nranks > st::kMailboxRanks)
        return fail(ST_ERR_INVALID, "nranks must be in [2, %d]", st::kMailboxRanks);
    if (rank < 0 || rank >= nranks) return fail(ST_ERR_INVALID, "rank out of range");
    if (!peer_mailboxes) return fail(ST_ERR_INVALID, "NULL peer mailbox table");
    for (int r = 0; r < nranks; ++r)
        if (!peer_mailboxes[r] || !aligned16(peer_mailboxes[r]))
            return fail(ST_ERR_INVALID, "peer mailbox %d is NULL or misaligned", r);
    return ST_OK;
}

// set-batched forms: the checks both entry points share, after the problem's own: rows, offsets, sizes
int check_sets(const int64_t* rows, const int64_t* set_offsets, int64_t n_sets) {
    if (!rows || !set_offsets) return fail(ST_ERR_INVALID, "rows/set_offsets pointer is NULL");
    if (!aligned8(rows) || !aligned8(set_offsets)) return fail(ST_ERR_INVALID, "rows/set_offsets must be 8-byte aligned");
    switch (st::sets_check_offsets(set_offsets, n_sets)) {
        case 1: return fail(ST_ERR_INVALID, "set_offsets[0] must be 0 (got %lld)", (long long)set_offsets[0]);
        case 2: return fail(ST_ERR_INVALID, "set_offsets must not decrease");
        case 3: return fail(ST_ERR_INVALID, "empty index set");
        default: break;
    }
    if (n_sets > 0x7FFFFFFFll || st::sets_item_count(set_offsets, n_sets) > 0x7FFFFFFFll)
        return fail(ST_ERR_UNSUPPORTED, "too many sets / column blocks for one grid");
    return ST_OK;
}

double* bank(void* ws, int32_t d, int b) {
    return reinterpret_cast<double*>(static_cast<char*>(ws) + st::kWsControlBytes) +
           (int64_t)b * st::kMaxBlocks * st::cand_stride(d);
}

st::GreedyArgs make_args(const double* x, const double* g, const double* w, int64_t n, int32_t d,
                         int64_t ld, double l, double tr, double* A) {
    st::GreedyArgs a{};
    a.x = x; a.g = g; a.w = w; a.A = A;
    a.n = n; a.ld = ld; a.d = d; a.l = l; a.tr = tr;
    a.row_offset = 0;
    a.rec_stride = st::cand_stride(d);
    a.compact = st::arith_compact();
    return a;
}

// one step of a run that the caller distributes over ranks (st_greedy_step, st_greedy_step_exchange): the
// shard at row_offset reads the ranks' records of step t - 1 and leaves its blocks' records in bank 0
st::GreedyArgs step_args(const double* x, const double* g, const double* w, int64_t n, int32_t d, int64_t ld,
                         double l, double tr, int64_t row_offset, int64_t t, const double* recs_in, int32_t nranks,
                         uint32_t* idx_out, double* a_work, void* workspace) {
    st::GreedyArgs a = make_args(x, g, w, n, d, ld, l, tr, a_work);
    a.row_offset = row_offset;
    a.t = t;
    a.recs_in = recs_in;
    a.nrecs_in = nranks;
    a.recs_out = bank(workspace, d, 0);
    a.idx_out = idx_out;
    return a;
}

// peers: the ranks' mailboxes, or NULL (a plan-only query: no peer is touched)
st::RankSpec rank_spec(int64_t row_begin, int64_t row_end, int32_t rank, int32_t nranks, uint64_t seq_base,
                       void* inbox, void* const* peers) {
    st::RankSpec rs{};
    rs.row_begin = row_begin;
    rs.row_end = row_end;
    rs.rank = rank;
    rs.nranks = nranks;
    rs.seq_base = seq_base;
    rs.inbox = static_cast<uint64_t*>(inbox);
    for (int r = 0; peers && r < nranks; ++r) rs.peer[r] = static_cast<uint64_t*>(peers[r]);
    return rs;
}

st::MailboxPeers mailbox_peers(void* const* peer_mailboxes, int32_t nranks) {
    st::MailboxPeers peers{};
    for (int r = 0; r < nranks; ++r) peers.p[r] = static_cast<uint64_t*>(peer_mailboxes[r]);
    return peers;
}

// a run starts: no near-tie word of an earlier run may survive (the step kernels run unguarded: -2)
int reset_near_tie(void* workspace, hipStream_t s) {
    return hip_check(hipMemsetAsync(static_cast<char*>(workspace) + st::kWsTieOff, 0,
                                    (size_t)(st::kWsBoundsOff + 40 - st::kWsTieOff), s),
                     "near-tie words reset");
}

// steps [t_begin, t_end) of a run of n_points, one launch each, through the two record banks; then the
// finalize launch if that completes the run.  Dense preconditioner (a.linv set): its own grid, and its own
// launcher after the diagonal step (t = 0, shared)
int run_steps(st::GreedyArgs& a, void* workspace, int64_t t_begin, int64_t t_end, int64_t n_points,
              hipStream_t s) {
    const bool dense = a.linv != nullptr;
    const int blocks = dense ? st::greedy_dense_blocks(a.n, a.d) : st::greedy_blocks(a.n, a.d);
    int rc = t_begin == 0 ? reset_near_tie(workspace, s) : ST_OK;
    if (rc) return rc;
    for (int64_t t = t_begin; t < t_end; ++t) {
        a.t = t;
        a.recs_in = bank(workspace, a.d, (int)((t + 1) & 1));
        a.nrecs_in = blocks;
        a.recs_out = bank(workspace, a.d, (int)(t & 1));
        rc = hip_check(dense && t > 0 ? st::launch_greedy_step_dense(a, blocks, s)
                                      : st::launch_greedy_step(a, t == 0, blocks, s),
                       dense ? "dense greedy step launch" : "greedy step launch");
        if (rc) return rc;
    }
    if (t_end < n_points || t_end == t_begin) return ST_OK;
    return hip_check(st::launch_greedy_finalize(bank(workspace, a.d, (int)((n_points - 1) & 1)), blocks,
                                                a.rec_stride, a.idx_out, n_points - 1, s),
                     "greedy finalize launch");
}

// diagonal / dense twins: dense = the (d, d) array linv and l = 0; else linv = NULL and the scale l
int kernel_pairs(const double* x, const double* g, const double* w, int64_t ld, int32_t d, bool dense,
                 const double* linv, double l, double tr, const int64_t* i1, const int64_t* i2, int64_t n_pairs,
                 double* out, void* stream) {
    if (n_pairs == 0) return ST_OK;
    if (!x || !g) return fail(ST_ERR_INVALID, "sample/gradient pointer is NULL");
    if (dense) {
        if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1 (got %d)", d);
        int rc = check_dense(linv, d);
        if (rc) return rc;
    } else if (d < 1 || d > st::kMaxDim) {
        return fail(ST_ERR_UNSUPPORTED, "unsupported d = %d", d);
    }
    if (ld < 1) return fail(ST_ERR_INVALID, "ld must be >= 1");
    if (n_pairs < 0 || !i1 || !i2 || !out) return fail(ST_ERR_INVALID, "bad pair list");
    return hip_check(st::launch_pairs(st::PairArgs{x, g, w, ld, d, l, tr, linv}, i1, i2, n_pairs, out,
                                      static_cast<hipStream_t>(stream)),
                     dense ? "dense pairs launch" : "pairs launch");
}

int ksd_cumulative(const double* x, const double* g, const double* w, int64_t m, int64_t ld, int32_t d, bool dense,
                   const double* linv, double l, double tr, double* ks_out, void* workspace,
                   int64_t workspace_bytes, void* stream) {
    int rc = check_problem(x, g, w, m, d, ld);
    if (rc) return rc;
    if (dense) rc = check_dense(linv, d);
    if (rc) return rc;
    if (!ks_out || !workspace) return fail(ST_ERR_INVALID, "NULL output/workspace");
    if (workspace_bytes < st_ksd_workspace_bytes(m, ld))
        return fail(ST_ERR_INVALID, "workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const st::PairArgs p{x, g, w, ld, d, l, tr, linv};
    double* csum = static_cast<double*>(workspace);
    rc = hip_check(st::launch_ksd_colsum(p, m, 0, m, csum, s),
                   dense ? "dense ksd column-sum launch" : "ksd column-sum launch");
    if (rc) return rc;
    // the finish reads the diagonal only: k(x, x) depends on tr, not on L
    return hip_check(st::launch_ksd_finish(p, m, csum, ks_out, s), "ksd finish launch");
}

int ksd_colsum(const double* x, const double* g, const double* w, int64_t n, int64_t ld, int32_t d, bool dense,
               const double* linv, double l, double tr, int64_t row_begin, int64_t row_end, double* csum_out,
               void* stream) {
    int rc = check_problem(x, g, w, n, d, ld);
    if (rc) return rc;
    if (dense) rc = check_dense(linv, d);
    if (rc) return rc;
    if (!csum_out) return fail(ST_ERR_INVALID, "NULL output");
    if (row_begin < 0 || row_end < row_begin || row_end > n)
        return fail(ST_ERR_INVALID, "need 0 <= row_begin <= row_end <= n");
    return hip_check(st::launch_ksd_colsum(st::PairArgs{x, g, w, ld, d, l, tr, linv}, n, row_begin, row_end,
                                           csum_out, static_cast<hipStream_t>(stream)),
                     dense ? "dense ksd column-sum launch" : "ksd column-sum launch");
}

int kmat(const double* x, const double* g, const double* w, int64_t k, int64_t ld, int32_t d, bool dense,
         const double* linv, double l, double tr, double* kmat_out, void* stream) {
    int rc = check_problem(x, g, w, k, d, ld);
    if (rc) return rc;
    if (dense) rc = check_dense(linv, d);
    if (rc) return rc;
    if (!kmat_out) return fail(ST_ERR_INVALID, "NULL output");
    if ((k + 63) / 64 > 65535) return fail(ST_ERR_UNSUPPORTED, "k too large for the tiled grid");
    return hip_check(st::launch_kmat(st::PairArgs{x, g, w, ld, d, l, tr, linv}, nullptr, k, kmat_out,
                                     static_cast<hipStream_t>(stream)),
                     dense ? "dense kmat launch" : "kmat launch");
}

// kernel densities: df = NULL for the Gaussian kernel, which tests d before the sizes (Student-t: after df)
int kde_logpdf_grad(const double* p_soa, int64_t ldp, int64_t n, const double* log_weights,
                    double log_weight_uniform, const double* q_soa, int64_t ldq, int64_t m, int32_t d,
                    const double* df, double log_norm, const double* whiten, double* log_q_out, double* grad_out,
                    void* workspace, int64_t workspace_bytes, void* stream) {
    if (m == 0) return ST_OK;
    if (!p_soa || !q_soa || !whiten || !log_q_out || !grad_out) return fail(ST_ERR_INVALID, "NULL pointer");
    const bool bad_d = d < 1 || d > st::kMaxDim;
    if (!df && bad_d) return fail(ST_ERR_UNSUPPORTED, "unsupported d = %d", d);
    if (n < 1 || m < 0 || ldp < n || ldq < m) return fail(ST_ERR_INVALID, "bad sizes (need n >= 1, ld >= count)");
    if (df && (!(*df > 0.0) || *df == INFINITY)) return fail(ST_ERR_INVALID, "df must be finite and > 0");
    if (bad_d) return fail(ST_ERR_UNSUPPORTED, "unsupported d = %d", d);
    if ((m + 255) / 256 > 0x7FFFFFFFll) return fail(ST_ERR_UNSUPPORTED, "m too large");
    if (workspace_bytes < st::kde_workspace_bytes(m, d) || (st::kde_workspace_bytes(m, d) > 0 && !workspace))
        return fail(ST_ERR_INVALID, "workspace too small (%lld < %lld)", (long long)workspace_bytes,
                    (long long)st::kde_workspace_bytes(m, d));
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* ws = static_cast<double*>(workspace);
    if (df)
        return hip_check(st::launch_kde_t(p_soa, ldp, n, log_weights, log_weight_uniform, q_soa, ldq, m, d, *df,
                                          log_norm, whiten, log_q_out, grad_out, ws, s),
                         "kde_t launch");
    return hip_check(st::launch_kde(p_soa, ldp, n, log_weights, log_weight_uniform, q_soa, ldq, m, d, log_norm,
                                    whiten, log_q_out, grad_out, ws, s),
                     "kde launch");
}

// accepted RK45 steps recorded per point by the two-phase gradient (typical: ~32 at the reference's
// tolerances); a point that takes more is recomputed by the single-phase kernel
constexpr int kLvStepCap = 64;

// the part of their arguments that every LV entry point shares, checked and stored in one place; whiten
// may be NULL where the kernels do not read U (the gradient)
int lv_problem(st::LvProblem& p, const double* t_eval, int32_t t_n, const double* y_obs,
               const double* span_u0_tol, const double* whiten, double c_log, double norm_logc,
               int64_t max_steps, bool need_data) {
    if (t_n < 1) return fail(ST_ERR_INVALID, "t_n must be >= 1");
    if (!span_u0_tol) return fail(ST_ERR_INVALID, "NULL solver settings");
    if (max_steps < 1) return fail(ST_ERR_INVALID, "max_steps must be >= 1");
    if (need_data && (!t_eval || !y_obs)) return fail(ST_ERR_INVALID, "NULL pointer");
    if (!(span_u0_tol[1] > span_u0_tol[0])) return fail(ST_ERR_INVALID, "need t1 > t0 (forward integration)");
    if (!(span_u0_tol[4] > 0) || !(span_u0_tol[5] > 0)) return fail(ST_ERR_INVALID, "rtol and atol must be > 0");
    p.t_eval = t_eval;
    p.t_n = t_n;
    p.y_obs = y_obs;
    p.t0 = span_u0_tol[0];
    p.t1 = span_u0_tol[1];
    p.u0[0] = span_u0_tol[2];
    p.u0[1] = span_u0_tol[3];
    p.rtol = span_u0_tol[4];
    p.atol = span_u0_tol[5];
    for (int q = 0; q < 4 && whiten; ++q) p.U[q] = whiten[q];
    p.c_log = c_log;
    p.norm_logc = norm_logc;
    p.max_steps = max_steps;
    return ST_OK;
}

int lv_common(st::LvArgs& a, const double* theta, int64_t n, const double* t_eval, int32_t t_n,
              const double* y_obs, const double* span_u0_tol, const double* whiten, double c_log,
              double norm_logc, int64_t max_steps, double* out, int32_t* status) {
    if (n < 0) return fail(ST_ERR_INVALID, "n must be >= 0");
    int rc = lv_problem(a.p, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc, max_steps, n > 0);
    if (rc) return rc;
    if (n > 0 && (!theta || !out || !status)) return fail(ST_ERR_INVALID, "NULL pointer");
    a.theta = theta;
    a.n = n;
    a.out = out;
    a.status = status;
    return ST_OK;
}

// two_phase: with the step table in the caller's workspace (st_lv_grad_log_posterior_ws)
int lv_grad(const double* theta, int64_t n, const double* t_eval, int32_t t_n, const double* y_obs,
            const double* span_u0_tol, const double* cov_inv, int64_t max_steps, double* grad_out,
            int32_t* status, bool two_phase, void* workspace, int64_t workspace_bytes, void* stream) {
    st::LvArgs a{};
    int rc = lv_common(a, theta, n, t_eval, t_n, y_obs, span_u0_tol, nullptr, 0.0, 0.0, max_steps, grad_out, status);
    if (rc) return rc;
    if (!cov_inv) return fail(ST_ERR_INVALID, "NULL cov_inv");
    for (int q = 0; q < 4; ++q) a.cinv[q] = cov_inv[q];
    if (two_phase) {
        if (n > 0 && !workspace) return fail(ST_ERR_INVALID, "NULL workspace");
        if (workspace_bytes < st::lv_grad_workspace_bytes(n, kLvStepCap))
            return fail(ST_ERR_INVALID, "workspace too small");
        a.step_cap = kLvStepCap;
        a.steps = static_cast<double*>(workspace);
        // the step counts follow the step table, whose bytes are what the capacity adds to the workspace
        a.nsteps = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) +
                                              (st::lv_grad_workspace_bytes(n, kLvStepCap) -
                                               st::lv_grad_workspace_bytes(n, 0)));
    }
    if (n == 0) return ST_OK;
    return hip_check(st::launch_lv(a, true, static_cast<hipStream_t>(stream)), "lv gradient launch");
}

// the LV samplers' common checks (all before any HIP call) and the kernel arguments that LvMcmcArgs and
// LvMalaArgs share, once; step_size: the random walk's step, MALA's eps (checked here, copied by the caller);
// host_step false: the sampler's step sizes are device arrays, which it checks for NULL itself
template <class Args>
int lv_rwmh_args(Args& a, double* state, int64_t chains, int64_t first_chain, int64_t first_step,
                 int64_t steps, int32_t init, const double* step_size, int32_t noise_mode, uint64_t seed,
                 double* z, double* log_u, int64_t noise_ld, int64_t noise_row0, const double* t_eval,
                 int32_t t_n, const double* y_obs, const double* span_u0_tol, const double* whiten,
                 double c_log, double norm_logc, int64_t max_steps, double* samples, double* log_p,
                 int64_t out_ld, int64_t out_row0, bool host_step = true) {
    if (chains < 1) return fail(ST_ERR_INVALID, "chains must be >= 1 (got %lld)", (long long)chains);
    if (steps < 1) return fail(ST_ERR_INVALID, "steps must be >= 1 (got %lld)", (long long)steps);
    int rc = lv_problem(a.p, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc, max_steps, true);
    if (rc) return rc;
    if (first_step < 1) return fail(ST_ERR_INVALID, "first_step must be >= 1 (got %lld)", (long long)first_step);
    if (first_chain < 0) return fail(ST_ERR_INVALID, "first_chain must be >= 0");
    if (init != 0 && init != 1) return fail(ST_ERR_INVALID, "init must be 0 or 1");
    if (noise_mode < 0 || noise_mode > 2) return fail(ST_ERR_INVALID, "noise_mode must be 0, 1 or 2");
    if (!state || !samples || !log_p) return fail(ST_ERR_INVALID, "NULL pointer");
    if ((host_step && !step_size) || !whiten) return fail(ST_ERR_INVALID, "NULL host settings");
    if (noise_mode != 1) {
        if (!z || !log_u)
            return fail(ST_ERR_INVALID, "NULL noise arrays (z, log_u): noise_mode %d needs them", noise_mode);
        if (noise_row0 < 0 || noise_ld < 1 || noise_row0 > noise_ld - steps)
            return fail(ST_ERR_INVALID, "noise rows [%lld, %lld) outside the noise arrays' %lld rows",
                        (long long)noise_row0, (long long)(noise_row0 + steps), (long long)noise_ld);
        if (!aligned16(z) || !aligned8(log_u))
            return fail(ST_ERR_INVALID, "noise arrays must be aligned (z: 16 bytes, log_u: 8)");
    }
    if (!aligned16(state) || !aligned16(samples))
        return fail(ST_ERR_INVALID, "state and samples must be 16-byte aligned");
    if (!aligned8(log_p) || !aligned8(t_eval) || !aligned8(y_obs))
        return fail(ST_ERR_INVALID, "log_p, t_eval and y_obs must be 8-byte aligned");
    if (out_ld < 1 || out_row0 < init || out_row0 > out_ld - steps)
        return fail(ST_ERR_INVALID, "output rows [%lld, %lld) outside the output arrays' %lld rows",
                    (long long)(out_row0 - init), (long long)(out_row0 + steps), (long long)out_ld);
    if (init && first_step != 1) return fail(ST_ERR_INVALID, "init needs first_step = 1");
    for (int j = 0; host_step && j < 4; ++j)
        if (!isfinite(step_size[j]) || !(step_size[j] > 0))
            return fail(ST_ERR_INVALID, "step size %d must be finite and > 0 (got %g)", j, step_size[j]);
    a.state = state;
    a.chains = chains;
    a.first_chain = first_chain;
    a.first_step = first_step;
    a.steps = steps;
    a.init = init;
    a.noise_mode = noise_mode;
    a.seed = seed;
    a.z = z;
    a.log_u = log_u;
    a.noise_ld = noise_ld;
    a.noise_row0 = noise_row0;
    a.samples = samples;
    a.log_p = log_p;
    a.out_ld = out_ld;
    a.out_row0 = out_row0;
    return ST_OK;
}

// the random-walk sampler in either layout: launch = one chain per thread, or one wave per chain
int lv_rwmh(hipError_t (*launch)(const st::LvMcmcArgs&, hipStream_t), const char* what, double* state,
            int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps, int32_t init,
            const double* step_size, int32_t noise_mode, uint64_t seed, double* z, double* log_u, int64_t noise_ld,
            int64_t noise_row0, const double* t_eval, int32_t t_n, const double* y_obs, const double* span_u0_tol,
            const double* whiten, double c_log, double norm_logc, int64_t max_steps, double* samples,
            double* log_p, int64_t out_ld, int64_t out_row0, void* stream) {
    st::LvMcmcArgs a{};
    int rc = lv_rwmh_args(a, state, chains, first_chain, first_step, steps, init, step_size, noise_mode, seed, z,
                          log_u, noise_ld, noise_row0, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc,
                          max_steps, samples, log_p, out_ld, out_row0);
    if (rc) return rc;
    for (int j = 0; j < 4; ++j) a.step[j] = step_size[j];
    return hip_check(launch(a, static_cast<hipStream_t>(stream)), what);
}

// the gradient samplers' own checks, after lv_rwmh_args and before any HIP call, and the arguments they share, once:
// grad, the clip (clip_name, "drift" or "kick", is its name in the messages) and cov_inv.  hw: MALA's h[4] and w[4],
// a component's checked before its clip.  more: the metric samplers' further device arrays, checked for NULL
// (more_null) after those three and for 8-byte alignment (more_aligned) after grad's.
template <class Args>
int lv_grad_args(Args& a, double* grad, const double* clip, const char* clip_name, const double* cov_inv,
                 const double* hw = nullptr, std::initializer_list<const void*> more = {},
                 const char* more_null = nullptr, const char* more_aligned = nullptr) {
    if (!grad || !clip || !cov_inv) return fail(ST_ERR_INVALID, "NULL pointer (grad, %s_clip, cov_inv)", clip_name);
    for (const void* m : more)
        if (!m) return fail(ST_ERR_INVALID, "%s", more_null);
    if (!aligned16(grad)) return fail(ST_ERR_INVALID, "grad must be 16-byte aligned");
    for (const void* m : more)
        if (!aligned8(m)) return fail(ST_ERR_INVALID, "%s", more_aligned);
    for (int j = 0; j < 4; ++j) {
        if (hw && !(isfinite(hw[j]) && hw[j] > 0 && isfinite(hw[4 + j]) && hw[4 + j] > 0))
            return fail(ST_ERR_INVALID, "h and w of component %d must be finite and > 0 (got %g, %g)", j, hw[j],
                        hw[4 + j]);
        if (!(clip[j] > 0)) return fail(ST_ERR_INVALID, "%s clip %d must be > 0 (got %g)", clip_name, j, clip[j]);
        a.clip[j] = clip[j];
        a.cinv[j] = cov_inv[j];
    }
    a.grad = grad;
    return ST_OK;
}

// the metric samplers' (st_lv_hmc_metric_wave, st_lv_nuts_wave) own checks and the arguments they share, once:
// lv_grad_args with `more` = eps_chain, metric_chol and every per-step output, then the sampler's trajectory-length
// check (length_ok; length_fmt takes `length`), adapt and delta
template <class Args>
int lv_metric_args(Args& a, double* grad, const double* kick_clip, const double* cov_inv, const double* eps_chain,
                   const double* metric_chol, double* accept_stat, double* step_size,
                   std::initializer_list<const void*> more, const char* more_null, const char* more_aligned,
                   bool length_ok, const char* length_fmt, int32_t length, int32_t adapt, double delta) {
    int rc = lv_grad_args(a, grad, kick_clip, "kick", cov_inv, nullptr, more, more_null, more_aligned);
    if (rc) return rc;
    if (!length_ok) return fail(ST_ERR_INVALID, length_fmt, (int)length);
    if (adapt != 0 && adapt != 1) return fail(ST_ERR_INVALID, "adapt must be 0 or 1");
    if (!(delta > 0 && delta < 1)) return fail(ST_ERR_INVALID, "delta must lie in (0, 1) (got %g)", delta);
    a.eps_chain = eps_chain;
    a.metric_chol = metric_chol;
    a.adapt = adapt;
    a.delta = delta;
    a.accept_stat = accept_stat;
    a.step_size = step_size;
    return ST_OK;
}

// st_autocov / st_autocov_workspace_bytes: the shape checks both share (0 ok)
int check_autocov_shape(int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int32_t plan) {
    if (groups < 1) return fail(ST_ERR_INVALID, "groups must be >= 1 (got %lld)", (long long)groups);
    if (S < 1) return fail(ST_ERR_INVALID, "S must be >= 1 (got %lld)", (long long)S);
    if (h < 4) return fail(ST_ERR_INVALID, "h must be >= 4 (got %lld)", (long long)h);
    if (lag0 < 0 || lag0 >= lag1)
        return fail(ST_ERR_INVALID, "need 0 <= lag0 < lag1 (got %lld, %lld)", (long long)lag0, (long long)lag1);
    if (lag1 > h) return fail(ST_ERR_INVALID, "lag1 must be <= h (got %lld > %lld)", (long long)lag1, (long long)h);
    if (plan < 0 || plan > 2) return fail(ST_ERR_INVALID, "plan must be 0 (by shape), 1 (long) or 2 (short)");
    if (S > ((int64_t)1 << 40) / groups || h > ((int64_t)1 << 40) / (groups * S))
        return fail(ST_ERR_UNSUPPORTED, "groups * S * h exceeds 2^40");
    if (plan == 2 && !st::autocov_short_ok(h))
        return fail(ST_ERR_UNSUPPORTED, "the short plan holds a series in LDS: h = %lld is too long", (long long)h);
    if (!st::autocov_grid_ok(groups, S, h, lag0, lag1, plan))
        return fail(ST_ERR_UNSUPPORTED, "too many series or lags for one launch");
    return ST_OK;
}

}  // namespace

extern "C" {

int st_abi_version(void) { return ST_ABI_VERSION; }

const char* st_last_error(void) { return g_err; }

int64_t st_greedy_workspace_bytes(int64_t n, int32_t d, int32_t nranks) {
    (void)n; (void)nranks;
    if (d < 1 || d > st::kMaxDim) return -1;
    return greedy_ws_bytes(d);
}

int st_tune(int32_t key, int32_t value) {
    const TuneKey k = tune_key(key);
    const int rc = k.read_only                       ? -1
                   : k.owner == TuneKey::kSetter     ? k.set(value)
                   : k.owner == TuneKey::kPersistent ? st::persistent_tune(key, value)
                                                     : st::tune(key, value);
    if (rc != 0) return fail(ST_ERR_INVALID, "bad tuning key/value %d=%d", key, value);
    return ST_OK;
}

int32_t st_tune_get(int32_t key) {
    const TuneKey k = tune_key(key);
    if (k.owner == TuneKey::kSetter) return INT32_MIN;   // write-only
    return k.owner == TuneKey::kPersistent ? st::persistent_tune_get(key) : st::tune_get(key);
}

int64_t st_candidate_stride(int32_t d) {
    if (d < 1 || d > st::kMaxDim) return -1;
    return st::cand_stride(d);
}

int st_greedy_steps(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                    int32_t d, int64_t ld, double linv_scale, double linv_trace, int64_t t_begin,
                    int64_t t_end, int64_t n_points, uint32_t* idx_out, double* a_work,
                    void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    if (n_points < 1) return fail(ST_ERR_INVALID, "n_points must be >= 1");
    if (t_begin < 0 || t_end < t_begin || t_end > n_points)
        return fail(ST_ERR_INVALID, "need 0 <= t_begin <= t_end <= n_points");
    rc = check_greedy_buffers("", idx_out, a_work, workspace, workspace_bytes, d);
    if (rc) return rc;
    st::GreedyArgs a = make_args(x_soa, g_soa, weights, n, d, ld, linv_scale, linv_trace, a_work);
    a.idx_out = idx_out;
    return run_steps(a, workspace, t_begin, t_end, n_points, static_cast<hipStream_t>(stream));
}

int st_greedy(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
              int32_t d, int64_t ld, double linv_scale, double linv_trace, int64_t n_points,
              uint32_t* idx_out, double* a_work, void* workspace, int64_t workspace_bytes,
              void* stream) {
    if (n_points < 1) return fail(ST_ERR_INVALID, "n_points must be >= 1");
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    rc = check_greedy_buffers("", idx_out, a_work, workspace, workspace_bytes, d);
    if (rc) return rc;
    int used = 0;
    const hipError_t pe = st::launch_greedy_persistent(
        x_soa, g_soa, weights, a_work, n, d, ld, linv_scale, linv_trace, n_points, idx_out, workspace,
        workspace_bytes, static_cast<hipStream_t>(stream), &used);
    if (used) return ST_OK;
    if (pe != hipErrorNotSupported) (void)hipGetLastError();   // clear a failed launch
    return st_greedy_steps(x_soa, g_soa, weights, n, d, ld, linv_scale, linv_trace, 0, n_points,
                           n_points, idx_out, a_work, workspace, workspace_bytes, stream);
}

int st_greedy_dense(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                    int32_t d, int64_t ld, const double* linv, double linv_trace, int64_t n_points,
                    uint32_t* idx_out, double* a_work, void* workspace, int64_t workspace_bytes,
                    void* stream) {
    if (n_points < 1) return fail(ST_ERR_INVALID, "n_points must be >= 1");
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    rc = check_dense(linv, d);
    if (rc) return rc;
    rc = check_greedy_buffers("", idx_out, a_work, workspace, workspace_bytes, d);
    if (rc) return rc;
    st::GreedyArgs a = make_args(x_soa, g_soa, weights, n, d, ld, 0.0, linv_trace, a_work);
    a.compact = 0;   // one dense arithmetic; the diagonal is the exact one's
    a.linv = linv;
    a.idx_out = idx_out;
    return run_steps(a, workspace, 0, n_points, n_points, static_cast<hipStream_t>(stream));
}

int st_greedy_near_tie(const void* workspace, int64_t workspace_bytes, int64_t* step_out, void* stream) {
    if (!workspace || !step_out) return fail(ST_ERR_INVALID, "NULL workspace/output");
    if (workspace_bytes < st::kWsControlBytes) return fail(ST_ERR_INVALID, "workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t w[12];   // status [0], [1] ... tie words [8 .. 11]
    int rc = hip_check(hipMemcpyAsync(w, static_cast<const char*>(workspace) + st::kWsStatusOff, sizeof(w),
                                      hipMemcpyDeviceToHost, s), "near-tie read-back");
    if (rc) return rc;
    rc = hip_check(hipStreamSynchronize(s), "near-tie read-back sync");
    if (rc) return rc;
    constexpr int kTie = (int)((st::kWsTieOff - st::kWsStatusOff) / 4);
    if (w[kTie + 3] != 1u) {
        *step_out = -2;
        return ST_OK;
    }
    // the step kernels' word when they ran; else the gated general kernel's after a compact-only hand-off
    // words hold ~step (atomic max over blocks = the first flagged step), 0 = none
    const uint32_t tv = w[kTie + 2] ? w[kTie + 2] : (w[0] == 2u ? w[kTie + 1] : w[kTie]);
    *step_out = tv ? (int64_t)(uint32_t)~tv : -1;
    return ST_OK;
}

int st_greedy_batch(int32_t count, const double* const* x_soa, const double* const* g_soa,
                    const double* const* weights, const int64_t* n, int32_t d, const int64_t* ld,
                    const double* linv_scale, const double* linv_trace, int64_t n_points,
                    uint32_t* const* idx_out, double* const* a_work, void* const* workspace,
                    const int64_t* workspace_bytes, void* stream) {
    if (count < 1 || count > st::kMaxBatchProblems)
        return fail(ST_ERR_INVALID, "count must be in [1, %d]", st::kMaxBatchProblems);
    if (!x_soa || !g_soa || !n || !ld || !linv_scale || !linv_trace || !idx_out || !a_work || !workspace ||
        !workspace_bytes)
        return fail(ST_ERR_INVALID, "NULL argument array");
    if (n_points < 1) return fail(ST_ERR_INVALID, "n_points must be >= 1");
    st::BatchProblem pr[st::kMaxBatchProblems];
    for (int q = 0; q < count; ++q) {
        const double* w = weights ? weights[q] : nullptr;
        if ((w == nullptr) != (!weights || weights[0] == nullptr))
            return fail(ST_ERR_INVALID, "problem %d: weights must be given for every problem or none", q);
        int rc = check_problem(x_soa[q], g_soa[q], w, n[q], d, ld[q]);
        if (rc) return rc;
        char who[24];
        snprintf(who, sizeof(who), "problem %d: ", q);
        rc = check_greedy_buffers(who, idx_out[q], a_work[q], workspace[q], workspace_bytes[q], d);
        if (rc) return rc;
        pr[q] = st::BatchProblem{x_soa[q], g_soa[q], w, a_work[q], n[q], ld[q], linv_scale[q], linv_trace[q],
                                 idx_out[q], workspace[q], workspace_bytes[q]};
    }
    int used = 0;
    const hipError_t e = st::launch_greedy_persistent_batch(count, pr, d, n_points, static_cast<hipStream_t>(stream),
                                                            &used);
    if (used) return ST_OK;
    if (e == hipErrorNotSupported)
        return fail(ST_ERR_UNSUPPORTED, "batch launch does not apply (d = 2 / 4, every problem planned onto the same "
                    "kernel -- threads per block, register rows -- at #CU / count blocks); run st_greedy per problem");
    (void)hipGetLastError();
    return hip_check(e, "batch persistent launch");
}

int64_t st_mailbox_bytes(int32_t nranks) {
    if (nranks < 1 || nranks > st::kMailboxRanks) return -1;
    return st::kMailboxBytes;
}

int st_mailbox_alloc(int64_t bytes, void** mailbox) {
    if (!mailbox || bytes < st::kMailboxBytes) return fail(ST_ERR_INVALID, "bad mailbox request");
    *mailbox = nullptr;
    // uncached device memory: peers' xGMI stores land in HBM and local polls never hit a stale
    // L2 line
    void* p = nullptr;
    int rc = hip_check(hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocUncached),
                       "hipExtMallocWithFlags(uncached)");
    if (rc) return rc;
    rc = hip_check(hipMemset(p, 0, (size_t)bytes), "mailbox memset");
    if (rc) { (void)hipFree(p); return rc; }
    *mailbox = p;
    return ST_OK;
}

int st_mailbox_free(void* mailbox) {
    if (!mailbox) return ST_OK;
    return hip_check(hipFree(mailbox), "hipFree(mailbox)");
}

int st_ipc_get_handle(void* dev_ptr, void* handle_out) {
    if (!dev_ptr || !handle_out) return fail(ST_ERR_INVALID, "NULL pointer");
    hipIpcMemHandle_t h;
    int rc = hip_check(hipIpcGetMemHandle(&h, dev_ptr), "hipIpcGetMemHandle");
    if (rc) return rc;
    memcpy(handle_out, &h, sizeof(h));
    return ST_OK;
}

int st_ipc_handle_bytes(void) { return (int)sizeof(hipIpcMemHandle_t); }

int st_ipc_open_handle(const void* handle, void** dev_ptr) {
    if (!handle || !dev_ptr) return fail(ST_ERR_INVALID, "NULL pointer");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    *dev_ptr = nullptr;
    return hip_check(hipIpcOpenMemHandle(dev_ptr, h, hipIpcMemLazyEnablePeerAccess),
                     "hipIpcOpenMemHandle");
}

int st_ipc_close_handle(void* dev_ptr) {
    if (!dev_ptr) return ST_OK;
    return hip_check(hipIpcCloseMemHandle(dev_ptr), "hipIpcCloseMemHandle");
}

int st_mailbox_handshake(void* const* peer_mailboxes, int32_t nranks, int32_t rank,
                         uint64_t token, int32_t* ok_device, void* stream) {
    int rc = check_peers(peer_mailboxes, nranks, rank);
    if (rc) return rc;
    if (!ok_device) return fail(ST_ERR_INVALID, "NULL ok flag");
    if (token >> 63) return fail(ST_ERR_INVALID, "token must be < 2^63");
    const st::MailboxPeers peers = mailbox_peers(peer_mailboxes, nranks);
    return hip_check(st::launch_mailbox_handshake(peers, peers.p[rank], rank, nranks,
                                                  token | (1ull << 63), ok_device,
                                                  static_cast<hipStream_t>(stream)),
                     "handshake launch");
}

int st_greedy_sharded(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                      int32_t d, int64_t ld, double linv_scale, double linv_trace,
                      int64_t row_begin, int64_t row_end, int32_t rank, int32_t nranks,
                      void* const* peer_mailboxes, uint64_t seq_base, int64_t n_points,
                      uint32_t* idx_out, double* a_work, void* workspace,
                      int64_t workspace_bytes, void* stream) {
    if (n_points < 1) return fail(ST_ERR_INVALID, "n_points must be >= 1");
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    rc = check_peers(peer_mailboxes, nranks, rank);
    if (rc) return rc;
    if (row_begin < 0 || row_end <= row_begin || row_end > n)
        return fail(ST_ERR_INVALID, "need 0 <= row_begin < row_end <= n");
    rc = check_greedy_buffers("", idx_out, a_work, workspace, workspace_bytes, d);
    if (rc) return rc;
    const st::RankSpec rs = rank_spec(row_begin, row_end, rank, nranks, seq_base, peer_mailboxes[rank],
                                      peer_mailboxes);
    int used = 0;
    const hipError_t e = st::launch_greedy_persistent(
        x_soa, g_soa, weights, a_work, n, d, ld, linv_scale, linv_trace, n_points, idx_out, workspace,
        workspace_bytes, static_cast<hipStream_t>(stream), &used, &rs);
    if (used) return ST_OK;
    if (e == hipErrorNotSupported)
        return fail(ST_ERR_UNSUPPORTED, "multi-rank persistent kernel: d = %d not supported (d = 2, 4; d = 50 "
                    "with at most 256 rows per CU)", d);
    (void)hipGetLastError();
    return hip_check(e, "multi-rank persistent launch");
}

int st_greedy_sharded_supported(int64_t n, int32_t d, int32_t has_weights, int64_t row_begin,
                                int64_t row_end, int32_t rank, int32_t nranks, int64_t n_points) {
    if (d < 1 || d > st::kMaxDim || n < 1 || n_points < 1)
        return fail(ST_ERR_INVALID, "bad problem (n = %lld, d = %d)", (long long)n, d);
    if (nranks < 2 || nranks > st::kMailboxRanks || rank < 0 || rank >= nranks)
        return fail(ST_ERR_INVALID, "bad rank %d of %d", rank, nranks);
    if (row_begin < 0 || row_end <= row_begin || row_end > n)
        return fail(ST_ERR_INVALID, "need 0 <= row_begin < row_end <= n");
    // the same decision st_greedy_sharded takes, without touching any buffer: placeholders for the
    // pointers, a non-null inbox, the workspace size the caller allocates (st_greedy_workspace_bytes)
    static uint64_t dummy_box[2];
    const st::RankSpec rs = rank_spec(row_begin, row_end, rank, nranks, 0, dummy_box, nullptr);
    static double dummy_w;
    int used = 0;
    const hipError_t e = st::launch_greedy_persistent(
        nullptr, nullptr, has_weights ? &dummy_w : nullptr, nullptr, n, d, 0, 1.0, 1.0, n_points, nullptr,
        nullptr, greedy_ws_bytes(d), nullptr, &used, &rs, true);
    if (e == hipErrorInvalidValue) return fail(ST_ERR_INVALID, "invalid shard");
    return used ? 1 : 0;
}

int st_greedy_step(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                   int32_t d, int64_t ld, double linv_scale, double linv_trace, int64_t row_offset,
                   int64_t t, int32_t nranks, const double* cands_in, double* cand_out,
                   uint32_t* idx_out, double* a_work, void* workspace, int64_t workspace_bytes,
                   void* stream) {
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    if (t < 0) return fail(ST_ERR_INVALID, "t must be >= 0");
    if (nranks < 1 || nranks > 64) return fail(ST_ERR_INVALID, "nranks must be in [1, 64]");
    if (t > 0 && !cands_in) return fail(ST_ERR_INVALID, "cands_in is NULL for t > 0");
    // the NULL test of check_greedy_buffers, early: it precedes the idx_out and row_offset checks (also below)
    if (!cand_out || !a_work || !workspace) return fail(ST_ERR_INVALID, "NULL output/workspace");
    if (t > 0 && !idx_out) return fail(ST_ERR_INVALID, "idx_out is NULL");
    if (row_offset < 0) return fail(ST_ERR_INVALID, "row_offset must be >= 0");
    rc = check_greedy_buffers("", cand_out, a_work, workspace, workspace_bytes, d);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const st::GreedyArgs a = step_args(x_soa, g_soa, weights, n, d, ld, linv_scale, linv_trace, row_offset, t,
                                       cands_in, nranks, idx_out, a_work, workspace);
    const int blocks = st::greedy_blocks(n, d);
    rc = hip_check(st::launch_greedy_step(a, t == 0, blocks, s), "greedy step launch");
    if (rc) return rc;
    return hip_check(st::launch_greedy_publish(a.recs_out, blocks, a.rec_stride, d, cand_out, s),
                     "greedy publish launch");
}

int st_greedy_step_exchange(const double* x_soa, const double* g_soa, const double* weights,
                            int64_t n, int32_t d, int64_t ld, double linv_scale, double linv_trace,
                            int64_t row_offset, int64_t t, int32_t rank, int32_t nranks,
                            void* const* peer_mailboxes, double* cands, uint32_t* idx_out,
                            double* a_work, void* workspace, int64_t workspace_bytes,
                            uint32_t* status_device, void* stream) {
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    rc = check_peers(peer_mailboxes, nranks, rank);
    if (rc) return rc;
    if (t < 0) return fail(ST_ERR_INVALID, "t must be >= 0");
    if (!cands || !a_work || !workspace || !status_device) return fail(ST_ERR_INVALID, "NULL output/workspace");
    if (t > 0 && !idx_out) return fail(ST_ERR_INVALID, "idx_out is NULL");
    if (row_offset < 0) return fail(ST_ERR_INVALID, "row_offset must be >= 0");
    rc = check_greedy_buffers("", cands, a_work, workspace, workspace_bytes, d);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const st::GreedyArgs a = step_args(x_soa, g_soa, weights, n, d, ld, linv_scale, linv_trace, row_offset, t,
                                       cands, nranks, idx_out, a_work, workspace);
    const int blocks = st::greedy_blocks(n, d);
    rc = hip_check(st::launch_greedy_step(a, t == 0, blocks, s), "greedy step launch");
    if (rc) return rc;
    return hip_check(st::launch_greedy_rank_exchange(a.recs_out, blocks, a.rec_stride, d,
                                                     mailbox_peers(peer_mailboxes, nranks), rank, nranks, t,
                                                     cands, status_device, s),
                     "rank exchange launch");
}

int64_t st_kde_workspace_bytes(int64_t m, int32_t d) {
    if (m < 0 || d < 1 || d > st::kMaxDim) return -1;
    return st::kde_workspace_bytes(m, d);
}

int st_kde_logpdf_grad(const double* p_soa, int64_t ldp, int64_t n, const double* log_weights,
                       double log_weight_uniform, const double* q_soa, int64_t ldq, int64_t m, int32_t d,
                       double log_norm, const double* whiten, double* log_q_out, double* grad_out,
                       void* workspace, int64_t workspace_bytes, void* stream) {
    return kde_logpdf_grad(p_soa, ldp, n, log_weights, log_weight_uniform, q_soa, ldq, m, d, nullptr, log_norm,
                           whiten, log_q_out, grad_out, workspace, workspace_bytes, stream);
}

int64_t st_kde_t_workspace_bytes(int64_t m, int32_t d) {
    if (m < 0 || d < 1 || d > st::kMaxDim) return -1;
    return st::kde_workspace_bytes(m, d);
}

int st_kde_t_logpdf_grad(const double* p_soa, int64_t ldp, int64_t n, const double* log_weights,
                         double log_weight_uniform, const double* q_soa, int64_t ldq, int64_t m, int32_t d,
                         double df, double log_norm, const double* whiten, double* log_q_out, double* grad_out,
                         void* workspace, int64_t workspace_bytes, void* stream) {
    return kde_logpdf_grad(p_soa, ldp, n, log_weights, log_weight_uniform, q_soa, ldq, m, d, &df, log_norm,
                           whiten, log_q_out, grad_out, workspace, workspace_bytes, stream);
}

int st_proxy_logpdf_grad(const double* x, int64_t n, int32_t d, const double* loc,
                         const double* whiten, const double* precision, double df, double c_log,
                         double* log_q_out, double* grad_out, void* stream) {
    if (n < 0) return fail(ST_ERR_INVALID, "n must be >= 0");
    if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1");
    if (d > st::kMaxDim) return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds %d", d, st::kMaxDim);
    if (!(df >= 0.0) || df == INFINITY) return fail(ST_ERR_INVALID, "df must be 0 (Gaussian) or finite > 0");
    if (n == 0) return ST_OK;
    if (!x || !loc || !whiten || !precision || !log_q_out || !grad_out)
        return fail(ST_ERR_INVALID, "NULL pointer");
    st::ProxyArgs a{x, loc, whiten, precision, n, d, df, c_log, log_q_out, grad_out};
    return hip_check(st::launch_proxy(a, static_cast<hipStream_t>(stream)), "proxy launch");
}

int st_mixture_logpdf_score(const double* x, int64_t n, int32_t d, int32_t k, const double* log_coef,
                            const double* means, const double* precision, double* log_p_out,
                            double* score_out, void* stream) {
    if (n < 0) return fail(ST_ERR_INVALID, "n must be >= 0 (got %lld)", (long long)n);
    if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1 (got %d)", d);
    if (k < 1) return fail(ST_ERR_INVALID, "k must be >= 1 (got %d)", k);
    if (!log_coef || !means || !precision || (n > 0 && (!x || !log_p_out || !score_out)))
        return fail(ST_ERR_INVALID, "NULL pointer");
    if (!aligned8(x) || !aligned8(log_coef) || !aligned8(means) || !aligned8(precision) || !aligned8(log_p_out) ||
        !aligned8(score_out))
        return fail(ST_ERR_INVALID, "device arrays must be 8-byte aligned");
    if (d > st::kMixtureMaxDim)
        return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds the mixture kernels' maximum %d", d, st::kMixtureMaxDim);
    if (k > st::kMixtureMaxComponents)
        return fail(ST_ERR_UNSUPPORTED, "k = %d components exceed the maximum %d", k, st::kMixtureMaxComponents);
    if (n == 0) return ST_OK;
    st::MixtureArgs a{x, log_coef, means, precision, n, d, k, log_p_out, score_out};
    return hip_check(st::launch_mixture(a, static_cast<hipStream_t>(stream)), "mixture launch");
}

int64_t st_mvt_moments_workspace_bytes(int64_t n, int32_t d) {
    if (n < 1 || d < 1 || d > st::kMvtMaxDim) return -1;
    return st::mvt_moments_ws_bytes(n, d);
}

int st_mvt_moments(const double* x, int64_t n, int32_t d, const double* loc, const double* whiten, double df,
                   int32_t want_grad, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (n < 1) return fail(ST_ERR_INVALID, "n must be >= 1 (got %lld)", (long long)n);
    if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1 (got %d)", d);
    if (!(df > 0.0) || df == INFINITY) return fail(ST_ERR_INVALID, "df must be finite and > 0");
    if (!x || !loc || !whiten || !out || !workspace) return fail(ST_ERR_INVALID, "NULL pointer");
    if (!aligned8(x) || !aligned8(loc) || !aligned8(whiten) || !aligned8(out) || !aligned8(workspace))
        return fail(ST_ERR_INVALID, "device arrays must be 8-byte aligned");
    if (d > st::kMvtMaxDim)
        return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds the moment kernels' maximum %d", d, st::kMvtMaxDim);
    if (workspace_bytes < st::mvt_moments_ws_bytes(n, d))
        return fail(ST_ERR_INVALID, "workspace too small (%lld < %lld)", (long long)workspace_bytes,
                    (long long)st::mvt_moments_ws_bytes(n, d));
    st::MvtMomentsArgs a{x, loc, whiten, n, d, df, want_grad != 0, out, static_cast<double*>(workspace)};
    return hip_check(st::launch_mvt_moments(a, static_cast<hipStream_t>(stream)), "mvt moments launch");
}

int64_t st_mixture_em_workspace_bytes(int64_t n, int32_t d, int32_t k) {
    if (n < 1 || d < 1 || d > st::kMixtureEmMaxDim || k < 1 || k > st::kMixtureEmMaxComponents) return -1;
    return st::mixture_em_ws_bytes(n, d, k);
}

int st_mixture_em_stats(const double* x, int64_t n, int32_t d, int32_t k, const double* log_coef, const double* means,
                        const double* precision, const double* row_weights, double* out, double* log_p_out,
                        void* workspace, int64_t workspace_bytes, void* stream) {
    if (n < 1) return fail(ST_ERR_INVALID, "n must be >= 1 (got %lld)", (long long)n);
    if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1 (got %d)", d);
    if (k < 1) return fail(ST_ERR_INVALID, "k must be >= 1 (got %d)", k);
    if (!x || !log_coef || !means || !precision || !out || !workspace) return fail(ST_ERR_INVALID, "NULL pointer");
    if (!aligned8(x) || !aligned8(log_coef) || !aligned8(means) || !aligned8(precision) || !aligned8(row_weights) ||
        !aligned8(out) || !aligned8(log_p_out) || !aligned8(workspace))
        return fail(ST_ERR_INVALID, "device arrays must be 8-byte aligned");
    if (d > st::kMixtureEmMaxDim)
        return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds the EM kernel's maximum %d", d, st::kMixtureEmMaxDim);
    if (k > st::kMixtureEmMaxComponents)
        return fail(ST_ERR_UNSUPPORTED, "k = %d components exceed the EM kernel's maximum %d", k,
                    st::kMixtureEmMaxComponents);
    if (workspace_bytes < st::mixture_em_ws_bytes(n, d, k))
        return fail(ST_ERR_INVALID, "workspace too small (%lld < %lld)", (long long)workspace_bytes,
                    (long long)st::mixture_em_ws_bytes(n, d, k));
    st::MixtureEmArgs a{x, log_coef, means, precision, row_weights, n, d, k, out, log_p_out, static_cast<double*>(workspace)};
    return hip_check(st::launch_mixture_em(a, static_cast<hipStream_t>(stream)), "mixture EM launch");
}

int st_lv_grad_log_posterior(const double* theta, int64_t n, const double* t_eval, int32_t t_n,
                             const double* y_obs, const double* span_u0_tol, const double* cov_inv,
                             int64_t max_steps, double* grad_out, int32_t* status, void* stream) {
    return lv_grad(theta, n, t_eval, t_n, y_obs, span_u0_tol, cov_inv, max_steps, grad_out, status, false, nullptr,
                   0, stream);
}

int64_t st_lv_grad_workspace_bytes(int64_t n, int32_t t_n) {
    if (n < 0 || t_n < 1) return -1;
    return st::lv_grad_workspace_bytes(n, kLvStepCap);
}

int st_lv_grad_log_posterior_ws(const double* theta, int64_t n, const double* t_eval, int32_t t_n,
                                const double* y_obs, const double* span_u0_tol, const double* cov_inv,
                                int64_t max_steps, double* grad_out, int32_t* status, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    return lv_grad(theta, n, t_eval, t_n, y_obs, span_u0_tol, cov_inv, max_steps, grad_out, status, true, workspace,
                   workspace_bytes, stream);
}

int64_t st_lv_log_density_workspace_bytes(int64_t n, int32_t t_n) {
    if (n < 0 || t_n < 1) return -1;
    return n * (int64_t)t_n * 8;
}

int st_lv_log_target_density(const double* log_theta, const double* theta, int64_t n,
                             const double* t_eval, int32_t t_n, const double* y_obs,
                             const double* span_u0_tol, const double* whiten, double c_log,
                             double norm_logc, int64_t max_steps, double* out, int32_t* status,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    st::LvArgs a{};
    int rc = lv_common(a, theta, n, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc, max_steps, out, status);
    if (rc) return rc;
    if (!whiten) return fail(ST_ERR_INVALID, "NULL whiten");
    if (n > 0 && (!log_theta || !workspace)) return fail(ST_ERR_INVALID, "NULL log_theta / workspace");
    if (workspace_bytes < n * (int64_t)t_n * 8) return fail(ST_ERR_INVALID, "workspace too small");
    a.log_theta = log_theta;
    a.work = static_cast<double*>(workspace);
    if (n == 0) return ST_OK;
    return hip_check(st::launch_lv(a, false, static_cast<hipStream_t>(stream)), "lv log density launch");
}

int64_t st_lv_rwmh_workspace_bytes(int64_t chains) {
    if (chains < 1) return -1;
    return chains * 64;
}

int st_lv_rwmh(double* state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
               int32_t init, const double* step_size, int32_t noise_mode, uint64_t seed, double* z,
               double* log_u, int64_t noise_ld, int64_t noise_row0, const double* t_eval, int32_t t_n,
               const double* y_obs, const double* span_u0_tol, const double* whiten, double c_log,
               double norm_logc, int64_t max_steps, double* samples, double* log_p, int64_t out_ld,
               int64_t out_row0, void* stream) {
    return lv_rwmh(st::launch_lv_rwmh, "lv rwmh launch", state, chains, first_chain, first_step, steps, init,
                   step_size, noise_mode, seed, z, log_u, noise_ld, noise_row0, t_eval, t_n, y_obs, span_u0_tol,
                   whiten, c_log, norm_logc, max_steps, samples, log_p, out_ld, out_row0, stream);
}

int st_lv_rwmh_wave(double* state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                    int32_t init, const double* step_size, int32_t noise_mode, uint64_t seed, double* z,
                    double* log_u, int64_t noise_ld, int64_t noise_row0, const double* t_eval, int32_t t_n,
                    const double* y_obs, const double* span_u0_tol, const double* whiten, double c_log,
                    double norm_logc, int64_t max_steps, double* samples, double* log_p, int64_t out_ld,
                    int64_t out_row0, void* stream) {
    return lv_rwmh(st::launch_lv_rwmh_wave, "lv rwmh wave launch", state, chains, first_chain, first_step, steps,
                   init, step_size, noise_mode, seed, z, log_u, noise_ld, noise_row0, t_eval, t_n, y_obs,
                   span_u0_tol, whiten, c_log, norm_logc, max_steps, samples, log_p, out_ld, out_row0, stream);
}

int64_t st_lv_mala_workspace_bytes(int64_t chains) {
    if (chains < 1) return -1;
    return chains * 128;
}

int st_lv_mala_wave(double* state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                    int32_t init, const double* step_ehw, const double* drift_clip, int32_t noise_mode,
                    uint64_t seed, double* z, double* log_u, int64_t noise_ld, int64_t noise_row0,
                    const double* t_eval, int32_t t_n, const double* y_obs, const double* span_u0_tol,
                    const double* whiten, double c_log, double norm_logc, const double* cov_inv,
                    int64_t max_steps, double* samples, double* log_p, double* grad, int64_t out_ld,
                    int64_t out_row0, void* stream) {
    // the common checks (step_ehw[0 .. 3] = eps is their step size), then the sampler's own
    st::LvMalaArgs a{};
    int rc = lv_rwmh_args(a, state, chains, first_chain, first_step, steps, init, step_ehw, noise_mode, seed, z,
                          log_u, noise_ld, noise_row0, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc,
                          max_steps, samples, log_p, out_ld, out_row0);
    if (!rc) rc = lv_grad_args(a, grad, drift_clip, "drift", cov_inv, step_ehw + 4);
    if (rc) return rc;
    for (int j = 0; j < 4; ++j) {
        a.eps[j] = step_ehw[j];
        a.h[j] = step_ehw[4 + j];
        a.w[j] = step_ehw[8 + j];
    }
    return hip_check(st::launch_lv_mala_wave(a, static_cast<hipStream_t>(stream)), "lv mala wave launch");
}

int64_t st_lv_hmc_workspace_bytes(int64_t chains) {
    if (chains < 1) return -1;
    return chains * 128;
}

int st_lv_hmc_wave(double* state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                   int32_t init, const double* step_eps, const double* kick_clip, int32_t n_leapfrog,
                   int32_t noise_mode, uint64_t seed, double* z, double* log_u, int64_t noise_ld,
                   int64_t noise_row0, const double* t_eval, int32_t t_n, const double* y_obs,
                   const double* span_u0_tol, const double* whiten, double c_log, double norm_logc,
                   const double* cov_inv, int64_t max_steps, double* samples, double* log_p, double* grad,
                   int64_t out_ld, int64_t out_row0, void* stream) {
    // the common checks (step_eps is their step size), then the sampler's own
    st::LvHmcArgs a{};
    int rc = lv_rwmh_args(a, state, chains, first_chain, first_step, steps, init, step_eps, noise_mode, seed, z,
                          log_u, noise_ld, noise_row0, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc,
                          max_steps, samples, log_p, out_ld, out_row0);
    if (!rc) rc = lv_grad_args(a, grad, kick_clip, "kick", cov_inv);
    if (rc) return rc;
    if (n_leapfrog < 1) return fail(ST_ERR_INVALID, "n_leapfrog must be >= 1 (got %d)", (int)n_leapfrog);
    for (int j = 0; j < 4; ++j) a.eps[j] = step_eps[j];
    a.n_leapfrog = n_leapfrog;
    return hip_check(st::launch_lv_hmc_wave(a, static_cast<hipStream_t>(stream)), "lv hmc wave launch");
}

int64_t st_lv_hmc_metric_workspace_bytes(int64_t chains) {
    if (chains < 1) return -1;
    return chains * 192;
}

int st_lv_hmc_metric_wave(double* state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                          int32_t init, const double* eps_chain, const double* metric_chol, const double* kick_clip,
                          int32_t n_leapfrog, int32_t adapt, double delta, int32_t noise_mode, uint64_t seed,
                          double* z, double* log_u, int64_t noise_ld, int64_t noise_row0, const double* t_eval,
                          int32_t t_n, const double* y_obs, const double* span_u0_tol, const double* whiten,
                          double c_log, double norm_logc, const double* cov_inv, int64_t max_steps, double* samples,
                          double* log_p, double* grad, double* accept_stat, double* step_size, int64_t out_ld,
                          int64_t out_row0, void* stream) {
    // the common checks (the step sizes are a device array: not theirs), then the sampler's own
    st::LvHmcMetricArgs a{};
    int rc = lv_rwmh_args(a, state, chains, first_chain, first_step, steps, init, nullptr, noise_mode, seed, z,
                          log_u, noise_ld, noise_row0, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc,
                          max_steps, samples, log_p, out_ld, out_row0, false);
    if (!rc)
        rc = lv_metric_args(a, grad, kick_clip, cov_inv, eps_chain, metric_chol, accept_stat, step_size,
                            {eps_chain, metric_chol, accept_stat, step_size},
                            "NULL pointer (eps_chain, metric_chol, accept_stat, step_size)",
                            "eps_chain, metric_chol, accept_stat and step_size must be 8-byte aligned",
                            n_leapfrog >= 1, "n_leapfrog must be >= 1 (got %d)", n_leapfrog, adapt, delta);
    if (rc) return rc;
    a.n_leapfrog = n_leapfrog;
    return hip_check(st::launch_lv_hmc_metric_wave(a, static_cast<hipStream_t>(stream)), "lv hmc metric wave launch");
}

int64_t st_lv_nuts_workspace_bytes(int64_t chains) {
    if (chains < 1) return -1;
    return chains * 192;
}

int st_lv_nuts_wave(double* state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                    int32_t init, const double* eps_chain, const double* metric_chol, const double* kick_clip,
                    int32_t max_depth, int32_t adapt, double delta, int32_t noise_mode, uint64_t seed, double* z,
                    double* log_u, int64_t noise_ld, int64_t noise_row0, const double* t_eval, int32_t t_n,
                    const double* y_obs, const double* span_u0_tol, const double* whiten, double c_log,
                    double norm_logc, const double* cov_inv, int64_t max_steps, double* samples, double* log_p,
                    double* grad, double* accept_stat, double* step_size, double* tree_depth, double* n_leapfrog,
                    double* divergent, int64_t out_ld, int64_t out_row0, void* stream) {
    // the common checks (the step sizes are a device array: not theirs), then the sampler's own
    st::LvNutsArgs a{};
    int rc = lv_rwmh_args(a, state, chains, first_chain, first_step, steps, init, nullptr, noise_mode, seed, z,
                          log_u, noise_ld, noise_row0, t_eval, t_n, y_obs, span_u0_tol, whiten, c_log, norm_logc,
                          max_steps, samples, log_p, out_ld, out_row0, false);
    if (rc) return rc;
    if (noise_mode == 0)
        return fail(ST_ERR_INVALID, "noise_mode must be 1 or 2: the tree's draws have no supplied-noise form");
    rc = lv_metric_args(a, grad, kick_clip, cov_inv, eps_chain, metric_chol, accept_stat, step_size,
                        {eps_chain, metric_chol, accept_stat, step_size, tree_depth, n_leapfrog, divergent},
                        "NULL pointer (eps_chain, metric_chol, accept_stat, step_size, tree_depth, n_leapfrog, "
                        "divergent)",
                        "eps_chain, metric_chol and the per-step outputs must be 8-byte aligned",
                        max_depth >= 1 && max_depth <= 10, "max_depth must be 1 .. 10 (got %d)", max_depth, adapt,
                        delta);
    if (rc) return rc;
    a.max_depth = max_depth;
    a.tree_depth = tree_depth;
    a.n_leapfrog = n_leapfrog;
    a.divergent = divergent;
    return hip_check(st::launch_lv_nuts_wave(a, static_cast<hipStream_t>(stream)), "lv nuts wave launch");
}

int st_greedy_finalize(const double* cands_in, int32_t nranks, int32_t d, uint32_t* idx_out,
                       int64_t t, void* stream) {
    if (!cands_in || !idx_out) return fail(ST_ERR_INVALID, "NULL pointer");
    if (nranks < 1 || nranks > 64) return fail(ST_ERR_INVALID, "nranks must be in [1, 64]");
    if (d < 1 || d > st::kMaxDim) return fail(ST_ERR_UNSUPPORTED, "unsupported d");
    if (t < 0) return fail(ST_ERR_INVALID, "t must be >= 0");
    return hip_check(st::launch_greedy_finalize(cands_in, nranks, st::cand_stride(d), idx_out, t,
                                                static_cast<hipStream_t>(stream)),
                     "greedy finalize launch");
}

int st_kernel_pairs(const double* x_soa, const double* g_soa, const double* weights, int64_t ld,
                    int32_t d, double linv_scale, double linv_trace, const int64_t* i1,
                    const int64_t* i2, int64_t n_pairs, double* out, void* stream) {
    return kernel_pairs(x_soa, g_soa, weights, ld, d, false, nullptr, linv_scale, linv_trace, i1, i2, n_pairs, out,
                        stream);
}

int64_t st_ksd_workspace_bytes(int64_t m, int64_t ld) {
    if (m < 1 || ld < m) return -1;
    return ld * 8;   // the column-sum vector
}

int st_ksd_cumulative(const double* x_soa, const double* g_soa, const double* weights, int64_t m,
                      int64_t ld, int32_t d, double linv_scale, double linv_trace, double* ks_out,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    return ksd_cumulative(x_soa, g_soa, weights, m, ld, d, false, nullptr, linv_scale, linv_trace, ks_out,
                          workspace, workspace_bytes, stream);
}

int st_ksd_colsum(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                  int64_t ld, int32_t d, double linv_scale, double linv_trace, int64_t row_begin,
                  int64_t row_end, double* csum_out, void* stream) {
    return ksd_colsum(x_soa, g_soa, weights, n, ld, d, false, nullptr, linv_scale, linv_trace, row_begin, row_end,
                      csum_out, stream);
}

int st_ksd_finish(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                  int64_t ld, int32_t d, double linv_scale, double linv_trace, const double* csum,
                  double* ks_out, void* stream) {
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    if (!csum || !ks_out) return fail(ST_ERR_INVALID, "NULL pointer");
    st::PairArgs p{x_soa, g_soa, weights, ld, d, linv_scale, linv_trace};
    return hip_check(st::launch_ksd_finish(p, n, csum, ks_out, static_cast<hipStream_t>(stream)),
                     "ksd finish launch");
}

int64_t st_distance_workspace_bytes(int64_t na, int64_t b_begin, int64_t b_end) {
    if (na < 0 || b_begin < 0 || b_end < b_begin) return -1;
    const int64_t K = st::distance_chunks(na, b_begin, b_end);
    return K > 1 ? K * na * (int64_t)sizeof(double) : 0;
}

int st_distance_colsum(const double* a_soa, int64_t lda, int64_t na, const double* b_soa,
                       int64_t ldb, int64_t nb, int32_t d, int64_t b_begin, int64_t b_end,
                       int32_t triangle, double* out, void* stream) {
    return st_distance_colsum_ws(a_soa, lda, na, b_soa, ldb, nb, d, b_begin, b_end, triangle, out,
                                 nullptr, 0, stream);
}

int st_distance_colsum_ws(const double* a_soa, int64_t lda, int64_t na, const double* b_soa,
                          int64_t ldb, int64_t nb, int32_t d, int64_t b_begin, int64_t b_end,
                          int32_t triangle, double* out, void* workspace, int64_t workspace_bytes,
                          void* stream) {
    if (na == 0) return ST_OK;
    if (!a_soa || !b_soa || !out) return fail(ST_ERR_INVALID, "NULL pointer");
    if (d < 1 || d > st::kMaxDim) return fail(ST_ERR_UNSUPPORTED, "unsupported d = %d", d);
    if (na < 0 || nb < 0 || lda < na || ldb < nb || (lda & 7) || (ldb & 7))
        return fail(ST_ERR_INVALID, "bad sizes (ld must be a multiple of 8 and >= the row count)");
    if (b_begin < 0 || b_end < b_begin || b_end > nb)
        return fail(ST_ERR_INVALID, "need 0 <= b_begin <= b_end <= nb");
    if (triangle && (a_soa != b_soa || lda != ldb))
        return fail(ST_ERR_INVALID, "triangle=1 needs A and B to be the same array");
    if ((na + 255) / 256 > 0x7FFFFFFFll) return fail(ST_ERR_UNSUPPORTED, "na too large");
    if (workspace && !aligned16(workspace)) return fail(ST_ERR_INVALID, "workspace must be 16-byte aligned");
    return hip_check(st::launch_distance_colsum(a_soa, lda, na, b_soa, ldb, b_begin, b_end, d,
                                                triangle ? 1 : 0, out, static_cast<double*>(workspace),
                                                workspace ? workspace_bytes / 8 : 0,
                                                static_cast<hipStream_t>(stream)),
                     "distance column-sum launch");
}

// ---- set-batched forms: one resident problem, many index sets (csrc/sets.hpp) ----------------------
int64_t st_sets_work_items(const int64_t* set_offsets, int64_t n_sets, int32_t* items_out, int64_t capacity) {
    if (!set_offsets || n_sets < 0 || !aligned8(set_offsets)) return -1;
    if (n_sets == 0) return 0;
    if (st::sets_check_offsets(set_offsets, n_sets)) return -1;
    const int64_t count = st::sets_item_count(set_offsets, n_sets);
    if (n_sets > 0x7FFFFFFFll || count > 0x7FFFFFFFll) return -1;
    if (items_out) {
        if (capacity < count) return -1;
        st::sets_build_items(set_offsets, n_sets, items_out);
    }
    return count;
}

int64_t st_ksd_sets_workspace_bytes(int64_t total_rows, int64_t n_sets, int32_t d) {
    if (total_rows < 0 || n_sets < 0 || d < 1 || d > st::kMaxDim) return -1;
    return st::sets_ws_bytes(total_rows, n_sets, 2 * d + 1);
}

int st_ksd_sets(const double* x_soa, const double* g_soa, const double* weights, int64_t n, int64_t ld,
                int32_t d, double linv_scale, double linv_trace, const int64_t* rows,
                const int64_t* set_offsets, int64_t n_sets, double* ks_out, double* csum_out,
                void* workspace, int64_t workspace_bytes, void* stream) {
    if (n_sets < 0) return fail(ST_ERR_INVALID, "n_sets must be >= 0 (got %lld)", (long long)n_sets);
    if (n_sets == 0) return ST_OK;
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    rc = check_sets(rows, set_offsets, n_sets);
    if (rc) return rc;
    if (!ks_out || !workspace) return fail(ST_ERR_INVALID, "NULL output/workspace");
    if (!aligned8(ks_out) || !aligned8(csum_out) || !aligned16(workspace))
        return fail(ST_ERR_INVALID, "outputs must be 8-byte and the workspace 16-byte aligned");
    if (workspace_bytes < st_ksd_sets_workspace_bytes(set_offsets[n_sets], n_sets, d))
        return fail(ST_ERR_INVALID, "workspace too small");
    st::PairArgs p{x_soa, g_soa, weights, ld, d, linv_scale, linv_trace};
    return hip_check(st::launch_ksd_sets(p, n, rows, set_offsets, n_sets, ks_out, csum_out, workspace,
                                         static_cast<hipStream_t>(stream)),
                     "ksd sets launch");
}

int64_t st_distance_sets_workspace_bytes(int64_t total_rows, int64_t n_sets, int32_t d) {
    if (total_rows < 0 || n_sets < 0 || d < 1 || d > st::kMaxDim) return -1;
    return st::sets_ws_bytes(total_rows, n_sets, d);
}

int st_distance_sets(const double* p_soa, int64_t ldp, int64_t n, int32_t d, const int64_t* rows,
                     const int64_t* set_offsets, int64_t n_sets, double* self_out, const double* row_values,
                     double* segsum_out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (n_sets < 0) return fail(ST_ERR_INVALID, "n_sets must be >= 0 (got %lld)", (long long)n_sets);
    if (n_sets == 0) return ST_OK;
    if (!p_soa) return fail(ST_ERR_INVALID, "point pointer is NULL");
    if (d < 1) return fail(ST_ERR_INVALID, "d must be >= 1 (got %d)", d);
    if (d > st::kMaxDim) return fail(ST_ERR_UNSUPPORTED, "d = %d exceeds the supported maximum %d", d, st::kMaxDim);
    if (n < 1 || ldp < n || (ldp & 7))
        return fail(ST_ERR_INVALID, "bad sizes (ld must be a multiple of 8 and >= the row count)");
    if (!aligned16(p_soa)) return fail(ST_ERR_INVALID, "device arrays must be 16-byte aligned");
    int rc = check_sets(rows, set_offsets, n_sets);
    if (rc) return rc;
    if (!self_out || !workspace) return fail(ST_ERR_INVALID, "NULL output/workspace");
    if ((segsum_out != nullptr) != (row_values != nullptr))
        return fail(ST_ERR_INVALID, "row_values and segsum_out go together (both or neither)");
    if (!aligned8(self_out) || !aligned8(row_values) || !aligned8(segsum_out) || !aligned16(workspace))
        return fail(ST_ERR_INVALID, "arrays must be 8-byte and the workspace 16-byte aligned");
    if (workspace_bytes < st_distance_sets_workspace_bytes(set_offsets[n_sets], n_sets, d))
        return fail(ST_ERR_INVALID, "workspace too small");
    return hip_check(st::launch_distance_sets(p_soa, ldp, n, d, rows, set_offsets, n_sets, self_out, row_values,
                                              segsum_out, workspace, static_cast<hipStream_t>(stream)),
                     "distance sets launch");
}

int st_kmat(const double* x_soa, const double* g_soa, const double* weights, int64_t k, int64_t ld,
            int32_t d, double linv_scale, double linv_trace, double* kmat_out, void* stream) {
    return kmat(x_soa, g_soa, weights, k, ld, d, false, nullptr, linv_scale, linv_trace, kmat_out, stream);
}

int st_kernel_pairs_dense(const double* x_soa, const double* g_soa, const double* weights, int64_t ld,
                          int32_t d, const double* linv, double linv_trace, const int64_t* i1,
                          const int64_t* i2, int64_t n_pairs, double* out, void* stream) {
    return kernel_pairs(x_soa, g_soa, weights, ld, d, true, linv, 0.0, linv_trace, i1, i2, n_pairs, out, stream);
}

int st_ksd_colsum_dense(const double* x_soa, const double* g_soa, const double* weights, int64_t n,
                        int64_t ld, int32_t d, const double* linv, double linv_trace, int64_t row_begin,
                        int64_t row_end, double* csum_out, void* stream) {
    return ksd_colsum(x_soa, g_soa, weights, n, ld, d, true, linv, 0.0, linv_trace, row_begin, row_end, csum_out,
                      stream);
}

int st_ksd_cumulative_dense(const double* x_soa, const double* g_soa, const double* weights, int64_t m,
                            int64_t ld, int32_t d, const double* linv, double linv_trace, double* ks_out,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    return ksd_cumulative(x_soa, g_soa, weights, m, ld, d, true, linv, 0.0, linv_trace, ks_out, workspace,
                          workspace_bytes, stream);
}

int st_kmat_dense(const double* x_soa, const double* g_soa, const double* weights, int64_t k, int64_t ld,
                  int32_t d, const double* linv, double linv_trace, double* kmat_out, void* stream) {
    return kmat(x_soa, g_soa, weights, k, ld, d, true, linv, 0.0, linv_trace, kmat_out, stream);
}

int st_layout_soa(const double* rowmajor, int64_t n, int32_t d, int64_t ld, double* soa,
                  void* stream) {
    if (!rowmajor || !soa) return fail(ST_ERR_INVALID, "NULL pointer");
    if (n < 1 || d < 1 || ld < n) return fail(ST_ERR_INVALID, "bad sizes");
    return hip_check(st::launch_layout_soa(rowmajor, n, d, ld, soa, static_cast<hipStream_t>(stream)),
                     "layout launch");
}

int st_layout_soa_scaled(const double* rowmajor, int64_t n, int32_t d, int64_t ld, const double* scale,
                         int32_t divide, double* soa, void* stream) {
    if (!rowmajor || !soa || !scale) return fail(ST_ERR_INVALID, "NULL pointer");
    if (n < 1 || d < 1 || ld < n) return fail(ST_ERR_INVALID, "bad sizes");
    return hip_check(st::launch_layout_soa_scaled(rowmajor, n, d, ld, scale, divide ? 1 : 0, soa,
                                                  static_cast<hipStream_t>(stream)),
                     "scaled layout launch");
}

int st_pdist(const double* rows, int64_t k, int32_t d, double* out, void* stream) {
    if (!rows || !out) return fail(ST_ERR_INVALID, "NULL pointer");
    if (k < 2 || k > 65535 || d < 1 || d > st::kMaxDim)
        return fail(ST_ERR_INVALID, "need 2 <= k <= 65535 rows and 1 <= d <= %d", st::kMaxDim);
    return hip_check(st::launch_pdist(rows, k, d, out, static_cast<hipStream_t>(stream)), "pdist launch");
}

// workspace of st_run_starts / st_run_compact: [0, 8) the run count (int64), then the per-tile
// counts and offsets (int32 each)
int64_t st_run_workspace_bytes(int64_t n) {
    if (n < 1) return 16;
    return (8 + 8 * st::run_tiles(n) + 15) / 16 * 16;
}

int st_run_starts(const double* x_soa, const double* g_soa, const double* weights, int64_t n, int32_t d,
                  int64_t ld, uint8_t* starts_out, void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    if (n > 0x7FFFFFFFll) return fail(ST_ERR_UNSUPPORTED, "n >= 2^31 rows");
    if (!starts_out || !workspace) return fail(ST_ERR_INVALID, "NULL output/workspace");
    if (!aligned16(workspace)) return fail(ST_ERR_INVALID, "workspace must be 16-byte aligned");
    if (workspace_bytes < st_run_workspace_bytes(n))
        return fail(ST_ERR_INVALID, "workspace too small (%lld < %lld)", (long long)workspace_bytes,
                    (long long)st_run_workspace_bytes(n));
    int64_t* count = static_cast<int64_t*>(workspace);
    int32_t* tile_count = reinterpret_cast<int32_t*>(count + 1);
    int32_t* tile_off = tile_count + st::run_tiles(n);
    return hip_check(st::launch_run_starts(x_soa, g_soa, weights, n, d, ld, starts_out, tile_count, tile_off,
                                           count, static_cast<hipStream_t>(stream)),
                     "run-start launch");
}

int st_run_compact(const double* x_soa, const double* g_soa, const double* weights, int64_t n, int32_t d,
                   int64_t ld, const uint8_t* starts, const void* workspace, int64_t count, int64_t ld_out,
                   double* x_out, double* g_out, double* w_out, int32_t* rows_out, void* stream) {
    int rc = check_problem(x_soa, g_soa, weights, n, d, ld);
    if (rc) return rc;
    if (n > 0x7FFFFFFFll) return fail(ST_ERR_UNSUPPORTED, "n >= 2^31 rows");
    if (!starts || !workspace || !x_out || !g_out || !rows_out || (weights && !w_out))
        return fail(ST_ERR_INVALID, "NULL input/output");
    if (count < 1 || count > n || ld_out < count || (ld_out & 7))
        return fail(ST_ERR_INVALID, "need 1 <= count <= n and ld_out >= count, a multiple of 8");
    const int32_t* tile_off = reinterpret_cast<const int32_t*>(static_cast<const int64_t*>(workspace) + 1) +
                              st::run_tiles(n);
    return hip_check(st::launch_run_compact(x_soa, g_soa, weights, n, d, ld, starts, tile_off, count, ld_out,
                                            x_out, g_out, weights ? w_out : nullptr, rows_out,
                                            static_cast<hipStream_t>(stream)),
                     "run-compact launch");
}

int st_rank_normalize(const double* sorted, const int64_t* perm, int64_t vars, int64_t count, double* p_out,
                      double* z_out, void* stream) {
    if (!sorted || !perm || !z_out) return fail(ST_ERR_INVALID, "NULL pointer");
    if (!aligned8(sorted) || !aligned8(perm) || !aligned8(z_out) || (p_out && !aligned8(p_out)))
        return fail(ST_ERR_INVALID, "device arrays must be 8-byte aligned");
    if (vars < 1) return fail(ST_ERR_INVALID, "vars must be >= 1 (got %lld)", (long long)vars);
    if (count < 1) return fail(ST_ERR_INVALID, "count must be >= 1 (got %lld)", (long long)count);
    if (count > ((int64_t)1 << 38) / vars) return fail(ST_ERR_UNSUPPORTED, "vars * count exceeds 2^38");
    st::RankArgs a{sorted, perm, vars, count, p_out, z_out};
    return hip_check(st::launch_rank_normalize(a, static_cast<hipStream_t>(stream)), "rank-normalize launch");
}

int64_t st_autocov_workspace_bytes(int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int32_t plan) {
    if (check_autocov_shape(groups, S, h, lag0, lag1, plan)) return -1;
    return st::autocov_ws_bytes(groups, S, h, lag0, lag1, plan);
}

int st_autocov(const double* series, int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int32_t plan,
               double* acov_mean, double* series_mean, double* series_var0, double* acov_series, void* workspace,
               int64_t workspace_bytes, void* stream) {
    if (!series || !acov_mean || !series_mean || !series_var0 || !workspace)
        return fail(ST_ERR_INVALID, "NULL pointer");
    if (!aligned8(series) || !aligned8(acov_mean) || !aligned8(series_mean) || !aligned8(series_var0) ||
        !aligned8(workspace) || (acov_series && !aligned8(acov_series)))
        return fail(ST_ERR_INVALID, "device arrays must be 8-byte aligned");
    int rc = check_autocov_shape(groups, S, h, lag0, lag1, plan);
    if (rc) return rc;
    const int64_t need = st::autocov_ws_bytes(groups, S, h, lag0, lag1, plan);
    if (workspace_bytes < need)
        return fail(ST_ERR_INVALID, "workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)need);
    st::AutocovArgs a{series, groups, S, h, lag0, lag1, plan, acov_mean, series_mean, series_var0, acov_series,
                      static_cast<double*>(workspace)};
    return hip_check(st::launch_autocov(a, static_cast<hipStream_t>(stream)), "autocov launch");
}

int st_autocov_plan(int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int32_t plan) {
    if (check_autocov_shape(groups, S, h, lag0, lag1, plan)) return -1;
    return st::autocov_plan(groups, S, h, lag0, lag1, plan);
}

}  // extern "C"
