/*
 * stein_thinning_hip.h -- C ABI of the MI355X (gfx950) Stein-thinning engine.
 *
 * Drop-in boundary for the hot path of the reference's third-party dependency `stein_thinning`
 * (imported at code/src/thinning.py:5, code/src/utils/ksd.py:5-6, code/tests/test_ksd.py:3 of
 * aglebov/gradient-free-mcmc-postprocessing).  The Python shim package `stein_thinning`
 * (gradient-free-mcmc-postprocessing_amd/stein_thinning) binds these symbols with ctypes; see
 * INTEGRATION.md for the binding a maintainer adds.
 *
 * Conventions (all functions):
 *   - plain C types only; device pointers are HIP device memory owned by the caller;
 *   - `stream` is a hipStream_t (NULL = default stream); every function is asynchronous on it,
 *     allocates nothing and never synchronises (graph-capturable) -- except the one-time
 *     multi-GPU setup calls st_mailbox_alloc / st_mailbox_free / st_ipc_*, which are synchronous;
 *   - sample / gradient arrays are SoA: element (i, k) of the (n, d) array lives at p[k * ld + i],
 *     ld a multiple of 8 and >= n (the ABI's requirement, checked; the Python shim pads to a
 *     multiple of 64, one wave's rows, which the kernels do not require); per-row arrays (weights, running sums) have ld entries (rows
 *     n..ld-1 are padding: read, and in the running sums overwritten, never selected);
 *     all device pointers 16-byte aligned;
 *   - the preconditioner is isotropic Gamma^-1 = linv_scale * I ('id', 'med', 'sclmed', float
 *     options of the reference); linv_trace = np.trace(Gamma^-1) computed on the host;
 *     the *_dense entry points take a dense symmetric positive-definite Gamma^-1 instead ('smpcov',
 *     the inverse sample covariance): `linv` = (d, d) row-major doubles on the device, d <= 16
 *     (see "Dense preconditioners" below); symmetry and definiteness are the caller's to check;
 *   - weights == NULL selects the Langevin Stein kernel k_P; weights = w = exp(log q - log p)
 *     (anchored) selects the gradient-free kernel k_PQ(i,j) = w_i w_j k_Q(i,j) (report.tex:390-400);
 *   - return value: ST_OK (0) or a negative ST_ERR_*; st_last_error() describes the last failure
 *     of the calling thread.  No C++ exception crosses the ABI.
 */
#ifndef STEIN_THINNING_HIP_H
#define STEIN_THINNING_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ABI_VERSION 1

#define ST_OK 0
#define ST_ERR_INVALID (-1)     /* bad argument: sizes, null pointers, alignment */
#define ST_ERR_UNSUPPORTED (-2) /* e.g. d > 128; a dense preconditioner with d > 16 */
#define ST_ERR_HIP (-3)         /* HIP runtime error (launch / memset) */

int st_abi_version(void);
const char *st_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Greedy selection -- replaces stein_thinning.thinning._greedy_search(n_points, integrand)
 * (restated at code/notebooks/examples/JAX_Stein_Thinning.ipynb cell 22, json lines ~281-295;
 * Algorithm 3, report/report.tex:413-426) for the integrands built by _make_stein_integrand /
 * _make_stein_gf_integrand (called at code/src/utils/ksd.py:25, Gaussian_mixture.ipynb cell 93).
 * ---------------------------------------------------------------------------------------- */

/* bytes of device workspace st_greedy / st_greedy_steps / st_greedy_step need (no zeroing needed) */
int64_t st_greedy_workspace_bytes(int64_t n, int32_t d, int32_t nranks);

/*
 * Kernel-variant tuning (process-wide, host side; for measurement sweeps -- defaults are the
 * measured best on MI355X): key 0 = grid cap (blocks, 1..1024), key 1 = candidates per lane
 * (1, 2, 4; d = 2 and 4 kernels; -1 = automatic), key 2 = register prefetch of the next tile
 * (0/1; -1 = automatic), key 3 = persistent kernel register rows per thread (4, 8 on 512-thread blocks;
 * 1, 2, 4 on 256-thread blocks; -1 = automatic: 1 / 2 for blocks of at most 256 / 512 rows, 4 on other
 * 256-thread blocks, 8 on 512-thread blocks unless that leaves slots empty, then 4; 0 = disable the
 * persistent kernel; round 6 pruned the plans that won nothing), key 4 = persistent kernel threads per
 * block (256, 512; -1 = automatic: 512 with dynamic chunks above 1280 rows per block), key 5 = persistent kernel grid cap (blocks per device,
 * 1..256; -1 = one per CU), key 6 = grid cap of the d > 8 step kernel (1..1024), key 7 = proxy
 * kernel (0 = automatic: matrix cores for 16 < d <= 64; 1 = always the VALU kernel), key 8 =
 * persistent kernel blocks per CU (1 / -1 only: the two-block plans were pruned in round 6), key 9 = persistent kernel
 * record pitch in bytes (power of two, 16..4096; -1 = automatic = 256 with one replica, 16 with
 * several, narrowed to what the workspace holds), key 10 = persistent kernel record replicas
 * (power of two, 1..32: every block stores its per-step record into each replica and block b
 * sweeps replica b % replicas; -1 = automatic), key 11 = arithmetic of the d <= 8 greedy kernels
 * (1 = compact, the default: the kernel value regrouped around one reciprocal square root, a few
 * ulps from NumPy's evaluation, for every pair whose two rows and l, tr lie in [2^-60, 2^60];
 * 0 = exact: NumPy's evaluation order rounding for rounding; other pairs are always exact -- see
 * oracle/stein_ref.c and DESIGN.md §3; all ranks of a sharded run must use the same value), key 12 =
 * register rows per thread of the one-device compact-only persistent kernel, used from 8 x 512 rows per
 * block (8, 9; 0 = do not use it; -1 = automatic: 9, or 8 under the near-tie guard), key 13 = energy-distance kernel variant (0 / -1 = automatic = 1:
 * one partial sum per thread, 4 blocks per CU; 2..5: more partial sums or 8 blocks per CU; 6: the
 * round-2 zero-distance select -- measured alternatives; same distances, sums within
 * rounding), key 14 = energy-distance work units: grid blocks (256 columns x one B chunk) that
 * st_distance_colsum_ws aims for (256 .. 2^22; -1 = automatic = 32768; the B range is split into
 * that many / ceil(na / 256) chunks of at least 1024 points -- sums within rounding), key 15 = the
 * 512-thread persistent kernels keep the streamed rows' running sums in LDS (1) instead of HBM (0;
 * -1 = automatic: 1 under the near-tie guard, whose rescans read them every step, else 0 -- measured
 * slower there; same results), key 16 = persistent kernels:
 * ticks of the 100 MHz s_memrealtime clock added to a step's first winner poll before it is aligned
 * to the chip-wide poll grid (0 .. 450; -1 = automatic = 10 for the one-device compact-only kernel,
 * 0 otherwise;
 * timing only, same results), key 17 = LV gradient phase B: 1 reads the observation times / data
 * from global memory as round 3 did (0 / -1 = automatic: staged in LDS when 3 t_n doubles fit
 * 64 KB; same results), key 18 = LV gradient phase B: observation pieces per lane (1, 2, 3; -1 =
 * automatic; the per-point sum is reassociated differently, within the 1e-8 tolerance), key 19 =
 * 512-thread persistent kernels: two LDS-row chunks computed as two independent chains (1 / -1 =
 * automatic) or one after the other (0; same results), key 20 = near-tie guard of the compact
 * arithmetic (1 / -1 = on, the default; 0 = off; see st_greedy_near_tie; same indices and sums), key 22 = key 11 for the
 * launches of the CALLING HOST THREAD only (-1 = none: key 11 applies; 0 / 1 as key 11) -- the library keeps
 * it per thread, so threads thinning side by side (one per GPU) never change each other's arithmetic, key
 * 23 = key 5 for the calling host thread only (-1 = none; 1..512 blocks), key 24 = power path of the
 * Student-t KDE (st_kde_t_logpdf_grad): 0 / -1 = automatic (a multiplication chain when df + d is an integer
 * of at most 256, exp(h log) otherwise), 1 = exp(h log) for every df, 2 = the chain with a run-time exponent for
 * every df (d <= 8: no sweep compiled for the exponent) -- the two A/Bs of DESIGN.md; within rounding.
 */
int st_tune(int32_t key, int32_t value);

/* the current value of a greedy-kernel st_tune key (0 .. 6, 8 .. 12, 15, 16, 19, 20, 22, 23; -1 = automatic);
 * INT32_MIN for other keys (save / restore around a temporary setting).
 * Keys 100 .. 110 are read-only (st_tune rejects them): the persistent-kernel plan the CALLING HOST THREAD
 * last made for a launch of one thin (st_greedy / st_greedy_sharded; not the eligibility query
 * st_greedy_sharded_supported, and not st_greedy_batch, whose chains share one grid), every one -1 before the thread has planned anything -- 100 = blocks,
 * 101 = rows per block, 102 = 1 if the compact-only kernel runs first (the general kernel gated behind
 * it), 103 = 1 if the near-tie GUARD kernels were chosen; of the kernel that runs first: 104 = threads per
 * block, 105 = register rows per thread, 106 = LDS rows per block, 107 = 1 if the streamed rows' sums live
 * in LDS (key 15's decision); of the general kernel (the same kernel when 102 = 0): 108 = register rows,
 * 109 = LDS rows, 110 = streamed sums in LDS.  Rows of a block, by offset: register rows
 * [0, register rows x threads), then the LDS rows, then the streamed rows up to rows per block. */
int32_t st_tune_get(int32_t key);

/* doubles per rank-candidate record {value, global index bits, x[d], g[d], w} (even) */
int64_t st_candidate_stride(int32_t d);

/*
 * Whole greedy run on one device: idx_out[0..n_points) (device, uint32) receives the selected
 * row indices exactly as the reference's `thin` / `thin_gf` / `_greedy_search` return them;
 * a_work (ld doubles, device) ends holding the running sums A after the last step.
 * For d = 2 and 4 the run is ONE launch of the persistent on-chip-resident kernel (grid checked
 * against the occupancy query first)
 * (one block per CU; rows held in VGPRs/LDS across steps); if its internal bounded wait times
 * out, the unwritten entries of idx_out are set to UINT32_MAX (callers check idx < n).
 * Other d: one fused launch per step.
 */
int st_greedy(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
              int32_t d, int64_t ld, double linv_scale, double linv_trace, int64_t n_points,
              uint32_t *idx_out, double *a_work, void *workspace, int64_t workspace_bytes,
              void *stream);

/*
 * Near-tie guard of the compact arithmetic (st_tune key 20).  A guarded run (the compact arithmetic, d = 2
 * or 4; persistent kernel, batch and multi-rank included) flags the first step t whose selection the
 * arithmetic could have decided differently from the reference's NumPy evaluation: the smallest running
 * sum of any row other than the winner and the rows equal to it bit for bit (x, g, w: repeated MCMC rows,
 * adjacent or not, tie in every arithmetic and lose to the lower index on both paths) -- any other exact
 * tie included -- within thr(t) of the winner's, thr(t) a bound on how far two rows' sums may move between
 * the compact arithmetic, the exact one and NumPy's (oracle/stein_ref.c sr_greedy_mt_ties states the rule
 * and the bound; the reference's argmin is JAX_Stein_Thinning.ipynb:291-292, np.argmin of the running
 * sums).  A multi-rank run (st_greedy_sharded) flags in each rank's workspace the steps its own rows
 * flag against the global winner (bounds over all n rows): the first flagged step of the thin is the
 * minimum over the ranks (one all-reduce after the run).  Reads the workspace of a completed st_greedy /
 * st_greedy_batch / st_greedy_sharded problem after synchronising `stream` (the one exception to the
 * enqueue-only rule: a few bytes come back): *step_out = the first flagged step, -1 when none, -2 when the
 * run was not guarded (exact arithmetic, guard off, other d, or the launch-per-step kernels).  Callers
 * re-run a flagged thin with the exact arithmetic (st_tune key 11 = 0, or key 22 for the calling thread).
 */
int st_greedy_near_tie(const void *workspace, int64_t workspace_bytes, int64_t *step_out, void *stream);

/*
 * Up to 8 independent whole greedy runs of one d (2 or 4) and one n_points in ONE launch of the
 * persistent kernel: problem q gets about #CU / count blocks and runs on them exactly as st_greedy
 * would on a grid of that many blocks -- idx_out[q] and a_work[q] as st_greedy's, same indices.
 * The arrays are host arrays of count entries (device pointers / sizes per problem, as st_greedy
 * takes them); weights is NULL or has an entry for every problem.  Returns ST_ERR_UNSUPPORTED
 * (nothing enqueued) when the problems do not all plan onto the same kernel at that grid (threads
 * per block and register rows follow each problem's rows per block, as in st_greedy; e.g. a 2e5-row
 * problem next to a 2e4-row one); the caller then runs st_greedy per problem.  A timed-out
 * run poisons its own idx_out only.  Replaces the reference's loop of thin() calls over chains
 * (Stein_thinning.ipynb; code/src/utils/parallel.py:48-52 fans them out to processes).
 */
int st_greedy_batch(int32_t count, const double *const *x_soa, const double *const *g_soa,
                    const double *const *weights, const int64_t *n, int32_t d, const int64_t *ld,
                    const double *linv_scale, const double *linv_trace, int64_t n_points,
                    uint32_t *const *idx_out, double *const *a_work, void *const *workspace,
                    const int64_t *workspace_bytes, void *stream);

/*
 * Steps [t_begin, t_end) of the same single-device run (t = 0 is the diagonal); when t_end ==
 * n_points the finalize kernel writing idx_out[n_points-1] follows.  The workspace carries the
 * per-block candidate records between calls, so consecutive ranges on one stream compose into
 * st_greedy.  Used to time single step launches.
 */
int st_greedy_steps(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                    int32_t d, int64_t ld, double linv_scale, double linv_trace, int64_t t_begin,
                    int64_t t_end, int64_t n_points, uint32_t *idx_out, double *a_work,
                    void *workspace, int64_t workspace_bytes, void *stream);

/*
 * One greedy step of a row-sharded run (multi-GPU; one process per GPU).  This rank holds rows
 * [row_offset, row_offset + n) of the global sample.  Step t = 0 evaluates the diagonal; step
 * t >= 1 reads the R = nranks candidate records of step t-1 (cands_in, R * stride doubles),
 * writes idx_out[t-1] and updates the running sums.  Every step writes this rank's candidate
 * record (stride doubles) to cand_out; the caller all-gathers the records (RCCL) into the next
 * step's cands_in.
 * After the last step, st_greedy_finalize writes idx_out[n_points-1].
 */
int st_greedy_step(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                   int32_t d, int64_t ld, double linv_scale, double linv_trace,
                   int64_t row_offset, int64_t t, int32_t nranks, const double *cands_in,
                   double *cand_out, uint32_t *idx_out, double *a_work, void *workspace,
                   int64_t workspace_bytes, void *stream);

int st_greedy_finalize(const double *cands_in, int32_t nranks, int32_t d, uint32_t *idx_out,
                       int64_t t, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU greedy with device-side exchange (one process per GPU of one node, up to 8).
 * Same result as st_greedy on the whole sample (and as the reference's _greedy_search).
 *
 * Every rank holds the FULL standardised arrays (replicated, read-only: the winner's row is then
 * local) and runs ONE persistent launch over its row block [row_begin, row_end).  Per step the
 * ranks exchange their local winners {A_min, global index} through per-rank mailboxes: each rank
 * allocates one (st_mailbox_alloc: uncached device memory), exports it (st_ipc_get_handle), the
 * handles are all-gathered out of band (torch.distributed), each rank maps its peers'
 * (st_ipc_open_handle) and passes the table peer_mailboxes[0..nranks) (its own at [rank]).
 * st_mailbox_handshake verifies the round trip (ok_device[0] = 1) before the first run.
 * seq_base: exchange sequence number of this run's step 0; every rank passes the same value and
 * a following run on the same mailboxes uses seq_base + n_points.
 * Returns ST_ERR_UNSUPPORTED when d is not 2 or 4, or d = 50 with more than 256 rows per CU in
 * this rank's block (use st_greedy_step_exchange or st_greedy_step + RCCL instead); a run
 * whose peers do not answer within the kernel's bounded waits poisons idx_out (UINT32_MAX).
 * ---------------------------------------------------------------------------------------- */
int64_t st_mailbox_bytes(int32_t nranks);
int st_mailbox_alloc(int64_t bytes, void **mailbox);
int st_mailbox_free(void *mailbox);
int st_ipc_handle_bytes(void);
int st_ipc_get_handle(void *dev_ptr, void *handle_out);
int st_ipc_open_handle(const void *handle, void **dev_ptr);
int st_ipc_close_handle(void *dev_ptr);
int st_mailbox_handshake(void *const *peer_mailboxes, int32_t nranks, int32_t rank,
                         uint64_t token, int32_t *ok_device, void *stream);
int st_greedy_sharded(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                      int32_t d, int64_t ld, double linv_scale, double linv_trace,
                      int64_t row_begin, int64_t row_end, int32_t rank, int32_t nranks,
                      void *const *peer_mailboxes, uint64_t seq_base, int64_t n_points,
                      uint32_t *idx_out, double *a_work, void *workspace,
                      int64_t workspace_bytes, void *stream);
/* 1 if st_greedy_sharded would run this rank's block [row_begin, row_end) on the current device
 * (the launcher's exact decision: d, rows per block against the kernel's register/LDS budget, the
 * st_tune grid cap), 0 if it would return ST_ERR_UNSUPPORTED, < 0 on invalid arguments.  No GPU
 * work; callers agree on it across ranks before choosing the engine. */
int st_greedy_sharded_supported(int64_t n, int32_t d, int32_t has_weights, int64_t row_begin,
                                int64_t row_end, int32_t rank, int32_t nranks, int64_t n_points);
/*
 * Any d (the launch-per-step path of st_greedy_step) with the per-step rank exchange through the
 * same mailboxes instead of an RCCL all-gather: one call = the step kernel over this rank's shard
 * + a one-block exchange kernel that pushes this rank's candidate record into slot `rank` of every
 * peer's mailbox and collects the nranks records of this step into cands (nranks * stride
 * doubles; the next call's input, as st_greedy_step's cands_in).  No host synchronisation or
 * collective inside, so the m-step loop can be captured into one HIP graph and replayed; flags
 * carry a device-side exchange counter, so replays never see stale records.  All ranks must make
 * the same sequence of calls.  A peer that does not answer within the bounded wait (10 s at t = 0,
 * 2 s otherwise) sets status_device[0] = 1; later exchanges then return at once (the indices of
 * that run are garbage and the mailbox set must not be reused).  Finish with st_greedy_finalize
 * (cands, nranks).
 */
int st_greedy_step_exchange(const double *x_soa, const double *g_soa, const double *weights,
                            int64_t n, int32_t d, int64_t ld, double linv_scale, double linv_trace,
                            int64_t row_offset, int64_t t, int32_t rank, int32_t nranks,
                            void *const *peer_mailboxes, double *cands, uint32_t *idx_out,
                            double *a_work, void *workspace, int64_t workspace_bytes,
                            uint32_t *status_device, void *stream);

/* ------------------------------------------------------------------------------------------
 * Proxy producers for thin_gf -- replaces the O(n d^2) host prep of
 *   gaussian_thin (code/src/thinning.py:15-16): scipy.stats.multivariate_normal.logpdf(x, mean,
 *     cov) and -np.einsum('ij,kj->ki', np.linalg.inv(cov), x - mean)           (df = 0)
 *   thin_gf_t (Gradient_free_Student_t.ipynb cells 29, 31, 40): scipy.stats.multivariate_t.logpdf
 *     (x, loc, shape, df) and t_grad_log_pdf(x, loc, shape, df)                (df > 0)
 * x: row-major (n, d) device array (the caller's NumPy layout); loc (d); whiten (d, d) row-major =
 * scipy's _PSD(cov).U; precision (d, d) row-major = np.linalg.inv(cov); c_log = rank * log(2 pi) +
 * log_pdet (Gaussian) or A - B - C - D of scipy's multivariate_t._logpdf (t).  Writes log_q_out (n)
 * and grad_out (row-major (n, d)).  Per-row dot products are summed in a different order than
 * NumPy/BLAS (fp64 rounding, not bit-identical).  For 16 < d <= 64 (the matrix-core kernels) the
 * Mahalanobis term of log_q is evaluated as dev . precision dev, not as scipy's |dev whiten|^2: the
 * two agree up to the gap between the caller's two float64 factors (whiten whiten^T against
 * precision), which is rounding-sized for well-scaled covariances and grows with cond(cov) -- about
 * 7e-9 of the term at cond 2e8.  A row's outputs depend on the row alone (not on n or its position).
 * ---------------------------------------------------------------------------------------- */
int st_proxy_logpdf_grad(const double *x, int64_t n, int32_t d, const double *loc,
                         const double *whiten, const double *precision, double df, double c_log,
                         double *log_q_out, double *grad_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Gaussian mixture -- replaces logpdf / score of make_mvn_mixture (code/src/utils/mvn.py), the
 * target of Gaussian_mixture.ipynb, and serves as a mixture proxy q for thin_gf.  Per row x and
 * component c, with dev_c = x - mu_c, y_c = P_c dev_c, l_c = a_c - dev_c . y_c / 2:
 *   log_p = logsumexp_c l_c,    score = - sum_c exp(l_c - log_p) y_c
 * evaluated in log space (finite where the reference's sum of densities underflows).
 * x: row-major (n, d) device array; log_coef (k): a_c = log w_c - (d log 2 pi + log det Sigma_c) / 2,
 * -inf for a zero weight (the component contributes nothing); means (k, d) row-major; precision
 * (k, d, d) row-major = np.linalg.inv(Sigma_c); all HOST-computed, on the DEVICE.  Writes log_p_out
 * (n) and score_out (row-major (n, d)).  A row holding a NaN or an inf gets NaN outputs, no other
 * row is affected.  A row's outputs depend only on that row and the parameters (not on n or the
 * row's position).  Asynchronous on `stream`, allocates nothing.
 * ST_ERR_INVALID: NULL (x and the outputs may be NULL when n == 0) or not 8-byte aligned pointers,
 * n < 0, d < 1, k < 1.  ST_ERR_UNSUPPORTED: d > 64 or k > 1024.  n == 0: ST_OK, nothing enqueued.
 * All checked before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int st_mixture_logpdf_score(const double *x, int64_t n, int32_t d, int32_t k,
                            const double *log_coef /* k: a_c */, const double *means /* (k, d) */,
                            const double *precision /* (k, d, d) row-major */,
                            double *log_p_out /* n */, double *score_out /* (n, d) row-major */,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * Sample moments of the multivariate-t likelihood -- what one evaluation of the objective of fit_mvt /
 * fit_mvt2 (Gradient_free_Student_t.ipynb: -sum multivariate_t.logpdf(Y, loc, shape, df) under
 * scipy.optimize.minimize) and of its analytic gradient needs from the rows.  With the whitening
 * U (U U^T = inv(shape)), per row z = (x - loc) @ U, delta = |z|^2, w = (df + d) / (df + delta):
 *   S0 = sum log(1 + (1 / df) delta),  S1 = sum w,  Sz = sum w z (d),  Szz = sum w z z^T (symmetric)
 * x: row-major (n, d) device array (the caller's NumPy layout); loc (d) and whiten (d, d) row-major = U
 * on the DEVICE.  out (device, 2 + d + d (d + 1) / 2 doubles): S0, S1, Sz[d], then the upper triangle
 * of Szz row-major; want_grad = 0 computes and writes out[0] = S0 only, the same bits as want_grad = 1.
 * Two launches on `stream` (per-block partial sums into the workspace, then one block adding them in
 * block order): no atomics, the same inputs give the same bits on every call at a given grid (the
 * grid follows n, the device's CU count and the st_tune grid cap, keys 5 / 23).  Allocates nothing.
 * workspace: st_mvt_moments_workspace_bytes(n, d) bytes (host only; -1 if n < 1, d < 1 or d > 16).
 * ST_ERR_INVALID: NULL or not 8-byte aligned pointers, n < 1, d < 1, df not finite or not > 0, a
 * workspace that is too small.  ST_ERR_UNSUPPORTED: d > 16.  All checked before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int64_t st_mvt_moments_workspace_bytes(int64_t n, int32_t d);
int st_mvt_moments(const double *x, int64_t n, int32_t d, const double *loc, const double *whiten,
                   double df, int32_t want_grad,
                   double *out /* device: S0, S1, Sz[d], Szz upper triangle row-major */,
                   void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * One EM pass of a Gaussian-mixture fit (no counterpart in the reference, which never fits a mixture):
 * the log likelihood of the rows under the current parameters and the sufficient statistics of the
 * M-step, centred on the CURRENT means.  Parameters as st_mixture_logpdf_score takes them (log_coef,
 * means, precision, on the DEVICE); row_weights (n, device) non-negative, or NULL for 1.  Per row x_i
 * and component c, dev_ic = x_i - mu_c, l_ic = a_c - dev_ic . (P_c dev_ic) / 2:
 *   log_p_i = logsumexp_c l_ic,   r_ic = exp(l_ic - log_p_i)
 *   LL = sum_i w_i log_p_i,  N_c = sum_i w_i r_ic,  S_c = sum_i w_i r_ic dev_ic (d),
 *   Q_c = sum_i w_i r_ic dev_ic dev_ic^T (symmetric)
 * out (device, 1 + k (1 + d + d (d + 1) / 2) doubles): LL, then per component N_c, S_c[d] and the upper
 * triangle of Q_c row-major.  The M-step is mu_c + S_c / N_c and Q_c / N_c - (S_c / N_c)(S_c / N_c)^T.
 * log_p_out (n, device) or NULL: log_p_i, bit for bit st_mixture_logpdf_score's log_p (NaN for a row
 * holding a NaN or an inf).  A component with a_c = -inf is skipped: its statistics are exactly 0.  A row
 * of weight 0 adds nothing whatever it holds; a non-finite row of positive weight makes LL NaN.
 * Two launches on `stream` (per-block partial sums into the workspace, then their sum in block order):
 * no atomics, the same inputs give the same bits on every call at a given grid (the grid follows n, d,
 * k, the device's CU count and the st_tune grid cap, keys 5 / 23).  Allocates nothing.
 * workspace: st_mixture_em_workspace_bytes(n, d, k) bytes (host only; -1 if n < 1, d < 1, d > 16, k < 1
 * or k > 32; bounded by the grid, not by n).
 * ST_ERR_INVALID: n < 1, d < 1, k < 1, NULL (row_weights and log_p_out may be NULL) or not 8-byte
 * aligned pointers, a workspace that is too small.  ST_ERR_UNSUPPORTED: d > 16 or k > 32.  All checked
 * before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int64_t st_mixture_em_workspace_bytes(int64_t n, int32_t d, int32_t k);
int st_mixture_em_stats(const double *x, int64_t n, int32_t d, int32_t k,
                        const double *log_coef /* k: a_c */, const double *means /* (k, d) */,
                        const double *precision /* (k, d, d) row-major */,
                        const double *row_weights /* n, or NULL */,
                        double *out /* device: LL, then k x {N_c, S_c[d], Q_c upper triangle} */,
                        double *log_p_out /* n, or NULL */,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * KDE proxy -- replaces jax.scipy.stats.gaussian_kde(sample.T, bw_method, weights).logpdf and its
 * jax.grad as the reference's Gaussian-mixture study feeds them to thin_gf (Gaussian_mixture.ipynb
 * cells 42-48, 51).  Whitened data p = x L (n points, SoA (d, ldp)) and queries q = y L (m points,
 * SoA (d, ldq)), L = cholesky(KDE precision) (HOST-computed; `whiten` = L on the DEVICE, (d, d)
 * row-major); log_weights (n, device) or NULL for the uniform log_weight_uniform:
 *   log_q[j] = logsumexp_i(log w_i + log_norm - |p_i - q_j|^2 / 2),
 *   grad[j]  = (sum_i softmax_i(.) p_i - q_j) L^T   (row-major (m, d)).
 * workspace: st_kde_workspace_bytes(m, d) bytes (0 for d <= 8).
 * ---------------------------------------------------------------------------------------- */
int64_t st_kde_workspace_bytes(int64_t m, int32_t d);
int st_kde_logpdf_grad(const double *p_soa, int64_t ldp, int64_t n, const double *log_weights,
                       double log_weight_uniform, const double *q_soa, int64_t ldq, int64_t m, int32_t d,
                       double log_norm, const double *whiten, double *log_q_out, double *grad_out,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Student-t KDE proxy -- the KDE above with the fat-tailed kernel multivariate_t(y; loc = x_i, shape =
 * the KDE's covariance, df) in place of the Gaussian one (the report's "Further Work": KDE kernels other
 * than Gaussian).  Same layout and conventions as st_kde_logpdf_grad, with df added; log_norm is
 *   log_norm_t = sum(log diag L) + lgamma((df + d) / 2) - lgamma(df / 2) - d / 2 log(df pi)   (HOST):
 *   log_q[j] = logsumexp_i(log w_i + log_norm_t - (df + d) / 2 log(1 + |p_i - q_j|^2 / df)),
 *   grad[j]  = (sum_i softmax_i(.) (df + d) / (df + |p_i - q_j|^2) (p_i - q_j)) L^T   (row-major (m, d)).
 * A log weight of -inf drops its point out exactly (its coordinates are not used); all of them -inf gives
 * log_q = -inf.  Nothing underflows where the result is finite, for non-zero weights spanning a ratio of
 * at most 2^900 (the per-query shift is the nearest weighted point and the largest weight; csrc/kde.hip).
 * Deterministic (sums sequential in i, no atomics).  m = 0 is a no-op.
 * workspace: st_kde_t_workspace_bytes(m, d) bytes (0 for d <= 8; -1 if m < 0 or d outside 1 .. 128).
 * ST_ERR_INVALID: NULL pointers, n < 1, m < 0, ldp < n, ldq < m, df not finite or not > 0, a workspace
 * that is too small.  ST_ERR_UNSUPPORTED: d outside 1 .. 128.  All checked before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int64_t st_kde_t_workspace_bytes(int64_t m, int32_t d);
int st_kde_t_logpdf_grad(const double *p_soa, int64_t ldp, int64_t n, const double *log_weights,
                         double log_weight_uniform, const double *q_soa, int64_t ldq, int64_t m, int32_t d,
                         double df, double log_norm, const double *whiten, double *log_q_out, double *grad_out,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Lotka-Volterra inputs, batched over n parameter points (one RK45 integration per point, scipy's
 * solve_ivp algorithm step for step -- code/src/lotka_volterra.py):
 *   st_lv_grad_log_posterior: grad_out (n, 4) row-major = grad_log_posterior(theta) of
 *     Sensitivity_analysis.ipynb cells 40, 46 (forward sensitivities, solve_ivp(
 *     lotka_volterra_sensitivity, ..., dense_output=True).sol(t));
 *   st_lv_log_target_density: out (n) = lotka_volterra.log_target_density(log_theta) (2-state
 *     system), theta = exp(log_theta) computed by the caller (NumPy's exp, as the reference).
 * theta, log_theta: (n, 4) row-major device arrays; t_eval (t_n) ascending and y_obs (t_n, 2)
 * row-major: the observation times and data (device); span_u0_tol: HOST array {t0, t1, u0_1,
 * u0_2, rtol, atol}; cov_inv: HOST (2, 2) row-major inv(C); whiten: HOST (2, 2) row-major scipy
 * _PSD(C).U with c_log = rank * log(2 pi) + log_pdet; norm_logc = log(sqrt(2 pi)) (scipy.stats.norm).
 * status (n, device): 0 ok, 1 step size fell below scipy's min_step (output NaN), 2 max_steps
 * reached (output NaN).  Results agree with scipy to rounding (BLAS summation orders differ).
 * ---------------------------------------------------------------------------------------- */
int st_lv_grad_log_posterior(const double *theta, int64_t n, const double *t_eval, int32_t t_n,
                             const double *y_obs, const double *span_u0_tol, const double *cov_inv,
                             int64_t max_steps, double *grad_out, int32_t *status, void *stream);
/* Two-phase form of st_lv_grad_log_posterior (same arguments and results, faster): the integration
 * records each accepted step's dense-output polynomial in the workspace and the observation points
 * are evaluated one wave per parameter point; workspace: st_lv_grad_workspace_bytes(n, t_n) bytes
 * of device memory. */
int64_t st_lv_grad_workspace_bytes(int64_t n, int32_t t_n);
int st_lv_grad_log_posterior_ws(const double *theta, int64_t n, const double *t_eval, int32_t t_n,
                                const double *y_obs, const double *span_u0_tol, const double *cov_inv,
                                int64_t max_steps, double *grad_out, int32_t *status, void *workspace,
                                int64_t workspace_bytes, void *stream);
int64_t st_lv_log_density_workspace_bytes(int64_t n, int32_t t_n);
int st_lv_log_target_density(const double *log_theta, const double *theta, int64_t n,
                             const double *t_eval, int32_t t_n, const double *y_obs,
                             const double *span_u0_tol, const double *whiten, double c_log,
                             double norm_logc, int64_t max_steps, double *out, int32_t *status,
                             void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Random-walk Metropolis sampler for the LV log posterior (Sampling.ipynb's hand-written loop over
 * lotka_volterra.log_target_density), batched over chains: one thread per chain, `steps` Metropolis
 * steps per launch inside the kernel (csrc/lv_mcmc.hip).  At global step t = first_step + k a chain
 * proposes p = x + step_size * z (one multiply, one add per component), evaluates
 * lp_new = log_target_density(p) as st_lv_log_target_density does (theta = exp(p) on the device; the
 * sum over the observation times in time order), accepts exactly when log_u < lp_new - lp, and writes
 * row out_row0 + k of samples (chains, out_ld, 4) and log_p (chains, out_ld).  A proposal whose theta
 * has a zero or non-finite component, or whose integration fails, is rejected and counted.
 *   state: st_lv_rwmh_workspace_bytes(chains) = 64 chains bytes of device memory, 8 words per chain:
 *     x[4], lp, accepted (int64), n_failed (int64), one unused; read at launch start, written at launch
 *     end, so consecutive launches continue the chains.  init = 1 (first_step must be 1): the kernel
 *     first evaluates lp of the state's x (lp NaN when that fails), writes the start as row
 *     out_row0 - 1; the caller zeroes the counts.
 *   noise_mode 0: z (chains, noise_ld, 4) and log_u (chains, noise_ld) are read, step k from row
 *     noise_row0 + k.  1: NumPy's Philox4x64-10 on the device, key (seed, first_chain + chain), step t
 *     from the blocks with counter word 0 = 2t - 1 and 2t, i.e. random_raw values r0 .. r7 =
 *     np.random.Philox(key=[seed, c], counter=[0, 0, 0, 0]).random_raw(8 t)[8 (t - 1):]:
 *     u_k = ((r_k >> 11) + 1) 2^-53, (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1), (z2, z3) from u2, u3,
 *     log_u = log((r4 >> 11) 2^-53); z and log_u may be NULL.  2: as 1, and the noise used is written
 *     to z / log_u.
 *   step_size: HOST (4); span_u0_tol, whiten, c_log, norm_logc: as st_lv_log_target_density.
 * ST_ERR_INVALID (all checked before any HIP call): NULL or misaligned pointers (state, samples, z: 16
 * bytes; the others 8), chains < 1, steps < 1, t_n < 1, first_step < 1, first_chain < 0, a step size
 * that is not finite or <= 0, noise_mode 0 or 2 without noise arrays, rows outside the arrays.
 * ---------------------------------------------------------------------------------------- */
int64_t st_lv_rwmh_workspace_bytes(int64_t chains);
int st_lv_rwmh(double *state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
               int32_t init, const double *step_size, int32_t noise_mode, uint64_t seed, double *z,
               double *log_u, int64_t noise_ld, int64_t noise_row0, const double *t_eval, int32_t t_n,
               const double *y_obs, const double *span_u0_tol, const double *whiten, double c_log,
               double norm_logc, int64_t max_steps, double *samples, double *log_p, int64_t out_ld,
               int64_t out_row0, void *stream);
/* The same sampler with one WAVE (64 lanes) per chain, for a few long chains (the reference's 5 chains of
 * 500 000 rows): the arguments, the checks, the state record and the workspace of st_lv_rwmh, so launches of
 * either entry point may continue a chain.  Every lane of a wave holds the chain's state, reads or draws the
 * step's noise, forms the proposal and runs the RK45 integration (same inputs, same instructions); lane l
 * evaluates the observation points k = l (mod 64), with st_lv_rwmh's per-point values bit for bit.
 * Summation order (part of the contract): lane l adds its terms to 0.0 in increasing k; the 64 partial sums
 * are combined by the xor butterfly v += shuffle_xor(v, off) for off = 32, 16, 8, 4, 2, 1; then the prior term
 * is added.  The order depends on t_n only, never on the RK45 step sequence, the grid or the launch split.
 * Bit-identical to st_lv_rwmh: proposals, device noise, and log_p for t_n <= 2 (the two orders coincide).
 * For t_n >= 3 log_p differs by the summation order alone (~1e-13 relative), and the chains are equal row for
 * row as long as no accept / reject decision is closer than that. */
int st_lv_rwmh_wave(double *state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                    int32_t init, const double *step_size, int32_t noise_mode, uint64_t seed, double *z,
                    double *log_u, int64_t noise_ld, int64_t noise_row0, const double *t_eval, int32_t t_n,
                    const double *y_obs, const double *span_u0_tol, const double *whiten, double c_log,
                    double norm_logc, int64_t max_steps, double *samples, double *log_p, int64_t out_ld,
                    int64_t out_row0, void *stream);

/* ------------------------------------------------------------------------------------------
 * Metropolis-adjusted Langevin (MALA) sampler for the LV log posterior, one WAVE per chain
 * (csrc/lv_mcmc.hip: lv_mala_wave_kernel).  The reference's gradient-based sampler is Stan's HMC, which is not
 * part of its tree; the sampler is this project's own definition:
 *   The chain runs in x = log theta.  eps is the step size; the HOST computes h = 0.5 eps eps,
 *   w = 0.5 / (eps eps) and c = drift_cap eps (+inf: no cap) once and hands them over as doubles.  All device
 *   arithmetic below is uncontracted.  ONE 10-state RK45 integration (the system with its forward
 *   sensitivities, as st_lv_grad_log_posterior) at theta = exp(x) (the device's exp) gives u and J = du/dtheta at
 *   the observation times, and from them
 *     lp(x)  = sum_k mvn.logpdf(y_k - u_k, 0, C) + sum_j norm.logpdf(x_j)   (the terms of st_lv_rwmh)
 *     acc_j  = sum_k (J_k^T C^-1 (y_k - u_k))_j           (st_lv_grad_log_posterior's per-point expression)
 *     g_j(x) = theta_j acc_j - x_j          (= exp(x) * grad_log_posterior(exp(x)) to rounding)
 *   lp comes from the 10-state solution, whose step sequence is not the 2-state one of
 *   st_lv_log_target_density / st_lv_rwmh: the two differ by the integrator's tolerance, not by rounding.
 *   One Metropolis step at global step t = first_step + k:
 *     d_j(x) = min(max(h_j g_j(x), -c_j), c_j)
 *     p_j    = (x_j + d_j(x)) + eps_j z_j
 *     rf_j   = (p_j - x_j) - d_j(x),   rr_j = (x_j - p_j) - d_j(p)
 *     qf     = sum_j w_j rf_j rf_j,    qr = sum_j w_j rr_j rr_j     (each ((w rf) rf), from 0.0, j ascending)
 *     accept exactly when log_u < (lp(p) - lp(x)) + (qf - qr)       (strict; a NaN anywhere rejects)
 *   A theta with a zero or non-finite component, or an integration that ends with a non-zero status, rejects
 *   and counts in n_failed.  Row out_row0 + k of samples, log_p and grad (= g of that row) is written.
 * Layout: every lane of the wave holds the state (x, lp, g), forms the proposal and runs the integration; lane l
 * evaluates the observation points k = l (mod 64).  Summation order (part of the contract): lane l adds its
 * terms to 0.0 in increasing k -- one sum for the likelihood, one for each acc_j; each of the five is combined
 * by the xor butterfly v += shuffle_xor(v, off) for off = 32, 16, 8, 4, 2, 1; then the prior term is added.  The
 * order depends on t_n only, never on the RK45 step sequence, the grid or the launch split.
 * Arguments as st_lv_rwmh_wave (noise modes, Philox keys and counters, init, first_step, first_chain, out_row0,
 * noise_row0 included: for one seed the noise is st_lv_rwmh's), except:
 *   state: st_lv_mala_workspace_bytes(chains) = 128 chains bytes, 16 words per chain: x[4], lp, accepted
 *     (int64), n_failed (int64), one spare, g[4], four spare.
 *   step_ehw: HOST (12) = eps[4], h[4], w[4];  drift_clip: HOST (4) = c (may be +inf);
 *   cov_inv: HOST (2, 2) inv(C) row-major;  grad: (chains, out_ld, 4) device output.
 * ST_ERR_INVALID (all checked before any HIP call): the conditions of st_lv_rwmh (eps is its step size); grad
 * NULL or not 16-byte aligned; drift_clip or cov_inv NULL; an h or w that is not finite or <= 0; a c that is
 * NaN or <= 0.
 * ---------------------------------------------------------------------------------------- */
int64_t st_lv_mala_workspace_bytes(int64_t chains);
int st_lv_mala_wave(double *state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                    int32_t init, const double *step_ehw, const double *drift_clip, int32_t noise_mode,
                    uint64_t seed, double *z, double *log_u, int64_t noise_ld, int64_t noise_row0,
                    const double *t_eval, int32_t t_n, const double *y_obs, const double *span_u0_tol,
                    const double *whiten, double c_log, double norm_logc, const double *cov_inv,
                    int64_t max_steps, double *samples, double *log_p, double *grad, int64_t out_ld,
                    int64_t out_row0, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hamiltonian Monte Carlo (HMC) sampler for the LV log posterior, one WAVE per chain
 * (csrc/lv_mcmc.hip: lv_hmc_wave_kernel): a Metropolis step whose proposal is a trajectory of n_leapfrog
 * leapfrog stages; st_lv_mala_wave's proposal is its one-stage case up to rounding.  Stan's sampler is not part
 * of the reference's tree; this is the project's own definition:
 *   The chain runs in x = log theta with unit-variance momenta.  eps[4] is the step size (a vector eps is a
 *   diagonal mass matrix), c[4] the kick cap (+inf: none), L = n_leapfrog >= 1.  lp(x) and g(x) are
 *   st_lv_mala_wave's (one 10-state integration at theta = exp(x), the same summation order).  All device
 *   arithmetic is uncontracted and in this order, at global step t = first_step + k:
 *     kick_j(q) = min(max(eps_j g_j(q), -c_j), c_j)     (two comparisons: a NaN stays a NaN)
 *     hk_j(q)   = 0.5 kick_j(q)
 *     r^0 = z, the step's four normals;   K(r) = 0.5 s,  s = sum_j r_j r_j from 0.0, j ascending
 *     stage l = 1 .. L from (q^0, r^0) = (x, z):
 *       r'  = r^(l-1) + hk(q^(l-1))
 *       q^l = q^(l-1) + eps r'                           (one multiply and one add per component)
 *       lp(q^l), g(q^l)
 *       r^l = r' + hk(q^l)
 *     accept exactly when log_u < (lp(q^L) - lp(x)) + (K(r^0) - K(r^L))    (strict; a NaN anywhere rejects)
 *   An interior kick is two half-kick additions, so a trajectory of L stages is, bit for bit, L one-stage
 *   trajectories chained through (q, r).  The capped force depends on q alone: every stage stays a shear, the
 *   map reversible and volume-preserving, and with the true lp in the ratio the chain targets the posterior.
 *   A stage fails when its theta has a zero or non-finite component or its integration ends with a non-zero
 *   status; its NaN gradient carries through the later q of the trajectory, whose stages run no integration;
 *   the trajectory is rejected and counted ONCE in n_failed.  Row out_row0 + k of samples, log_p and grad
 *   (= g of that row) is written.
 * Arguments as st_lv_mala_wave (layout, summation order, noise modes, Philox keys and counters, init,
 * first_step, first_chain, out_row0, noise_row0 and the 16-word state record included: for one seed the noise
 * is st_lv_rwmh's), except:
 *   state: st_lv_hmc_workspace_bytes(chains) = 128 chains bytes;
 *   step_eps: HOST (4) = eps;  kick_clip: HOST (4) = c (may be +inf);  n_leapfrog: L.
 * ST_ERR_INVALID (all checked before any HIP call): the conditions of st_lv_rwmh (eps is its step size); grad
 * NULL or not 16-byte aligned; kick_clip or cov_inv NULL; a c that is NaN or <= 0; n_leapfrog < 1.
 * ---------------------------------------------------------------------------------------- */
int64_t st_lv_hmc_workspace_bytes(int64_t chains);
int st_lv_hmc_wave(double *state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                   int32_t init, const double *step_eps, const double *kick_clip, int32_t n_leapfrog,
                   int32_t noise_mode, uint64_t seed, double *z, double *log_u, int64_t noise_ld,
                   int64_t noise_row0, const double *t_eval, int32_t t_n, const double *y_obs,
                   const double *span_u0_tol, const double *whiten, double c_log, double norm_logc,
                   const double *cov_inv, int64_t max_steps, double *samples, double *log_p, double *grad,
                   int64_t out_ld, int64_t out_row0, void *stream);

/* ------------------------------------------------------------------------------------------
 * HMC with a per-chain step size, a per-chain dense metric and step-size adaptation, one WAVE per chain
 * (csrc/lv_mcmc.hip: lv_hmc_metric_wave_kernel).  st_lv_hmc_wave's definition with three
 * additions, every device operation uncontracted and in this order:
 *   (1) eps is one double per chain and the metric a per-chain factor Lam, lower triangular with M^-1 = Lam Lam^T.
 *       The momentum stays r ~ N(0, I) (the noise and K(r) are st_lv_hmc_wave's).  In a stage
 *         f_j(q)    = Lam_jj g_j(q) + sum_{k > j} Lam_kj g_k(q)      (the first term alone, then k ascending)
 *         kick_j(q) = min(max(eps f_j(q), -c_j), c_j),  hk = 0.5 kick
 *         r' = r + hk(q);  v_j = sum_{k <= j} Lam_jk r'_k (from the k = 0 term, k ascending);  q_j <- q_j + eps v_j
 *         r  = r' + hk(q) at the new q
 *       and the accept, failure and NaN rules are st_lv_hmc_wave's.  With Lam = I and one eps for all chains the
 *       rows, log_p, grad and counts are st_lv_hmc_wave's bit for bit.
 *   (2) per step, accept_stat = alpha = min(1, exp(a)), a = (lp(q^L) - lp(x)) + (K(r^0) - K(r^L)), 0 when a is NaN,
 *       and step_size = the eps the step used.
 *   (3) adapt = 1: eps is read from the state record and follows Stan's dual averaging after every step, with
 *       gamma = 0.05, t0 = 10, kappa = 0.75:  m <- m + 1;  eta = 1 / (m + t0);
 *       sbar <- (1 - eta) sbar + eta (delta - alpha);  ell = mu - (sbar sqrt(m)) / gamma;  w = pow(m, -kappa);
 *       xbar <- (1 - w) xbar + w ell;  eps <- exp(ell).  adapt = 0: these words are neither read nor written and
 *       eps stays eps_chain[chain].
 * Arguments as st_lv_hmc_wave, except:
 *   state: DEVICE, st_lv_hmc_metric_workspace_bytes(chains) = 192 chains bytes: 24 words per chain, st_lv_mala_wave's
 *       16, then eps, m, sbar, xbar, mu (doubles; the caller sets them before an adapt = 1 launch: mu = log(10 eps),
 *       m = sbar = xbar = 0 starts an adaptation) and three spare.  A launch ends on a step boundary and leaves the
 *       whole state in the record, so results do not depend on how a run is split into launches;
 *   eps_chain: DEVICE (chains);  metric_chol: DEVICE (chains, 10), the row-major packed lower triangle of Lam
 *       (Lam_jk at j (j + 1) / 2 + k);  kick_clip: HOST (4);  adapt: 0 or 1;  delta: the target acceptance;
 *   accept_stat, step_size: DEVICE (chains, out_ld); the step that writes row r of samples writes their row r (the
 *       start row has none).
 * ST_ERR_INVALID (all checked before any HIP call): the conditions of st_lv_hmc_wave but those on step_eps; eps_chain,
 * metric_chol, accept_stat or step_size NULL or not 8-byte aligned; adapt not 0 or 1; delta not in (0, 1).
 * ---------------------------------------------------------------------------------------- */
int64_t st_lv_hmc_metric_workspace_bytes(int64_t chains);
int st_lv_hmc_metric_wave(double *state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                          int32_t init, const double *eps_chain, const double *metric_chol, const double *kick_clip,
                          int32_t n_leapfrog, int32_t adapt, double delta, int32_t noise_mode, uint64_t seed,
                          double *z, double *log_u, int64_t noise_ld, int64_t noise_row0, const double *t_eval,
                          int32_t t_n, const double *y_obs, const double *span_u0_tol, const double *whiten,
                          double c_log, double norm_logc, const double *cov_inv, int64_t max_steps, double *samples,
                          double *log_p, double *grad, double *accept_stat, double *step_size, int64_t out_ld,
                          int64_t out_row0, void *stream);

/* ------------------------------------------------------------------------------------------
 * No-U-turn sampler (NUTS) on st_lv_hmc_metric_wave's chain, one WAVE per chain (csrc/lv_mcmc.hip:
 * lv_nuts_wave_kernel; DESIGN.md section 22 is the contract).  The stage, eps_chain, metric_chol, the kick cap, the
 * 24-word state record and the dual averaging (adapt, delta) are st_lv_hmc_metric_wave's; the number of stages of a
 * step is chosen by the tree: doubling in a random direction (a stage in direction -1 is the stage with -eps), the
 * U-turn test on every aligned sub-tree from checkpoints, multinomial selection of the next row, and the divergence
 * rule (a leaf whose a = (lp(q) - lp(x)) + (K(z) - K(r)) is NaN or below -1000 ends the step).  The project's own
 * definition: Stan's bits and its further cross-sub-tree checks are not claimed.
 * Noise is the device's Philox only, key (seed, chain): step t takes its momentum from st_lv_hmc_wave's noise of
 * (seed, chain, t) -- the same z -- and stage l = 1, 2, ... of the step draws the block with counter (t, l, 0, 0), i.e.
 * np.random.Philox(key=[seed, chain], counter=[t - 1, l, 0, 0]).random_raw(4) = r0 .. r3: log u_l = log((r0 >> 11) 2^-53)
 * for the choice inside a sub-tree; at the first stage of a doubling the direction is +1 when r1 >> 63 is 0 and
 * log u_T = log((r2 >> 11) 2^-53) decides between the tree and the new sub-tree.
 * Arguments as st_lv_hmc_metric_wave, except:
 *   max_depth (in n_leapfrog's place): the largest number of doublings of a step, 1 .. 10 (a step is at most
 *       2^max_depth - 1 stages);
 *   noise_mode: 1 (Philox) or 2 (Philox, z written to the caller's array); log_u is checked as st_lv_hmc_metric_wave
 *       checks it and is neither read nor written;
 *   accept_stat: the mean over the step's stages of min(1, exp(a)) (0 for a NaN a);
 *   tree_depth, n_leapfrog, divergent: DEVICE (chains, out_ld) doubles after step_size: the doublings started, the
 *       stages done, and 0.0 or 1.0; the step that writes row r of samples writes their row r.
 * The state's accepted counts the steps whose row was replaced at least once, n_failed the divergent steps.
 * state: st_lv_nuts_workspace_bytes(chains) = 192 chains bytes.
 * ST_ERR_INVALID (all checked before any HIP call): the conditions of st_lv_hmc_metric_wave but that on n_leapfrog;
 * noise_mode 0; max_depth outside 1 .. 10; tree_depth, n_leapfrog or divergent NULL or not 8-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int64_t st_lv_nuts_workspace_bytes(int64_t chains);
int st_lv_nuts_wave(double *state, int64_t chains, int64_t first_chain, int64_t first_step, int64_t steps,
                    int32_t init, const double *eps_chain, const double *metric_chol, const double *kick_clip,
                    int32_t max_depth, int32_t adapt, double delta, int32_t noise_mode, uint64_t seed, double *z,
                    double *log_u, int64_t noise_ld, int64_t noise_row0, const double *t_eval, int32_t t_n,
                    const double *y_obs, const double *span_u0_tol, const double *whiten, double c_log,
                    double norm_logc, const double *cov_inv, int64_t max_steps, double *samples, double *log_p,
                    double *grad, double *accept_stat, double *step_size, double *tree_depth, double *n_leapfrog,
                    double *divergent, int64_t out_ld, int64_t out_row0, void *stream);

/* ------------------------------------------------------------------------------------------
 * Integrand protocol -- replaces integrand(ind1, ind2) of the closures returned by
 * stein_thinning.thinning._make_stein_integrand / _make_stein_gf_integrand and
 * stein_thinning.kernel.vfk0_imq (restated at JAX_Stein_Thinning.ipynb cell 27, json ~354-361;
 * Kernel_Stein_discrepancy.ipynb cell 7): out[p] = k(row i1[p], row i2[p]) (weights: w_i1 w_i2).
 * ---------------------------------------------------------------------------------------- */
int st_kernel_pairs(const double *x_soa, const double *g_soa, const double *weights, int64_t ld,
                    int32_t d, double linv_scale, double linv_trace, const int64_t *i1,
                    const int64_t *i2, int64_t n_pairs, double *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Kernel Stein discrepancy -- replaces stein_thinning.stein.ksd(integrand, n) (called at
 * code/src/utils/ksd.py:27 via calculate_ksd; Gaussian_mixture.ipynb cell 83) and
 * stein_thinning.stein.kmat(integrand, n) (code/tests/test_ksd.py:20; Gaussian_mixture.ipynb
 * cell 94).  Both take a COMPACT problem of m (k) rows (gather the selected rows first).
 * ks_out[i] = sqrt(sum_{a,b <= i} k(a,b)) / (i+1).  kmat_out is the full symmetric (k, k)
 * row-major matrix K[r][c] = k(min(r,c), max(r,c)).
 * ---------------------------------------------------------------------------------------- */
int64_t st_ksd_workspace_bytes(int64_t m, int64_t ld);   /* ld doubles: the column-sum vector */
int st_ksd_cumulative(const double *x_soa, const double *g_soa, const double *weights, int64_t m,
                      int64_t ld, int32_t d, double linv_scale, double linv_trace, double *ks_out,
                      void *workspace, int64_t workspace_bytes, void *stream);
/*
 * Full-sample KSD at scale, row-sharded across GPUs (the n-length column-sum all-reduce):
 *   st_ksd_colsum:  csum_out[i] = sum_{a in [row_begin, row_end), a < i} k(i, a)   (i < n)
 *                   -- the 2*np.sum(k0[:i]) / 2 term of the reference's ksd loop restricted to a
 *                   row range; ranks cover disjoint row ranges and all-reduce (sum) csum;
 *   st_ksd_finish:  ks_out[i] = sqrt(sum_{a <= i} (2 csum[a] + k(a, a))) / (i + 1).
 * st_ksd_cumulative == st_ksd_colsum over [0, m) followed by st_ksd_finish.
 * Summation order differs from the reference's NumPy pairwise sums (floating-point tolerance).
 */
int st_ksd_colsum(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                  int64_t ld, int32_t d, double linv_scale, double linv_trace, int64_t row_begin,
                  int64_t row_end, double *csum_out, void *stream);
int st_ksd_finish(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                  int64_t ld, int32_t d, double linv_scale, double linv_trace, const double *csum,
                  double *ks_out, void *stream);

int st_kmat(const double *x_soa, const double *g_soa, const double *weights, int64_t k,
            int64_t ld, int32_t d, double linv_scale, double linv_trace, double *kmat_out,
            void *stream);

/* ------------------------------------------------------------------------------------------
 * Set-batched KSD and distance sums -- ONE resident problem, n_sets arbitrary index sets over its
 * rows, one result per set: the reference's naive-thinning curves, whose index sets
 * np.linspace(0, n - 1, m).astype(int) are not nested (Gaussian_mixture.ipynb ksd_naive / naive_st,
 * m = 1..1000; lotka_volterra/Comparison.ipynb rw_ksd_naive / rw_energy_distance_naive over
 * thinned_sizes), evaluated there as one full KSD / energy distance per size.
 * rows (DEVICE, total_rows = set_offsets[n_sets] int64): the sets' row indices, each in [0, n),
 * concatenated in the caller's order (repeats allowed; the caller validates the range -- a row outside
 * it is never dereferenced and makes its set's results NaN).  set_offsets (HOST, n_sets + 1 int64):
 * set s is rows[set_offsets[s] .. set_offsets[s+1]); read only during the call.
 *   st_ksd_sets:       csum_out[j] = sum_{a < j, same set} k(r_j, r_a) ((k w_j) w_a with weights), in the
 *                      concatenated order -- for each set the bits of st_ksd_colsum on its compact
 *                      subset -- and ks_out[s] = sqrt(sum_j (2 csum[j] + k(r_j, r_j))) / m_s, i.e.
 *                      stein.ksd(reindex_integrand(integrand, set), m_s)[-1].  csum_out may be NULL.
 *   st_distance_sets:  self_out[s] = sum_{a < b} |p_a - p_b| over the set's points (K7's distance); with
 *                      row_values (device, n) and segsum_out both given, segsum_out[s] = sum over the
 *                      set's rows of row_values[row] (per-row cross sums computed once per unique row
 *                      with st_distance_colsum_ws); both NULL: skipped.
 * A fixed number of launches and ONE host-to-device copy (offsets + work-item table) whatever n_sets is.
 * Work items are (set, block of 256 columns) pairs, heaviest first (st_sets_work_items); per column a
 * sequential sum in increasing a; per set, thread t of one block adds columns t, t + 256, ... and a
 * fixed binary tree joins the 256 partials: the order depends on m_s only.  No atomics, the same
 * inputs give the same bits.  Nothing waits on the host except that the table is copied from ordinary
 * host memory, which the runtime has read when the call returns.  Allocates no device memory.
 * workspace: st_*_sets_workspace_bytes(total_rows, n_sets, d) bytes (host only; -1 for bad arguments).
 * ST_ERR_INVALID: NULL or misaligned pointers (device arrays 16, index / output arrays 8 bytes),
 * n_sets < 0, offsets not starting at 0 or decreasing, an empty set, a workspace that is too small.
 * ST_ERR_UNSUPPORTED: d > 128.  All checked before any HIP call.  n_sets == 0: ST_OK, nothing done.
 *   st_sets_work_items: host only -- the work-item table of these offsets: items_out[2 q] = set,
 *     items_out[2 q + 1] = column block of item q, non-increasing in the block's pair count.  Returns
 *     the item count (items_out NULL: count only), -1 for invalid offsets or capacity < count.
 * ---------------------------------------------------------------------------------------- */
int64_t st_sets_work_items(const int64_t *set_offsets, int64_t n_sets, int32_t *items_out, int64_t capacity);
int64_t st_ksd_sets_workspace_bytes(int64_t total_rows, int64_t n_sets, int32_t d);
int st_ksd_sets(const double *x_soa, const double *g_soa, const double *weights, int64_t n, int64_t ld,
                int32_t d, double linv_scale, double linv_trace,
                const int64_t *rows /* device, total_rows */,
                const int64_t *set_offsets /* HOST, n_sets + 1 */, int64_t n_sets,
                double *ks_out /* device, n_sets */, double *csum_out /* device, total_rows, or NULL */,
                void *workspace, int64_t workspace_bytes, void *stream);
int64_t st_distance_sets_workspace_bytes(int64_t total_rows, int64_t n_sets, int32_t d);
int st_distance_sets(const double *p_soa, int64_t ldp, int64_t n, int32_t d,
                     const int64_t *rows /* device, total_rows */,
                     const int64_t *set_offsets /* HOST, n_sets + 1 */, int64_t n_sets,
                     double *self_out /* device, n_sets */, const double *row_values /* device, n, or NULL */,
                     double *segsum_out /* device, n_sets, or NULL */,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dense preconditioners -- Gamma^-1 = L, any symmetric positive-definite (d, d) matrix, d <= 16 (the
 * reference's vfk0_imq takes any linv; upstream's preconditioner='smpcov' is the inverse sample
 * covariance).  Each function takes the arguments of its isotropic twin with linv_scale replaced by
 * `linv`: (d, d) row-major doubles on the device, 16-byte aligned; linv_trace = np.trace(L) from the host.
 * Validation before any HIP call: NULL or misaligned pointers ST_ERR_INVALID, d > 16 ST_ERR_UNSUPPORTED.
 *
 * Arithmetic -- one definition for every dense kernel, so a pair's bits do not depend on the entry
 * point (separately rounded operations except where fma is written).  With dx = x_i - x_j, ds = g_i - g_j:
 *   for r = 0 .. d-1:  y_r = L[r][0] dx_0, then y_r = fma(L[r][k], dx_k, y_r) for k = 1 .. d-1;
 *   qs  = y_0 dx_0, then fma(y_r, dx_r, qs);  t1s = y_0 y_0, then fma(y_r, y_r, t1s);
 *   t2s = y_0 ds_0, then fma(y_r, ds_r, t2s)                                          (r = 1 .. d-1);
 *   t3s = sum_k g_i,k g_j,k in NumPy's pairwise order, as the isotropic kernels compute it;
 *   qf = 1 + qs;  k = (-3 t1s / qf^2.5 + (linv_trace + t2s) / qf^1.5) + t3s / sqrt(qf), the powers
 *   correctly rounded.
 * This is the reference's formula with two changes that hold for symmetric L only: dx' L^2 dx is
 * evaluated as |L dx|^2 and (L ds) . dx as (L dx) . ds.  Swapping i and j negates dx, ds and y
 * exactly, so k(i, j) and k(j, i) are equal bit for bit; k(i, i) = linv_trace + t3s as in the isotropic
 * kernels.  d = 9 .. 16 run at a padded width of 16 (exact zeros added).  st_tune key 11 and the near-tie
 * guard do not apply: after st_greedy_dense, st_greedy_near_tie reports -2.
 *
 * st_greedy_dense always takes one launch per step (the step kernels' hand-off, no wait inside a
 * kernel); workspace as st_greedy (st_greedy_workspace_bytes).
 * st_ksd_cumulative_dense == st_ksd_colsum_dense over [0, m) followed by st_ksd_finish (k(a, a)
 * depends on linv_trace only).
 * ---------------------------------------------------------------------------------------- */
int st_greedy_dense(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                    int32_t d, int64_t ld, const double *linv, double linv_trace, int64_t n_points,
                    uint32_t *idx_out, double *a_work, void *workspace, int64_t workspace_bytes,
                    void *stream);
int st_kernel_pairs_dense(const double *x_soa, const double *g_soa, const double *weights, int64_t ld,
                          int32_t d, const double *linv, double linv_trace, const int64_t *i1,
                          const int64_t *i2, int64_t n_pairs, double *out, void *stream);
int st_kmat_dense(const double *x_soa, const double *g_soa, const double *weights, int64_t k,
                  int64_t ld, int32_t d, const double *linv, double linv_trace, double *kmat_out,
                  void *stream);
int st_ksd_colsum_dense(const double *x_soa, const double *g_soa, const double *weights, int64_t n,
                        int64_t ld, int32_t d, const double *linv, double linv_trace, int64_t row_begin,
                        int64_t row_end, double *csum_out, void *stream);
int st_ksd_cumulative_dense(const double *x_soa, const double *g_soa, const double *weights, int64_t m,
                            int64_t ld, int32_t d, const double *linv, double linv_trace, double *ks_out,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Energy distance -- replaces dcor.energy_distance(x, y) (V-statistic, exponent 1) as used by the
 * reference's fit_quality (code/notebooks/lotka_volterra/Comparison.ipynb cell 19,
 * Gradient_free_Student_t.ipynb; Gaussian_mixture.ipynb cells 63-71):
 *   out[i] = sum_{b in [b_begin, b_end), (!triangle or b < i)} ||A_i - B_b||_2,   i < na
 * A, B SoA (d, lda) / (d, ldb); triangle = 1 requires B == A (strict lower triangle: self sums).
 * ED(x, y) = 2 sum(out(x; y)) / (nx ny) - 2 sum(out(x; x, tri)) / nx^2 - 2 sum(out(y; y, tri)) / ny^2.
 * ---------------------------------------------------------------------------------------- */
int st_distance_colsum(const double *a_soa, int64_t lda, int64_t na, const double *b_soa,
                       int64_t ldb, int64_t nb, int32_t d, int64_t b_begin, int64_t b_end,
                       int32_t triangle, double *out, void *stream);
/* The same with the B range split over blockIdx.y chunks (~32768 blocks in all, st_tune key 14: a
 * short A -- e.g. the 1 000 selected points against a 2e5-point validation sample -- still fills
 * the chip, and a long triangle is dealt to the CUs in many small units): the chunk
 * partials go to `workspace` (st_distance_workspace_bytes(na, b_begin, b_end) bytes, 16-B aligned;
 * 0 means no split) and are summed per point in chunk order (deterministic). */
int64_t st_distance_workspace_bytes(int64_t na, int64_t b_begin, int64_t b_end);
int st_distance_colsum_ws(const double *a_soa, int64_t lda, int64_t na, const double *b_soa,
                          int64_t ldb, int64_t nb, int32_t d, int64_t b_begin, int64_t b_end,
                          int32_t triangle, double *out, void *workspace, int64_t workspace_bytes,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Host-side input preparation -- stein_thinning.thinning._validate_and_standardize (restated at
 * JAX_Stein_Thinning.ipynb cells 15-18): NaN / inf checks, then per-dimension
 * loc = mean(x, 0), scl = mean(|x - loc|, 0), x / scl, g * scl, bit-identical to the NumPy
 * expressions (their reduction orders reproduced).  Row-major (n, d) host arrays; outputs may
 * alias the inputs.  *status: 0 ok, 1 NaN, 2 inf, 3 a zero scale.  No HIP calls.
 * ---------------------------------------------------------------------------------------- */
int st_standardize_host(const double *sample, const double *gradient, int64_t n, int32_t d,
                        int32_t standardize, double *sample_out, double *gradient_out,
                        double *loc_out, double *scl_out, int32_t *status);

/* scipy.spatial.distance.pdist(rows) (euclidean) of row-major (k, d) device rows into out
 * (k (k - 1) / 2 doubles, scipy's condensed order), bit-identical to scipy 1.15: the 'med'
 * preconditioner's median heuristic (stein_thinning.kernel.make_precon, report.tex:432) sorts them on
 * the device.  2 <= k <= 65535. */
int st_pdist(const double *rows, int64_t k, int32_t d, double *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Repeated-row compaction (stein_thinning.device.DeviceProblem.dedup_view; no reference
 * counterpart -- an exact shortcut in front of st_greedy).  A row equal bit for bit (x, g, w) to the
 * row before it ties with its run's first row at every step of _greedy_search
 * (JAX_Stein_Thinning.ipynb:281-295) and loses the tie to the lower index, so st_greedy on the run
 * starts, mapped back through rows_out, returns the same indices.
 *   st_run_starts:  starts_out[i] = 1 iff row i starts a run (n bytes); the number of runs lands in
 *                   the first 8 bytes of `workspace` (int64; st_run_workspace_bytes(n), 16-B aligned);
 *   st_run_compact: after the caller read that count: the run starts into (d, ld_out) SoA arrays
 *                   x_out / g_out (and w_out when weights is non-NULL) in row order, rows_out[k] = the
 *                   source row of compact row k (int32), rows [count, ld_out) zeroed.
 * n < 2^31.  Same stream for both calls.
 * ---------------------------------------------------------------------------------------- */
int64_t st_run_workspace_bytes(int64_t n);
int st_run_starts(const double *x_soa, const double *g_soa, const double *weights, int64_t n, int32_t d,
                  int64_t ld, uint8_t *starts_out, void *workspace, int64_t workspace_bytes, void *stream);
int st_run_compact(const double *x_soa, const double *g_soa, const double *weights, int64_t n, int32_t d,
                   int64_t ld, const uint8_t *starts, const void *workspace, int64_t count, int64_t ld_out,
                   double *x_out, double *g_out, double *w_out, int32_t *rows_out, void *stream);

/* The same with the upload underneath: thread 0 computes loc / scl (st_standardize_host's column
 * passes, bit-identical) while the other threads copy the RAW arrays into the page-locked staging
 * buffers stage_x / stage_g (16-B aligned, n d doubles; g's NaN / inf scan fused in) and queue each
 * copied chunk's host-to-device copy into dev_x / dev_g (row-major) on `stream`.  The caller scales
 * on the device (st_layout_soa_scaled with loc_out / scl_out).  d = 2 .. 8 and n >= 65536 only
 * (ST_ERR_UNSUPPORTED otherwise: use st_standardize_host); *status as st_standardize_host's (on a
 * nonzero status the queued copies have finished when it returns). */
int st_standardize_upload(const double *sample, const double *gradient, int64_t n, int32_t d,
                          double *stage_x, double *stage_g, double *dev_x, double *dev_g,
                          double *loc_out, double *scl_out, int32_t *status, void *stream);

/* The device-resident counterpart (the drop-in thin called with ROCm tensors; replaces the reference's
 * np.asarray of the inputs + _validate_and_standardize's statistics): x (row-major (n, d) on the device)
 * comes back into the page-locked stage_x in 64 K-row chunks on `stream`, each chunk's column sums taken
 * as it lands (NumPy's sequential axis-0 order, bit-identical); loc_out / scl_out as st_standardize_host's.
 * g stays on the device (its NaN / inf check is the caller's).  *status: 0 ok, 1 NaN in x, 2 inf in x, 3 a
 * zero scale.  Any n >= 1, d >= 1 (outside d = 2 .. 8, n >= 65536: one copy, then st_standardize_host's
 * column passes; d = 1 assumes NumPy's default bufsize).  Returns when x is on the host and the
 * statistics are done. */
int st_standardize_download(const double *dev_x, int64_t n, int32_t d, double *stage_x, double *loc_out,
                            double *scl_out, int32_t *status, void *stream);

/* row-major (n, d) -> SoA (d, ld) layout helper (device to device) */
int st_layout_soa(const double *rowmajor, int64_t n, int32_t d, int64_t ld, double *soa,
                  void *stream);
/* the same with x / scale[k] (divide = 1) or x * scale[k] (divide = 0) per element: the scaling of
 * _validate_and_standardize on the device (scale: d doubles in device memory) */
int st_layout_soa_scaled(const double *rowmajor, int64_t n, int32_t d, int64_t ld, const double *scale,
                         int32_t divide, double *soa, void *stream);

/* ------------------------------------------------------------------------------------------
 * Many short chains in one launch -- stein_thinning.thinning.thin_many / thin_gf_many: the loop
 * [thin(s, g, m) for s, g in chains] (the reference's per-chain loop, Stein_thinning.ipynb cells
 * 12-14; the randomised-starts experiment of report.tex:791) for `chains` chains of the same length,
 * row-major (chains, n, d) RAW device arrays, one workgroup per chain and no traffic between the
 * blocks.  These entry points read row-major arrays (not the SoA layout above); double arrays are
 * 8-byte aligned, int32 / uint32 arrays 4-byte aligned.  ST_ERR_INVALID: a NULL or misaligned
 * pointer, chains < 1, n < 1, d < 1, n_points < 1; ST_ERR_UNSUPPORTED: a d or n outside the stated
 * range; either way nothing is enqueued.
 * ---------------------------------------------------------------------------------------- */

/* _validate_and_standardize's statistics per chain, bit-identical to NumPy: loc = np.mean(x_c, 0)
 * (the sum over rows in row order, divided once by n), scl = np.mean(np.abs(x_c - loc), 0) (the same
 * order, no fma), written to loc_out / scl_out (chains, d); status_out (chains) int32 with
 * st_standardize_host's meaning and precedence: 0 ok, 1 a NaN in x or g, 2 an inf, 3 a zero scale.
 * standardize = 0: scl = 1, loc = 0, finiteness only.  d = 2 .. 8 (d = 1: NumPy's pairwise sum of a
 * contiguous column is st_standardize_host's). */
int st_chain_stats(const double *x, const double *g, int64_t chains, int64_t n, int32_t d,
                   int32_t standardize, double *loc_out, double *scl_out, int32_t *status_out,
                   void *stream);

/* st_pdist per chain on standardised rows: for chain c the condensed scipy pdist of the k rows
 * x[c, sub_rows[0..k)] / scl[c] (sub_rows: k int32 row indices on the device, shared by all chains,
 * entries outside [0, n) are clamped; NULL: all rows, k == n) into out + c k (k - 1) / 2.  Every
 * value has the bits of st_pdist on x / scl (the 'med' / 'sclmed' median heuristic,
 * kernel.make_precon).  2 <= k <= min(n, 65535), d <= 128, chains (k - 1) < 2^31. */
int st_pdist_many(const double *x, const double *scl, const int32_t *sub_rows, int64_t chains,
                  int64_t n, int32_t d, int64_t k, double *out, void *stream);

/* The thin: for every chain the n_points indices _greedy_search selects on (x_c / scl_c,
 * g_c * scl_c) -- the scaling applied on load with NumPy's bits -- with Gamma^-1 = linv_scale[c] I,
 * linv_trace[c] = np.trace of it (device arrays of `chains` doubles), weights (chains, n) or NULL.
 * One workgroup per chain: rows and running sums stay in registers for all steps; every pair in
 * the EXACT arithmetic (NumPy's evaluation order, st_tune key 11 does not apply; no near-tie guard,
 * no dedup).  idx_out (chains, n_points) uint32; a_out (chains, n) receives the final running sums,
 * or NULL.  Bit model: oracle/stein_ref.c sr_greedy(arith = exact) per chain, idx and a_out.
 * d in {2, 4} and n <= st_greedy_many_max_n(d, has_weights) (>= 4096), else ST_ERR_UNSUPPORTED;
 * n_points > n and repeated selections are allowed. */
int st_greedy_many(const double *x, const double *g, const double *scl, const double *weights,
                   const double *linv_scale, const double *linv_trace, int64_t chains, int64_t n,
                   int32_t d, int64_t n_points, uint32_t *idx_out, double *a_out, void *stream);
/* host only: the largest n st_greedy_many takes at this d (0: d unsupported) */
int64_t st_greedy_many_max_n(int32_t d, int32_t has_weights);
/* host only: threads per block and rows per thread st_greedy_many uses at this n (tests place their
 * shapes on both sides of every change) */
int st_greedy_many_plan(int64_t n, int32_t d, int32_t has_weights, int32_t *threads_out,
                        int32_t *rows_out);

/* ----------------------------------------------------------------------------------------------
 * Convergence diagnostics (csrc/convergence.hip; stein_thinning.convergence)
 *
 * st_rank_normalize: sorted (vars, count) holds every variable's values in ascending order (NaN last)
 * and perm (vars, count) the original position of each, as a stable sort returns them.  For every value
 * the kernel finds its tie run, the run's average 1-based rank r, p = (r - 0.375) / (count + 0.25) (one
 * exact subtraction, one IEEE division) and z = the inverse normal cdf of p (AS241 PPND16), and writes z
 * (and p, when p_out is given) at the value's original position of a (vars, count) array.  A NaN value
 * gives NaN.  A perm entry outside [0, count) writes nothing.
 * ST_ERR_INVALID: NULL or not 8-byte aligned pointers, vars < 1, count < 1.
 *
 * st_autocov: series (groups, S, h) contiguous.  For every series s of group g, with mu its mean,
 *     acov[g, s, t] = (1 / h) sum_{i < h - t} (a[i] - mu) (a[i + t] - mu),   lag0 <= t < lag1;
 * acov_mean[g, t - lag0] = the mean over the group's series (slabs of 256 series, each in series order,
 * the slabs in order), series_mean[g, s] = mu, series_var0[g, s] = acov[g, s, 0] (its own sum, whatever
 * lag0 is), acov_series (groups, S, lag1 - lag0) the per-series values when given (NULL: not written).
 * plan 0 chooses by shape, 1 is the long plan (blocks tile i chunks x lag tiles, any h), 2 the short
 * plan (a wave per series, the series in LDS, h <= 2048); st_autocov_plan returns the plan a call
 * would take.  No atomics: the same arguments give the same bits on every call and every device.
 * workspace: st_autocov_workspace_bytes(...) bytes (host only; -1 for arguments st_autocov rejects).
 * ST_ERR_INVALID: NULL or not 8-byte aligned pointers, groups < 1, S < 1, h < 4, lag0 < 0,
 * lag0 >= lag1, lag1 > h, plan outside 0..2, a workspace that is too small.  ST_ERR_UNSUPPORTED: the
 * short plan with h > 2048, more series or lags than one launch holds.  All checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
int st_rank_normalize(const double *sorted, const int64_t *perm, int64_t vars, int64_t count,
                      double *p_out /* or NULL */, double *z_out, void *stream);
int64_t st_autocov_workspace_bytes(int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1,
                                   int32_t plan);
int st_autocov_plan(int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int32_t plan);
int st_autocov(const double *series, int64_t groups, int64_t S, int64_t h, int64_t lag0, int64_t lag1,
               int32_t plan, double *acov_mean, double *series_mean, double *series_var0,
               double *acov_series /* or NULL */, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* STEIN_THINNING_HIP_H */
