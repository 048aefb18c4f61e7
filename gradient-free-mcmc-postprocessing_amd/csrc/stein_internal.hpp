// Internal (non-ABI) declarations shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace st {

constexpr int kMaxDim = 128;     // NumPy pairwise_sum modelled without recursion up to 128 lanes
constexpr int kMaxCtDim = 8;     // compile-time-d kernels for d <= 8
constexpr int kMaxDenseDim = 16; // dense preconditioners: d <= 16 (a 32-wide pair needs 256 VGPRs: one wave per SIMD)
constexpr int kMaxBlocks = 1024; // greedy step grid cap (4 x 256-thread blocks per CU)
constexpr int kCandHeader = 2;   // candidate record: {val, gidx(bits)} then x[d], g[d], w
constexpr int64_t kWsControlBytes = 8 * 128 + 128;   // persistent kernel: arrival counters + status
// control block words (byte offsets into the greedy workspace):
constexpr int64_t kWsStatusOff = 8 * 128;   // u32 status: [0] persistent kernel, [1] the general kernel behind
                                            // a compact-only run
constexpr int64_t kWsTieOff = kWsStatusOff + 32;     // u32 near-tie words (first flagged step + 1, 0 = none):
                                                     // [0] persistent kernel, [1] gated general kernel, [2] step
                                                     // kernels; [3] = 1: the run is guarded (bounds computed)
constexpr int64_t kWsBoundsOff = kWsStatusOff + 64;  // near-tie bounds: max_i |g_i|^2, max_i w_i^2 (f64 bits),
                                                     // then the persistent run's final Q, E, thr (tests)
static_assert(kWsBoundsOff + 40 <= kWsControlBytes, "control block layout");
// peer mailbox (u64 words), one per rank, uncached device memory:
//   [0, 32)        persistent kernel: 2 banks x kMailboxRanks slots x 2 tagged granules
//   [32, 40)       handshake words (one per rank)
//   [40]           exchange counter of the step-kernel path (written by this rank only)
//   [64, ...)      step-kernel path: 2 banks x kMailboxRanks record slots, each a flag word then
//                  the candidate record (cand_stride(d) doubles) at word 8
constexpr int kMailboxRanks = 8;
constexpr int kMailboxHandshake = 2 * kMailboxRanks * 2;
constexpr int kMailboxXchgCount = kMailboxHandshake + kMailboxRanks;
constexpr int kMailboxRecBase = 64;
constexpr int kMailboxRecSlotWords = 272;   // 8 header words + cand_stride(kMaxDim) = 260, 64-B multiple
constexpr int64_t kMailboxBytes = (int64_t)(kMailboxRecBase + 2 * kMailboxRanks * kMailboxRecSlotWords) * 8;
static_assert(kMailboxXchgCount < kMailboxRecBase, "mailbox layout");

struct MailboxPeers {
    uint64_t* p[kMailboxRanks];
};

// row block and peers of one rank of a multi-GPU persistent run (nranks == 1: one device)
struct RankSpec {
    int64_t row_begin, row_end;
    int rank, nranks;
    uint64_t seq_base;
    uint64_t* inbox;
    uint64_t* peer[kMailboxRanks];
};

inline int64_t cand_stride(int d) { return ((kCandHeader + 2 * d + 1) + 1) & ~int64_t(1); }
static_assert(8 + ((kCandHeader + 2 * kMaxDim + 1) + 1) / 2 * 2 <= kMailboxRecSlotWords, "record slot");

struct GreedyArgs {
    const double* x;      // SoA (d, ld) standardised sample shard
    const double* g;      // SoA (d, ld) standardised gradient (or gradient_q) shard
    const double* w;      // (ld) gradient-free weights, or nullptr for the Langevin kernel
    double* A;            // (ld) running sums, in place
    int64_t n;            // rows in this shard
    int64_t ld;           // leading dimension (multiple of 8, >= n)
    int d;
    double l;             // isotropic preconditioner Gamma^-1 = l * I
    double tr;            // np.trace(Gamma^-1), computed on the host exactly as the reference
    int64_t row_offset;   // global index of shard row 0
    const double* recs_in;  // K candidate records of the previous step (unused for the diagonal)
    int nrecs_in;
    int64_t rec_stride;   // doubles per record
    double* recs_out;     // one record per block of this launch
    uint32_t* idx_out;    // device index array; launch t writes idx[t-1]
    int64_t t;            // step being computed (0 = diagonal)
    int compact;          // 1: the compact arithmetic for pairs in range (d <= 8; stein_math.hpp)
    const double* linv;   // dense Gamma^-1: (d, d) row-major device array (stein_dense.hpp); nullptr: l * I
};

int greedy_blocks(int64_t n, int d);
// near-tie guard of the compact arithmetic (st_tune key 20: 1 = on, the default; 0 = off)
int tie_guard();
// st_tune key 11: arithmetic of the d <= 8 greedy kernels (1 = compact, the default; 0 = exact)
int arith_compact();
int tune(int key, int value);
int persistent_tune(int key, int value);
int persistent_tune_get(int key);
int tune_get(int key);
int64_t persistent_ws_bytes(int d, int G, int rec_stride, int nrep);
int64_t persistent_ws_max_bytes();
hipError_t launch_greedy_persistent(const double* x, const double* g, const double* w, double* A,
                                    int64_t n, int d, int64_t ld, double l, double tr, int64_t m,
                                    uint32_t* idx_out, void* ws, int64_t ws_bytes, hipStream_t s,
                                    int* used, const RankSpec* ranks = nullptr, bool plan_only = false);
// one thin of a batch launch (st_greedy_batch): the st_greedy arguments of one problem
struct BatchProblem {
    const double* x;
    const double* g;
    const double* w;
    double* A;
    int64_t n, ld;
    double l, tr;
    uint32_t* idx_out;
    void* ws;
    int64_t ws_bytes;
};
constexpr int kMaxBatchProblems = 8;
hipError_t launch_greedy_persistent_batch(int count, const BatchProblem* problems, int d, int64_t m,
                                          hipStream_t s, int* used);
hipError_t launch_mailbox_handshake(const MailboxPeers& peers, uint64_t* inbox, int rank,
                                    int nranks, uint64_t token, int* ok, hipStream_t s);
hipError_t launch_greedy_step(const GreedyArgs& a, bool diag, int blocks, hipStream_t s);
// dense preconditioner (a.linv set, d <= kMaxDenseDim): grid of a run, and one step t >= 1 (step 0 is
// launch_greedy_step's diagonal with the same grid)
int greedy_dense_blocks(int64_t n, int d);
hipError_t launch_greedy_step_dense(const GreedyArgs& a, int blocks, hipStream_t s);
hipError_t launch_greedy_publish(const double* recs, int K, int64_t stride, int d, double* out,
                                 hipStream_t s);
hipError_t launch_greedy_finalize(const double* recs, int K, int64_t stride, uint32_t* idx_out,
                                  int64_t t, hipStream_t s);
struct ProxyArgs {
    const double* x;     // row-major (n, d) raw sample
    const double* loc;   // (d)
    const double* U;     // (d, d) row-major, scipy _PSD factor: maha = |(x - loc) @ U|^2
    const double* P;     // (d, d) row-major, np.linalg.inv(cov / shape)
    int64_t n;
    int d;
    double df;           // 0: Gaussian; > 0: Student-t degrees of freedom
    double c_log;        // Gaussian: rank*log(2 pi) + log_pdet; t: A - B - C - D
    double* log_q;       // (n)
    double* grad;        // row-major (n, d)
};
int64_t proxy_lds_bytes(int d);
int64_t kde_workspace_bytes(int64_t m, int d);
hipError_t launch_kde(const double* p, int64_t ldp, int64_t n, const double* logw, double logw0,
                      const double* q, int64_t ldq, int64_t m, int d, double log_norm, const double* L,
                      double* log_q, double* grad, double* ws, hipStream_t s);
// Student-t kernel density (same workspace as launch_kde); log_norm = log_norm_t of the header
hipError_t launch_kde_t(const double* p, int64_t ldp, int64_t n, const double* logw, double logw0,
                        const double* q, int64_t ldq, int64_t m, int d, double df, double log_norm,
                        const double* L, double* log_q, double* grad, double* ws, hipStream_t s);
int kde_t_tune(int value);   // st_tune key 24 (power path of the Student-t KDE)
hipError_t launch_proxy(const ProxyArgs& a, hipStream_t s);
int proxy_tune(int value);   // st_tune key 7
constexpr int kMixtureMaxDim = 64;     // the matrix-core kernel's widest instantiation
constexpr int kMixtureMaxComponents = 1024;
struct MixtureArgs {
    const double* x;         // row-major (n, d) raw sample
    const double* log_coef;  // (k) a_c = log w_c - (d log 2 pi + log det Sigma_c) / 2; -inf: skipped
    const double* means;     // (k, d) row-major
    const double* P;         // (k, d, d) row-major, np.linalg.inv(Sigma_c)
    int64_t n;
    int d;
    int k;
    double* log_p;           // (n)
    double* score;           // row-major (n, d)
};
hipError_t launch_mixture(const MixtureArgs& a, hipStream_t s);   // csrc/mixture.hpp (in proxy.hip)
constexpr int kMvtMaxDim = 16;         // the moment kernels' widest instantiation
struct MvtMomentsArgs {
    const double* x;     // row-major (n, d) raw sample
    const double* loc;   // (d)
    const double* U;     // (d, d) row-major whitening: z = (x - loc) @ U
    int64_t n;
    int d;
    double df;           // > 0
    int want_grad;       // 0: S0 only
    double* out;         // S0, S1, Sz[d], Szz upper triangle row-major (want_grad = 0: out[0] only)
    double* ws;          // mvt_moments_ws_bytes(n, d) bytes: one record per block
};
int64_t mvt_moments_ws_bytes(int64_t n, int d);                            // host only
hipError_t launch_mvt_moments(const MvtMomentsArgs& a, hipStream_t s);     // csrc/mvt_moments.hpp (in proxy.hip)
constexpr int kMixtureEmMaxDim = 16;          // the EM-pass kernel's widest instantiation
constexpr int kMixtureEmMaxComponents = 32;
struct MixtureEmArgs {
    const double* x;         // row-major (n, d) raw sample
    const double* log_coef;  // (k), means (k, d), P (k, d, d): as MixtureArgs
    const double* means;
    const double* P;
    const double* w;         // (n) row weights >= 0, or NULL: 1
    int64_t n;
    int d;
    int k;
    double* out;             // LL, then per component N_c, S_c[d], Q_c upper triangle row-major
    double* log_p;           // (n), or NULL: not written
    double* ws;              // mixture_em_ws_bytes(n, d, k) bytes: one record per block of grid.x
};
int64_t mixture_em_ws_bytes(int64_t n, int d, int k);                      // host only
hipError_t launch_mixture_em(const MixtureEmArgs& a, hipStream_t s);       // csrc/mixture_fit.hpp (in proxy.hip)
int dist_tune(int value);    // st_tune key 13 (energy kernel variant)

// the Lotka-Volterra posterior and its RK45 settings, as every LV kernel reads them (csrc/lv_rk45.hpp)
struct LvProblem {
    const double* t_eval;     // (t_n) ascending observation times
    int t_n;
    const double* y_obs;      // (t_n, 2) row-major observations
    double t0, t1;            // integration span
    double u0[2];             // initial state
    double rtol, atol;
    double U[4];              // scipy _PSD(C).U row-major (log density)
    double c_log;             // rank * log(2 pi) + log_pdet of C
    double norm_logc;         // scipy.stats.norm's log(sqrt(2 pi))
    int64_t max_steps;
};

struct LvArgs {
    const double* theta;      // (n, 4) row-major ODE parameters
    const double* log_theta;  // (n, 4) row-major, log density only
    int64_t n;
    LvProblem p;
    double cinv[4];           // inv(C) row-major (gradient)
    double* out;              // gradient: (n, 4); log density: (n)
    double* work;             // log density: (t_n, n) per-time terms
    int32_t* status;          // (n): 0 ok, 1 step size too small, 2 step limit reached
    double* steps;            // gradient, two-phase: (n, step_cap, 56) step table, or nullptr
    int32_t* nsteps;          // (n) recorded steps per point
    int step_cap;
};
hipError_t launch_lv(const LvArgs& a, bool gradient, hipStream_t s);
int64_t lv_grad_workspace_bytes(int64_t n, int step_cap);

// random-walk Metropolis over the LV log posterior, one chain per thread (csrc/lv_mcmc.hip)
struct LvMcmcArgs {
    double* state;            // (chains, 8) words: x[4], lp, accepted (int64), n_failed (int64), unused
    int64_t chains;
    int64_t first_chain;      // chain id of local chain 0 (Philox key word 1)
    int64_t first_step;       // global step t of this launch's first step (>= 1)
    int64_t steps;            // Metropolis steps in this launch
    int init;                 // 1: evaluate the start row first, write it as row out_row0 - 1
    double step[4];           // proposal step sizes
    int noise_mode;           // 0 supplied, 1 device (Philox), 2 device + record into z / log_u
    uint64_t seed;            // Philox key word 0
    double* z;                // (chains, noise_ld, 4): read (mode 0) or written (mode 2)
    double* log_u;            // (chains, noise_ld)
    int64_t noise_ld, noise_row0;   // this launch's first step uses noise row noise_row0
    LvProblem p;
    double* samples;          // (chains, out_ld, 4)
    double* log_p;            // (chains, out_ld)
    int64_t out_ld, out_row0; // this launch's first step writes row out_row0
};
hipError_t launch_lv_rwmh(const LvMcmcArgs& a, hipStream_t s);
// the same sampler with one wave per chain: the observation points of a step split over the 64 lanes
hipError_t launch_lv_rwmh_wave(const LvMcmcArgs& a, hipStream_t s);

// Metropolis-adjusted Langevin sampler over the LV log posterior in x = log theta, one wave per chain
// (csrc/lv_mcmc.hip: lv_mala_wave_kernel); the fields it shares with LvMcmcArgs mean the same
struct LvMalaArgs {
    double* state;            // (chains, 16) words: x[4], lp, accepted (int64), n_failed (int64), spare, g[4], 4 spare
    int64_t chains;
    int64_t first_chain;
    int64_t first_step;
    int64_t steps;
    int init;
    double eps[4];            // step size epsilon
    double h[4];              // 0.5 eps^2, computed by the host
    double w[4];              // 0.5 / eps^2, computed by the host
    double clip[4];           // drift cap c = drift_cap * eps (> 0, may be +inf)
    int noise_mode;
    uint64_t seed;
    double* z;
    double* log_u;
    int64_t noise_ld, noise_row0;
    LvProblem p;
    double cinv[4];           // inv(C) row-major
    double* samples;          // (chains, out_ld, 4)
    double* log_p;            // (chains, out_ld)
    double* grad;             // (chains, out_ld, 4): the gradient of log p with respect to log theta
    int64_t out_ld, out_row0;
};
hipError_t launch_lv_mala_wave(const LvMalaArgs& a, hipStream_t s);

// Hamiltonian Monte Carlo sampler over the LV log posterior in x = log theta, one wave per chain
// (csrc/lv_mcmc.hip: lv_hmc_wave_kernel); the fields it shares with LvMalaArgs mean the same
struct LvHmcArgs {
    double* state;            // (chains, 16) words, LvMalaArgs' record
    int64_t chains;
    int64_t first_chain;
    int64_t first_step;
    int64_t steps;            // Metropolis steps (trajectories) in this launch
    int init;
    double eps[4];            // leapfrog step size epsilon
    double clip[4];           // kick cap c (> 0, may be +inf): bounds every component of eps * g
    int n_leapfrog;           // leapfrog stages per trajectory, L >= 1
    int noise_mode;
    uint64_t seed;
    double* z;
    double* log_u;
    int64_t noise_ld, noise_row0;
    LvProblem p;
    double cinv[4];           // inv(C) row-major
    double* samples;          // (chains, out_ld, 4)
    double* log_p;            // (chains, out_ld)
    double* grad;             // (chains, out_ld, 4)
    int64_t out_ld, out_row0;
};
hipError_t launch_lv_hmc_wave(const LvHmcArgs& a, hipStream_t s);

// HMC with a per-chain step size, a per-chain dense metric and step-size adaptation, one wave per chain
// (csrc/lv_mcmc.hip: lv_hmc_metric_wave_kernel); the fields it shares with LvHmcArgs mean the same
struct LvHmcMetricArgs {
    double* state;            // (chains, 24) words: LvMalaArgs' 16, then eps, m, sbar, xbar, mu, 3 spare
    int64_t chains;
    int64_t first_chain;
    int64_t first_step;
    int64_t steps;
    int init;
    const double* eps_chain;  // (chains): the step size of every chain (adapt = 0)
    const double* metric_chol;    // (chains, 10): packed row-major lower triangle of Lam, M^-1 = Lam Lam^T
    double clip[4];
    int n_leapfrog;
    int adapt;                // 1: eps from the state record, dual averaging after every step
    double delta;             // dual averaging's target acceptance, in (0, 1)
    int noise_mode;
    uint64_t seed;
    double* z;
    double* log_u;
    int64_t noise_ld, noise_row0;
    LvProblem p;
    double cinv[4];
    double* samples;          // (chains, out_ld, 4)
    double* log_p;            // (chains, out_ld)
    double* grad;             // (chains, out_ld, 4)
    double* accept_stat;      // (chains, out_ld): min(1, exp(a)) of the step that wrote the row
    double* step_size;        // (chains, out_ld): the eps that step used
    int64_t out_ld, out_row0;
};
hipError_t launch_lv_hmc_metric_wave(const LvHmcMetricArgs& a, hipStream_t s);

// No-U-turn sampler on lv_hmc_metric_wave_kernel's chain, one wave per chain (csrc/lv_mcmc.hip: lv_nuts_wave_kernel);
// the fields it shares with LvHmcMetricArgs mean the same.  noise_mode is 1 or 2: there is no supplied-noise form
struct LvNutsArgs {
    double* state;            // (chains, 24) words, LvHmcMetricArgs' record
    int64_t chains;
    int64_t first_chain;
    int64_t first_step;
    int64_t steps;
    int init;
    const double* eps_chain;
    const double* metric_chol;
    double clip[4];
    int max_depth;            // doublings per step at most, 1 .. 10
    int adapt;
    double delta;
    int noise_mode;
    uint64_t seed;
    double* z;                // (chains, noise_ld, 4): the momenta drawn (noise_mode 2)
    double* log_u;            // neither read nor written
    int64_t noise_ld, noise_row0;
    LvProblem p;
    double cinv[4];
    double* samples;          // (chains, out_ld, 4)
    double* log_p;            // (chains, out_ld)
    double* grad;             // (chains, out_ld, 4)
    double* accept_stat;      // (chains, out_ld): the mean of min(1, exp(a)) over the step's stages
    double* step_size;        // (chains, out_ld): the eps that step used
    double* tree_depth;       // (chains, out_ld): doublings started, as a double
    double* n_leapfrog;       // (chains, out_ld): stages done, as a double
    double* divergent;        // (chains, out_ld): 0.0 or 1.0
    int64_t out_ld, out_row0;
};
hipError_t launch_lv_nuts_wave(const LvNutsArgs& a, hipStream_t s);

hipError_t launch_greedy_rank_exchange(const double* recs, int K, int64_t stride, int d,
                                       const MailboxPeers& peers, int rank, int nranks, int64_t t,
                                       double* recv, unsigned* status, hipStream_t s);

struct PairArgs {
    const double* x;
    const double* g;
    const double* w;
    int64_t ld;
    int d;
    double l;
    double tr;
    const double* linv;   // dense Gamma^-1 (d, d) row-major, d <= kMaxDenseDim; nullptr: l * I
};

hipError_t launch_pairs(const PairArgs& p, const int64_t* i1, const int64_t* i2, int64_t L,
                        double* out, hipStream_t s);
hipError_t launch_kmat(const PairArgs& p, const int64_t* idx, int64_t k, double* out,
                       hipStream_t s);
hipError_t launch_ksd_colsum(const PairArgs& p, int64_t n, int64_t a0, int64_t a1, double* csum,
                             hipStream_t s);
hipError_t launch_ksd_finish(const PairArgs& p, int64_t n, const double* csum, double* ks,
                             hipStream_t s);
// set-batched forms (csrc/sets.hpp, in pairwise.hip): one resident problem, many index sets
int sets_check_offsets(const int64_t* off, int64_t n_sets);     // host; 0 ok, 1 off[0] != 0, 2 decreasing, 3 empty set
int64_t sets_item_count(const int64_t* off, int64_t n_sets);    // host: (set, column block) work items
void sets_build_items(const int64_t* off, int64_t n_sets, int32_t* items);   // host: {set, block}, heaviest first
int64_t sets_ws_bytes(int64_t total, int64_t n_sets, int nvec); // host: nvec SoA vectors per gathered row
hipError_t launch_ksd_sets(const PairArgs& p, int64_t n, const int64_t* rows, const int64_t* set_offsets,
                           int64_t n_sets, double* ks_out, double* csum_out, void* ws, hipStream_t s);
hipError_t launch_distance_sets(const double* pts, int64_t ldp, int64_t n, int d, const int64_t* rows,
                                const int64_t* set_offsets, int64_t n_sets, double* self_out,
                                const double* row_values, double* segsum_out, void* ws, hipStream_t s);
int64_t distance_chunks(int64_t na, int64_t b_begin, int64_t b_end);
int dist_units_tune(int value);   // st_tune key 14
int lv_tune(int value);           // st_tune key 17
int lv_pieces_tune(int value);    // st_tune key 18
hipError_t launch_distance_colsum(const double* a, int64_t lda, int64_t na, const double* b,
                                  int64_t ldb, int64_t b0, int64_t b1, int d, int tri,
                                  double* out, double* ws, int64_t ws_doubles, hipStream_t s);
hipError_t launch_layout_soa(const double* rowmajor, int64_t n, int d, int64_t ld, double* soa,
                             hipStream_t s);
hipError_t launch_layout_soa_scaled(const double* rowmajor, int64_t n, int d, int64_t ld, const double* scale,
                                    int divide, double* soa, hipStream_t s);
// 'med' preconditioner distances (precon.hip)
hipError_t launch_pdist(const double* rows, int64_t k, int d, double* out, hipStream_t s);
// repeated-row compaction (dedup.hip)
int64_t run_tiles(int64_t n);
hipError_t launch_run_starts(const double* x, const double* g, const double* w, int64_t n, int d, int64_t ld,
                             uint8_t* starts, int32_t* tile_count, int32_t* tile_off, int64_t* count,
                             hipStream_t s);
hipError_t launch_run_compact(const double* x, const double* g, const double* w, int64_t n, int d, int64_t ld,
                              const uint8_t* starts, const int32_t* tile_off, int64_t count, int64_t ld_out,
                              double* xo, double* go, double* wo, int32_t* rows_out, hipStream_t s);

// convergence diagnostics (convergence.hip)
struct RankArgs {
    const double* sorted;   // (vars, N) each row ascending (NaN last)
    const int64_t* perm;    // (vars, N) original position of every sorted value
    int64_t vars, N;
    double* p_out;          // (vars, N) at the original positions, or nullptr
    double* z_out;          // (vars, N) at the original positions
};
hipError_t launch_rank_normalize(const RankArgs& a, hipStream_t s);
struct AutocovArgs {
    const double* series;   // (G, S, h) contiguous
    int64_t G, S, h, lag0, lag1;
    int plan;               // 0: by shape, 1: long, 2: short
    double* acov_mean;      // (G, lag1 - lag0)
    double* series_mean;    // (G, S)
    double* series_var0;    // (G, S)
    double* acov_series;    // (G, S, lag1 - lag0) or nullptr
    double* ws;
};
int autocov_plan(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want);   // 1 long, 2 short
bool autocov_short_ok(int64_t h);
bool autocov_grid_ok(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want);
int64_t autocov_ws_bytes(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want);
hipError_t launch_autocov(const AutocovArgs& a, hipStream_t s);

}  // namespace st
