// Random-walk Metropolis sampler for the Lotka-Volterra log posterior, batched over chains: one
// thread owns one chain and runs the Metropolis loop inside the kernel.  A second
// layout, lv_rwmh_wave_kernel below, gives a chain a whole wave: for a few long chains (the reference's five)
// it is ~10 times faster per chain; what follows holds for both, the wave layout's summation order is
// stated at its kernel.
//
// Reference (Sampling.ipynb: a hand-written random-walk Metropolis-Hastings loop over
// lotka_volterra.log_target_density, 5 chains of 500 000 rows, proposal step 0.0025; its sampler
// package is not part of the reference tree, so the proposal x + step * N(0, I) is this project's
// own definition).  At global step t = 1, 2, ... a chain with row x and log density lp
//   proposes     p[j] = x[j] + step[j] * z[j]         (one multiply, one add, uncontracted: NumPy's
//                                                       x + step * z bit for bit)
//   evaluates    lp_new = log_target_density(p)        theta = exp(p); a theta that is zero or not
//                                                       finite, or an integration that ends with a
//                                                       non-zero status, rejects and counts in n_failed
//   accepts      exactly when log_u < lp_new - lp      (strict; a NaN on either side rejects)
//   writes       row t of the chain and log_p[t].
// log_target_density is what lv_kernel<2> + lv_logdens_finish (lv.hip) compute, through the same code
// (lv_rk45.hpp: the integrator, the dense output at the observation times, the whitening by U and the
// prior term), with ONE difference: the sum over the observation times runs in time order in a register
// instead of NumPy's pairwise order over a stored (t_n, n) array.  That moves the value by ~1e-13
// relative, inside the 1e-8 the LV tests hold to scipy.  theta = exp(p) is the device's exp (lv.hip takes
// NumPy's from the caller): at most an ulp of theta apart, ~1e-15 relative in the density.
//
// Noise, a template parameter:
//   supplied   z (chains, noise_ld, 4) and log_u (chains, noise_ld) written by the caller;
//   device     NumPy's Philox (Philox4x64-10): chain c with seed s uses key (s, c); step t uses the
//              two blocks with counter word 0 equal to 2t - 1 and 2t (the other words 0) -- the eight
//              values np.random.Philox(key=[s, c], counter=[0, 0, 0, 0]).random_raw(8 t)[8 (t - 1):]
//              (NumPy adds 1 to the counter before its first block).  From r0 .. r7:
//              u_k = ((r_k >> 11) + 1) 2^-53 (k < 4), (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1),
//              (z2, z3) likewise from u2, u3, log_u = log((r4 >> 11) 2^-53) (zero: -inf, accepts).
//              The noise depends on (seed, chain id, t) only; RECORD also writes the z and log_u used.
// The chain state (x, lp, accepted, n_failed: 8 words per chain) is read from a.state when the
// launch starts and written back when it ends, so a long run is a sequence of short launches with
// identical results.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include "lv_rk45.hpp"

namespace st {
namespace {

constexpr int kMcmcThreads = 64;

// log_target_density(lth), theta = exp(lth) given; NaN when the integration fails (lv_integrate's status 1:
// step size below min_step, 2: max_steps reached).  lv_kernel<2>'s integration and per-time term, the term
// added to `ll` in time order instead of stored.
__device__ __forceinline__ double lv_logdens_one(const LvProblem& p, const double lth[4], const double th[4]) {
    int kk = 0;
    double ll = 0.0;                  // sum of the per-time terms, in time order
    const int status = lv_integrate<2>(th, p, [&](double t_old, double t_new, double inv_hd, const double* y,
                                                  const double (*Q)[rk45::kDenseOrder], bool last) {
        lv_observe<2>(p, kk, t_old, t_new, inv_hd, y, Q, last,
                      [&](int k, const double* u) { ll += lv_loglik_term(p, k, u); });
        return 0;
    });
    if (status) return NAN;
    return ll + lv_log_prior(lth, p.norm_logc);
}

// Philox4x64-10 (Random123; numpy/random/src/philox): one block for counter (c0, c1, 0, 0), key (k0, k1)
__device__ inline void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t k1, uint64_t out[4]) {
    constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
    uint64_t c[4] = {c0, c1, 0, 0};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += W0; k1 += W1; }
        const uint64_t hi0 = __umul64hi(M0, c[0]), lo0 = M0 * c[0];
        const uint64_t hi1 = __umul64hi(M1, c[2]), lo1 = M1 * c[2];
        const uint64_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = c[q];
}

// the noise of step t of chain `chain` (file header)
__device__ inline void device_noise(uint64_t seed, uint64_t chain, uint64_t t, double z[4], double& log_u) {
    uint64_t r[4], q[4];
    philox4x64_10(2 * t - 1, 0, seed, chain, r);
    philox4x64_10(2 * t, 0, seed, chain, q);
    constexpr double k2m53 = 0x1.0p-53, kTwoPi = 6.283185307179586;
    double u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = (double)((r[k] >> 11) + 1) * k2m53;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const double rad = sqrt(-2.0 * log(u[k])), ang = kTwoPi * u[k + 1];
        z[k] = rad * cos(ang);
        z[k + 1] = rad * sin(ang);
    }
    log_u = log((double)(q[0] >> 11) * k2m53);
}

// ---- the blocks the six kernels share, one copy of each; the loops stay in the kernels ----
// four doubles at a 16-byte aligned address, as two 16-byte accesses
__device__ __forceinline__ void load4(const double* src, double v[4]) {
    const double2 lo = reinterpret_cast<const double2*>(src)[0], hi = reinterpret_cast<const double2*>(src)[1];
    v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
}
__device__ __forceinline__ void store4(double* dst, const double v[4]) {
    reinterpret_cast<double2*>(dst)[0] = make_double2(v[0], v[1]);
    reinterpret_cast<double2*>(dst)[1] = make_double2(v[2], v[3]);
}

// the chain's state record: x[4], lp, accepted, n_failed, one spare (8 words); the gradient samplers' records go on
// with g[4] at word 8 (16 words, read and written by hand in those kernels).  The caller decides which lanes store.
__device__ __forceinline__ void load_chain8(const double* st, double x[4], double& lp, int64_t& accepted,
                                            int64_t& failed) {
    load4(st, x);
    lp = st[4];
    accepted = reinterpret_cast<const int64_t*>(st)[5];
    failed = reinterpret_cast<const int64_t*>(st)[6];
}
__device__ __forceinline__ void store_chain8(double* st, const double x[4], double lp, int64_t accepted,
                                             int64_t failed) {
    store4(st, x);
    st[4] = lp;
    reinterpret_cast<int64_t*>(st)[5] = accepted;
    reinterpret_cast<int64_t*>(st)[6] = failed;
}

// row k of the chain's output: the row and its log density
__device__ __forceinline__ void store_row(double* rows, double* lps, int64_t k, const double x[4], double lp) {
    store4(rows + 4 * k, x);
    lps[k] = lp;
}

// The noise of the step written to row k: z[4] and log_u.  DEVICE_NOISE: Philox noise of global step t (else zs / lus
// are read); RECORD (device noise only): the `writer` lanes write the values used to zs / lus.
template <bool DEVICE_NOISE, bool RECORD>
__device__ __forceinline__ void step_noise(uint64_t seed, uint64_t chain, uint64_t t, double* zs, double* lus,
                                           int64_t k, bool writer, double z[4], double& log_u) {
    if constexpr (DEVICE_NOISE) {
        device_noise(seed, chain, t, z, log_u);
        if constexpr (RECORD) {
            if (writer) {
                store4(zs + 4 * k, z);
                lus[k] = log_u;
            }
        }
    } else {
        load4(zs + 4 * k, z);
        log_u = lus[k];
    }
}

// DEVICE_NOISE, RECORD: step_noise's.  a.init: the thread first evaluates its start row, stores it as row
// out_row0 - 1 and takes its density as lp (NaN when that evaluation fails: every later proposal is then
// rejected and the caller sees the NaN in log_p).
template <bool DEVICE_NOISE, bool RECORD>
__global__ __launch_bounds__(kMcmcThreads) void lv_rwmh_kernel(LvMcmcArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x;
    if (i >= a.chains) return;
    double* st = a.state + 8 * i;
    double x[4], lp;
    int64_t accepted, failed;
    load_chain8(st, x, lp, accepted, failed);
    double* rows = a.samples + (i * a.out_ld + a.out_row0) * 4;
    double* lps = a.log_p + i * a.out_ld + a.out_row0;
    double* zs = nullptr;
    double* lus = nullptr;
    if (!DEVICE_NOISE || RECORD) {
        zs = a.z + (i * a.noise_ld + a.noise_row0) * 4;
        lus = a.log_u + i * a.noise_ld + a.noise_row0;
    }
    const uint64_t chain = (uint64_t)(a.first_chain + i);
    // k = -1: the start row itself (a.init), evaluated by the same code as every proposal
#pragma unroll 1
    for (int64_t k = a.init ? -1 : 0; k < a.steps; ++k) {
        const bool start = k < 0;
        double z[4] = {0.0, 0.0, 0.0, 0.0}, log_u = 0.0;
        if (!start)
            step_noise<DEVICE_NOISE, RECORD>(a.seed, chain, (uint64_t)(a.first_step + k), zs, lus, k, true, z, log_u);
        double p[4], th[4];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[j] = start ? x[j] : x[j] + a.step[j] * z[j];
            th[j] = exp(p[j]);
            ok = ok && isfinite(th[j]) && th[j] != 0.0;
        }
        double lp_new = NAN;
        if (ok) lp_new = lv_logdens_one(a.p, p, th);
        if (start) {
            lp = lp_new;
        } else {
            if (!(lp_new == lp_new)) ++failed;      // theta out of range, or the integration failed
            if (log_u < lp_new - lp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = p[j];
                lp = lp_new;
                ++accepted;
            }
        }
        store_row(rows, lps, k, x, lp);
    }
    store_chain8(st, x, lp, accepted, failed);
}

// ---- wave layout: one wave (64 lanes) per chain, for a few long chains (file header) ----
constexpr int kWaveLanes = 64;
constexpr int kWaveChainsPerBlock = 4;      // one wave on each SIMD of a CU

// lane 0's value in every lane, provably wave-uniform
__device__ __forceinline__ double wave_first(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// The same Metropolis loop, with the same arguments and state record, as lv_rwmh_kernel.  Everything but the
// observation terms is replicated: every lane of the wave holds the chain's state, reads or draws the step's
// noise, forms the proposal, takes exp and runs lv_integrate<2> -- same inputs, same instructions, so the 64
// lanes hold the same bits and every branch of the integrator goes one way for the whole wave.  The chain
// id comes from blockIdx and a readfirstlane of the wave's index in its block, so the compiler knows it.
// After each accepted RK45 step lane l evaluates the observation points k = l (mod 64) of that step
// (lv_observe_strided: lv_observe's segment rule per point, per-term values bit-identical to the thread
// layout's).  The cursors are per lane and there is no cross-lane operation inside the integration.
// SUMMATION ORDER (part of the contract): lane l adds its terms to 0.0 in increasing k over the whole
// integration; the 64 partials are then combined by the xor butterfly v += shfl_xor(v, off), off = 32, 16,
// 8, 4, 2, 1 (IEEE addition is commutative: every lane ends with the same bits); lp_new = that sum +
// lv_log_prior.  The order depends on t_n only -- not on the RK45 step sequence, the grid or the launch
// split.  For t_n <= 2 it is the thread layout's order ((0 + term_0) + term_1).  The butterfly runs in every
// step of every live wave, outside any data-dependent branch, and the accept decision is taken from lane 0's
// sum (wave_first), so no lane can leave its wave.  Lane 0 alone stores.
template <bool DEVICE_NOISE, bool RECORD>
__global__ __launch_bounds__(kWaveLanes * kWaveChainsPerBlock) void lv_rwmh_wave_kernel(LvMcmcArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWaveLanes));
    const int lane = (int)(threadIdx.x % kWaveLanes);
    const int64_t i = (int64_t)blockIdx.x * kWaveChainsPerBlock + wave;
    if (i >= a.chains) return;            // the whole wave (partial last block)
    double* st = a.state + 8 * i;
    double x[4], lp;
    int64_t accepted, failed;
    load_chain8(st, x, lp, accepted, failed);
    double* rows = a.samples + (i * a.out_ld + a.out_row0) * 4;
    double* lps = a.log_p + i * a.out_ld + a.out_row0;
    double* zs = nullptr;
    double* lus = nullptr;
    if (!DEVICE_NOISE || RECORD) {
        zs = a.z + (i * a.noise_ld + a.noise_row0) * 4;
        lus = a.log_u + i * a.noise_ld + a.noise_row0;
    }
    const uint64_t chain = (uint64_t)(a.first_chain + i);
#pragma unroll 1
    for (int64_t k = a.init ? -1 : 0; k < a.steps; ++k) {
        const bool start = k < 0;
        double z[4] = {0.0, 0.0, 0.0, 0.0}, log_u = 0.0;
        if (!start)
            step_noise<DEVICE_NOISE, RECORD>(a.seed, chain, (uint64_t)(a.first_step + k), zs, lus, k, lane == 0, z,
                                             log_u);
        double p[4], th[4];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[j] = start ? x[j] : x[j] + a.step[j] * z[j];
            th[j] = exp(p[j]);
            ok = ok && isfinite(th[j]) && th[j] != 0.0;
        }
        double ll = 0.0;                  // this lane's terms, in increasing k
        int status = 0;
        if (ok) {
            int kq = lane;
            double tq = lane < a.p.t_n ? a.p.t_eval[lane] : 0.0;
            status = lv_integrate<2>(th, a.p, [&](double t_old, double t_new, double inv_hd, const double* y,
                                                  const double (*Q)[rk45::kDenseOrder], bool last) {
                lv_observe_strided<2>(a.p, kq, tq, kWaveLanes, t_old, t_new, inv_hd, y, Q, last,
                                      [&](int kk, const double* u) { ll += lv_loglik_term(a.p, kk, u); });
                return 0;
            });
        }
#pragma unroll
        for (int off = kWaveLanes / 2; off >= 1; off >>= 1) ll += __shfl_xor(ll, off);
        double lp_new = NAN;              // theta out of range, or the integration failed
        if (ok && status == 0) lp_new = wave_first(ll) + lv_log_prior(p, a.p.norm_logc);
        if (start) {
            lp = lp_new;
        } else {
            if (!(lp_new == lp_new)) ++failed;
            if (log_u < lp_new - lp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = p[j];
                lp = lp_new;
                ++accepted;
            }
        }
        if (lane == 0) store_row(rows, lps, k, x, lp);
    }
    if (lane == 0) store_chain8(st, x, lp, accepted, failed);
}

// ---- Metropolis-adjusted Langevin (MALA) sampler, one wave per chain ----
// The chain runs in x = log theta.  The host hands over eps, h = 0.5 eps^2, w = 0.5 / eps^2 and the drift cap
// c = drift_cap * eps (+inf: no cap) as doubles.  ONE 10-state integration (lv_integrate<10>: the system with
// its forward sensitivities) at theta = exp(x) (the device's exp) gives u and J = du/dtheta at the observation
// times, and from them
//   lp(x)  = sum_k lv_loglik_term(k, u_k) + lv_log_prior(x)
//   acc_j  = sum_k (J_k^T C^-1 (y_k - u_k))_j                        (lv_grad_term: lv_kernel<10>'s expression)
//   g_j(x) = theta_j acc_j - x_j                                     (the gradient of lp with respect to x)
// One Metropolis step, every operation uncontracted and in this order:
//   d_j(x) = min(max(h_j g_j(x), -c_j), c_j)                         (a NaN stays a NaN)
//   p_j    = (x_j + d_j(x)) + eps_j z_j
//   rf_j   = (p_j - x_j) - d_j(x),   rr_j = (x_j - p_j) - d_j(p)
//   qf     = sum_j w_j rf_j rf_j,    qr = sum_j w_j rr_j rr_j        (((w rf) rf), from 0.0, j ascending)
//   accept exactly when log_u < (lp(p) - lp(x)) + (qf - qr)          (strict; a NaN anywhere rejects)
// A theta with a zero or non-finite component, or an integration that ends with a non-zero status, rejects and
// counts in n_failed.  Row t, log_p[t] and grad[t] = g(row t) are written for every row.
// lp comes from the 10-state solution, whose RK45 step sequence is not the 2-state one of lv_rwmh*: the two
// densities differ by the integrator's tolerance, not by rounding.
// Layout, noise, init and the hand-off between launches are lv_rwmh_wave_kernel's; the state record has 16 words
// per chain (x[4], lp, accepted, n_failed, one spare, g[4], four spare).
// SUMMATION ORDER (part of the contract): lane l adds the terms of its points k = l (mod 64) to 0.0 in
// increasing k over the whole integration -- one sum for ll, one for each acc_j; each of the five is then
// combined by the xor butterfly v += shfl_xor(v, off), off = 32, 16, 8, 4, 2, 1; lp = that sum + lv_log_prior.
// The order depends on t_n only.  For t_n <= 2 it is the time order ((0 + term_0) + term_1).  The butterflies run
// once per Metropolis step, outside any data-dependent branch, also for a proposal rejected without
// integrating; the decision is taken from lane 0's values (wave_first); lane 0 alone stores.
__device__ __forceinline__ double mala_clip(double v, double c) {
    v = v < -c ? -c : v;                  // (comparisons, not fmax / fmin: a NaN drift stays a NaN and rejects)
    return v > c ? c : v;
}

// Written out in each of the four gradient kernels, not helpers (DESIGN.md section 17.1 has the measurements): the
// 16-word state record and the row stores, K(r), the wave evaluation (lv_integrate<10>, the butterflies, lp_new /
// g_new), the Lam position update and the accept statistic.  Shared: step_noise above and dual_average below.

template <bool DEVICE_NOISE, bool RECORD>
__global__ __launch_bounds__(kWaveLanes * kWaveChainsPerBlock) void lv_mala_wave_kernel(LvMalaArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWaveLanes));
    const int lane = (int)(threadIdx.x % kWaveLanes);
    const int64_t i = (int64_t)blockIdx.x * kWaveChainsPerBlock + wave;
    if (i >= a.chains) return;            // the whole wave (partial last block)
    double* st = a.state + 16 * i;
    int64_t* sti = reinterpret_cast<int64_t*>(st);
    double x[4], g[4], lp;
    {
        const double2* s2 = reinterpret_cast<const double2*>(st);
        const double2 s0 = s2[0], s1 = s2[1], g0 = s2[4], g1 = s2[5];
        x[0] = s0.x; x[1] = s0.y; x[2] = s1.x; x[3] = s1.y;
        g[0] = g0.x; g[1] = g0.y; g[2] = g1.x; g[3] = g1.y;
    }
    lp = st[4];
    int64_t accepted = sti[5], failed = sti[6];
    double* rows = a.samples + (i * a.out_ld + a.out_row0) * 4;
    double* grads = a.grad + (i * a.out_ld + a.out_row0) * 4;
    double* lps = a.log_p + i * a.out_ld + a.out_row0;
    double* zs = nullptr;
    double* lus = nullptr;
    if (!DEVICE_NOISE || RECORD) {
        zs = a.z + (i * a.noise_ld + a.noise_row0) * 4;
        lus = a.log_u + i * a.noise_ld + a.noise_row0;
    }
    const uint64_t chain = (uint64_t)(a.first_chain + i);
    // k = -1: the start row itself (a.init), evaluated by the same code as every proposal
#pragma unroll 1
    for (int64_t k = a.init ? -1 : 0; k < a.steps; ++k) {
        const bool start = k < 0;
        double z[4] = {0.0, 0.0, 0.0, 0.0}, log_u = 0.0;
        if (!start)
            step_noise<DEVICE_NOISE, RECORD>(a.seed, chain, (uint64_t)(a.first_step + k), zs, lus, k, lane == 0, z,
                                             log_u);
        double d[4], p[4], th[4];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = mala_clip(a.h[j] * g[j], a.clip[j]);
            p[j] = start ? x[j] : (x[j] + d[j]) + a.eps[j] * z[j];
            th[j] = exp(p[j]);
            ok = ok && isfinite(th[j]) && th[j] != 0.0;
        }
        double ll = 0.0, acc[4] = {0.0, 0.0, 0.0, 0.0};     // this lane's terms, in increasing k
        int status = 0;
        if (ok) {
            int kq = lane;
            double tq = lane < a.p.t_n ? a.p.t_eval[lane] : 0.0;
            status = lv_integrate<10>(th, a.p, [&](double t_old, double t_new, double inv_hd, const double* y,
                                                   const double (*Q)[rk45::kDenseOrder], bool last) {
                lv_observe_strided<10>(a.p, kq, tq, kWaveLanes, t_old, t_new, inv_hd, y, Q, last,
                                       [&](int kk, const double* u) {
                                           ll += lv_loglik_term(a.p, kk, u);
                                           lv_grad_term(a.p, a.cinv, kk, u, acc);
                                       });
                return 0;
            });
        }
#pragma unroll
        for (int off = kWaveLanes / 2; off >= 1; off >>= 1) {
            ll += __shfl_xor(ll, off);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off);
        }
        double lp_new = NAN, g_new[4] = {NAN, NAN, NAN, NAN};   // theta out of range, or the integration failed
        if (ok && status == 0) {
            lp_new = wave_first(ll) + lv_log_prior(p, a.p.norm_logc);
#pragma unroll
            for (int j = 0; j < 4; ++j) g_new[j] = th[j] * wave_first(acc[j]) - p[j];
        }
        if (start) {
            lp = lp_new;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = g_new[j];
        } else {
            if (!(lp_new == lp_new)) ++failed;
            double qf = 0.0, qr = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double rf = (p[j] - x[j]) - d[j];
                const double rr = (x[j] - p[j]) - mala_clip(a.h[j] * g_new[j], a.clip[j]);
                qf += a.w[j] * rf * rf;
                qr += a.w[j] * rr * rr;
            }
            if (log_u < (lp_new - lp) + (qf - qr)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { x[j] = p[j]; g[j] = g_new[j]; }
                lp = lp_new;
                ++accepted;
            }
        }
        if (lane == 0) {
            reinterpret_cast<double2*>(rows + 4 * k)[0] = make_double2(x[0], x[1]);
            reinterpret_cast<double2*>(rows + 4 * k)[1] = make_double2(x[2], x[3]);
            reinterpret_cast<double2*>(grads + 4 * k)[0] = make_double2(g[0], g[1]);
            reinterpret_cast<double2*>(grads + 4 * k)[1] = make_double2(g[2], g[3]);
            lps[k] = lp;
        }
    }
    if (lane == 0) {
        double2* s2 = reinterpret_cast<double2*>(st);
        s2[0] = make_double2(x[0], x[1]);
        s2[1] = make_double2(x[2], x[3]);
        s2[4] = make_double2(g[0], g[1]);
        s2[5] = make_double2(g[2], g[3]);
        st[4] = lp;
        sti[5] = accepted;
        sti[6] = failed;
    }
}

// ---- Hamiltonian Monte Carlo (HMC) sampler, one wave per chain ----
// The chain runs in x = log theta with unit-variance momenta; the host hands over eps[4] (a vector eps is a diagonal
// mass matrix), the kick cap c[4] (+inf: none) and the trajectory length L >= 1.  lp(x) and g(x) are
// lv_mala_wave_kernel's: one lv_integrate<10> at theta = exp(x), the same per-lane sums and xor butterflies.  One
// Metropolis step, every operation uncontracted and in this order:
//   kick_j(q) = min(max(eps_j g_j(q), -c_j), c_j)   (mala_clip: a NaN stays a NaN),   hk_j(q) = 0.5 kick_j(q)
//   r^0 = z (the step's four normals),   K(r) = 0.5 s,  s = sum_j r_j r_j from 0.0, j ascending
//   stage l = 1 .. L from (q^0, r^0) = (x, z):
//       r'  = r^(l-1) + hk(q^(l-1))
//       q^l = q^(l-1) + eps r'                       (one multiply, one add per component)
//       lp(q^l), g(q^l)                              (one integration)
//       r^l = r' + hk(q^l)
//   accept exactly when log_u < (lp(q^L) - lp(x)) + (K(r^0) - K(r^L))     (strict; a NaN anywhere rejects)
// An interior kick is two half-kick additions, so a trajectory of L stages is, bit for bit, L one-stage trajectories
// chained through (q, r).  The clipped force depends on q alone, so every stage stays a shear (reversible, volume-
// preserving) and, with the true lp in the ratio, the chain still targets the posterior.  A stage whose theta has a
// zero or non-finite component, or whose integration ends with a non-zero status, has lp = g = NaN: the NaN goes
// through r into every later q of the trajectory, whose stages then run no integration, and the trajectory is
// rejected and counted ONCE in n_failed.  Row t, log_p[t] and grad[t] = g(row t) are written for every row.
// The step and stage loops are one flat loop (the start row is iteration -1), so the kernel has ONE lv_integrate<10>
// call site.  Layout, noise, init, the 16-word state record, the summation order and the hand-off between launches
// are lv_mala_wave_kernel's; a launch ends on a step boundary.  The butterflies run once per stage in every live
// wave, outside any data-dependent branch; decisions come from lane 0's values (wave_first); lane 0 alone stores.
template <bool DEVICE_NOISE, bool RECORD>
__global__ __launch_bounds__(kWaveLanes * kWaveChainsPerBlock) void lv_hmc_wave_kernel(LvHmcArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWaveLanes));
    const int lane = (int)(threadIdx.x % kWaveLanes);
    const int64_t i = (int64_t)blockIdx.x * kWaveChainsPerBlock + wave;
    if (i >= a.chains) return;            // the whole wave (partial last block)
    double* st = a.state + 16 * i;
    int64_t* sti = reinterpret_cast<int64_t*>(st);
    double x[4], g[4], lp;
    {
        const double2* s2 = reinterpret_cast<const double2*>(st);
        const double2 s0 = s2[0], s1 = s2[1], g0 = s2[4], g1 = s2[5];
        x[0] = s0.x; x[1] = s0.y; x[2] = s1.x; x[3] = s1.y;
        g[0] = g0.x; g[1] = g0.y; g[2] = g1.x; g[3] = g1.y;
    }
    lp = st[4];
    int64_t accepted = sti[5], failed = sti[6];
    double* rows = a.samples + (i * a.out_ld + a.out_row0) * 4;
    double* grads = a.grad + (i * a.out_ld + a.out_row0) * 4;
    double* lps = a.log_p + i * a.out_ld + a.out_row0;
    double* zs = nullptr;
    double* lus = nullptr;
    if (!DEVICE_NOISE || RECORD) {
        zs = a.z + (i * a.noise_ld + a.noise_row0) * 4;
        lus = a.log_u + i * a.noise_ld + a.noise_row0;
    }
    const uint64_t chain = (uint64_t)(a.first_chain + i);
    // the trajectory: its current point q with g(q), its momentum r, K(r^0) and the step's log_u
    double q[4], gq[4], r[4] = {0.0, 0.0, 0.0, 0.0}, k0 = 0.0, log_u = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { q[j] = x[j]; gq[j] = g[j]; }
    int l = 0;                            // stages of step k done
    // k = -1: the start row itself (a.init), evaluated by the same code as every stage
#pragma unroll 1
    for (int64_t k = a.init ? -1 : 0; k < a.steps;) {
        const bool start = k < 0;
        if (!start && l == 0) {
            step_noise<DEVICE_NOISE, RECORD>(a.seed, chain, (uint64_t)(a.first_step + k), zs, lus, k, lane == 0, r,
                                             log_u);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += r[j] * r[j];
            k0 = 0.5 * s;
        }
        double rp[4], p[4], th[4];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rp[j] = r[j] + 0.5 * mala_clip(a.eps[j] * gq[j], a.clip[j]);
            p[j] = start ? q[j] : q[j] + a.eps[j] * rp[j];
            th[j] = exp(p[j]);
            ok = ok && isfinite(th[j]) && th[j] != 0.0;
        }
        double ll = 0.0, acc[4] = {0.0, 0.0, 0.0, 0.0};     // this lane's terms, in increasing k
        int status = 0;
        if (ok) {
            int kq = lane;
            double tq = lane < a.p.t_n ? a.p.t_eval[lane] : 0.0;
            status = lv_integrate<10>(th, a.p, [&](double t_old, double t_new, double inv_hd, const double* y,
                                                   const double (*Q)[rk45::kDenseOrder], bool last) {
                lv_observe_strided<10>(a.p, kq, tq, kWaveLanes, t_old, t_new, inv_hd, y, Q, last,
                                       [&](int kk, const double* u) {
                                           ll += lv_loglik_term(a.p, kk, u);
                                           lv_grad_term(a.p, a.cinv, kk, u, acc);
                                       });
                return 0;
            });
        }
#pragma unroll
        for (int off = kWaveLanes / 2; off >= 1; off >>= 1) {
            ll += __shfl_xor(ll, off);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off);
        }
        double lp_new = NAN, g_new[4] = {NAN, NAN, NAN, NAN};   // theta out of range, or the integration failed
        if (ok && status == 0) {
            lp_new = wave_first(ll) + lv_log_prior(p, a.p.norm_logc);
#pragma unroll
            for (int j = 0; j < 4; ++j) g_new[j] = th[j] * wave_first(acc[j]) - p[j];
        }
        if (start) {
            lp = lp_new;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = g_new[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = rp[j] + 0.5 * mala_clip(a.eps[j] * g_new[j], a.clip[j]);
                q[j] = p[j];
                gq[j] = g_new[j];
            }
            if (++l < a.n_leapfrog) continue;
            // the trajectory's end: a failed stage has made every later lp NaN
            if (!(lp_new == lp_new)) ++failed;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += r[j] * r[j];
            if (log_u < (lp_new - lp) + (k0 - 0.5 * s)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { x[j] = q[j]; g[j] = gq[j]; }
                lp = lp_new;
                ++accepted;
            }
        }
        if (lane == 0) {
            reinterpret_cast<double2*>(rows + 4 * k)[0] = make_double2(x[0], x[1]);
            reinterpret_cast<double2*>(rows + 4 * k)[1] = make_double2(x[2], x[3]);
            reinterpret_cast<double2*>(grads + 4 * k)[0] = make_double2(g[0], g[1]);
            reinterpret_cast<double2*>(grads + 4 * k)[1] = make_double2(g[2], g[3]);
            lps[k] = lp;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { q[j] = x[j]; gq[j] = g[j]; }
        l = 0;
        ++k;
    }
    if (lane == 0) {
        double2* s2 = reinterpret_cast<double2*>(st);
        s2[0] = make_double2(x[0], x[1]);
        s2[1] = make_double2(x[2], x[3]);
        s2[4] = make_double2(g[0], g[1]);
        s2[5] = make_double2(g[2], g[3]);
        st[4] = lp;
        sti[5] = accepted;
        sti[6] = failed;
    }
}

// ---- HMC with a per-chain step size and a dense metric, with step-size adaptation ----
// lv_hmc_wave_kernel's definition with three additions; every operation uncontracted and in the stated order.
// (1) eps is a scalar per chain and the metric a per-chain factor Lam (lower triangular, M^-1 = Lam Lam^T), both read
// from device memory: a.eps_chain[i] and the packed row-major lower triangle a.metric_chol[10 i ..] (Lam_jk at
// j (j + 1) / 2 + k).  The momentum stays r ~ N(0, I): the noise and K(r) are unchanged.  In a stage
//   f_j(q)    = Lam_jj g_j(q) + sum_{k > j} Lam_kj g_k(q)        (the first term alone, then k ascending)
//   kick_j(q) = min(max(eps f_j(q), -c_j), c_j),   hk = 0.5 kick
//   r'  = r + hk(q);   v_j = sum_{k <= j} Lam_jk r'_k  (from the k = 0 term, k ascending);   q_j <- q_j + eps v_j
//   r   = r' + hk(q)                                             (at the new q)
// which is unit-mass HMC in y = Lam^-1 x: the clipped force depends on q alone, so every stage stays a shear.  Lam is
// read again in every stage (uniform loads), not kept across the integration.
// (2) per step, a.accept_stat = alpha = min(1, exp(a)), a = (lp(q^L) - lp(x)) + (K(r^0) - K(r^L)), 0 when a is NaN, and
// a.step_size = the eps the step used (rows out_row0 + k of (chains, out_ld) arrays; the start row has none).
// (3) a.adapt = 1: eps comes from the state record and follows Stan's dual averaging after every step (dual_average;
// delta handed over, gamma 0.05, t0 10, kappa 0.75):  m <- m + 1;  eta = 1 / (m + t0);
// sbar <- (1 - eta) sbar + eta (delta - alpha);  ell = mu - (sbar sqrt(m)) / gamma;  w = pow(m, -kappa);
// xbar <- (1 - w) xbar + w ell;  eps <- exp(ell).
// The state record has 24 words per chain: LvMalaArgs' 16, then eps, m, sbar, xbar, mu and three spare.  The five are
// loaded and stored at the step's end -- only eps is live across the integration -- by EVERY lane (the same bits to the
// same address), so that each lane reads back what it wrote itself.  With a.adapt = 0 they are neither read nor
// written and eps stays a.eps_chain[i].  A launch ends on a step boundary with the whole state in the record.
constexpr int kHmcMetricStateWords = 24;
constexpr double kDaGamma = 0.05, kDaT0 = 10.0, kDaKappa = 0.75;

// hk(q) from g(q): the force through Lam^T, the cap, the half
__device__ __forceinline__ void metric_half_kick(const double* lam, const double g[4], double eps, const double c[4],
                                                 double hk[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double f = lam[j * (j + 1) / 2 + j] * g[j];
#pragma unroll
        for (int k = j + 1; k < 4; ++k) f += lam[k * (k + 1) / 2 + j] * g[k];
        hk[j] = 0.5 * mala_clip(eps * f, c[j]);
    }
}

// One step of the dual averaging (3) on the record's words 16 .. 20 (eps, m, sbar, xbar, mu); returns the new eps.
// Called by EVERY lane: each stores the same bits to the same address and reads back what it wrote itself.
__device__ __forceinline__ double dual_average(double* st, double delta, double alpha) {
    const double m = st[17] + 1.0, eta = 1.0 / (m + kDaT0);
    const double sbar = (1.0 - eta) * st[18] + eta * (delta - alpha);
    const double ell = st[20] - (sbar * sqrt(m)) / kDaGamma;
    const double w = pow(m, -kDaKappa);
    const double xbar = (1.0 - w) * st[19] + w * ell;
    const double eps = exp(ell);
    st[16] = eps;
    st[17] = m;
    st[18] = sbar;
    st[19] = xbar;
    return eps;
}

template <bool DEVICE_NOISE, bool RECORD>
__global__ __launch_bounds__(kWaveLanes * kWaveChainsPerBlock) void lv_hmc_metric_wave_kernel(LvHmcMetricArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWaveLanes));
    const int lane = (int)(threadIdx.x % kWaveLanes);
    const int64_t i = (int64_t)blockIdx.x * kWaveChainsPerBlock + wave;
    if (i >= a.chains) return;            // the whole wave (partial last block)
    double* st = a.state + kHmcMetricStateWords * i;
    int64_t* sti = reinterpret_cast<int64_t*>(st);
    double x[4], g[4], lp;
    {
        const double2* s2 = reinterpret_cast<const double2*>(st);
        const double2 s0 = s2[0], s1 = s2[1], g0 = s2[4], g1 = s2[5];
        x[0] = s0.x; x[1] = s0.y; x[2] = s1.x; x[3] = s1.y;
        g[0] = g0.x; g[1] = g0.y; g[2] = g1.x; g[3] = g1.y;
    }
    lp = st[4];
    int64_t accepted = sti[5], failed = sti[6];
    double eps = a.adapt ? st[16] : a.eps_chain[i];
    const double* lam = a.metric_chol + 10 * i;
    double* rows = a.samples + (i * a.out_ld + a.out_row0) * 4;
    double* grads = a.grad + (i * a.out_ld + a.out_row0) * 4;
    double* lps = a.log_p + i * a.out_ld + a.out_row0;
    double* alphas = a.accept_stat + i * a.out_ld + a.out_row0;
    double* epss = a.step_size + i * a.out_ld + a.out_row0;
    double* zs = nullptr;
    double* lus = nullptr;
    if (!DEVICE_NOISE || RECORD) {
        zs = a.z + (i * a.noise_ld + a.noise_row0) * 4;
        lus = a.log_u + i * a.noise_ld + a.noise_row0;
    }
    const uint64_t chain = (uint64_t)(a.first_chain + i);
    // the trajectory: its current point q with g(q), its momentum r, K(r^0) and the step's log_u
    double q[4], gq[4], r[4] = {0.0, 0.0, 0.0, 0.0}, k0 = 0.0, log_u = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { q[j] = x[j]; gq[j] = g[j]; }
    int l = 0;                            // stages of step k done
    // k = -1: the start row itself (a.init), evaluated by the same code as every stage
#pragma unroll 1
    for (int64_t k = a.init ? -1 : 0; k < a.steps;) {
        const bool start = k < 0;
        if (!start && l == 0) {
            step_noise<DEVICE_NOISE, RECORD>(a.seed, chain, (uint64_t)(a.first_step + k), zs, lus, k, lane == 0, r,
                                             log_u);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += r[j] * r[j];
            k0 = 0.5 * s;
        }
        double rp[4], p[4], th[4];
        bool ok = true;
        {
            double hk[4];
            metric_half_kick(lam, gq, eps, a.clip, hk);
#pragma unroll
            for (int j = 0; j < 4; ++j) rp[j] = r[j] + hk[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = lam[j * (j + 1) / 2] * rp[0];
#pragma unroll
                for (int kk = 1; kk <= j; ++kk) v += lam[j * (j + 1) / 2 + kk] * rp[kk];
                p[j] = start ? q[j] : q[j] + eps * v;
                th[j] = exp(p[j]);
                ok = ok && isfinite(th[j]) && th[j] != 0.0;
            }
        }
        double ll = 0.0, acc[4] = {0.0, 0.0, 0.0, 0.0};     // this lane's terms, in increasing k
        int status = 0;
        if (ok) {
            int kq = lane;
            double tq = lane < a.p.t_n ? a.p.t_eval[lane] : 0.0;
            status = lv_integrate<10>(th, a.p, [&](double t_old, double t_new, double inv_hd, const double* y,
                                                   const double (*Q)[rk45::kDenseOrder], bool last) {
                lv_observe_strided<10>(a.p, kq, tq, kWaveLanes, t_old, t_new, inv_hd, y, Q, last,
                                       [&](int kk, const double* u) {
                                           ll += lv_loglik_term(a.p, kk, u);
                                           lv_grad_term(a.p, a.cinv, kk, u, acc);
                                       });
                return 0;
            });
        }
        // a compiler barrier (no instruction): Lam is loaded again below instead of being held in 24 further
        // registers across the integration
        asm volatile("" ::: "memory");
#pragma unroll
        for (int off = kWaveLanes / 2; off >= 1; off >>= 1) {
            ll += __shfl_xor(ll, off);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off);
        }
        double lp_new = NAN, g_new[4] = {NAN, NAN, NAN, NAN};   // theta out of range, or the integration failed
        if (ok && status == 0) {
            lp_new = wave_first(ll) + lv_log_prior(p, a.p.norm_logc);
#pragma unroll
            for (int j = 0; j < 4; ++j) g_new[j] = th[j] * wave_first(acc[j]) - p[j];
        }
        if (start) {
            lp = lp_new;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = g_new[j];
        } else {
            double hk[4];
            metric_half_kick(lam, g_new, eps, a.clip, hk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = rp[j] + hk[j];
                q[j] = p[j];
                gq[j] = g_new[j];
            }
            if (++l < a.n_leapfrog) continue;
            // the trajectory's end: a failed stage has made every later lp NaN
            if (!(lp_new == lp_new)) ++failed;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += r[j] * r[j];
            const double da = (lp_new - lp) + (k0 - 0.5 * s);
            if (log_u < da) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { x[j] = q[j]; g[j] = gq[j]; }
                lp = lp_new;
                ++accepted;
            }
            const double ea = exp(da);
            const double alpha = da == da ? (ea < 1.0 ? ea : 1.0) : 0.0;
            if (lane == 0) {
                alphas[k] = alpha;
                epss[k] = eps;
            }
            if (a.adapt) eps = dual_average(st, a.delta, alpha);
        }
        if (lane == 0) {
            reinterpret_cast<double2*>(rows + 4 * k)[0] = make_double2(x[0], x[1]);
            reinterpret_cast<double2*>(rows + 4 * k)[1] = make_double2(x[2], x[3]);
            reinterpret_cast<double2*>(grads + 4 * k)[0] = make_double2(g[0], g[1]);
            reinterpret_cast<double2*>(grads + 4 * k)[1] = make_double2(g[2], g[3]);
            lps[k] = lp;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { q[j] = x[j]; gq[j] = g[j]; }
        l = 0;
        ++k;
    }
    if (lane == 0) {
        double2* s2 = reinterpret_cast<double2*>(st);
        s2[0] = make_double2(x[0], x[1]);
        s2[1] = make_double2(x[2], x[3]);
        s2[4] = make_double2(g[0], g[1]);
        s2[5] = make_double2(g[2], g[3]);
        st[4] = lp;
        sti[5] = accepted;
        sti[6] = failed;
    }
}

// ---- No-U-turn sampler (NUTS), one wave per chain ----
// lv_hmc_metric_wave_kernel's chain -- its stage, eps, Lam, cap, state record and dual averaging -- with the trajectory
// length chosen per step by a binary tree (Hoffman & Gelman's NUTS in Betancourt's multinomial form, built iteratively
// with checkpoints; the project's own definition, DESIGN.md section 22 is the contract).  A stage in direction v = +-1
// is the metric kernel's stage with eps replaced by v eps.  Noise is the device's Philox only: step t takes its
// momentum z from device_noise(seed, chain, t); stage l = 1, 2, ... of the step draws the block with counter
// (t, l, 0, 0) = r0 .. r3: log u_l = log((r0 >> 11) 2^-53); at the first stage of a doubling v = +1 when r1 >> 63 is 0
// and log u_T = log((r2 >> 11) 2^-53).
// One step from the row (x, lp, g): K0 = K(z); both ends (x, z, g); rho = z; W = 0; the proposal is the row.  Doubling
// j = 0, 1, ... builds 2^j leaves from the end on side v; leaf n = (q, r) has a_n = (lp(q) - lp) + (K0 - K(r)):
//   sum_alpha += min(1, exp(a_n))  (0 for a NaN);  a NaN a_n or a_n < -1000: divergent, the sub-tree is dropped, stop
//   W' = a_0, then W' <- lse(W', a_n), lse(p, s) = max(p, s) + log1p(exp(-|p - s|))
//   the sub-tree's proposal is leaf 0; leaf n > 0 replaces it exactly when log u_l < a_n - W' (W' updated; strict)
//   rho' = r_0, then rho' <- rho' + r_n
//   even n: the checkpoint (r_n, rho') goes to slot popcount(n >> 1)
//   odd n: for k = 1 .. (trailing one bits of n), the block of 2^k leaves that ends at n, first leaf m = n with its low
//          k bits cleared and checkpoint (r_a, rho'_a) in slot popcount(m >> 1): rho_b = (rho' - rho'_a) + r_a; the block
//          turns when NOT (dot(rho_b, r_a) > 0 AND dot(rho_b, r_n) > 0), dot from its j = 0 term; a turn drops the
//          sub-tree and stops
// A complete sub-tree's proposal replaces the tree's exactly when log u_T < W' - W; then W <- lse(W, W'), rho <- rho + rho',
// the end on side v becomes the last leaf, and the trajectory stops when the whole tree turns (rho, the two ends'
// momenta) or after max_depth doublings.  The new row is the proposal.
// Only q, g(q), r, eps and integer flags live across the integration; the tree (ends, proposals, rho, rho', checkpoints,
// scalars: 132 doubles) lives in a per-wave slab of LDS.  All of it is wave-uniform: EVERY lane stores the same bits to
// the same address and reads them back after a compiler barrier, so no ordering between lanes is relied on.  There is
// no block barrier: the four waves of a block are independent chains with different trip counts.  Branches on tree
// values go through readfirstlane (nuts_uniform); the butterflies stay in the loop's common path.
constexpr int kNutsMaxDepth = 10;
constexpr int kNutsEnd = 0;               // [side][q 4, r 4, g 4], side 0: the backward end, 1: the forward end
constexpr int kNutsProp = 24;             // the tree's proposal: x 4, g 4, lp
constexpr int kNutsSub = 34;              // the sub-tree's proposal, likewise
constexpr int kNutsRho = 44, kNutsRhoSub = 48;
constexpr int kNutsW = 52, kNutsWSub = 53, kNutsSumAlpha = 54, kNutsK0 = 55, kNutsLp0 = 56, kNutsLogU = 57,
              kNutsLogUT = 58;
constexpr int kNutsCk = 60;               // [slot][r 4, rho' 4], kNutsMaxDepth - 1 slots
constexpr int kNutsSlabWords = kNutsCk + 8 * (kNutsMaxDepth - 1);

__device__ __forceinline__ bool nuts_uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

__device__ __forceinline__ double nuts_lse(double p, double s) {
    return (p > s ? p : s) + log1p(exp(-fabs(p - s)));
}

// NOT (dot(rho, ra) > 0 AND dot(rho, rb) > 0)
__device__ __forceinline__ bool nuts_turns(const double rho[4], const double* ra, const double* rb) {
    double da = rho[0] * ra[0], db = rho[0] * rb[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) { da += rho[j] * ra[j]; db += rho[j] * rb[j]; }
    return !(da > 0.0 && db > 0.0);
}

template <bool RECORD>
__global__ __launch_bounds__(kWaveLanes * kWaveChainsPerBlock) void lv_nuts_wave_kernel(LvNutsArgs a) {
    __shared__ double slabs[kWaveChainsPerBlock][kNutsSlabWords];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWaveLanes));
    const int lane = (int)(threadIdx.x % kWaveLanes);
    const int64_t i = (int64_t)blockIdx.x * kWaveChainsPerBlock + wave;
    if (i >= a.chains) return;            // the whole wave (partial last block)
    double* sl = slabs[wave];
    double* st = a.state + kHmcMetricStateWords * i;
    int64_t* sti = reinterpret_cast<int64_t*>(st);
    // the trajectory: its current point q with g(q) and its momentum r
    double q[4], gq[4], r[4] = {0.0, 0.0, 0.0, 0.0};
    {
        const double2* s2 = reinterpret_cast<const double2*>(st);
        const double2 s0 = s2[0], s1 = s2[1], g0 = s2[4], g1 = s2[5];
        q[0] = s0.x; q[1] = s0.y; q[2] = s1.x; q[3] = s1.y;
        gq[0] = g0.x; gq[1] = g0.y; gq[2] = g1.x; gq[3] = g1.y;
#pragma unroll
        for (int j = 0; j < 4; ++j) { sl[kNutsProp + j] = q[j]; sl[kNutsProp + 4 + j] = gq[j]; }
        sl[kNutsProp + 8] = st[4];
    }
    int64_t accepted = sti[5], failed = sti[6];
    double eps = a.adapt ? st[16] : a.eps_chain[i];
    const double* lam = a.metric_chol + 10 * i;
    const int64_t row0 = i * a.out_ld + a.out_row0;
    double* rows = a.samples + row0 * 4;
    double* grads = a.grad + row0 * 4;
    double* lps = a.log_p + row0;
    double* zs = nullptr;
    if (RECORD) zs = a.z + (i * a.noise_ld + a.noise_row0) * 4;
    const uint64_t chain = (uint64_t)(a.first_chain + i);
    constexpr double k2m53 = 0x1.0p-53;
    int l = 0;                            // stages of step k done
    int n = 0;                            // leaves of the current sub-tree done
    int depth = 0;                        // doublings started
    int back = 0;                         // the current sub-tree's direction: 1 is v = -1
    int replaced = 0;                     // the tree's proposal has been replaced in this step
    // k = -1: the start row itself (a.init), evaluated by the same code as every stage
#pragma unroll 1
    for (int64_t k = a.init ? -1 : 0; k < a.steps;) {
        const bool start = k < 0;
        if (!start) {
            const uint64_t t = (uint64_t)(a.first_step + k);
            if (l == 0) {                 // the step begins: (q, gq) is the row
                double unused;
                device_noise(a.seed, chain, t, r, unused);
                if constexpr (RECORD) {
                    if (lane == 0) store4(zs + 4 * k, r);
                }
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) s += r[j] * r[j];
                sl[kNutsK0] = 0.5 * s;
                sl[kNutsLp0] = sl[kNutsProp + 8];
                sl[kNutsW] = 0.0;
                sl[kNutsSumAlpha] = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sl[kNutsRho + j] = r[j];
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        sl[kNutsEnd + 12 * side + j] = q[j];
                        sl[kNutsEnd + 12 * side + 4 + j] = r[j];
                        sl[kNutsEnd + 12 * side + 8 + j] = gq[j];
                    }
                }
                n = 0;
                depth = 0;
                replaced = 0;
            }
            uint64_t u[4];
            philox4x64_10(t, (uint64_t)(l + 1), a.seed, chain, u);
            sl[kNutsLogU] = log((double)(u[0] >> 11) * k2m53);
            if (n == 0) {                 // a doubling begins: its direction, its end
                back = (int)(u[1] >> 63);
                sl[kNutsLogUT] = log((double)(u[2] >> 11) * k2m53);
                const double* e = sl + kNutsEnd + (back ? 0 : 12);
#pragma unroll
                for (int j = 0; j < 4; ++j) { q[j] = e[j]; r[j] = e[4 + j]; gq[j] = e[8 + j]; }
                ++depth;
            }
        }
        const double ve = back ? -eps : eps;
        double rp[4], p[4], th[4];
        bool ok = true;
        {
            double hk[4];
            metric_half_kick(lam, gq, ve, a.clip, hk);
#pragma unroll
            for (int j = 0; j < 4; ++j) rp[j] = r[j] + hk[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = lam[j * (j + 1) / 2] * rp[0];
#pragma unroll
                for (int kk = 1; kk <= j; ++kk) v += lam[j * (j + 1) / 2 + kk] * rp[kk];
                p[j] = start ? q[j] : q[j] + ve * v;
                th[j] = exp(p[j]);
                ok = ok && isfinite(th[j]) && th[j] != 0.0;
            }
        }
        // compiler barriers (no instruction): nothing of the slab is held in registers across the integration
        asm volatile("" ::: "memory");
        double ll = 0.0, acc[4] = {0.0, 0.0, 0.0, 0.0};     // this lane's terms, in increasing k
        int status = 0;
        if (ok) {
            int kq = lane;
            double tq = lane < a.p.t_n ? a.p.t_eval[lane] : 0.0;
            status = lv_integrate<10>(th, a.p, [&](double t_old, double t_new, double inv_hd, const double* y,
                                                   const double (*Q)[rk45::kDenseOrder], bool last) {
                lv_observe_strided<10>(a.p, kq, tq, kWaveLanes, t_old, t_new, inv_hd, y, Q, last,
                                       [&](int kk, const double* u) {
                                           ll += lv_loglik_term(a.p, kk, u);
                                           lv_grad_term(a.p, a.cinv, kk, u, acc);
                                       });
                return 0;
            });
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int off = kWaveLanes / 2; off >= 1; off >>= 1) {
            ll += __shfl_xor(ll, off);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off);
        }
        double lp_new = NAN, g_new[4] = {NAN, NAN, NAN, NAN};   // theta out of range, or the integration failed
        if (ok && status == 0) {
            lp_new = wave_first(ll) + lv_log_prior(p, a.p.norm_logc);
#pragma unroll
            for (int j = 0; j < 4; ++j) g_new[j] = th[j] * wave_first(acc[j]) - p[j];
        }
        if (start) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { sl[kNutsProp + j] = q[j]; sl[kNutsProp + 4 + j] = g_new[j]; }
            sl[kNutsProp + 8] = lp_new;
        } else {
            {
                double hk[4];
                metric_half_kick(lam, g_new, ve, a.clip, hk);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    r[j] = rp[j] + hk[j];
                    q[j] = p[j];
                    gq[j] = g_new[j];
                }
            }
            ++l;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += r[j] * r[j];
            const double da = wave_first((lp_new - sl[kNutsLp0]) + (sl[kNutsK0] - 0.5 * s));
            const double ea = exp(da);
            sl[kNutsSumAlpha] = sl[kNutsSumAlpha] + (da == da ? (ea < 1.0 ? ea : 1.0) : 0.0);
            const bool divergent = nuts_uniform(!(da == da) || da < -1000.0);
            bool stop = divergent;
            if (!stop) {
                double wp = da, rs[4];
                bool take = true;
                if (n == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) rs[j] = r[j];
                } else {
                    wp = nuts_lse(sl[kNutsWSub], da);
#pragma unroll
                    for (int j = 0; j < 4; ++j) rs[j] = sl[kNutsRhoSub + j] + r[j];
                    take = nuts_uniform(sl[kNutsLogU] < da - wp);
                }
                sl[kNutsWSub] = wp;
#pragma unroll
                for (int j = 0; j < 4; ++j) sl[kNutsRhoSub + j] = rs[j];
                if (take) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { sl[kNutsSub + j] = q[j]; sl[kNutsSub + 4 + j] = gq[j]; }
                    sl[kNutsSub + 8] = lp_new;
                }
                if ((n & 1) == 0) {
                    double* ck = sl + kNutsCk + 8 * __builtin_popcount((unsigned)(n >> 1));
#pragma unroll
                    for (int j = 0; j < 4; ++j) { ck[j] = r[j]; ck[4 + j] = rs[j]; }
                } else {
#pragma unroll 1
                    for (int kk = 1; ((n >> (kk - 1)) & 1) && !stop; ++kk) {
                        const int m = n & ~((1 << kk) - 1);
                        const double* ck = sl + kNutsCk + 8 * __builtin_popcount((unsigned)(m >> 1));
                        double rb[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) rb[j] = (rs[j] - ck[4 + j]) + ck[j];
                        stop = nuts_uniform(nuts_turns(rb, ck, r));
                    }
                }
            }
            if (!stop) {
                if (++n < (1 << (depth - 1))) continue;      // the sub-tree's next leaf
                // the sub-tree is complete: merge it
                const double w = sl[kNutsW], wp = sl[kNutsWSub];
                if (nuts_uniform(sl[kNutsLogUT] < wp - w)) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) sl[kNutsProp + j] = sl[kNutsSub + j];
                    replaced = 1;
                }
                sl[kNutsW] = nuts_lse(w, wp);
                double rho[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    rho[j] = sl[kNutsRho + j] + sl[kNutsRhoSub + j];
                    sl[kNutsRho + j] = rho[j];
                }
                double* e = sl + kNutsEnd + (back ? 0 : 12);
#pragma unroll
                for (int j = 0; j < 4; ++j) { e[j] = q[j]; e[4 + j] = r[j]; e[8 + j] = gq[j]; }
                n = 0;
                stop = nuts_uniform(nuts_turns(rho, sl + kNutsEnd + 4, sl + kNutsEnd + 12 + 4)) || depth >= a.max_depth;
                if (!stop) continue;                         // the next doubling
            }
            // the step's end
            const double alpha = sl[kNutsSumAlpha] / (double)l;
            accepted += replaced;
            failed += divergent ? 1 : 0;
            if (lane == 0) {
                a.accept_stat[row0 + k] = alpha;
                a.step_size[row0 + k] = eps;
                a.tree_depth[row0 + k] = (double)depth;
                a.n_leapfrog[row0 + k] = (double)l;
                a.divergent[row0 + k] = divergent ? 1.0 : 0.0;
            }
            if (a.adapt) eps = dual_average(st, a.delta, alpha);
        }
        // the row: the proposal
#pragma unroll
        for (int j = 0; j < 4; ++j) { q[j] = sl[kNutsProp + j]; gq[j] = sl[kNutsProp + 4 + j]; }
        if (lane == 0) {
            reinterpret_cast<double2*>(rows + 4 * k)[0] = make_double2(q[0], q[1]);
            reinterpret_cast<double2*>(rows + 4 * k)[1] = make_double2(q[2], q[3]);
            reinterpret_cast<double2*>(grads + 4 * k)[0] = make_double2(gq[0], gq[1]);
            reinterpret_cast<double2*>(grads + 4 * k)[1] = make_double2(gq[2], gq[3]);
            lps[k] = sl[kNutsProp + 8];
        }
        l = 0;
        ++k;
    }
    if (lane == 0) {
        double2* s2 = reinterpret_cast<double2*>(st);
        s2[0] = make_double2(q[0], q[1]);
        s2[1] = make_double2(q[2], q[3]);
        s2[4] = make_double2(gq[0], gq[1]);
        s2[5] = make_double2(gq[2], gq[3]);
        st[4] = sl[kNutsProp + 8];
        sti[5] = accepted;
        sti[6] = failed;
    }
}

// kernel[noise_mode] (supplied, Philox, Philox + record) over a.chains chains, chains_per_block to a block
template <class Args>
hipError_t launch_noise_mode(void (*const (&kernel)[3])(Args), const Args& a, int chains_per_block,
                             unsigned threads, hipStream_t s) {
    const unsigned blocks = (unsigned)((a.chains + chains_per_block - 1) / chains_per_block);
    kernel[a.noise_mode]<<<blocks, threads, 0, s>>>(a);
    return hipGetLastError();
}
constexpr unsigned kWaveThreads = kWaveLanes * kWaveChainsPerBlock;

}  // namespace

hipError_t launch_lv_mala_wave(const LvMalaArgs& a, hipStream_t s) {
    return launch_noise_mode<LvMalaArgs>({lv_mala_wave_kernel<false, false>, lv_mala_wave_kernel<true, false>,
                                          lv_mala_wave_kernel<true, true>}, a, kWaveChainsPerBlock, kWaveThreads, s);
}

hipError_t launch_lv_hmc_wave(const LvHmcArgs& a, hipStream_t s) {
    return launch_noise_mode<LvHmcArgs>({lv_hmc_wave_kernel<false, false>, lv_hmc_wave_kernel<true, false>,
                                         lv_hmc_wave_kernel<true, true>}, a, kWaveChainsPerBlock, kWaveThreads, s);
}

hipError_t launch_lv_hmc_metric_wave(const LvHmcMetricArgs& a, hipStream_t s) {
    return launch_noise_mode<LvHmcMetricArgs>({lv_hmc_metric_wave_kernel<false, false>,
                                               lv_hmc_metric_wave_kernel<true, false>,
                                               lv_hmc_metric_wave_kernel<true, true>}, a, kWaveChainsPerBlock,
                                              kWaveThreads, s);
}

hipError_t launch_lv_nuts_wave(const LvNutsArgs& a, hipStream_t s) {
    const unsigned blocks = (unsigned)((a.chains + kWaveChainsPerBlock - 1) / kWaveChainsPerBlock);
    if (a.noise_mode == 2)
        lv_nuts_wave_kernel<true><<<blocks, kWaveThreads, 0, s>>>(a);
    else
        lv_nuts_wave_kernel<false><<<blocks, kWaveThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_lv_rwmh_wave(const LvMcmcArgs& a, hipStream_t s) {
    return launch_noise_mode<LvMcmcArgs>({lv_rwmh_wave_kernel<false, false>, lv_rwmh_wave_kernel<true, false>,
                                          lv_rwmh_wave_kernel<true, true>}, a, kWaveChainsPerBlock, kWaveThreads, s);
}

hipError_t launch_lv_rwmh(const LvMcmcArgs& a, hipStream_t s) {
    return launch_noise_mode<LvMcmcArgs>({lv_rwmh_kernel<false, false>, lv_rwmh_kernel<true, false>,
                                          lv_rwmh_kernel<true, true>}, a, kMcmcThreads, kMcmcThreads, s);
}

}  // namespace st
