// Many short chains in one launch (stein_thinning.thinning.thin_many / thin_gf_many): per-chain column
// statistics, per-chain 'med' distances and the greedy thin with ONE WORKGROUP PER CHAIN.
//
// A chain of a few hundred to a few thousand rows fits one workgroup's registers, so its thin needs no
// inter-block winner exchange, no bounded wait and no poll: a block loads its chain once (x / scl, g * scl
// applied on load, NumPy's bits), keeps the rows and their running sums in registers for all n_points steps,
// and a step is: winner row broadcast through LDS, one pair per row in the EXACT arithmetic
// (st::pair_value_ct / diag_value_ct: NumPy's evaluation order rounding for rounding, so no near-tie guard
// and no re-run), A += 2k, block-wide first-minimum argmin (per-thread scan in index order, the DPP wave
// reduction, one LDS hop over the waves).  Bit model: oracle/stein_ref.c sr_greedy(arith = exact) on each
// chain's standardised rows -- idx and the final running sums.
//
// Plan (greedy_many_plan): threads T and rows per thread R by n alone, row i of a chain lives in thread
// i % T, register slot i / T:   n <= 64: (64, 1)   n <= 256: (256, 1)   n <= 1024: (256, 4)
// n <= 4096: (1024, 4).  Rows i >= n are padding: never read from memory, never offered to the argmin.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/stein_thinning_hip.h"
#include "stein_internal.hpp"
#include "stein_math.hpp"

#pragma clang fp contract(off)

namespace st {
int report_error(int code, const char* msg);   // capi.hip: sets st_last_error()
}  // namespace st

namespace {

constexpr int64_t kManyMaxN = 4096;
constexpr int kStatsTileRows = 256;
constexpr int kStatsMaxDim = st::kMaxCtDim;
constexpr int kPdistManyBlock = 256;

// ---- st_chain_stats ----------------------------------------------------------------------------------
// One wave per chain.  A tile of kStatsTileRows rows is loaded into LDS by all 64 lanes (coalesced), then
// lane k < d adds column k's values in row order: NumPy's axis-0 reduction of an (n, d >= 2) array is that
// sequential sum, and np.mean divides it once by n.  Two passes (the sum, then the absolute deviations).
__global__ __launch_bounds__(64) void chain_stats_kernel(const double* __restrict__ x, const double* __restrict__ g,
                                                         int64_t n, int d, int standardize,
                                                         double* __restrict__ loc, double* __restrict__ scl,
                                                         int32_t* __restrict__ status) {
    __shared__ double tile[kStatsTileRows * kStatsMaxDim];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const double* xc = x + c * n * d;
    const double* gc = g + c * n * d;
    const int64_t total = n * d;
    // finiteness of g (any order: flags only)
    int nan = 0, inf = 0;
    for (int64_t e = lane; e < total; e += 64) {
        const double v = gc[e];
        nan |= (int)(v != v);
        inf |= (int)(__builtin_fabs(v) == INFINITY);
    }
    const double dn = (double)n;
    double acc = 0.0, mean = 0.0;
    for (int pass = 0; pass < (standardize ? 2 : 1); ++pass) {
        for (int64_t r0 = 0; r0 < n; r0 += kStatsTileRows) {
            const int rows = (int)(n - r0 < kStatsTileRows ? n - r0 : kStatsTileRows);
            __syncthreads();
            for (int e = lane; e < rows * d; e += 64) {
                const double v = xc[r0 * d + e];
                if (pass == 0) {
                    nan |= (int)(v != v);
                    inf |= (int)(__builtin_fabs(v) == INFINITY);
                }
                tile[e] = v;
            }
            __syncthreads();
            if (lane < d && standardize) {
                for (int r = 0; r < rows; ++r) {
                    const double v = tile[r * d + lane];
                    const double t = pass == 0 ? v : __builtin_fabs(v - mean);
                    acc = (r0 == 0 && r == 0) ? t : acc + t;
                }
            }
        }
        if (pass == 0) mean = acc / dn;
    }
    const double s = standardize ? acc / dn : 1.0;
    if (lane < d) {
        loc[c * d + lane] = standardize ? mean : 0.0;
        scl[c * d + lane] = s;
    }
    const int any_nan = __builtin_amdgcn_ballot_w64(nan != 0) != 0;
    const int any_inf = __builtin_amdgcn_ballot_w64(inf != 0) != 0;
    const int any_zero = __builtin_amdgcn_ballot_w64(lane < d && s == 0.0) != 0;
    if (lane == 0) status[c] = any_nan ? 1 : any_inf ? 2 : any_zero ? 3 : 0;
}

// ---- st_pdist_many -----------------------------------------------------------------------------------
// pdist_kernel (precon.hip) per chain on rows standardised on the fly: block (chain c, row i), threads over
// j > i; every coordinate is fl(x / scl) -- the IEEE division NumPy's x / scl does -- then the same
// differences, squares, left-to-right sum and correctly rounded square root.
__global__ __launch_bounds__(kPdistManyBlock) void pdist_many_kernel(const double* __restrict__ x,
                                                                     const double* __restrict__ scl,
                                                                     const int32_t* __restrict__ sub, int64_t n,
                                                                     int d, int64_t k, double* __restrict__ out) {
    __shared__ double u[st::kMaxDim], sc[st::kMaxDim];
    const int64_t c = blockIdx.x / (k - 1);
    const int64_t i = blockIdx.x % (k - 1);
    const double* xc = x + c * n * d;
    auto row_of = [&](int64_t r) -> int64_t {
        if (!sub) return r;
        const int64_t v = sub[r];
        return v < 0 ? 0 : (v >= n ? n - 1 : v);   // a bad entry reads a wrong row, never out of bounds
    };
    if ((int)threadIdx.x < d) {
        const double s = scl[c * d + threadIdx.x];
        sc[threadIdx.x] = s;
        u[threadIdx.x] = xc[row_of(i) * d + threadIdx.x] / s;
    }
    __syncthreads();
    const int64_t cnt = k * (k - 1) / 2;
    const int64_t base = i * k - i * (i + 1) / 2 - i - 1;   // + j: the condensed index of (i, j)
    double* oc = out + c * cnt;
    for (int64_t j = i + 1 + threadIdx.x; j < k; j += kPdistManyBlock) {
        const double* v = xc + row_of(j) * d;
        double s = 0.0;
        for (int q = 0; q < d; ++q) {
            const double t = u[q] - v[q] / sc[q];
            s = s + t * t;
        }
        oc[base + j] = __builtin_sqrt(s);
    }
}

// ---- st_greedy_many ----------------------------------------------------------------------------------
template <int D>
struct ManyShared {
    double wv[16];      // per-wave minimum of a step
    int64_t wi[16];     // and its row
    double x[D], g[D];  // the winner's row
    double w;           // and weight
};

template <int D, int T, int R, bool W>
__global__ __launch_bounds__(T) void greedy_many_kernel(const double* __restrict__ x, const double* __restrict__ g,
                                                        const double* __restrict__ scl,
                                                        const double* __restrict__ weights,
                                                        const double* __restrict__ linv_scale,
                                                        const double* __restrict__ linv_trace, int64_t n,
                                                        int64_t m, uint32_t* __restrict__ idx_out,
                                                        double* __restrict__ a_out) {
    __shared__ ManyShared<D> sm;
    constexpr int NW = T / 64;
    const int64_t c = blockIdx.x;
    const int tid = threadIdx.x;
    const double l = linv_scale[c], tr = linv_trace[c];
    const double l2 = l * l;
    double s[D];
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] = scl[c * D + k];
    double xr[R][D], gr[R][D], wr[R], A[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = (int64_t)r * T + tid;
        const bool valid = i < n;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xr[r][k] = valid ? x[(c * n + i) * D + k] / s[k] : 0.0;
            gr[r][k] = valid ? g[(c * n + i) * D + k] * s[k] : 0.0;
        }
        wr[r] = (W && valid) ? weights[c * n + i] : 0.0;
        double kd = st::diag_value_ct<D>(gr[r], tr);
        if (W) kd = (kd * wr[r]) * wr[r];
        A[r] = valid ? kd : INFINITY;
    }
    for (int64_t t = 0; t < m; ++t) {
        if (t > 0) {
            const double wj = sm.w;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double kv = st::pair_value_ct<D>(xr[r], gr[r], sm.x, sm.g, l, l2, tr);
                if (W) kv = (kv * wr[r]) * wj;
                A[r] = A[r] + 2.0 * kv;
            }
        }
        double bv = INFINITY;
        int64_t bi = INT64_MAX;
#pragma unroll
        for (int r = 0; r < R; ++r) {   // ascending rows: the first minimum of this thread's rows
            const int64_t i = (int64_t)r * T + tid;
            const bool take = i < n && st::better(A[r], i, bv, bi);
            bv = take ? A[r] : bv;
            bi = take ? i : bi;
        }
        st::wave_minloc(bv, bi);
        if (NW > 1) {
            if ((tid & 63) == 0) {
                sm.wv[tid >> 6] = bv;
                sm.wi[tid >> 6] = bi;
            }
            __syncthreads();
            bv = sm.wv[0];
            bi = sm.wi[0];
#pragma unroll
            for (int q = 1; q < NW; ++q) st::take_if_better(sm.wv[q], sm.wi[q], bv, bi);
        }
        if (tid == 0) idx_out[c * m + t] = (uint32_t)bi;
        if (t + 1 < m) {
            if (tid == (int)(bi % T)) {   // the winner's owner publishes its row
                const int rw = (int)(bi / T);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r == rw) {
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            sm.x[k] = xr[r][k];
                            sm.g[k] = gr[r][k];
                        }
                        sm.w = wr[r];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (a_out) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = (int64_t)r * T + tid;
            if (i < n) a_out[c * n + i] = A[r];
        }
    }
}

struct ManyPlan {
    int threads, rows;
};

bool greedy_many_plan(int64_t n, int d, ManyPlan& p) {
    if ((d != 2 && d != 4) || n < 1 || n > kManyMaxN) return false;
    if (n <= 64) p = {64, 1};
    else if (n <= 256) p = {256, 1};
    else if (n <= 1024) p = {256, 4};
    else p = {1024, 4};
    return true;
}

template <int D, int T, int R>
hipError_t launch_many(const double* x, const double* g, const double* scl, const double* w, const double* l,
                       const double* tr, int64_t chains, int64_t n, int64_t m, uint32_t* idx, double* a,
                       hipStream_t s) {
    if (w) greedy_many_kernel<D, T, R, true><<<(unsigned)chains, T, 0, s>>>(x, g, scl, w, l, tr, n, m, idx, a);
    else greedy_many_kernel<D, T, R, false><<<(unsigned)chains, T, 0, s>>>(x, g, scl, w, l, tr, n, m, idx, a);
    return hipGetLastError();
}

template <int D>
hipError_t launch_many_d(const ManyPlan& p, const double* x, const double* g, const double* scl, const double* w,
                         const double* l, const double* tr, int64_t chains, int64_t n, int64_t m, uint32_t* idx,
                         double* a, hipStream_t s) {
    if (p.threads == 64) return launch_many<D, 64, 1>(x, g, scl, w, l, tr, chains, n, m, idx, a, s);
    if (p.threads == 256 && p.rows == 1) return launch_many<D, 256, 1>(x, g, scl, w, l, tr, chains, n, m, idx, a, s);
    if (p.threads == 256) return launch_many<D, 256, 4>(x, g, scl, w, l, tr, chains, n, m, idx, a, s);
    return launch_many<D, 1024, 4>(x, g, scl, w, l, tr, chains, n, m, idx, a, s);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int fail(int code, const char* what, const char* msg) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, msg);
    return st::report_error(code, buf);
}

int hip_result(hipError_t e, const char* what) {
    return e == hipSuccess ? ST_OK : fail(ST_ERR_HIP, what, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int st_chain_stats(const double* x, const double* g, int64_t chains, int64_t n, int32_t d, int32_t standardize,
                   double* loc_out, double* scl_out, int32_t* status_out, void* stream) {
    const char* me = "st_chain_stats";
    if (!x || !g || !loc_out || !scl_out || !status_out) return fail(ST_ERR_INVALID, me, "NULL pointer");
    if (!aligned(x, 8) || !aligned(g, 8) || !aligned(loc_out, 8) || !aligned(scl_out, 8) || !aligned(status_out, 4))
        return fail(ST_ERR_INVALID, me, "arrays must be aligned (doubles: 8 bytes, status: 4)");
    if (chains < 1 || chains > 0x7FFFFFFFll) return fail(ST_ERR_INVALID, me, "chains must be in [1, 2^31)");
    if (n < 1) return fail(ST_ERR_INVALID, me, "n must be >= 1");
    if (d < 1) return fail(ST_ERR_INVALID, me, "d must be >= 1");
    if (d < 2 || d > kStatsMaxDim)   // d = 1: NumPy sums a contiguous column pairwise (st_standardize_host)
        return fail(ST_ERR_UNSUPPORTED, me, "d = 2 .. 8 only");
    if (n > (int64_t)1 << 40) return fail(ST_ERR_UNSUPPORTED, me, "n too large");
    chain_stats_kernel<<<(unsigned)chains, 64, 0, static_cast<hipStream_t>(stream)>>>(
        x, g, n, d, standardize ? 1 : 0, loc_out, scl_out, status_out);
    return hip_result(hipGetLastError(), "st_chain_stats launch");
}

int st_pdist_many(const double* x, const double* scl, const int32_t* sub_rows, int64_t chains, int64_t n, int32_t d,
                  int64_t k, double* out, void* stream) {
    const char* me = "st_pdist_many";
    if (!x || !scl || !out) return fail(ST_ERR_INVALID, me, "NULL pointer");
    if (!aligned(x, 8) || !aligned(scl, 8) || !aligned(out, 8) || !aligned(sub_rows, 4))
        return fail(ST_ERR_INVALID, me, "arrays must be aligned (doubles: 8 bytes, sub_rows: 4)");
    if (chains < 1) return fail(ST_ERR_INVALID, me, "chains must be >= 1");
    if (n < 1) return fail(ST_ERR_INVALID, me, "n must be >= 1");
    if (d < 1) return fail(ST_ERR_INVALID, me, "d must be >= 1");
    if (k < 2 || k > n || (!sub_rows && k != n))
        return fail(ST_ERR_INVALID, me, "need 2 <= k <= n sub-sample rows (k == n without sub_rows)");
    if (d > st::kMaxDim || k > 65535) return fail(ST_ERR_UNSUPPORTED, me, "d <= 128 and k <= 65535 only");
    if (chains > 0x7FFFFFFFll / (k - 1)) return fail(ST_ERR_UNSUPPORTED, me, "chains * (k - 1) must be below 2^31");
    pdist_many_kernel<<<(unsigned)(chains * (k - 1)), kPdistManyBlock, 0, static_cast<hipStream_t>(stream)>>>(
        x, scl, sub_rows, n, d, k, out);
    return hip_result(hipGetLastError(), "st_pdist_many launch");
}

int64_t st_greedy_many_max_n(int32_t d, int32_t has_weights) {
    (void)has_weights;
    return (d == 2 || d == 4) ? kManyMaxN : 0;
}

int st_greedy_many_plan(int64_t n, int32_t d, int32_t has_weights, int32_t* threads_out, int32_t* rows_out) {
    (void)has_weights;
    const char* me = "st_greedy_many_plan";
    if (!threads_out || !rows_out) return fail(ST_ERR_INVALID, me, "NULL pointer");
    if (n < 1) return fail(ST_ERR_INVALID, me, "n must be >= 1");
    if (d < 1) return fail(ST_ERR_INVALID, me, "d must be >= 1");
    ManyPlan p;
    if (!greedy_many_plan(n, d, p)) return fail(ST_ERR_UNSUPPORTED, me, "d in {2, 4} and n <= 4096 only");
    *threads_out = p.threads;
    *rows_out = p.rows;
    return ST_OK;
}

int st_greedy_many(const double* x, const double* g, const double* scl, const double* weights,
                   const double* linv_scale, const double* linv_trace, int64_t chains, int64_t n, int32_t d,
                   int64_t n_points, uint32_t* idx_out, double* a_out, void* stream) {
    const char* me = "st_greedy_many";
    if (!x || !g || !scl || !linv_scale || !linv_trace || !idx_out) return fail(ST_ERR_INVALID, me, "NULL pointer");
    if (!aligned(x, 8) || !aligned(g, 8) || !aligned(scl, 8) || !aligned(weights, 8) || !aligned(linv_scale, 8) ||
        !aligned(linv_trace, 8) || !aligned(a_out, 8) || !aligned(idx_out, 4))
        return fail(ST_ERR_INVALID, me, "arrays must be aligned (doubles: 8 bytes, idx_out: 4)");
    if (chains < 1 || chains > 0x7FFFFFFFll) return fail(ST_ERR_INVALID, me, "chains must be in [1, 2^31)");
    if (n < 1) return fail(ST_ERR_INVALID, me, "n must be >= 1");
    if (d < 1) return fail(ST_ERR_INVALID, me, "d must be >= 1");
    if (n_points < 1) return fail(ST_ERR_INVALID, me, "n_points must be >= 1");
    ManyPlan p;
    if (!greedy_many_plan(n, d, p)) return fail(ST_ERR_UNSUPPORTED, me, "d in {2, 4} and n <= 4096 only");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = d == 2
        ? launch_many_d<2>(p, x, g, scl, weights, linv_scale, linv_trace, chains, n, n_points, idx_out, a_out, s)
        : launch_many_d<4>(p, x, g, scl, weights, linv_scale, linv_trace, chains, n, n_points, idx_out, a_out, s);
    return hip_result(e, "st_greedy_many launch");
}

}  // extern "C"
