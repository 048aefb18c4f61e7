// Convergence diagnostics (stein_thinning.convergence): rank normalisation and the autocovariances behind
// the rank-normalised R-hat, the effective sample sizes and the Monte-Carlo standard errors (DESIGN.md
// section 20).
//
// st_rank_normalize: one thread per sorted value.  The tie run of a value is found by two binary searches
// in the sorted column (a constant column costs log N per value, not N), its average rank r = (lo + hi + 1) / 2
// is a half-integer and exact, p = (r - 0.375) / (N + 0.25) is one exact subtraction and one IEEE division,
// z = PPND16(p) (Wichura 1988, AS241), scattered to the value's original position.
//
// st_autocov: biased, centred autocovariances of G * S contiguous series of length h for lags [lag0, lag1),
// two plans, no atomics, every sum in an order fixed by the plan alone (not by the device):
//   long  -- series_moments_kernel (a block per series: two-pass mean, lag-0 value), then autocov_long_kernel:
//            a block is (series, tile of 256 lags, split of the i range).  Per chunk of 2048 i it stages the
//            centred x window (2048 values) and the y window (2304 values, starting at the tile's first lag)
//            in LDS, zero past the series' end, so the inner loop has no bounds test.  Thread (lt, sl) owns 8
//            consecutive lags and slice sl of 256 i; it keeps y[i + t .. i + t + 7] in registers and slides
//            them: per i one broadcast read of x and one read of y feed 8 FMAs.  The y image carries two pad
//            doubles per 8, so the lag threads read 16-byte pairs (ds_read_b128) at a stride of 10 doubles: the
//            16 lanes of each ds_read_b128 group fall on 16 different 16-byte slots of the 64 banks.  Chunk sums
//            are added to the thread's running sums, the 8 slices in slice order through LDS, the splits in
//            split order by the finishing kernel.
//   short -- autocov_short_kernel: a wave per series, the whole centred series in LDS (h <= 2048), lane l
//            takes lags lag0 + l + 64 j, four at a time sharing the x read.
// autocov_finish_kernel / autocov_mean_kernel then divide by h and average the series of a group in slabs of
// 256 series, each slab and the slabs themselves in index order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stein_thinning_hip.h"
#include "stein_internal.hpp"

#pragma clang fp contract(off)

namespace {

// ---- st_rank_normalize ----------------------------------------------------------------------------------
// AS241 PPND16; p in (0, 1).  Evaluated as written there (Horner, no contraction).
__device__ double ppnd16(double p) {
    const double q = p - 0.5;
    if (__builtin_fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r
                                + 45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r
                             + 133.14166789178437745) * r + 3.387132872796366608);
        const double den = (((((((r * 5226.495278852545925 + 28729.085735721942674) * r + 39307.89580009271061) * r
                                + 21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r
                             + 42.313330701600911252) * r + 1.0);
        return q * num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double val;
    if (r <= 5.0) {
        r = r - 1.6;
        const double num = (((((((r * 7.7454501427834140764e-4 + .0227238449892691845833) * r + .24178072517745061177) * r
                                + 1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r
                             + 4.6303378461565452959) * r + 1.42343711074968357734);
        const double den = (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r
                                 + .0151986665636164571966) * r + .14810397642748007459) * r + .68976733498510000455) * r
                              + 1.6763848301838038494) * r + 2.05319162663775882187) * r + 1.0);
        val = num / den;
    } else {
        r = r - 5.0;
        const double num = (((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r
                                 + .0012426609473880784386) * r + .026532189526576123093) * r + .29656057182850489123) * r
                              + 1.7848265399172913358) * r + 5.4637849111641143699) * r + 6.6579046435011037772);
        const double den = (((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r
                                 + 1.8463183175100546818e-5) * r + 7.868691311456132591e-4) * r
                               + .0148753612908506148525) * r + .13692988092273580531) * r + .59983220655588793769) * r
                            + 1.0);
        val = num / den;
    }
    return q < 0.0 ? -val : val;
}

__global__ __launch_bounds__(256) void rank_normalize_kernel(const double* __restrict__ sorted,
                                                             const int64_t* __restrict__ perm, int64_t vars,
                                                             int64_t N, double* __restrict__ p_out,
                                                             double* __restrict__ z_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= vars * N) return;
    const int64_t k = e / N, j = e - k * N;
    const double* col = sorted + k * N;
    const double v = col[j];
    int64_t dst = perm[e];
    if (dst < 0 || dst >= N) return;   // a bad permutation writes nothing, never out of bounds
    dst += k * N;
    if (v != v) {
        if (p_out) p_out[dst] = NAN;
        z_out[dst] = NAN;
        return;
    }
    // lo: first index with col[] >= v, in [0, j]; hi: first index with col[] > v, in (j, N] (NaN sorts last)
    int64_t a = 0, b = j;
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if (col[m] < v) a = m + 1; else b = m;
    }
    const int64_t lo = a;
    a = j + 1, b = N;
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if (col[m] <= v) a = m + 1; else b = m;
    }
    const int64_t hi = a;
    const double r = (double)(lo + hi + 1) * 0.5;         // mean of the 1-based ranks lo + 1 .. hi: exact
    const double p = (r - 0.375) / ((double)N + 0.25);
    if (p_out) p_out[dst] = p;
    z_out[dst] = ppnd16(p);
}

// ---- st_autocov -----------------------------------------------------------------------------------------
constexpr int kR = 8;              // consecutive lags per thread
constexpr int kLagThreads = 32;    // lag threads per block: a half-wave
constexpr int kSlices = 8;         // i slices per block
constexpr int kM = 256;            // i per slice and chunk
constexpr int kTile = kR * kLagThreads;        // 256 lags per block
constexpr int kChunk = kSlices * kM;           // 2048 i per chunk
constexpr int kYLen = kChunk + kTile;          // y window
constexpr int kYPad = kYLen + 2 * (kYLen / kR);      // two pad doubles per kR: 16-byte groups stay aligned
constexpr int kLongBlock = kLagThreads * kSlices;
constexpr int kMaxSplit = 64;
constexpr int64_t kTargetBlocks = 2048;
constexpr int kShortMaxH = 2048;
constexpr int kShortLags = 4;      // lags a lane carries at once in the short plan
constexpr int kSlab = 256;         // series per slab of the mean over a group's series
constexpr int kMomBlock = 256;

static_assert(kLongBlock == 256 && kTile == kLongBlock, "the slice reduction maps one thread to one lag of the tile");
static_assert(kM % kR == 0 && kChunk % kR == 0, "the padded index is linear inside a group of kR");

struct Plan {
    int kind;          // 1 long, 2 short
    int64_t tiles;     // lag tiles (long)
    int64_t chunks;    // i chunks of the series (long)
    int64_t split;     // i splits (long); 1 (short)
    int64_t slabs;     // slabs of series per group
};

Plan make_plan(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want) {
    Plan p;
    // by the group's own shape, never by the number of groups: a variable's bits do not depend on its neighbours
    p.kind = want ? want : ((h <= kShortMaxH && S >= 64) ? 2 : 1);
    const int64_t L = lag1 - lag0;
    p.tiles = (L + kTile - 1) / kTile;
    p.chunks = (h + kChunk - 1) / kChunk;
    p.split = 1;
    if (p.kind == 1) {
        const int64_t blocks = S * p.tiles;
        int64_t sp = (kTargetBlocks + blocks - 1) / blocks;
        if (sp > kMaxSplit) sp = kMaxSplit;
        if (sp > p.chunks) sp = p.chunks;
        p.split = sp < 1 ? 1 : sp;
    }
    p.slabs = (S + kSlab - 1) / kSlab;
    return p;
}

// sum of one value per thread, T threads (a power of two), in the order of a binary tree over the thread
// index: the same bits on every call
template <int T>
__device__ double block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = T / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// mean of a series in two passes (m0, then m0 + mean(a - m0)) and the centred lag-0 value sum((a - mu)^2) / h;
// thread j adds elements j, j + T, ... in order
template <int T>
__device__ void series_moments(const double* __restrict__ a, int64_t h, double* red, double& mu, double& v0) {
    const double dh = (double)h;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < h; i += T) acc = acc + a[i];
    const double m0 = block_sum<T>(acc, red) / dh;
    acc = 0.0;
    for (int64_t i = threadIdx.x; i < h; i += T) acc = acc + (a[i] - m0);
    mu = m0 + block_sum<T>(acc, red) / dh;
    acc = 0.0;
    for (int64_t i = threadIdx.x; i < h; i += T) {
        const double c = a[i] - mu;
        acc = __builtin_fma(c, c, acc);
    }
    v0 = block_sum<T>(acc, red) / dh;
}

__global__ __launch_bounds__(kMomBlock) void series_moments_kernel(const double* __restrict__ series, int64_t h,
                                                                   double* __restrict__ mean_out,
                                                                   double* __restrict__ var0_out) {
    __shared__ double red[kMomBlock];
    const int64_t gs = blockIdx.x;
    double mu, v0;
    series_moments<kMomBlock>(series + gs * h, h, red, mu, v0);
    if (threadIdx.x == 0) {
        mean_out[gs] = mu;
        var0_out[gs] = v0;
    }
}

// block = (series gs, lag tile, split); partial[(gs * split_n + split) * L + (lag - lag0)] = this split's sum
__global__ __launch_bounds__(kLongBlock) void autocov_long_kernel(const double* __restrict__ series,
                                                                  const double* __restrict__ mean, int64_t h,
                                                                  int64_t lag0, int64_t lag1, int64_t tiles,
                                                                  int64_t chunks, int64_t split_n,
                                                                  double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double X[kChunk];
    __shared__ __attribute__((aligned(16))) double Y[kYPad];
    const int64_t b = blockIdx.x;
    const int64_t tile = b % tiles;
    const int64_t split = (b / tiles) % split_n;
    const int64_t gs = b / (tiles * split_n);
    const double* a = series + gs * h;
    const double mu = mean[gs];
    const int64_t T0 = lag0 + tile * kTile;
    const int tid = threadIdx.x;
    const int lt = tid & (kLagThreads - 1);
    const int sl = tid / kLagThreads;
    const int base = sl * kM + lt * kR;      // first y element of this thread's window, a multiple of kR
    double tot[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) tot[r] = 0.0;
    // chunks ck = split, split + split_n, ... ; a chunk whose first pair (i0, i0 + T0) is past the end adds zeros
    for (int64_t ck = split; ck < chunks; ck += split_n) {
        const int64_t i0 = ck * kChunk;
        if (i0 + T0 >= h) break;
        __syncthreads();
        for (int e = tid; e < kChunk; e += kLongBlock) {
            const int64_t gi = i0 + e;
            X[e] = gi < h ? a[gi] - mu : 0.0;
        }
        for (int e = tid; e < kYLen; e += kLongBlock) {
            const int64_t gi = i0 + T0 + e;
            Y[e + 2 * (e / kR)] = gi < h ? a[gi] - mu : 0.0;
        }
        __syncthreads();
        double acc[kR], w[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            acc[r] = 0.0;
            w[r] = Y[base + 2 * (base / kR) + r];
        }
        for (int j0 = 0; j0 < kM; j0 += kR) {
            const int q = base + j0;
            const int pq = q + 2 * (q / kR) + kR + 2;      // padded index of y element q + kR
#pragma unroll
            for (int u = 0; u < kR; ++u) {
                const double x = X[sl * kM + j0 + u];
                // w[(u + r) % kR] holds y[q + u + r]
#pragma unroll
                for (int r = 0; r < kR; ++r) acc[r] = __builtin_fma(x, w[(u + r) % kR], acc[r]);
                w[u] = Y[pq + u];                    // y[q + u + kR] replaces y[q + u]
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) tot[r] = tot[r] + acc[r];
    }
    // the 8 slices of a lag, in slice order (X is free again: kSlices * kTile == kChunk doubles)
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kR; ++r) X[sl * kTile + lt * kR + r] = tot[r];
    __syncthreads();
    const int64_t lag = T0 + tid;
    if (lag < lag1) {
        double s = X[tid];
#pragma unroll
        for (int k = 1; k < kSlices; ++k) s = s + X[k * kTile + tid];
        partial[(gs * split_n + split) * (lag1 - lag0) + (lag - lag0)] = s;
    }
}

// a wave per series; partial[gs * L + (lag - lag0)] = the series' sum for that lag
__global__ __launch_bounds__(64) void autocov_short_kernel(const double* __restrict__ series, int64_t h, int64_t lag0,
                                                           int64_t lag1, double* __restrict__ mean_out,
                                                           double* __restrict__ var0_out,
                                                           double* __restrict__ partial) {
    __shared__ double c[kShortMaxH + 64 * kShortLags];   // zero past h: a lane's lags need no bounds test
    __shared__ double red[64];
    const int64_t gs = blockIdx.x;
    const double* a = series + gs * h;
    const int lane = threadIdx.x;
    const int n = (int)h;
    double mu, v0;
    series_moments<64>(a, h, red, mu, v0);
    if (lane == 0) {
        mean_out[gs] = mu;
        var0_out[gs] = v0;
    }
    for (int e = lane; e < kShortMaxH + 64 * kShortLags; e += 64) c[e] = e < n ? a[e] - mu : 0.0;
    __syncthreads();
    const int64_t L = lag1 - lag0;
    for (int64_t t0 = lag0; t0 < lag1; t0 += 64 * kShortLags) {
        // lags t0 + lane + 64 r; a lag >= h has no pair
        int t[kShortLags];
        double acc[kShortLags];
        int tmin = n;
#pragma unroll
        for (int r = 0; r < kShortLags; ++r) {
            const int64_t lag = t0 + lane + 64 * r;
            t[r] = lag < (int64_t)n ? (int)lag : n;
            acc[r] = 0.0;
            tmin = t[r] < tmin ? t[r] : tmin;
        }
        // every lane runs i < h - (the wave's smallest lag); the zeros past h make the surplus pairs 0
        const int first = (int)(t0 < (int64_t)n ? t0 : (int64_t)n);
        for (int i = 0; i < n - first; ++i) {
            const double x = c[i];
#pragma unroll
            for (int r = 0; r < kShortLags; ++r) {
                const int e = i + t[r];
                acc[r] = __builtin_fma(x, c[e < kShortMaxH + 64 * kShortLags ? e : kShortMaxH + 64 * kShortLags - 1],
                                       acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kShortLags; ++r) {
            const int64_t lag = t0 + lane + 64 * r;
            if (lag < lag1) partial[gs * L + (lag - lag0)] = acc[r];
        }
    }
}

// thread = (group g, slab, lag): acov of the slab's series (split sums in split order, / h), optionally
// written per series, and their sum in series order
__global__ __launch_bounds__(256) void autocov_finish_kernel(const double* __restrict__ partial, int64_t S, int64_t h,
                                                             int64_t L, int64_t split_n, int64_t slabs,
                                                             double* __restrict__ acov_series,
                                                             double* __restrict__ slab_sum) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slab = blockIdx.y;
    const int64_t g = blockIdx.z;
    if (l >= L) return;
    const double dh = (double)h;
    const int64_t s1 = (slab + 1) * kSlab < S ? (slab + 1) * kSlab : S;
    double sum = 0.0;
    for (int64_t s = slab * kSlab; s < s1; ++s) {
        const int64_t gs = g * S + s;
        double v = partial[gs * split_n * L + l];
        for (int64_t k = 1; k < split_n; ++k) v = v + partial[(gs * split_n + k) * L + l];
        v = v / dh;
        if (acov_series) acov_series[gs * L + l] = v;
        sum = sum + v;
    }
    slab_sum[(g * slabs + slab) * L + l] = sum;
}

__global__ __launch_bounds__(256) void autocov_mean_kernel(const double* __restrict__ slab_sum, int64_t S, int64_t L,
                                                           int64_t slabs, double* __restrict__ acov_mean) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t g = blockIdx.y;
    if (l >= L) return;
    double sum = slab_sum[g * slabs * L + l];
    for (int64_t k = 1; k < slabs; ++k) sum = sum + slab_sum[(g * slabs + k) * L + l];
    acov_mean[g * L + l] = sum / (double)S;
}

}  // namespace

namespace st {

hipError_t launch_rank_normalize(const RankArgs& a, hipStream_t s) {
    const int64_t total = a.vars * a.N;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rank_normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.sorted, a.perm, a.vars, a.N,
                       a.p_out, a.z_out);
    return hipGetLastError();
}

int autocov_plan(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want) {
    return make_plan(G, S, h, lag0, lag1, want).kind;
}

bool autocov_short_ok(int64_t h) { return h <= kShortMaxH; }

int64_t autocov_ws_bytes(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want) {
    const Plan p = make_plan(G, S, h, lag0, lag1, want);
    const int64_t L = lag1 - lag0;
    return (G * S * p.split * L + G * p.slabs * L) * 8;
}

bool autocov_grid_ok(int64_t G, int64_t S, int64_t h, int64_t lag0, int64_t lag1, int want) {
    const Plan p = make_plan(G, S, h, lag0, lag1, want);
    return G * S * p.tiles * p.split <= 0x7FFFFFFFll && p.slabs <= 65535 && G <= 65535;
}

hipError_t launch_autocov(const AutocovArgs& a, hipStream_t s) {
    const Plan p = make_plan(a.G, a.S, a.h, a.lag0, a.lag1, a.plan);
    const int64_t L = a.lag1 - a.lag0;
    const int64_t GS = a.G * a.S;
    double* partial = a.ws;
    double* slab_sum = a.ws + GS * p.split * L;
    if (p.kind == 1) {
        hipLaunchKernelGGL(series_moments_kernel, dim3((unsigned)GS), dim3(kMomBlock), 0, s, a.series, a.h,
                           a.series_mean, a.series_var0);
        hipLaunchKernelGGL(autocov_long_kernel, dim3((unsigned)(GS * p.tiles * p.split)), dim3(kLongBlock), 0, s,
                           a.series, a.series_mean, a.h, a.lag0, a.lag1, p.tiles, p.chunks, p.split, partial);
    } else {
        hipLaunchKernelGGL(autocov_short_kernel, dim3((unsigned)GS), dim3(64), 0, s, a.series, a.h, a.lag0, a.lag1,
                           a.series_mean, a.series_var0, partial);
    }
    hipLaunchKernelGGL(autocov_finish_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)p.slabs, (unsigned)a.G),
                       dim3(256), 0, s, partial, a.S, a.h, L, p.split, p.slabs, a.acov_series, slab_sum);
    hipLaunchKernelGGL(autocov_mean_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)a.G), dim3(256), 0, s,
                       slab_sum, a.S, L, p.slabs, a.acov_mean);
    return hipGetLastError();
}

}  // namespace st
