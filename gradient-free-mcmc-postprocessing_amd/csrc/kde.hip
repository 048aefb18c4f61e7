// KDE proxy for the gradient-free operator: log q and grad log q of a Gaussian kernel density
// estimate at every query point -- what the reference's Gaussian-mixture study feeds thin_gf
// (Gaussian_mixture.ipynb cells 42-48: jax.scipy.stats.gaussian_kde(sample.T, bw_method='silverman'),
// log q = kde.logpdf, grad log q = jax.grad of it; cell 51 the weighted KDE).  With the whitening
// factor L (Cholesky of the KDE precision, lower) and whitened data p_i = x_i L, queries q_j = y_j L:
//   a_ij  = log w_i + log_norm - 0.5 |p_i - q_j|^2
//   log q_j = logsumexp_i a_ij
//   grad_j  = (sum_i s_ij p_i - q_j) L^T,   s_ij = exp(a_ij - log q_j)      (the autodiff of log q)
// Two sweeps over the data per query tile: the row maximum of a_ij, then the shifted exponential
// sums (one exp per pair).  One query per thread; data points staged 256 at a time in LDS and read
// as block-uniform broadcasts (as the energy-distance kernel K7).  Sums are sequential in i
// (scipy's logsumexp sums pairwise: fp64 tolerance).
// Below them the Student-t kernel density (kde_t_kernel / kde_t_rt_kernel: st_kde_t_logpdf_grad).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "stein_internal.hpp"
#include "stein_math.hpp"

namespace st {
namespace {

constexpr int kKdeBlock = 256;

struct KdeArgs {
    const double* p;      // whitened data, SoA (d, ldp)
    int64_t ldp, n;
    const double* logw;   // (n) log weights, or nullptr: logw0 for every point
    double logw0;
    const double* q;      // whitened queries, SoA (d, ldq)
    int64_t ldq, m;
    double log_norm;
    const double* L;      // (d, d) row-major whitening factor (grad = v L^T)
    double* log_q;        // (m)
    double* grad;         // (m, d) row-major
};

template <int D>
__global__ __launch_bounds__(kKdeBlock) void kde_kernel(KdeArgs a) {
    constexpr int R = kKdeBlock;
    __shared__ double sp[D][R];
    __shared__ double sw[R];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * R + tid;
    const bool live = j < a.m;
    double qj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) qj[k] = live ? a.q[k * a.ldq + j] : 0.0;
    auto stage = [&](int64_t i0) -> int {
        __syncthreads();
        const int64_t i = i0 + tid;
        if (i < a.n) {
#pragma unroll
            for (int k = 0; k < D; ++k) sp[k][tid] = a.p[k * a.ldp + i];
            sw[tid] = a.logw ? a.logw[i] : a.logw0;
        }
        __syncthreads();
        return (int)((a.n - i0) < R ? (a.n - i0) : R);
    };
    auto arg = [&](int e) {
        double ss = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double dk = sp[k][e] - qj[k];
            ss += dk * dk;
        }
        return sw[e] + (a.log_norm - 0.5 * ss);
    };
    double mx = -INFINITY;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        const int cnt = stage(i0);
        for (int e = 0; e < cnt; ++e) mx = fmax(mx, arg(e));
    }
    const double shift = mx == -INFINITY ? 0.0 : mx;   // all weights zero: log q = -inf
    double s = 0.0, sm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) sm[k] = 0.0;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        const int cnt = stage(i0);
        for (int e = 0; e < cnt; ++e) {
            const double t = exp(arg(e) - shift);
            s += t;
#pragma unroll
            for (int k = 0; k < D; ++k) sm[k] = fma(t, sp[k][e], sm[k]);
        }
    }
    if (!live) return;
    a.log_q[j] = log(s) + shift;
    double v[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = sm[k] / s - qj[k];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double gk = 0.0;
#pragma unroll
        for (int l = 0; l < D; ++l) gk = fma(v[l], a.L[k * D + l], gk);
        a.grad[j * D + k] = gk;
    }
}

// runtime d (9 .. kMaxDim): coordinates of the query re-read from L1/L2, data staged 32 at a time
constexpr int kKdeRowsRt = 32;

__global__ __launch_bounds__(kKdeBlock) void kde_rt_kernel(KdeArgs a, int d, double* scratch) {
    constexpr int R = kKdeRowsRt;
    __shared__ double sp[kMaxDim][R];
    __shared__ double sw[R];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kKdeBlock + tid;
    const bool live = j < a.m;
    const int64_t jc = live ? j : 0;
    double* smj = scratch + jc * d;   // (m, d) per-query weighted sums
    auto stage = [&](int64_t i0) -> int {
        const int cnt = (int)((a.n - i0) < R ? (a.n - i0) : R);
        __syncthreads();
        for (int e = tid; e < d * R; e += kKdeBlock) {
            const int k = e / R, r = e % R;
            if (r < cnt) sp[k][r] = a.p[(int64_t)k * a.ldp + i0 + r];
        }
        if (tid < cnt) sw[tid] = a.logw ? a.logw[i0 + tid] : a.logw0;
        __syncthreads();
        return cnt;
    };
    auto arg = [&](int e) {
        double ss = 0.0;
        for (int k = 0; k < d; ++k) {
            const double dk = sp[k][e] - a.q[(int64_t)k * a.ldq + jc];
            ss += dk * dk;
        }
        return sw[e] + (a.log_norm - 0.5 * ss);
    };
    double mx = -INFINITY;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        const int cnt = stage(i0);
        for (int e = 0; e < cnt; ++e) mx = fmax(mx, arg(e));
    }
    const double shift = mx == -INFINITY ? 0.0 : mx;
    if (live)
        for (int k = 0; k < d; ++k) smj[k] = 0.0;
    double s = 0.0;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        const int cnt = stage(i0);
        for (int e = 0; e < cnt; ++e) {
            const double t = exp(arg(e) - shift);
            s += t;
            if (live)
                for (int k = 0; k < d; ++k) smj[k] = fma(t, sp[k][e], smj[k]);
        }
    }
    if (!live) return;
    a.log_q[j] = log(s) + shift;
    for (int k = 0; k < d; ++k) smj[k] = smj[k] / s - a.q[(int64_t)k * a.ldq + j];
    for (int k = 0; k < d; ++k) {
        double gk = 0.0;
        for (int l = 0; l < d; ++l) gk = fma(smj[l], a.L[k * d + l], gk);
        a.grad[j * d + k] = gk;
    }
}

// ---------------------------------------------------------------------------------------------------
// Student-t kernel density proxy (st_kde_t_logpdf_grad): the same mixture with the fat-tailed kernel
// multivariate_t(y; loc = x_i, shape = KDE covariance, df = nu) in place of the Gaussian one.  With
// h = (nu + d) / 2, r2_ij = |p_i - q_j|^2, u_ij = 1 + r2_ij / nu:
//   a_ij    = log w_i + log_norm_t - h log(u_ij)
//   log q_j = logsumexp_i a_ij
//   grad_j  = [sum_i s_ij (nu + d) / (nu + r2_ij) (p_i - q_j)] L^T,   s_ij = exp(a_ij - log q_j)
// Shift (per query; nothing underflows where the true value is finite): the smallest r2 over the points of
// non-zero weight, r2min_j, and the largest log weight lwmax.  Every pair then contributes
//   t_ij = exp(log w_i - lwmax) rho_ij^h,   rho_ij = (nu + r2min_j) / (nu + r2_ij) <= 1
// (both factors <= 1; the nearest point of non-zero weight has rho = 1).  rho is clamped to 1: rounding can leave
// the nearest point an ulp above it, and a point of zero weight -- moved to the origin, below -- or a padding
// row of the runtime-d kernel can lie closer to the query than every weighted point, where rho^h may overflow
// and 0 * inf would poison the sums.  Then
//   log q_j = log(sum_i t_ij) + lwmax + log_norm_t - h log1p(r2min_j / nu).
// The first sweep needs no transcendental (d subtractions, d fma, one add, one min per pair).  Domain: the
// shift is not the row maximum of a_ij, so a point can matter whose t_ij is as small as (its weight / the
// largest weight); every term that matters stays a normal number when the non-zero weights span a ratio of
// at most 2^900 (and nu + r2 is a normal number).  A weight of exactly zero (log weight -inf) drops out
// exactly: its coordinates are replaced by 0 at staging (they may be NaN), it is kept out of the minimum by
// an additive +inf, and its t is exactly 0.  All weights zero: log q = -inf (the gradient is not pinned).
// Power rho^h: when nu + d is an integer <= 256 a square-and-multiply chain on the block-uniform exponent
// floor(h), times sqrt(rho) for odd nu + d -- no exp / log per pair; otherwise exp(h log(rho)).
// One reciprocal 1 / (nu + r2_ij) per pair (v_rcp_f64 and two Newton steps: recip2) serves rho and the
// gradient coefficient.  Sums sequential in i; staging as the Gaussian kernels above.
struct KdeTArgs {
    KdeArgs k;
    double nu, h;     // df, (df + d) / 2
    int half;         // chain paths: floor(h) >= 1
    int const_half;   // d <= 8 chain kernels: 1 = the sweep compiled for this floor(h) when it is <= 8
};

// the power paths: exp(h log rho); the chain for even nu + d; the chain times sqrt(rho) for odd nu + d
constexpr int kPowGeneral = 0, kPowEven = 1, kPowOdd = 2;

// rho^h.  Chain: rho^half by squaring past the exponent's trailing zero bits, then square-and-multiply over
// the rest.  HALF > 0: the exponent at compile time (the loops unroll: nu + d = 8 is two multiplications);
// HALF = 0: the block-uniform runtime exponent `half` (scalar loop control).
template <int POW, int HALF>
__device__ __forceinline__ double kde_t_power(double rho, double h, int half) {
    if constexpr (POW == kPowGeneral) {
        return exp(h * log(rho));
    } else {
        double b = rho;
        int e = HALF > 0 ? HALF : half;
        for (; !(e & 1); e >>= 1) b *= b;
        double pw = POW == kPowOdd ? __builtin_sqrt(rho) * b : b;
        for (e >>= 1; e; e >>= 1) {
            b *= b;
            if (e & 1) pw *= b;
        }
        return pw;
    }
}

// largest of the per-thread values over the block, through the (>= cnt)-entry LDS buffer `buf`
__device__ __forceinline__ double kde_block_max(double mine, double* buf, int cnt, int tid) {
    __syncthreads();
    if (tid < cnt) buf[tid] = mine;
    __syncthreads();
    double mx = -INFINITY;
    for (int e = 0; e < cnt; ++e) mx = fmax(mx, buf[e]);
    return mx;
}

template <int D, int POW>
__global__ __launch_bounds__(kKdeBlock) void kde_t_kernel(KdeTArgs ta) {
    constexpr int R = kKdeBlock;
    const KdeArgs& a = ta.k;
    __shared__ double sp[D][R];
    __shared__ double sw[R];   // sweep 1: 0, or +inf for a zero weight; sweep 2: exp(log w - lwmax)
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * R + tid;
    const bool live = j < a.m;
    double qj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) qj[k] = live ? a.q[k * a.ldq + j] : 0.0;
    double lwmine = -INFINITY, lwshift = 0.0;
    auto stage = [&](int64_t i0, bool second) -> int {
        __syncthreads();
        const int64_t i = i0 + tid;
        if (i < a.n) {
            const double lw = a.logw ? a.logw[i] : a.logw0;
            const bool zero = lw == -INFINITY;
#pragma unroll
            for (int k = 0; k < D; ++k) sp[k][tid] = zero ? 0.0 : a.p[k * a.ldp + i];
            if (second) {
                sw[tid] = zero ? 0.0 : exp(lw - lwshift);
            } else {
                sw[tid] = zero ? INFINITY : 0.0;
                lwmine = fmax(lwmine, lw);
            }
        }
        __syncthreads();
        return (int)((a.n - i0) < R ? (a.n - i0) : R);
    };
    double r2min = INFINITY;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        const int cnt = stage(i0, false);
        for (int e = 0; e < cnt; ++e) {
            double ss = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double dk = sp[k][e] - qj[k];
                ss = fma(dk, dk, ss);
            }
            r2min = fmin(r2min, ss + sw[e]);
        }
    }
    const double lwmax = kde_block_max(lwmine, sw, R, tid);
    lwshift = lwmax == -INFINITY ? 0.0 : lwmax;      // all weights zero: every t is 0, log q = -inf
    if (r2min == INFINITY) r2min = 0.0;
    const double dmin = ta.nu + r2min;
    double s = 0.0, sm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) sm[k] = 0.0;
    auto sweep2 = [&](auto hc) {
        constexpr int HALF = decltype(hc)::value;
        for (int64_t i0 = 0; i0 < a.n; i0 += R) {
            const int cnt = stage(i0, true);
            for (int e = 0; e < cnt; ++e) {
                double ss = 0.0, dk[D];
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    dk[k] = sp[k][e] - qj[k];
                    ss = fma(dk[k], dk[k], ss);
                }
                const double den = ta.nu + ss;
                const double rinv = recip2(den, __builtin_amdgcn_rcp(den));
                const double t = sw[e] * kde_t_power<POW, HALF>(fmin(dmin * rinv, 1.0), ta.h, ta.half);
                s += t;
                const double tc = t * rinv;
#pragma unroll
                for (int k = 0; k < D; ++k) sm[k] = fma(tc, dk[k], sm[k]);
            }
        }
    };
    if constexpr (POW == kPowGeneral) {
        sweep2(std::integral_constant<int, 0>{});
    } else {
        // block-uniform; floor(h) <= 8 (nu + d <= 17) gets its own copy of the sweep (const_half: st_tune key 24)
        switch (ta.const_half ? ta.half : 0) {
            case 1: sweep2(std::integral_constant<int, 1>{}); break;
            case 2: sweep2(std::integral_constant<int, 2>{}); break;
            case 3: sweep2(std::integral_constant<int, 3>{}); break;
            case 4: sweep2(std::integral_constant<int, 4>{}); break;
            case 5: sweep2(std::integral_constant<int, 5>{}); break;
            case 6: sweep2(std::integral_constant<int, 6>{}); break;
            case 7: sweep2(std::integral_constant<int, 7>{}); break;
            case 8: sweep2(std::integral_constant<int, 8>{}); break;
            default: sweep2(std::integral_constant<int, 0>{}); break;
        }
    }
    if (!live) return;
    a.log_q[j] = log(s) + (lwshift + (a.log_norm - ta.h * log1p(r2min / ta.nu)));
    const double c = (2.0 * ta.h) / s;
    double v[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = c * sm[k];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double gk = 0.0;
#pragma unroll
        for (int l = 0; l < D; ++l) gk = fma(v[l], a.L[k * D + l], gk);
        a.grad[j * D + k] = gk;
    }
}

// runtime d (9 .. kMaxDim): data staged 32 at a time as in kde_rt_kernel, but the pair loop is turned inside
// out.  The squared distances of 8 pairs (a quarter tile) live in registers and the coordinates go by in chunks
// of 8: a chunk of the query is loaded once per quarter tile (kde_rt_kernel re-reads every coordinate for every pair), and the d
// weighted sums per query -- in the workspace, laid out (d, m) so that a wave's accesses to one coordinate
// are contiguous -- are read and written once per quarter tile and chunk, not once per pair.  The tile is padded with
// exact zeros (coordinates d .. the next multiple of 8, rows past n: weight 0, +inf in the first sweep), so
// every loop over the tile has a compile-time trip count; the sums see the same terms in the same order (k
// ascending within a pair, i ascending within a sum).
constexpr int kKdeTChunk = 8;      // coordinates per register chunk
constexpr int kKdeTRegTile = 8;    // pairs per register tile (four per staged tile)
static_assert(kMaxDim % kKdeTChunk == 0, "the padded width must fit sp");
static_assert(kKdeRowsRt % kKdeTRegTile == 0, "register tiles must cover the staged tile");

template <int POW>
__global__ __launch_bounds__(kKdeBlock, 2) void kde_t_rt_kernel(KdeTArgs ta, int d, double* scratch) {
    constexpr int R = kKdeRowsRt;
    constexpr int C = kKdeTChunk;
    constexpr int T = kKdeTRegTile;
    const KdeArgs& a = ta.k;
    __shared__ double sp[kMaxDim][R];
    __shared__ double sw[R];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kKdeBlock + tid;
    const bool live = j < a.m;
    const int64_t jc = live ? j : 0;
    const int dpad = (d + C - 1) / C * C;
    double* smj = scratch + jc;       // (d, m): coordinate k at smj[k * m]; touched by live threads only
    double lwmine = -INFINITY, lwshift = 0.0;
    auto stage = [&](int64_t i0, bool second) {
        const int cnt = (int)((a.n - i0) < R ? (a.n - i0) : R);
        __syncthreads();
        for (int e = tid; e < dpad * R; e += kKdeBlock) {
            const int k = e / R, r = e % R;
            double v = 0.0;
            if (k < d && r < cnt) {
                const double lw = a.logw ? a.logw[i0 + r] : a.logw0;
                if (lw != -INFINITY) v = a.p[(int64_t)k * a.ldp + i0 + r];
            }
            sp[k][r] = v;
        }
        if (tid < R) {
            const double lw = tid < cnt ? (a.logw ? a.logw[i0 + tid] : a.logw0) : -INFINITY;
            const bool zero = lw == -INFINITY;
            if (second) {
                sw[tid] = zero ? 0.0 : exp(lw - lwshift);
            } else {
                sw[tid] = zero ? INFINITY : 0.0;
                lwmine = fmax(lwmine, lw);
            }
        }
        __syncthreads();
    };
    auto load_q = [&](int c, double (&qc)[C]) {
#pragma unroll
        for (int k = 0; k < C; ++k) qc[k] = c + k < d ? a.q[(int64_t)(c + k) * a.ldq + jc] : 0.0;
    };
    auto sqdist = [&](int e0, double (&ss)[T]) {
#pragma unroll
        for (int e = 0; e < T; ++e) ss[e] = 0.0;
#pragma unroll 1
        for (int c = 0; c < dpad; c += C) {
            double qc[C];
            load_q(c, qc);
#pragma unroll
            for (int e = 0; e < T; ++e) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const double dk = sp[c + k][e0 + e] - qc[k];
                    ss[e] = fma(dk, dk, ss[e]);
                }
            }
        }
    };
    double r2min = INFINITY;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        stage(i0, false);
#pragma unroll 1
        for (int e0 = 0; e0 < R; e0 += T) {
            double ss[T];
            sqdist(e0, ss);
#pragma unroll
            for (int e = 0; e < T; ++e) r2min = fmin(r2min, ss[e] + sw[e0 + e]);
        }
    }
    const double lwmax = kde_block_max(lwmine, sw, R, tid);
    lwshift = lwmax == -INFINITY ? 0.0 : lwmax;
    if (r2min == INFINITY) r2min = 0.0;
    const double dmin = ta.nu + r2min;
    if (live)
        for (int k = 0; k < d; ++k) smj[k * a.m] = 0.0;
    double s = 0.0;
    for (int64_t i0 = 0; i0 < a.n; i0 += R) {
        stage(i0, true);
#pragma unroll 1
        for (int e0 = 0; e0 < R; e0 += T) {
            double tc[T];
            sqdist(e0, tc);
#pragma unroll
            for (int e = 0; e < T; ++e) {
                const double den = ta.nu + tc[e];
                const double rinv = recip2(den, __builtin_amdgcn_rcp(den));
                const double t = sw[e0 + e] * kde_t_power<POW, 0>(fmin(dmin * rinv, 1.0), ta.h, ta.half);
                s += t;
                tc[e] = t * rinv;
            }
            if (live) {
#pragma unroll 1
                for (int c = 0; c < dpad; c += C) {
                    double qc[C], acc[C];
                    load_q(c, qc);
#pragma unroll
                    for (int k = 0; k < C; ++k) acc[k] = c + k < d ? smj[(c + k) * a.m] : 0.0;
#pragma unroll
                    for (int e = 0; e < T; ++e) {
#pragma unroll
                        for (int k = 0; k < C; ++k) acc[k] = fma(tc[e], sp[c + k][e0 + e] - qc[k], acc[k]);
                    }
#pragma unroll
                    for (int k = 0; k < C; ++k)
                        if (c + k < d) smj[(c + k) * a.m] = acc[k];
                }
            }
        }
    }
    if (!live) return;
    a.log_q[j] = log(s) + (lwshift + (a.log_norm - ta.h * log1p(r2min / ta.nu)));
    const double c = (2.0 * ta.h) / s;
    for (int k = 0; k < d; ++k) smj[k * a.m] = c * smj[k * a.m];
    for (int k = 0; k < d; ++k) {
        double gk = 0.0;
        for (int l = 0; l < d; ++l) gk = fma(smj[l * a.m], a.L[k * d + l], gk);
        a.grad[j * d + k] = gk;
    }
}

// st_tune key 24: 0 / -1 automatic, 1 = exp(h log rho) for every nu, 2 = the chain with its exponent in a scalar
// register for every floor(h) (no compile-time copies of the sweep)
int g_kde_t_power = 0;

template <int POW>
void launch_kde_t_path(const KdeTArgs& ta, int d, double* ws, unsigned grid, hipStream_t s) {
    switch (d) {
        case 1: kde_t_kernel<1, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 2: kde_t_kernel<2, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 3: kde_t_kernel<3, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 4: kde_t_kernel<4, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 5: kde_t_kernel<5, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 6: kde_t_kernel<6, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 7: kde_t_kernel<7, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        case 8: kde_t_kernel<8, POW><<<grid, kKdeBlock, 0, s>>>(ta); break;
        default: kde_t_rt_kernel<POW><<<grid, kKdeBlock, 0, s>>>(ta, d, ws); break;
    }
}

}  // namespace

int64_t kde_workspace_bytes(int64_t m, int d) { return d > 8 ? m * d * (int64_t)sizeof(double) : 0; }

int kde_t_tune(int value) {
    if (value < -1 || value > 2) return -1;
    g_kde_t_power = value > 0 ? value : 0;
    return 0;
}

// The integer power path applies when nu + d is an integer of at most kKdeTMaxIntPower (a chain of at most
// 7 squarings); other nu, and every nu under st_tune key 24 = 1, take exp(h log rho).
constexpr double kKdeTMaxIntPower = 256.0;

hipError_t launch_kde_t(const double* p, int64_t ldp, int64_t n, const double* logw, double logw0,
                        const double* q, int64_t ldq, int64_t m, int d, double df, double log_norm,
                        const double* L, double* log_q, double* grad, double* ws, hipStream_t s) {
    const double two_h = df + d;
    // the chain needs floor(h) >= 1 (its first loop ends at the exponent's lowest set bit): two_h >= 2, which
    // only a df below one ulp of d = 1 misses
    const bool integer = g_kde_t_power != 1 && two_h == floor(two_h) && two_h >= 2.0 && two_h <= kKdeTMaxIntPower;
    KdeTArgs ta{{p, ldp, n, logw, logw0, q, ldq, m, log_norm, L, log_q, grad}, df, 0.5 * two_h,
                integer ? (int)two_h / 2 : 0, g_kde_t_power != 2};
    const unsigned grid = (unsigned)((m + kKdeBlock - 1) / kKdeBlock);
    if (!integer) launch_kde_t_path<kPowGeneral>(ta, d, ws, grid, s);
    else if ((int)two_h % 2) launch_kde_t_path<kPowOdd>(ta, d, ws, grid, s);
    else launch_kde_t_path<kPowEven>(ta, d, ws, grid, s);
    return hipGetLastError();
}

hipError_t launch_kde(const double* p, int64_t ldp, int64_t n, const double* logw, double logw0,
                      const double* q, int64_t ldq, int64_t m, int d, double log_norm, const double* L,
                      double* log_q, double* grad, double* ws, hipStream_t s) {
    KdeArgs a{p, ldp, n, logw, logw0, q, ldq, m, log_norm, L, log_q, grad};
    const unsigned grid = (unsigned)((m + kKdeBlock - 1) / kKdeBlock);
    switch (d) {
        case 1: kde_kernel<1><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 2: kde_kernel<2><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 3: kde_kernel<3><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 4: kde_kernel<4><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 5: kde_kernel<5><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 6: kde_kernel<6><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 7: kde_kernel<7><<<grid, kKdeBlock, 0, s>>>(a); break;
        case 8: kde_kernel<8><<<grid, kKdeBlock, 0, s>>>(a); break;
        default: kde_rt_kernel<<<grid, kKdeBlock, 0, s>>>(a, d, ws); break;
    }
    return hipGetLastError();
}

}  // namespace st
