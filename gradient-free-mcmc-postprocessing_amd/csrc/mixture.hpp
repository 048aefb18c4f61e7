// Gaussian-mixture log density and score at every sample row (st_mixture_logpdf_score): the target of
// the reference's Gaussian-mixture study (code/src/utils/mvn.py make_mvn_mixture: logpdf / score) and
// a mixture proxy q for thin_gf.  Included by proxy.hip (its tile constants, kmap / jmap and dbl4).
//
// Per row x and component c (a_c = log w_c - (d log 2 pi + log det Sigma_c) / 2 and P_c = inv(Sigma_c)
// from the host):
//   dev_c = x - mu_c,  y_c = P_c dev_c,  q_c = dev_c . y_c,  l_c = a_c - q_c / 2
//   log_p = logsumexp_c l_c,           score = - sum_c exp(l_c - log_p) y_c
// evaluated in log space in ONE pass over c: a running maximum m with the sum s = sum exp(l_c - m)
// and the accumulator g = sum exp(l_c - m) y_c rescaled whenever the maximum moves (the reference
// sums densities: -inf and 0 / 0 once every component underflows).  A component with a_c = -inf (zero
// weight) is skipped -- wave-uniformly, before any arithmetic, so exp(-inf - (-inf)) is never formed.
// A row holding a NaN or an inf, or whose l_c is NaN, gets NaN outputs; no other row sees it.
// One row's arithmetic is sequential in c and k and never mixes with another row's: the outputs of a
// row do not depend on n or on where the row sits in a tile.
//
// Two widths:
//   d <= 16: VALU, one wave per block, lane = row of a 64-row tile.  The x tile comes in and the
//     score tile goes out through LDS (transposed, pitch 65) so global accesses are contiguous; a_c,
//     mu_c and P_c are wave-uniform scalar loads through the constant address space (the parameter
//     arrays are never written while the kernel runs), D is a compile-time width (no padding).
//   16 < d <= 64: y^T = P_c dev^T on v_mfma_f64_16x16x4_f64 with proxy.hip's streaming lane maps
//     (lane l holds sample row l & 15 and the k / output columns of group l >> 4, so q_c is a
//     register dot and two cross-lane adds and the running state lives in registers in the
//     accumulator layout).  One wave per 16-row block, 4 waves per block, two blocks per CU; P_c's A
//     fragments are staged per component in LDS in fragment order (conflict-free reads, shared by
//     the block's waves), so LDS use does not grow with k.  The next component's P_c and mu_c are
//     fetched into registers (contiguous loads) under the current component's MFMAs.
// x is read once and each output written once, whatever k is.
#pragma once

namespace st {
namespace {

typedef const __attribute__((address_space(4))) double* MixConstPtr;

__device__ __forceinline__ MixConstPtr mix_const(const double* p) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return (MixConstPtr)p;
#pragma clang diagnostic pop
}

// the running (m, s) of one row takes l; returns the factor e and whether the maximum moved:
//   moved: s <- s e + 1, g <- g e + y, m <- l       (e = exp(m - l); m = -inf at the start: e = 0)
//   else, taken: s <- s + e, g <- g + e y            (e = exp(l - m))
// l = -inf or NaN is not taken (state unchanged; the caller flags NaN rows).
__device__ __forceinline__ void mix_step(double l, double& m, double& s, double& e, bool& moved, bool& taken) {
    moved = l > m;
    taken = moved || l > -INFINITY;
    e = exp(moved ? m - l : l - m);
    if (moved) {
        s = fma(s, e, 1.0);
        m = l;
    } else if (taken) {
        s += e;
    }
}

template <int D>
__global__ __launch_bounds__(kRows) void mixture_valu_kernel(MixtureArgs a) {
    __shared__ double s_t[D * kPitch];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    const int rows = (int)min<int64_t>(kRows, a.n - r0);
    const int total = rows * D;
    {
        const double* xb = a.x + r0 * D;
        double v[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int e = lane + kRows * i;
            v[i] = e < total ? xb[e] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int e = lane + kRows * i;   // e < 64 D: always inside s_t
            const int r = e / D;
            s_t[(e - r * D) * kPitch + r] = v[i];   // rows >= `rows`: zeros, results dropped
        }
    }
    __syncthreads();
    double xv[D], g[D];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xv[k] = s_t[k * kPitch + lane];
        bad |= !(fabs(xv[k]) < INFINITY);
        g[k] = 0.0;
    }
    double m = -INFINITY, s = 0.0;
    const MixConstPtr coef = mix_const(a.log_coef);
    for (int c = 0; c < a.k; ++c) {
        const double ac = coef[c];
        if (ac == -INFINITY) continue;   // wave-uniform
        const MixConstPtr mu = mix_const(a.means + (int64_t)c * D);
        const MixConstPtr P = mix_const(a.P + (int64_t)c * D * D);
        double dev[D], y[D];
#pragma unroll
        for (int k = 0; k < D; ++k) dev[k] = xv[k] - mu[k];
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double t = P[j * D] * dev[0];
#pragma unroll
            for (int k = 1; k < D; ++k) t = fma(P[j * D + k], dev[k], t);
            y[j] = t;
            q = j == 0 ? dev[0] * t : fma(dev[j], t, q);
        }
        const double l = ac - 0.5 * q;
        bad |= l != l;
        double e;
        bool moved, taken;
        mix_step(l, m, s, e, moved, taken);
#pragma unroll
        for (int k = 0; k < D; ++k) g[k] = moved ? fma(g[k], e, y[k]) : (taken ? fma(e, y[k], g[k]) : g[k]);
    }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double inv = 1.0 / s;
    if (lane < rows) a.log_p[r0 + lane] = bad ? nan : m + log(s);
    __syncthreads();   // every lane has read its x column
#pragma unroll
    for (int k = 0; k < D; ++k) s_t[k * kPitch + lane] = bad ? nan : -(g[k] * inv);
    __syncthreads();
    double* gb = a.score + r0 * D;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const int e = lane + kRows * i;
        const int r = e / D;
        if (e < total) gb[e] = s_t[(e - r * D) * kPitch + r];
    }
}

constexpr int kMixThreads = 256;
constexpr int kMixWaves = kMixThreads / 64;

template <int T, int S>
__global__ __launch_bounds__(kMixThreads, 2) void mixture_mfma_kernel(MixtureArgs a) {
    static_assert(S % 2 == 0 && S <= 4 * T, "k steps pair up; every step has an output tile");
    // P_c's A fragments: fragment (s, c) at kFrag (s T + c) + lane.  kFrag = 64 + 2 shifts successive
    // fragments by 2 doubles (4 banks): a fragment read stays 64 consecutive doubles (conflict-free),
    // and the staging writes of one row of P_c (fixed lane slot, s and the k group varying) spread
    // over the banks instead of landing on two
    constexpr int kFrag = 64 + 2;
    constexpr int kStage = (64 * T * S + kMixThreads - 1) / kMixThreads;   // d^2 <= 64 T S elements of P_c
    __shared__ double s_pa[T * S * kFrag];
    __shared__ double s_mu[4 * S];        // mu_c, zero past d
    const int d = a.d;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int wave = tid >> 6;
    const int64_t ntiles = (a.n + 16 * kMixWaves - 1) / (16 * kMixWaves);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    // Staging plan, the same for every component: this thread carries elements e = tid + 256 i of the
    // row-major P_c (contiguous loads) to the fragment slot of (j, k) = (e / d, e % d) -- the inverse
    // of jmap / kmap -- or nowhere (slot < 0, e >= d^2).  The padding slots (j >= d or k >= d) are
    // zeroed once: no component writes them.
    __shared__ int s_slot[kStage * kMixThreads];   // [i][tid]: read back by the thread that wrote it
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
        const int e = tid + kMixThreads * i;
        const int j = e / d, k = e - j * d;
        const int c = j >> 4, row = 8 * ((j >> 3) & 1) + 4 * (j & 1) + ((j >> 1) & 3);
        const int sk = 2 * (k >> 3) + (k & 1), grp = (k >> 1) & 3;
        s_slot[e] = e < d * d ? (sk * T + c) * kFrag + 16 * grp + row : -1;
    }
    for (int e = tid; e < T * S * kFrag; e += kMixThreads) s_pa[e] = 0.0;
    double pf[kStage], pmu = 0.0;   // the next component's P_c elements and mean, in flight
    auto fetch = [&](int comp) {
        const double* Pc = a.P + (int64_t)comp * d * d;
#pragma unroll
        for (int i = 0; i < kStage; ++i) pf[i] = tid + kMixThreads * i < d * d ? Pc[tid + kMixThreads * i] : 0.0;
        pmu = tid < d ? a.means[(int64_t)comp * d + tid] : 0.0;
    };
    fetch(0);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // block-uniform: the barriers below
        const int64_t row = (tile * kMixWaves + wave) * 16 + li;
        const bool live = row < a.n;
        const double* xr = a.x + (live ? row : a.n - 1) * d;   // rows past n: a valid row, results dropped
        double xv[S];
        int badi = 0;
#pragma unroll
        for (int t = 0; t < S / 2; ++t) {
            const int k0 = 8 * t + 2 * lk;
            xv[2 * t] = k0 < d ? xr[k0] : 0.0;
            xv[2 * t + 1] = k0 + 1 < d ? xr[k0 + 1] : 0.0;
            badi |= !(fabs(xv[2 * t]) < INFINITY) || !(fabs(xv[2 * t + 1]) < INFINITY);
        }
        badi |= __shfl_xor(badi, 16);
        badi |= __shfl_xor(badi, 32);
        bool bad = badi != 0;
        double m = -INFINITY, s = 0.0;
        dbl4 g[T];
#pragma unroll
        for (int c = 0; c < T; ++c) g[c] = dbl4{0.0, 0.0, 0.0, 0.0};
        for (int comp = 0; comp < a.k; ++comp) {
            const double ac = a.log_coef[comp];
            const int next = comp + 1 < a.k ? comp + 1 : 0;   // the next tile starts over at component 0
            if (ac == -INFINITY) {   // block-uniform: drop the fetched component, fetch its successor
                fetch(next);
                continue;
            }
            __syncthreads();   // the previous component's (or tile's) readers are done; the zero fill
            int to[kStage];   // every slot read issued before the first store waits on one
#pragma unroll
            for (int i = 0; i < kStage; ++i) to[i] = s_slot[tid + kMixThreads * i];
            __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise pairs each read with its store)
#pragma unroll
            for (int i = 0; i < kStage; ++i)
                if (to[i] >= 0) s_pa[to[i]] = pf[i];
            if (tid < 4 * S) s_mu[tid] = pmu;
            __syncthreads();
            fetch(next);   // in flight under this component's MFMAs
            double dev[S];
#pragma unroll
            for (int sk = 0; sk < S; ++sk) dev[sk] = s_mu[kmap(sk, lk)];
            __builtin_amdgcn_sched_barrier(0);   // all of mu_c's reads in flight before the first subtraction
#pragma unroll
            for (int sk = 0; sk < S; ++sk) dev[sk] = xv[sk] - dev[sk];
            dbl4 acc[T];
            double af[2][T];
#pragma unroll
            for (int c = 0; c < T; ++c) acc[c] = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < T; ++c) af[0][c] = s_pa[c * kFrag + lane];
#pragma unroll
            for (int sk = 0; sk < S; ++sk) {   // step sk + 1's fragments are read under step sk's MFMAs
                if (sk + 1 < S) {
#pragma unroll
                    for (int c = 0; c < T; ++c) af[(sk + 1) & 1][c] = s_pa[((sk + 1) * T + c) * kFrag + lane];
                }
                // keep the reads ahead of the MFMAs: left alone, the scheduler sinks each read to its
                // use (fewest live registers) and every MFMA pair waits a full LDS latency
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < T; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[sk & 1][c], dev[sk], acc[c], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // q = dev . y: step 4c + r holds the input column of output (c, r); then the row's 4 lanes
            double part = 0.0;
#pragma unroll
            for (int c = 0; c < T; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * c + r < S) part = fma(dev[4 * c + r], acc[c][r], part);
            part += __shfl_xor(part, 16);
            const double q = part + __shfl_xor(part, 32);   // the same double in the row's 4 lanes
            const double l = ac - 0.5 * q;
            bad |= l != l;
            double e;
            bool moved, taken;
            mix_step(l, m, s, e, moved, taken);
#pragma unroll
            for (int c = 0; c < T; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (taken) g[c][r] = moved ? fma(g[c][r], e, acc[c][r]) : fma(e, acc[c][r], g[c][r]);
        }
        if (live) {
            const double inv = 1.0 / s;
            if (lk == 0) a.log_p[row] = bad ? nan : m + log(s);
            double* gr = a.score + row * d;
#pragma unroll
            for (int c = 0; c < T; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j0 = 16 * c + 8 * h + 2 * lk;
                    if (j0 < d) gr[j0] = bad ? nan : -(g[c][2 * h] * inv);
                    if (j0 + 1 < d) gr[j0 + 1] = bad ? nan : -(g[c][2 * h + 1] * inv);
                }
        }
    }
}

template <int D>
hipError_t launch_mixture_valu(const MixtureArgs& a, hipStream_t s) {
    const int64_t blocks = (a.n + kRows - 1) / kRows;
    mixture_valu_kernel<D><<<dim3((unsigned)blocks), kRows, 0, s>>>(a);
    return hipGetLastError();
}

template <int T, int S>
hipError_t launch_mixture_mfma(const MixtureArgs& a, hipStream_t s) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    const int64_t tiles = (a.n + 16 * kMixWaves - 1) / (16 * kMixWaves);
    const int64_t grid = tiles < 2 * (int64_t)cus ? tiles : 2 * (int64_t)cus;
    mixture_mfma_kernel<T, S><<<dim3((unsigned)grid), kMixThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

// a.n >= 1, 1 <= a.d <= kMixtureMaxDim, a.k >= 1 (st_mixture_logpdf_score validates)
hipError_t launch_mixture(const MixtureArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if ((a.n + kRows - 1) / kRows > 0x7FFFFFFFll) return hipErrorInvalidValue;
    switch (a.d) {
        case 1: return launch_mixture_valu<1>(a, s);
        case 2: return launch_mixture_valu<2>(a, s);
        case 3: return launch_mixture_valu<3>(a, s);
        case 4: return launch_mixture_valu<4>(a, s);
        case 5: return launch_mixture_valu<5>(a, s);
        case 6: return launch_mixture_valu<6>(a, s);
        case 7: return launch_mixture_valu<7>(a, s);
        case 8: return launch_mixture_valu<8>(a, s);
        case 9: return launch_mixture_valu<9>(a, s);
        case 10: return launch_mixture_valu<10>(a, s);
        case 11: return launch_mixture_valu<11>(a, s);
        case 12: return launch_mixture_valu<12>(a, s);
        case 13: return launch_mixture_valu<13>(a, s);
        case 14: return launch_mixture_valu<14>(a, s);
        case 15: return launch_mixture_valu<15>(a, s);
        case 16: return launch_mixture_valu<16>(a, s);
        default: break;
    }
    if (a.d < 1 || a.d > kMixtureMaxDim) return hipErrorInvalidValue;
    switch ((a.d + 7) / 8) {   // T = ceil(d / 16) output tiles, S = 2 ceil(d / 8) k steps
        case 3: return launch_mixture_mfma<2, 6>(a, s);
        case 4: return launch_mixture_mfma<2, 8>(a, s);
        case 5: return launch_mixture_mfma<3, 10>(a, s);
        case 6: return launch_mixture_mfma<3, 12>(a, s);
        case 7: return launch_mixture_mfma<4, 14>(a, s);
        default: return launch_mixture_mfma<4, 16>(a, s);
    }
}

}  // namespace st
