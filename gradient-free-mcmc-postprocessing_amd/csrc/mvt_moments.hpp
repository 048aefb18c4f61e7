// Sample moments of the multivariate-t likelihood (st_mvt_moments): everything fit_mvt / fit_mvt2 of
// Gradient_free_Student_t.ipynb need from the rows for one evaluation of the negative log likelihood
// and its full analytic gradient.  Included by proxy.hip (its tile constants kRows / kPitch).
//
// Per row x_i, with the whitening U (U U^T = inv(Sigma); rows of z = (x - loc) @ U):
//   z_i = (x_i - loc) @ U,   delta_i = |z_i|^2,   w_i = (df + d) / (df + delta_i)
// and the sums over the sample, the only thing that leaves the chip:
//   S0 = sum log(1 + (1 / df) delta_i)          (scipy's multivariate_t._logpdf operation order)
//   S1 = sum w_i,   Sz = sum w_i z_i,   Szz = sum w_i z_i z_i^T (upper triangle)
// z and delta are proxy_kernel's fma chains: z_j = fma(dev_k, U[k][j], z_j) over k, the squares summed
// per group of columns {4g .. 4g + 3} and the four group sums added as ((p0 + p1) + p2) + p3.
//
// No per-row output.  A block walks 64-row tiles (lane = row) in a grid-stride loop and keeps its
// partial sums in registers; two widths:
//   d <= 8 (mvt_moments_reg_kernel): every wave owns its own tiles and all 2 + d + d (d + 1) / 2 <= 46
//     accumulators of its rows; the x tile comes through a wave-private LDS slab (transposed, pitch 65:
//     contiguous global loads, conflict-free LDS both ways), the next tile's loads are in flight under
//     this tile's arithmetic.
//   8 < d <= 16 (mvt_moments_split_kernel): the block's four waves share one tile.  Wave g computes
//     the z columns of group g (as proxy_kernel's waves do) and z goes through LDS; the (d + 1) (d + 2) / 2
//     entries of the upper triangle of sum w [z 1] [z 1]^T (= Szz, Sz and S1 in one indexing) are dealt
//     round-robin to the waves: at most 39 accumulators per lane.
// Reduction, the same bits on every call at a given grid: per lane sequentially over its tiles, across
// the wave by a fixed DPP tree (mvt_wave_sum), across the waves in wave order, one record per block in the
// workspace; a second one-block launch on the same stream adds the records in block order (consecutive
// runs of blocks side by side, then the run sums in order).  No atomics, no flags, no dependence on the
// dispatch order.  want_grad = 0 runs the same S0 arithmetic and nothing else: the same S0 bits.
#pragma once

namespace st {
namespace {

constexpr int kMvtThreads = 256;
constexpr int kMvtWaves = kMvtThreads / 64;
constexpr int kMvtMaxBlocks = 1024;     // records in the workspace: 4 blocks per CU on 256 CUs
constexpr int kMvtBlocksPerCu = 4;
constexpr int kMvtSplitBlocksPerCu = 2;
constexpr int kMvtFinalThreads = 1024;
constexpr int kMvtFinalBatch = 16;

__host__ __device__ constexpr int mvt_nacc(int d) { return 2 + d + d * (d + 1) / 2; }

// the sum of v over the wave's 64 lanes, in every lane (a fixed tree: the same bits every time): DPP
// butterflies inside each row of 16 lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: VALU
// data movement, no LDS round trips -- with __shfl_down the 6 dependent ds_bpermute steps per accumulator
// were most of the small-n kernel time), then the four row sums in row order
__device__ __forceinline__ double mvt_wave_sum(double v) {
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    v += dpp_f64<0x141>(v);
    v += dpp_f64<0x140>(v);
    const long long b = __double_as_longlong(v);
    double row[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, 16 * r);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), 16 * r);
        row[r] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    return ((row[0] + row[1]) + row[2]) + row[3];
}

// the tile's rows (0 past the last tile) and the CH elements e = tid + stride i of its (rows, D)
// row-major block, zeros past its end
template <int D, int CH>
__device__ __forceinline__ void mvt_load(const MvtMomentsArgs& a, int64_t tile, int64_t ntiles, int tid,
                                         int stride, double (&v)[CH]) {
    const bool in = tile < ntiles;
    const int64_t r0 = in ? tile * kRows : 0;
    const int total = in ? (int)min<int64_t>(kRows, a.n - r0) * D : 0;
    const double* xb = a.x + r0 * D;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int e = tid + stride * i;
        v[i] = e < total ? xb[e] : 0.0;
    }
}

template <int D, bool GRAD>
__global__ __launch_bounds__(kMvtThreads) void mvt_moments_reg_kernel(MvtMomentsArgs a) {
    static_assert(D >= 1 && D <= 8, "all accumulators of a row in its lane's registers");
    constexpr int NACC = GRAD ? mvt_nacc(D) : 1;
    __shared__ double s_t[kMvtWaves][D * kPitch];
    __shared__ double s_red[kMvtWaves][NACC];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ntiles = (a.n + kRows - 1) / kRows;
    const int64_t stride = (int64_t)gridDim.x * kMvtWaves;
    const int64_t passes = (ntiles + stride - 1) / stride;   // block-uniform: the barrier below
    double* slab = s_t[w];
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    const double dfd = a.df + (double)D;
    double v[D];
    int64_t tile = (int64_t)blockIdx.x * kMvtWaves + w;
    mvt_load<D, D>(a, tile, ntiles, lane, kRows, v);
    for (int64_t p = 0; p < passes; ++p, tile += stride) {
        const int rows = tile < ntiles ? (int)min<int64_t>(kRows, a.n - tile * kRows) : 0;
        // the slab is this wave's alone and a wave's LDS accesses complete in order: the previous
        // tile's reads are behind these writes
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int e = lane + kRows * i;   // e < 64 D: always inside the slab
            const int r = e / D;
            slab[(e - r * D) * kPitch + r] = v[i];   // rows >= `rows`: zeros, masked below
        }
        __syncthreads();
        mvt_load<D, D>(a, tile + stride, ntiles, lane, kRows, v);   // in flight under this tile
        double dev[D], z[D];
#pragma unroll
        for (int k = 0; k < D; ++k) dev[k] = slab[k * kPitch + lane] - a.loc[k];
#pragma unroll
        for (int j = 0; j < D; ++j) z[j] = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k)
#pragma unroll
            for (int j = 0; j < D; ++j) z[j] = fma(dev[k], a.U[k * D + j], z[j]);
        double p0 = 0.0, p1 = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (j < 4) p0 = fma(z[j], z[j], p0);
            else p1 = fma(z[j], z[j], p1);
        }
        const double maha = D > 4 ? p0 + p1 : p0;
        const bool valid = lane < rows;
        const double l = log(1.0 + (1.0 / a.df) * maha);
        acc[0] += valid ? l : 0.0;
        if constexpr (GRAD) {
            const double wgt = valid ? dfd / (a.df + maha) : 0.0;
            acc[1] += wgt;
            int idx = 2 + D;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double wz = wgt * z[i];
                acc[2 + i] += wz;
#pragma unroll
                for (int j = i; j < D; ++j, ++idx) acc[idx] = fma(wz, z[j], acc[idx]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const double r = mvt_wave_sum(acc[i]);
        if (lane == 0) s_red[w][i] = r;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        const int t = threadIdx.x;
        a.ws[(int64_t)blockIdx.x * mvt_nacc(D) + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
    }
}

// entry e of the upper triangle (row-major) of the (D + 1) x (D + 1) matrix sum w [z 1] [z 1]^T: its
// row i <= column j, and its place in the output record {S0, S1, Sz[D], Szz upper triangle row-major}
__device__ __forceinline__ void mvt_entry(int e, int D, int& i, int& j) {
    i = 0;
    int len = D + 1;
    while (e >= len) {
        e -= len;
        --len;
        ++i;
    }
    j = i + e;
}

__device__ __forceinline__ int mvt_slot(int i, int j, int D) {
    if (j == D) return i == D ? 1 : 2 + i;
    return 2 + D + i * D - i * (i - 1) / 2 + (j - i);
}

template <int D, bool GRAD>
__global__ __launch_bounds__(kMvtThreads) void mvt_moments_split_kernel(MvtMomentsArgs a) {
    static_assert(D > 8 && D <= 16, "one group of four z columns per wave");
    constexpr int E = (D + 1) * (D + 2) / 2;
    constexpr int NA = GRAD ? (E + kMvtWaves - 1) / kMvtWaves : 1;
    constexpr int CH = (kRows * D + kMvtThreads - 1) / kMvtThreads;
    __shared__ double s_dev[D * kPitch];
    __shared__ double s_z[(D + 1) * kPitch];      // row D: the constant 1
    __shared__ double s_part[kMvtWaves * kRows];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t ntiles = (a.n + kRows - 1) / kRows;
    if (tid < kRows) s_z[D * kPitch + tid] = 1.0;   // read after the loop's barriers
    // this wave's entries e = w + 4 i: the LDS rows of their two factors, packed
    [[maybe_unused]] int pk[NA];
    if constexpr (GRAD) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = w + kMvtWaves * i;
            int r = 0, c = 0;
            if (e < E) mvt_entry(e, D, r, c);
            pk[i] = (r * kPitch) | ((c * kPitch) << 16);
        }
    }
    double acc[NA], s0 = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;
    const double dfd = a.df + (double)D;
    const int j0 = 4 * w;
    const int nc = min(4, max(0, D - j0));
    double v[CH];
    mvt_load<D, CH>(a, blockIdx.x, ntiles, tid, kMvtThreads, v);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // block-uniform
        const int rows = (int)min<int64_t>(kRows, a.n - tile * kRows);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = tid + kMvtThreads * i;
            if (e < kRows * D) {
                const int r = e / D;
                const int k = e - r * D;
                s_dev[k * kPitch + r] = v[i] - a.loc[k];   // rows >= `rows`: -loc, masked below
            }
        }
        __syncthreads();
        mvt_load<D, CH>(a, tile + gridDim.x, ntiles, tid, kMvtThreads, v);   // in flight under this tile
        double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
        if (nc > 0) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double dv = s_dev[k * kPitch + lane];
                const double* u = a.U + k * D + j0;
                z0 = fma(dv, u[0], z0);
                if (nc > 1) z1 = fma(dv, u[1], z1);
                if (nc > 2) z2 = fma(dv, u[2], z2);
                if (nc > 3) z3 = fma(dv, u[3], z3);
            }
        }
        double mz = 0.0;
        if (nc > 0) mz = fma(z0, z0, mz);
        if (nc > 1) mz = fma(z1, z1, mz);
        if (nc > 2) mz = fma(z2, z2, mz);
        if (nc > 3) mz = fma(z3, z3, mz);
        s_part[w * kRows + lane] = mz;
        if constexpr (GRAD) {
            if (nc > 0) s_z[(j0 + 0) * kPitch + lane] = z0;
            if (nc > 1) s_z[(j0 + 1) * kPitch + lane] = z1;
            if (nc > 2) s_z[(j0 + 2) * kPitch + lane] = z2;
            if (nc > 3) s_z[(j0 + 3) * kPitch + lane] = z3;
        }
        __syncthreads();
        const double maha = ((s_part[lane] + s_part[kRows + lane]) + s_part[2 * kRows + lane]) +
                            s_part[3 * kRows + lane];
        const bool valid = lane < rows;
        if (w == 0) {
            const double l = log(1.0 + (1.0 / a.df) * maha);
            s0 += valid ? l : 0.0;
        }
        if constexpr (GRAD) {
            const double wgt = valid ? dfd / (a.df + maha) : 0.0;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                if (w + kMvtWaves * i < E) {
                    const double zi = s_z[(pk[i] & 0xFFFF) + lane];
                    const double zj = s_z[(pk[i] >> 16) + lane];
                    acc[i] = fma(wgt * zi, zj, acc[i]);
                }
            }
        }
        // the next tile's s_dev writes follow this tile's last s_dev read (before the barrier above);
        // its s_z / s_part writes follow the next barrier, which every wave reaches after these reads
    }
    double* rec = a.ws + (int64_t)blockIdx.x * mvt_nacc(D);
    if (w == 0) {
        const double r = mvt_wave_sum(s0);
        if (lane == 0) rec[0] = r;
    }
    if constexpr (GRAD) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = w + kMvtWaves * i;
            const double r = mvt_wave_sum(acc[i]);
            if (e < E && lane == 0) {
                int ri, ci;
                mvt_entry(e, D, ri, ci);
                rec[mvt_slot(ri, ci, D)] = r;
            }
        }
    }
}

// out[t] = the records' entry t added in block order: `chunks` consecutive runs of `per` blocks
// summed side by side, then the run sums in order (chunks * count <= kMvtFinalThreads)
__global__ __launch_bounds__(kMvtFinalThreads) void mvt_moments_final_kernel(const double* ws, int blocks, int rec_stride,
                                                                             int count, int chunks, int per, double* out) {
    __shared__ double s_p[kMvtFinalThreads];
    const int tid = threadIdx.x;
    if (tid < chunks * count) {
        const int c = tid / count;
        const int t = tid - c * count;
        const int b1 = min(blocks, (c + 1) * per);
        const double* r = ws + t;
        double sum = 0.0;
        for (int b = c * per; b < b1; b += kMvtFinalBatch) {   // a batch of loads in flight, added in order
            double v[kMvtFinalBatch];
#pragma unroll
            for (int i = 0; i < kMvtFinalBatch; ++i) v[i] = b + i < b1 ? r[(int64_t)(b + i) * rec_stride] : 0.0;
#pragma unroll
            for (int i = 0; i < kMvtFinalBatch; ++i)
                if (b + i < b1) sum += v[i];
        }
        s_p[tid] = sum;
    }
    __syncthreads();
    if (tid < count) {
        double sum = s_p[tid];
        for (int c = 1; c < chunks; ++c) sum += s_p[c * count + tid];
        out[tid] = sum;
    }
}

template <int D>
hipError_t launch_mvt_d(const MvtMomentsArgs& a, int grid, hipStream_t s) {
    if constexpr (D <= 8) {
        if (a.want_grad) mvt_moments_reg_kernel<D, true><<<dim3((unsigned)grid), kMvtThreads, 0, s>>>(a);
        else mvt_moments_reg_kernel<D, false><<<dim3((unsigned)grid), kMvtThreads, 0, s>>>(a);
    } else {
        if (a.want_grad) mvt_moments_split_kernel<D, true><<<dim3((unsigned)grid), kMvtThreads, 0, s>>>(a);
        else mvt_moments_split_kernel<D, false><<<dim3((unsigned)grid), kMvtThreads, 0, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace

// records the largest grid of a launch writes (host only: no HIP call)
static int64_t mvt_max_blocks(int64_t n) {
    const int64_t tiles = (n + kRows - 1) / kRows;
    return tiles < kMvtMaxBlocks ? tiles : kMvtMaxBlocks;
}

int64_t mvt_moments_ws_bytes(int64_t n, int d) { return mvt_max_blocks(n) * mvt_nacc(d) * 8; }

// a.n >= 1, 1 <= a.d <= kMvtMaxDim, a.ws of mvt_moments_ws_bytes(a.n, a.d) bytes (st_mvt_moments validates)
hipError_t launch_mvt_moments(const MvtMomentsArgs& a, hipStream_t s) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    // grid: a block per pass of tiles (four tiles per pass for d <= 8, one above), at most
    // kMvtBlocksPerCu (d <= 8) / kMvtSplitBlocksPerCu per CU -- what is resident at once with the
    // gradient's registers --, under the st_tune grid cap (key 23 for this thread, else key 5)
    const int64_t tiles = (a.n + kRows - 1) / kRows;
    int64_t grid = a.d <= 8 ? (tiles + kMvtWaves - 1) / kMvtWaves : tiles;
    const int bpc = a.d <= 8 ? kMvtBlocksPerCu : kMvtSplitBlocksPerCu;
    if (grid > (int64_t)cus * bpc) grid = (int64_t)cus * bpc;
    const int cap = persistent_tune_get(23) > 0 ? persistent_tune_get(23) : persistent_tune_get(5);
    if (cap > 0 && grid > cap) grid = cap;
    if (grid > mvt_max_blocks(a.n)) grid = mvt_max_blocks(a.n);
    if (grid < 1) grid = 1;
    switch (a.d) {
        case 1: e = launch_mvt_d<1>(a, (int)grid, s); break;
        case 2: e = launch_mvt_d<2>(a, (int)grid, s); break;
        case 3: e = launch_mvt_d<3>(a, (int)grid, s); break;
        case 4: e = launch_mvt_d<4>(a, (int)grid, s); break;
        case 5: e = launch_mvt_d<5>(a, (int)grid, s); break;
        case 6: e = launch_mvt_d<6>(a, (int)grid, s); break;
        case 7: e = launch_mvt_d<7>(a, (int)grid, s); break;
        case 8: e = launch_mvt_d<8>(a, (int)grid, s); break;
        case 9: e = launch_mvt_d<9>(a, (int)grid, s); break;
        case 10: e = launch_mvt_d<10>(a, (int)grid, s); break;
        case 11: e = launch_mvt_d<11>(a, (int)grid, s); break;
        case 12: e = launch_mvt_d<12>(a, (int)grid, s); break;
        case 13: e = launch_mvt_d<13>(a, (int)grid, s); break;
        case 14: e = launch_mvt_d<14>(a, (int)grid, s); break;
        case 15: e = launch_mvt_d<15>(a, (int)grid, s); break;
        case 16: e = launch_mvt_d<16>(a, (int)grid, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    const int count = a.want_grad ? mvt_nacc(a.d) : 1;
    int chunks = kMvtFinalThreads / mvt_nacc(a.d);   // not / count: S0 is added in the same order with and without the rest
    if (chunks > (int)grid) chunks = (int)grid;
    const int per = ((int)grid + chunks - 1) / chunks;
    mvt_moments_final_kernel<<<dim3(1), kMvtFinalThreads, 0, s>>>(a.ws, (int)grid, mvt_nacc(a.d), count, chunks, per, a.out);
    return hipGetLastError();
}

}  // namespace st
