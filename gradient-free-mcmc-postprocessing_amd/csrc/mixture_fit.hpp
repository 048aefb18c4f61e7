// One EM pass of a Gaussian-mixture fit (st_mixture_em_stats): the responsibilities of every row under the
// current parameters and the weighted, mean-centred sufficient statistics of every component, in one pass
// over the rows.  Included by proxy.hip after mixture.hpp (mix_const, mix_step: the E-step is
// mixture_valu_kernel's arithmetic) and mvt_moments.hpp (mvt_wave_sum, mvt_entry, mvt_slot).
//
// Per row x_i with weight om_i (1 without row weights) and component c (a_c, mu_c, P_c as st_mixture_logpdf_score):
//   dev_ic = x_i - mu_c,  l_ic = a_c - dev_ic . (P_c dev_ic) / 2,  log_p_i = logsumexp_c l_ic,  r_ic = exp(l_ic - log_p_i)
//   LL = sum om_i log_p_i,   N_c = sum om_i r_ic,   S_c = sum om_i r_ic dev_ic,   Q_c = sum om_i r_ic dev_ic dev_ic^T
// N_c, S_c and the upper triangle of Q_c are the E = (d + 1)(d + 2) / 2 entries of the upper triangle of
// sum om_i r_ic [dev_ic 1] [dev_ic 1]^T (mvt_moments_split_kernel's indexing).  A component with a_c = -inf is
// skipped (wave-uniformly: its entries stay exactly 0); a row with om_i = 0 adds nothing, whatever it holds.
//
// k E accumulators per row do not fit in a lane's registers, so they are dealt twice: the block's four waves
// share one 64-row tile (lane = row) and take the entries e = wave + 4 i of a component, at most
// ceil(E / 4) <= 39 each; and gridDim.y deals the components in groups of em_cpb(d) (as many as keep the
// accumulators of a lane within kEmAccBudget doubles: 12 at d = 4, 4 at d = 8, 1 at d = 16).  Every block of
// a group recomputes the E-step of its tiles: the l_ic of a tile are dealt over the waves (component
// c to wave c mod 4), go through LDS, and every wave runs the running-maximum logsumexp over them in
// component order -- one row's log_p_i is the same sequence of operations as in mixture_valu_kernel.  The x
// tile is staged once per tile in LDS (transposed, pitch 65: contiguous global loads, conflict-free LDS both
// ways; row d holds the constant 1), the next tile's loads are in flight under this tile's arithmetic; the
// groups after the first find the tiles in L2 / Infinity Cache.
// Reduction, the same bits on every call at a given grid: per lane sequentially over its tiles, across the
// wave by the fixed DPP tree mvt_wave_sum, one record {LL, k x {N_c, S_c, Q_c}} per blockIdx.x in the
// workspace (every entry has exactly one writer); a second launch adds the records in block order (up to 32
// consecutive runs of blocks side by side, then the run sums in order).  No atomics, no flags.
#pragma once

namespace st {
namespace {

constexpr int kEmThreads = 256;
constexpr int kEmWaves = kEmThreads / 64;
constexpr int kEmMaxBlocks = 1024;      // records in the workspace at one component group: 4 blocks per CU on 256 CUs
constexpr int kEmMinBlocks = 64;        // ... and at least this many however many groups there are
constexpr int kEmBlocksPerCu = 4;
constexpr int kEmAccBudget = 48;        // accumulators (doubles) per lane
constexpr int kEmFinalEntries = 32;     // the final kernel: entries per block x runs of blocks = its 1024 threads
constexpr int kEmFinalChunks = 32;
constexpr int kEmFinalBatch = 16;

__host__ __device__ constexpr int em_entries(int d) { return (d + 1) * (d + 2) / 2; }
__host__ __device__ constexpr int em_na(int d) { return (em_entries(d) + kEmWaves - 1) / kEmWaves; }
__host__ __device__ constexpr int em_cpb(int d) {
    return kEmAccBudget / em_na(d) < 1 ? 1
           : kEmAccBudget / em_na(d) > kMixtureEmMaxComponents ? kMixtureEmMaxComponents : kEmAccBudget / em_na(d);
}

// the CH elements e = tid + 256 i of the tile's (rows, D) row-major block, zeros past its end and past the last tile
template <int D, int CH>
__device__ __forceinline__ void em_load(const MixtureEmArgs& a, int64_t tile, int64_t ntiles, int tid, double (&v)[CH]) {
    const bool in = tile < ntiles;
    const int64_t r0 = in ? tile * kRows : 0;
    const int total = in ? (int)min<int64_t>(kRows, a.n - r0) * D : 0;
    const double* xb = a.x + r0 * D;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int e = tid + kEmThreads * i;
        v[i] = e < total ? xb[e] : 0.0;
    }
}

template <int D>
__global__ __launch_bounds__(kEmThreads) void mixture_em_kernel(MixtureEmArgs a) {
    static_assert(D >= 1 && D <= kMixtureEmMaxDim, "entry indices are packed in bytes");
    constexpr int E = em_entries(D);
    constexpr int NA = em_na(D);
    constexpr int CPB = em_cpb(D);
    constexpr int CH = (kRows * D + kEmThreads - 1) / kEmThreads;
    __shared__ double s_x[(D + 1) * kPitch];                   // row D: the constant 1
    __shared__ double s_l[kMixtureEmMaxComponents * kRows];    // l_ic of the tile
    __shared__ double s_mu[kMixtureEmMaxComponents * (D + 1)]; // mu_c, then the 0 that row D's constant takes
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t ntiles = (a.n + kRows - 1) / kRows;
    const int c0 = (int)blockIdx.y * CPB;
    const bool first = blockIdx.y == 0;                        // this group also owns LL and log_p_out
    if (tid < kRows) s_x[D * kPitch + tid] = 1.0;              // read after the loop's barriers, as s_mu
    for (int e = tid; e < a.k * (D + 1); e += kEmThreads) {
        const int c = e / (D + 1), j = e - c * (D + 1);
        s_mu[e] = j < D ? a.means[c * D + j] : 0.0;
    }
    // this wave's entries e = w + 4 i: the rows of their two factors in s_x (row D: no mean), packed
    int pk[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int e = w + kEmWaves * i;
        int r = 0, c = 0;
        if (e < E) mvt_entry(e, D, r, c);
        pk[i] = r | (c << 8);
    }
    double acc[CPB][NA], ll = 0.0;
#pragma unroll
    for (int cc = 0; cc < CPB; ++cc)
#pragma unroll
        for (int i = 0; i < NA; ++i) acc[cc][i] = 0.0;
    const MixConstPtr coef = mix_const(a.log_coef);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double v[CH];
    em_load<D, CH>(a, blockIdx.x, ntiles, tid, v);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // block-uniform: the barriers below
        const int64_t r0 = tile * kRows;
        const int rows = (int)min<int64_t>(kRows, a.n - r0);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = tid + kEmThreads * i;
            if (e < kRows * D) {
                const int r = e / D;
                s_x[(e - r * D) * kPitch + r] = v[i];   // rows >= `rows`: zeros, their weight is 0
            }
        }
        const double om = lane < rows ? (a.w ? a.w[r0 + lane] : 1.0) : 0.0;
        __syncthreads();
        em_load<D, CH>(a, tile + gridDim.x, ntiles, tid, v);   // in flight under this tile
        bool bad = false;
        {
            double xv[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                xv[k] = s_x[k * kPitch + lane];
                bad |= !(fabs(xv[k]) < INFINITY);
            }
            for (int c = w; c < a.k; c += kEmWaves) {   // mixture_valu_kernel's l_c, operation for operation
                const double ac = coef[c];
                if (ac == -INFINITY) continue;   // wave-uniform
                const MixConstPtr mu = mix_const(a.means + (int64_t)c * D);
                const MixConstPtr P = mix_const(a.P + (int64_t)c * D * D);
                double dev[D];
#pragma unroll
                for (int k = 0; k < D; ++k) dev[k] = xv[k] - mu[k];
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    double t = P[j * D] * dev[0];
#pragma unroll
                    for (int k = 1; k < D; ++k) t = fma(P[j * D + k], dev[k], t);
                    q = j == 0 ? dev[0] * t : fma(dev[j], t, q);
                }
                s_l[c * kRows + lane] = ac - 0.5 * q;
            }
        }
        __syncthreads();
        double m = -INFINITY, s = 0.0;
        for (int c = 0; c < a.k; ++c) {   // every wave: the running-maximum logsumexp in component order
            if (coef[c] == -INFINITY) continue;
            const double l = s_l[c * kRows + lane];
            bad |= l != l;
            double e;
            bool moved, taken;
            mix_step(l, m, s, e, moved, taken);
        }
        const double log_p = bad ? nan : m + log(s);
        const bool live = om != 0.0;   // a row of weight 0 adds nothing, even a non-finite one
        if (first && w == 0) {
            if (a.log_p && lane < rows) a.log_p[r0 + lane] = log_p;
            const double t = om * log_p;
            ll += live ? t : 0.0;
        }
#pragma unroll
        for (int cc = 0; cc < CPB; ++cc) {
            const int c = c0 + cc;
            if (c >= a.k) break;                       // block-uniform
            if (coef[c] == -INFINITY) continue;        // its entries stay exactly 0
            const double* mu = s_mu + c * (D + 1);      // wave-uniform addresses: broadcast reads
            if (live) {
                const double wgt = om * exp(s_l[c * kRows + lane] - log_p);
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    if (w + kEmWaves * i < E) {
                        const int ri = pk[i] & 0xFF, ci = pk[i] >> 8;
                        const double zi = s_x[ri * kPitch + lane] - mu[ri];
                        const double zj = s_x[ci * kPitch + lane] - mu[ci];
                        acc[cc][i] = fma(wgt * zi, zj, acc[cc][i]);
                    }
                }
            }
        }
        __syncthreads();   // the next tile's s_x / s_l writes follow this tile's last reads
    }
    double* rec = a.ws + (int64_t)blockIdx.x * (1 + (int64_t)a.k * E);
    if (first && w == 0) {
        const double r = mvt_wave_sum(ll);
        if (lane == 0) rec[0] = r;
    }
#pragma unroll
    for (int cc = 0; cc < CPB; ++cc) {
        const int c = c0 + cc;
        if (c >= a.k) break;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = w + kEmWaves * i;
            if (e < E) {
                const double r = mvt_wave_sum(acc[cc][i]);
                if (lane == 0) {
                    const int ri = pk[i] & 0xFF, ci = pk[i] >> 8;
                    rec[(int64_t)c * E + mvt_slot(ri, ci, D)] = r;   // mvt_slot: 1 = N, 2 + i = S_i, then Q; slot 0 of c = 0 is LL
                }
            }
        }
    }
}

// out[t] = the records' entry t added in block order: `chunks` consecutive runs of `per` blocks summed side
// by side, then the run sums in order; a block of the grid takes kEmFinalEntries consecutive entries
__global__ __launch_bounds__(kEmFinalEntries * kEmFinalChunks) void mixture_em_final_kernel(const double* ws, int blocks,
                                                                                            int count, int chunks,
                                                                                            int per, double* out) {
    __shared__ double s_p[kEmFinalEntries * kEmFinalChunks];
    const int t = threadIdx.x % kEmFinalEntries;
    const int c = threadIdx.x / kEmFinalEntries;
    const int entry = (int)blockIdx.x * kEmFinalEntries + t;
    double sum = 0.0;
    if (entry < count && c < chunks) {
        const int b1 = min(blocks, (c + 1) * per);
        const double* r = ws + entry;
        for (int b = c * per; b < b1; b += kEmFinalBatch) {   // a batch of loads in flight, added in order
            double v[kEmFinalBatch];
#pragma unroll
            for (int i = 0; i < kEmFinalBatch; ++i) v[i] = b + i < b1 ? r[(int64_t)(b + i) * count] : 0.0;
#pragma unroll
            for (int i = 0; i < kEmFinalBatch; ++i)
                if (b + i < b1) sum += v[i];
        }
    }
    s_p[c * kEmFinalEntries + t] = sum;
    __syncthreads();
    if (c == 0 && entry < count) {
        sum = s_p[t];
        for (int q = 1; q < chunks; ++q) sum += s_p[q * kEmFinalEntries + t];
        out[entry] = sum;
    }
}

template <int D>
hipError_t launch_em_d(const MixtureEmArgs& a, int grid, hipStream_t s) {
    const int groups = (a.k + em_cpb(D) - 1) / em_cpb(D);
    mixture_em_kernel<D><<<dim3((unsigned)grid, (unsigned)groups), kEmThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

// records the largest grid of a launch writes (host only: no HIP call)
static int64_t em_max_blocks(int64_t n, int d, int k) {
    const int64_t tiles = (n + kRows - 1) / kRows;
    const int groups = (k + em_cpb(d) - 1) / em_cpb(d);
    int64_t cap = kEmMaxBlocks / groups;
    if (cap < kEmMinBlocks) cap = kEmMinBlocks;
    return tiles < cap ? tiles : cap;
}

int64_t mixture_em_ws_bytes(int64_t n, int d, int k) { return em_max_blocks(n, d, k) * (1 + (int64_t)k * em_entries(d)) * 8; }

// a.n >= 1, 1 <= a.d <= kMixtureEmMaxDim, 1 <= a.k <= kMixtureEmMaxComponents, a.ws of
// mixture_em_ws_bytes(a.n, a.d, a.k) bytes (st_mixture_em_stats validates)
hipError_t launch_mixture_em(const MixtureEmArgs& a, hipStream_t s) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    // grid.x: a block per tile, at most kEmBlocksPerCu per CU over all component groups (grid.y), under the
    // st_tune grid cap (key 23 for this thread, else key 5) and the records the workspace holds
    const int groups = (a.k + em_cpb(a.d) - 1) / em_cpb(a.d);
    int64_t grid = (a.n + kRows - 1) / kRows;
    int64_t resident = (int64_t)cus * kEmBlocksPerCu / groups;
    if (resident < kEmMinBlocks) resident = kEmMinBlocks;
    if (grid > resident) grid = resident;
    const int cap = persistent_tune_get(23) > 0 ? persistent_tune_get(23) : persistent_tune_get(5);
    if (cap > 0 && grid > cap) grid = cap;
    if (grid > em_max_blocks(a.n, a.d, a.k)) grid = em_max_blocks(a.n, a.d, a.k);
    if (grid < 1) grid = 1;
    switch (a.d) {
        case 1: e = launch_em_d<1>(a, (int)grid, s); break;
        case 2: e = launch_em_d<2>(a, (int)grid, s); break;
        case 3: e = launch_em_d<3>(a, (int)grid, s); break;
        case 4: e = launch_em_d<4>(a, (int)grid, s); break;
        case 5: e = launch_em_d<5>(a, (int)grid, s); break;
        case 6: e = launch_em_d<6>(a, (int)grid, s); break;
        case 7: e = launch_em_d<7>(a, (int)grid, s); break;
        case 8: e = launch_em_d<8>(a, (int)grid, s); break;
        case 9: e = launch_em_d<9>(a, (int)grid, s); break;
        case 10: e = launch_em_d<10>(a, (int)grid, s); break;
        case 11: e = launch_em_d<11>(a, (int)grid, s); break;
        case 12: e = launch_em_d<12>(a, (int)grid, s); break;
        case 13: e = launch_em_d<13>(a, (int)grid, s); break;
        case 14: e = launch_em_d<14>(a, (int)grid, s); break;
        case 15: e = launch_em_d<15>(a, (int)grid, s); break;
        case 16: e = launch_em_d<16>(a, (int)grid, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    const int count = 1 + a.k * em_entries(a.d);
    const int chunks = (int)grid < kEmFinalChunks ? (int)grid : kEmFinalChunks;
    const int per = ((int)grid + chunks - 1) / chunks;
    mixture_em_final_kernel<<<dim3((unsigned)((count + kEmFinalEntries - 1) / kEmFinalEntries)),
                              kEmFinalEntries * kEmFinalChunks, 0, s>>>(a.ws, (int)grid, count, chunks, per, a.out);
    return hipGetLastError();
}

}  // namespace st
