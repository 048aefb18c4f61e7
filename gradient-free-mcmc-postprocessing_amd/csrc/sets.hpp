// Set-batched KSD and distance sums (included at the end of pairwise.hip): ONE resident problem, many
// arbitrary index sets over its rows, one result per set -- the reference's naive-thinning curves
// (Gaussian_mixture.ipynb: ksd_naive / naive_st over np.linspace(0, n - 1, m).astype(int), m = 1..1000;
// lotka_volterra/Comparison.ipynb: rw_ksd_naive / rw_energy_distance_naive over thinned_sizes), whose
// index sets are not nested, so the prefix forms (K6's cumulative scan, the energy curve) do not apply.
//
// Schedule.  The rows of all sets are first gathered, in the caller's order, into ONE concatenated
// compact SoA (set s occupies columns [off[s], off[s+1]) of it), so every later read is a coalesced
// stream as in K6 / K7.  Work items are (set, column block of kColBlock columns) pairs, listed in a
// table built on the host from the set offsets (sets_build_items), heaviest first; a block takes item
// blockIdx.x and never spans two sets.  Within an item the kernels are K6 / K7 on that set's slice:
// one thread per column j, rows staged in LDS, a sequential sum per column in increasing a, the same
// pair functions selected the same way -- so a set's column sums carry the bits of st_ksd_colsum on
// its compact subset.  The per-set finish is one block per set: thread t adds columns t, t + 256, ...
// in order, then a fixed binary tree over the 256 partials -- an order that depends on the set's size
// only.  No floating-point atomics, no differences of a global prefix sum, no inter-workgroup waits.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

namespace st {

// ---- work-item table (host) -----------------------------------------------------------------------
// pairs (a < j) of column block cb of a set of m rows: sum of j over its columns
static inline int64_t sets_item_work(int64_t m, int64_t cb) {
    const int64_t c0 = cb * kColBlock;
    const int64_t c1 = c0 + kColBlock < m ? c0 + kColBlock : m;
    return (c0 + c1 - 1) * (c1 - c0) / 2;
}

// 0 when off[0 .. n_sets] starts at 0 and increases strictly (no empty set), else which rule failed
int sets_check_offsets(const int64_t* off, int64_t n_sets) {
    if (off[0] != 0) return 1;
    for (int64_t s = 0; s < n_sets; ++s) {
        if (off[s + 1] < off[s]) return 2;
        if (off[s + 1] == off[s]) return 3;
    }
    return 0;
}

int64_t sets_item_count(const int64_t* off, int64_t n_sets) {
    int64_t c = 0;
    for (int64_t s = 0; s < n_sets; ++s) c += (off[s + 1] - off[s] + kColBlock - 1) / kColBlock;
    return c;
}

// items[2 q] = set, items[2 q + 1] = column block of work item q; non-increasing in sets_item_work,
// ties in (set, block) order
void sets_build_items(const int64_t* off, int64_t n_sets, int32_t* items) {
    struct Item { int64_t work; int32_t set, block; };
    std::vector<Item> v;
    v.reserve((size_t)sets_item_count(off, n_sets));
    for (int64_t s = 0; s < n_sets; ++s) {
        const int64_t m = off[s + 1] - off[s];
        for (int64_t cb = 0; cb * kColBlock < m; ++cb) v.push_back({sets_item_work(m, cb), (int32_t)s, (int32_t)cb});
    }
    std::stable_sort(v.begin(), v.end(), [](const Item& a, const Item& b) { return a.work > b.work; });
    for (size_t q = 0; q < v.size(); ++q) {
        items[2 * q] = v[q].set;
        items[2 * q + 1] = v[q].block;
    }
}

// ---- gather ---------------------------------------------------------------------------------------
// dst[k * ldd + j] = src[k * lds + rows[j]], k < nvec, j < total (a row outside [0, n) gives NaN: the
// caller validates the indices; nothing is read out of bounds)
__global__ __launch_bounds__(256) void sets_gather_kernel(const double* __restrict__ src, int64_t lds, int64_t n,
                                                          int nvec, const int64_t* __restrict__ rows,
                                                          int64_t total, double* __restrict__ dst, int64_t ldd) {
    const int64_t work = total * nvec;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < work;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / total, j = e - k * total;
        const int64_t r = rows[j];
        dst[k * ldd + j] = (r >= 0 && r < n) ? src[k * lds + r] : __builtin_nan("");
    }
}

struct SetsArgs {
    const double* x;        // concatenated compact SoA (d, ld); distance kernels: the points
    const double* g;
    const double* w;
    int64_t ld;
    double l, tr;
    const int64_t* off;     // device copy of the set offsets (n_sets + 1)
    const int32_t* items;   // work items {set, column block}
    double* csum;           // (total rows) column sums, in the concatenated order
    int compact;
};

// ---- ragged-triangle KSD: ksd_colsum_kernel on the slice of one work item -------------------------
template <int D, bool GF>
__global__ __launch_bounds__(kColBlock, 4) void ksd_sets_colsum_kernel(SetsArgs p) {
    constexpr int R = kColBlock;
    __shared__ double sx[D][R];
    __shared__ double sg[D][R];
    __shared__ double sw[GF ? R : 1];
    const int tid = threadIdx.x;
    const int64_t set = p.items[2 * (int64_t)blockIdx.x], cb = p.items[2 * (int64_t)blockIdx.x + 1];
    const int64_t base = p.off[set], m = p.off[set + 1] - base;
    const double* __restrict__ px = p.x + base;
    const double* __restrict__ pg = p.g + base;
    const double* __restrict__ pw = GF ? p.w + base : nullptr;
    const int64_t c0 = cb * R;
    const int64_t i = c0 + tid;
    const int64_t ld = p.ld;
    double xi[D], gi[D];
    const bool live = i < m;
    int cok = fast_range_ok(p.l) & (int)(p.l > 0.0) & (int)(p.tr > 0.0) & (int)(p.tr <= 0x1p64);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xi[k] = live ? px[k * ld + i] : 0.0;
        gi[k] = live ? pg[k * ld + i] : 0.0;
        cok &= fast_range_ok(xi[k]) & fast_range_ok(gi[k]);
    }
    double wi = 1.0;
    if constexpr (GF) wi = live ? pw[i] : 1.0;
    const double l = p.l, l2 = p.l * p.l, m3l2 = -3.0 * l2, tr = p.tr;
    const bool col_ok = cok != 0;
    const int col_fast = __syncthreads_and(cok);
    const int64_t a_stop = m < c0 + R ? m : c0 + R;   // rows a < i <= c0 + R - 1
    double acc = 0.0;
    for (int64_t ac = 0; ac < a_stop; ac += R) {
        const int64_t a = ac + tid;
        int rok = 1;
        __syncthreads();
        if (a < a_stop) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double xv = px[k * ld + a], gv = pg[k * ld + a];
                sx[k][tid] = xv;
                sg[k][tid] = gv;
                rok &= fast_range_ok(xv) & fast_range_ok(gv);
            }
            if constexpr (GF) sw[tid] = pw[a];
        }
        const int fast = __syncthreads_and(rok) & col_fast;
        const int cnt = (int)((a_stop - ac) < R ? (a_stop - ac) : R);
        const bool below = ac + cnt <= c0;
        // AR as in ksd_colsum_kernel: 0 exact general, 1 exact range-guarded (same bits), 2 compact,
        // 3 compact per pair -- a pair's bits depend on the pair and the setting only
        auto sweep = [&](auto ar_tag, auto below_tag) {
            constexpr int AR = decltype(ar_tag)::value;
            constexpr bool BELOW = decltype(below_tag)::value;
            asm volatile(";; sets colsum variant" ::);
            auto pair_at = [&](int e) -> double {
                double xa[D], ga[D];
#pragma unroll
                for (int k = 0; k < D; ++k) { xa[k] = sx[k][e]; ga[k] = sg[k][e]; }
                double kv;
                if constexpr (AR == 2) kv = pair_compact_ct<D>(xi, gi, xa, ga, l, m3l2, tr);
                else if constexpr (AR == 3)
                    kv = pair_value_sel<D>(col_ok && row_in_range<D>(xa, ga), xi, gi, xa, ga, l, l2, m3l2, tr);
                else kv = pair_value_ct<D, AR == 1>(xi, gi, xa, ga, l, l2, tr);
                if constexpr (GF) kv = (kv * wi) * sw[e];
                return kv;
            };
            int e = 0;
            for (; e + kColsumUnroll <= cnt; e += kColsumUnroll) {
                double kv[kColsumUnroll];
#pragma unroll
                for (int u = 0; u < kColsumUnroll; ++u) kv[u] = pair_at(e + u);
#pragma unroll
                for (int u = 0; u < kColsumUnroll; ++u) {
                    if constexpr (BELOW) acc = acc + kv[u];
                    else acc = (ac + e + u < i) ? acc + kv[u] : acc;
                }
            }
            for (; e < cnt; ++e) {
                const double kv = pair_at(e);
                if constexpr (BELOW) acc = acc + kv;
                else acc = (ac + e < i) ? acc + kv : acc;
            }
        };
        using C0 = std::integral_constant<int, 0>;
        using C1 = std::integral_constant<int, 1>;
        using C2 = std::integral_constant<int, 2>;
        using C3 = std::integral_constant<int, 3>;
        if (fast && p.compact) {
            if (below) sweep(C2{}, std::true_type{});
            else sweep(C2{}, std::false_type{});
        } else if (p.compact) {
            if (below) sweep(C3{}, std::true_type{});
            else sweep(C3{}, std::false_type{});
        } else if (fast) {
            if (below) sweep(C1{}, std::true_type{});
            else sweep(C1{}, std::false_type{});
        } else {
            if (below) sweep(C0{}, std::true_type{});
            else sweep(C0{}, std::false_type{});
        }
    }
    if (live) p.csum[base + i] = acc;
}

// d > 8: ksd_colsum_rt_kernel on the slice of one work item
template <bool GF>
__global__ __launch_bounds__(kColBlock) void ksd_sets_colsum_rt_kernel(SetsArgs p, int d) {
    __shared__ double srow[2 * kMaxDim][kRowsRt];
    __shared__ double sw[kRowsRt];
    const int tid = threadIdx.x;
    const int64_t set = p.items[2 * (int64_t)blockIdx.x], cb = p.items[2 * (int64_t)blockIdx.x + 1];
    const int64_t base = p.off[set], m = p.off[set + 1] - base;
    const double* __restrict__ px = p.x + base;
    const double* __restrict__ pg = p.g + base;
    const double* __restrict__ pw = GF ? p.w + base : nullptr;
    const int64_t c0 = cb * kColBlock;
    const int64_t i = c0 + tid;
    const int64_t ld = p.ld;
    const bool live = i < m;
    const int64_t ic = live ? i : 0;
    double wi = 1.0;
    if constexpr (GF) wi = live ? pw[i] : 1.0;
    const double l = p.l, l2 = p.l * p.l, tr = p.tr;
    const int64_t a_stop = m < c0 + kColBlock ? m : c0 + kColBlock;
    double acc = 0.0;
    for (int64_t ac = 0; ac < a_stop; ac += kRowsRt) {
        const int cnt = (int)((a_stop - ac) < kRowsRt ? (a_stop - ac) : kRowsRt);
        __syncthreads();
        for (int e = tid; e < 2 * d * kRowsRt; e += kColBlock) {
            const int k = e / kRowsRt, r = e % kRowsRt;
            if (r < cnt) srow[k][r] = k < d ? px[(int64_t)k * ld + ac + r] : pg[(int64_t)(k - d) * ld + ac + r];
        }
        if constexpr (GF) {
            if (tid < cnt) sw[tid] = pw[ac + tid];
        }
        __syncthreads();
        for (int e = 0; e < cnt; ++e) {
            double kv = pair_value_rt(px + ic, pg + ic, ld, &srow[0][e], &srow[d][e], kRowsRt, d, l, l2, tr);
            if constexpr (GF) kv = (kv * wi) * sw[e];
            acc = (ac + e < i) ? acc + kv : acc;
        }
    }
    if (live) p.csum[base + i] = acc;
}

// 256 per-thread partials -> one sum, a fixed binary tree (block-wide; the result in every thread)
__device__ __forceinline__ double sets_tree_sum(double v, double* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int h = kColBlock / 2; h > 0; h >>= 1) {
        if (tid < h) s[tid] = s[tid] + s[tid + h];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// ks[s] = sqrt(sum_j (2 csum[j] + k(r_j, r_j))) / m_s; one block per set
__global__ __launch_bounds__(kColBlock) void ksd_sets_finish_kernel(SetsArgs p, int d, double* __restrict__ ks) {
    __shared__ double s_red[kColBlock];
    const int64_t set = blockIdx.x;
    const int64_t base = p.off[set], m = p.off[set + 1] - base;
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < m; j += kColBlock) {
        double kd = diag_value_rt(p.g + base + j, p.ld, d, p.tr);
        if (p.w) {
            const double wj = p.w[base + j];
            kd = (kd * wj) * wj;
        }
        acc += 2.0 * p.csum[base + j] + kd;
    }
    const double tot = sets_tree_sum(acc, s_red);
    if (threadIdx.x == 0) ks[set] = __builtin_sqrt(tot) / (double)m;
}

// ---- ragged-triangle distance sums: K7's arithmetic (one partial sum) on the slice of one item ----
template <int D>
__global__ __launch_bounds__(kColBlock, 4) void dist_sets_colsum_kernel(SetsArgs p) {
    constexpr int R = kColBlock;
    __shared__ double sb[D][R];
    const int tid = threadIdx.x;
    const int64_t set = p.items[2 * (int64_t)blockIdx.x], cb = p.items[2 * (int64_t)blockIdx.x + 1];
    const int64_t base = p.off[set], m = p.off[set + 1] - base;
    const double* __restrict__ pp = p.x + base;
    const int64_t ld = p.ld;
    const int64_t c0 = cb * R;
    const int64_t i = c0 + tid;
    const bool live = i < m;
    double ai[D];
    int aok = 1;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        ai[k] = live ? pp[k * ld + i] : 0.0;
        aok &= fast_range_ok(ai[k]);
    }
    const int64_t b_stop = m < c0 + R ? m : c0 + R;
    double acc = 0.0;
    for (int64_t bc = 0; bc < b_stop; bc += R) {
        __syncthreads();
        const int64_t bb = bc + tid;
        int tok = aok;
        if (bb < b_stop) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double v = pp[k * ld + bb];
                sb[k][tid] = v;
                tok &= fast_range_ok(v);
            }
        }
        const bool fast = __syncthreads_and(tok) != 0;
        const int cnt = (int)((b_stop - bc) < R ? (b_stop - bc) : R);
        const bool below = bc + cnt <= c0;
        auto tile = [&](auto fast_tag, auto below_tag) {
            constexpr bool FAST = decltype(fast_tag)::value, BELOW = decltype(below_tag)::value;
            for (int e = 0; e < cnt; ++e) {
                double ss = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double dk = ai[k] - sb[k][e];
                    ss += dk * dk;
                }
                double dist;
                if constexpr (FAST) dist = fast_dist<false>(ss);
                else dist = __builtin_sqrt(ss);
                if constexpr (BELOW) acc = acc + dist;
                else acc = (bc + e < i) ? acc + dist : acc;
            }
        };
        if (fast) {
            if (below) tile(std::true_type{}, std::true_type{});
            else tile(std::true_type{}, std::false_type{});
        } else {
            if (below) tile(std::false_type{}, std::true_type{});
            else tile(std::false_type{}, std::false_type{});
        }
    }
    if (live) p.csum[base + i] = acc;
}

__global__ __launch_bounds__(kColBlock) void dist_sets_colsum_rt_kernel(SetsArgs p, int d) {
    constexpr int R = kRowsRt;
    __shared__ double sb[kMaxDim][R];
    const int tid = threadIdx.x;
    const int64_t set = p.items[2 * (int64_t)blockIdx.x], cb = p.items[2 * (int64_t)blockIdx.x + 1];
    const int64_t base = p.off[set], m = p.off[set + 1] - base;
    const double* __restrict__ pp = p.x + base;
    const int64_t ld = p.ld;
    const int64_t c0 = cb * kColBlock;
    const int64_t i = c0 + tid;
    const bool live = i < m;
    const int64_t ic = live ? i : 0;
    const int64_t b_stop = m < c0 + kColBlock ? m : c0 + kColBlock;
    double acc = 0.0;
    for (int64_t bc = 0; bc < b_stop; bc += R) {
        const int cnt = (int)((b_stop - bc) < R ? (b_stop - bc) : R);
        __syncthreads();
        for (int e = tid; e < d * R; e += kColBlock) {
            const int k = e / R, r = e % R;
            if (r < cnt) sb[k][r] = pp[(int64_t)k * ld + bc + r];
        }
        __syncthreads();
        for (int e = 0; e < cnt; ++e) {
            double ss = 0.0;
            for (int k = 0; k < d; ++k) {
                const double dk = pp[(int64_t)k * ld + ic] - sb[k][e];
                ss += dk * dk;
            }
            const double dist = __builtin_sqrt(ss);
            acc = (bc + e < i) ? acc + dist : acc;
        }
    }
    if (live) p.csum[base + i] = acc;
}

// self_out[s] = sum_j colsum[j] over the set's columns; segsum_out[s] = sum_j row_values[rows[j]]
// (the per-row cross sums, computed once per unique row by the caller); one block per set
__global__ __launch_bounds__(kColBlock) void dist_sets_finish_kernel(const int64_t* __restrict__ off,
                                                                     const double* __restrict__ colsum,
                                                                     const int64_t* __restrict__ rows, int64_t n,
                                                                     const double* __restrict__ row_values,
                                                                     double* __restrict__ self_out,
                                                                     double* __restrict__ segsum_out) {
    __shared__ double s_red[kColBlock];
    const int64_t set = blockIdx.x;
    const int64_t base = off[set], m = off[set + 1] - base;
    double acc = 0.0, seg = 0.0;
    for (int64_t j = threadIdx.x; j < m; j += kColBlock) {
        acc += colsum[base + j];
        if (segsum_out) {
            const int64_t r = rows[base + j];
            seg += (r >= 0 && r < n) ? row_values[r] : __builtin_nan("");
        }
    }
    const double tot = sets_tree_sum(acc, s_red);
    if (threadIdx.x == 0) self_out[set] = tot;
    if (segsum_out) {   // kernel argument: block-uniform
        const double st = sets_tree_sum(seg, s_red);
        if (threadIdx.x == 0) segsum_out[set] = st;
    }
}

// ---- host: workspace layout and launch sequences ---------------------------------------------------
// [offsets (n_sets + 1) int64][items 2 x int32 each, at most total / kColBlock + n_sets][compact SoA:
// nvec vectors of ldc doubles][column sums: ldc doubles], every part 16-byte aligned
static inline int64_t sets_align16(int64_t b) { return (b + 15) & ~int64_t(15); }
static inline int64_t sets_ldc(int64_t total) { return (total + 7) & ~int64_t(7); }
static inline int64_t sets_max_items(int64_t total, int64_t n_sets) { return total / kColBlock + n_sets; }

int64_t sets_ws_bytes(int64_t total, int64_t n_sets, int nvec) {
    return sets_align16((n_sets + 1) * 8) + sets_align16(sets_max_items(total, n_sets) * 8) +
           ((int64_t)nvec + 1) * sets_ldc(total) * 8;
}

struct SetsPlan {
    int64_t* off;
    int32_t* items;
    double* soa;
    double* colsum;
    int64_t ldc, n_items;
};

// carve the workspace, build the table and queue its ONE copy to the device
static hipError_t sets_prepare(const int64_t* set_offsets, int64_t n_sets, void* ws, SetsPlan& pl, int nvec,
                               hipStream_t s) {
    const int64_t total = set_offsets[n_sets];
    char* base = static_cast<char*>(ws);
    const int64_t off_bytes = sets_align16((n_sets + 1) * 8);
    pl.off = reinterpret_cast<int64_t*>(base);
    pl.items = reinterpret_cast<int32_t*>(base + off_bytes);
    pl.soa = reinterpret_cast<double*>(base + off_bytes + sets_align16(sets_max_items(total, n_sets) * 8));
    pl.ldc = sets_ldc(total);
    pl.colsum = pl.soa + (int64_t)nvec * pl.ldc;
    pl.n_items = sets_item_count(set_offsets, n_sets);
    // offsets and items leave in one copy (the two regions are adjacent in the workspace); the source
    // is ordinary host memory, which the runtime has read by the time the copy call returns
    std::vector<char> host((size_t)(off_bytes + pl.n_items * 8), 0);
    memcpy(host.data(), set_offsets, (size_t)(n_sets + 1) * 8);
    sets_build_items(set_offsets, n_sets, reinterpret_cast<int32_t*>(host.data() + off_bytes));
    return hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, s);
}

static int sets_gather_grid(int64_t work) {
    int64_t b = (work + 255) / 256;
    if (b > 4096) b = 4096;
    return (int)(b < 1 ? 1 : b);
}

template <int D>
static void launch_ksd_sets_ct(const SetsArgs& a, unsigned grid, hipStream_t s) {
    if (a.w) ksd_sets_colsum_kernel<D, true><<<grid, kColBlock, 0, s>>>(a);
    else ksd_sets_colsum_kernel<D, false><<<grid, kColBlock, 0, s>>>(a);
}

hipError_t launch_ksd_sets(const PairArgs& p, int64_t n, const int64_t* rows, const int64_t* set_offsets,
                           int64_t n_sets, double* ks_out, double* csum_out, void* ws, hipStream_t s) {
    const int d = p.d;
    const int nvec = 2 * d + 1;
    SetsPlan pl;
    hipError_t e = sets_prepare(set_offsets, n_sets, ws, pl, nvec, s);
    if (e != hipSuccess) return e;
    const int64_t total = set_offsets[n_sets];
    double* cx = pl.soa;
    double* cg = pl.soa + (int64_t)d * pl.ldc;
    double* cw = p.w ? pl.soa + (int64_t)2 * d * pl.ldc : nullptr;
    sets_gather_kernel<<<sets_gather_grid(total * d), 256, 0, s>>>(p.x, p.ld, n, d, rows, total, cx, pl.ldc);
    sets_gather_kernel<<<sets_gather_grid(total * d), 256, 0, s>>>(p.g, p.ld, n, d, rows, total, cg, pl.ldc);
    if (p.w) sets_gather_kernel<<<sets_gather_grid(total), 256, 0, s>>>(p.w, p.ld, n, 1, rows, total, cw, pl.ldc);
    SetsArgs a{cx, cg, cw, pl.ldc, p.l, p.tr, pl.off, pl.items, csum_out ? csum_out : pl.colsum, arith_compact()};
    const unsigned grid = (unsigned)pl.n_items;
    switch (d) {
        case 1: launch_ksd_sets_ct<1>(a, grid, s); break;
        case 2: launch_ksd_sets_ct<2>(a, grid, s); break;
        case 3: launch_ksd_sets_ct<3>(a, grid, s); break;
        case 4: launch_ksd_sets_ct<4>(a, grid, s); break;
        case 5: launch_ksd_sets_ct<5>(a, grid, s); break;
        case 6: launch_ksd_sets_ct<6>(a, grid, s); break;
        case 7: launch_ksd_sets_ct<7>(a, grid, s); break;
        case 8: launch_ksd_sets_ct<8>(a, grid, s); break;
        default:
            if (a.w) ksd_sets_colsum_rt_kernel<true><<<grid, kColBlock, 0, s>>>(a, d);
            else ksd_sets_colsum_rt_kernel<false><<<grid, kColBlock, 0, s>>>(a, d);
            break;
    }
    ksd_sets_finish_kernel<<<(unsigned)n_sets, kColBlock, 0, s>>>(a, d, ks_out);
    return hipGetLastError();
}

hipError_t launch_distance_sets(const double* pts, int64_t ldp, int64_t n, int d, const int64_t* rows,
                                const int64_t* set_offsets, int64_t n_sets, double* self_out,
                                const double* row_values, double* segsum_out, void* ws, hipStream_t s) {
    SetsPlan pl;
    hipError_t e = sets_prepare(set_offsets, n_sets, ws, pl, d, s);
    if (e != hipSuccess) return e;
    const int64_t total = set_offsets[n_sets];
    sets_gather_kernel<<<sets_gather_grid(total * d), 256, 0, s>>>(pts, ldp, n, d, rows, total, pl.soa, pl.ldc);
    SetsArgs a{pl.soa, nullptr, nullptr, pl.ldc, 0.0, 0.0, pl.off, pl.items, pl.colsum, 0};
    const unsigned grid = (unsigned)pl.n_items;
    switch (d) {
        case 1: dist_sets_colsum_kernel<1><<<grid, kColBlock, 0, s>>>(a); break;
        case 2: dist_sets_colsum_kernel<2><<<grid, kColBlock, 0, s>>>(a); break;
        case 3: dist_sets_colsum_kernel<3><<<grid, kColBlock, 0, s>>>(a); break;
        case 4: dist_sets_colsum_kernel<4><<<grid, kColBlock, 0, s>>>(a); break;
        case 5: dist_sets_colsum_kernel<5><<<grid, kColBlock, 0, s>>>(a); break;
        case 6: dist_sets_colsum_kernel<6><<<grid, kColBlock, 0, s>>>(a); break;
        case 7: dist_sets_colsum_kernel<7><<<grid, kColBlock, 0, s>>>(a); break;
        case 8: dist_sets_colsum_kernel<8><<<grid, kColBlock, 0, s>>>(a); break;
        default: dist_sets_colsum_rt_kernel<<<grid, kColBlock, 0, s>>>(a, d); break;
    }
    dist_sets_finish_kernel<<<(unsigned)n_sets, kColBlock, 0, s>>>(pl.off, pl.colsum, rows, n, row_values,
                                                                   self_out, segsum_out);
    return hipGetLastError();
}

}  // namespace st
