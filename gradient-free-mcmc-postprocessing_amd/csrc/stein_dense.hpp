// Per-pair IMQ Stein-kernel arithmetic for a dense, symmetric positive-definite preconditioner
// Gamma^-1 = L (the reference's vfk0_imq takes any linv; 'smpcov' is the inverse sample covariance).
//
// One definition, used by every dense kernel (greedy step, pair list, Gram matrix, KSD column sums),
// so a pair's bits never depend on the path that evaluates it.  With dx = xi - xj, ds = gi - gj:
//   y_r = FMA_k L[r][k] dx_k          (first term a plain product, then one fma per k, k ascending)
//   qs  = FMA_r y_r dx_r     t1s = FMA_r y_r y_r     t2s = FMA_r y_r ds_r     (r ascending)
//   t3s = PAIRWISE_k fl(gi_k gj_k)    (NumPy pairwise_sum order, as pair_value_ct / pair_value_rt)
//   k   = finish_pair(qs, t1s, t2s, t3s, tr)         tr = np.trace(L), from the host
// This is the reference's formula (oracle/stein_numpy.py vfk0_imq) with two changes that hold only
// for symmetric L: dx' L^2 dx is evaluated as |L dx|^2 (d more fma instead of a second d^2 product,
// and a sum of squares: no cancellation), and (L ds) . dx as (L dx) . ds.
// Swapping i and j negates dx, ds and y exactly, so k(i, j) and k(j, i) are bit-identical.
// The diagonal is diag_value_ct / diag_value_rt (stein_math.hpp): it depends on tr only.
// There is one dense arithmetic: st_tune key 11 (compact / exact) and the near-tie guard do not
// apply to it.  Compile with -ffp-contract=off like the rest.
//
// Widths: compile-time D = 1 .. 8, and one padded width 16 for d = 9 .. 16 -- rows and L are
// zero-padded in registers, which adds exact zeros to every chain (t3s follows the true d).
// L is read through a block-uniform pointer to d * d doubles, row-major (D <= 8: scalar loads of the
// caller's array; width 16: each block first copies it, zero-padded to 16 x 16, into LDS).
#pragma once
#include "stein_math.hpp"
#include "stein_internal.hpp"

#pragma clang fp contract(off)

namespace st {

// t3s of d real coordinates held in D >= d registers (the padding is never read)
template <int D>
__device__ __forceinline__ double dense_t3(const double (&gi)[D], const double (&gj)[D], int d) {
    double t3s;
    if constexpr (D < 8) {
        t3s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) t3s += gi[k] * gj[k];
    } else {
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = gi[k] * gj[k];
        if constexpr (D == 16) {
            if (d == 16) {   // two full lanes of eight
#pragma unroll
                for (int k = 8; k < 16; ++k) r[k - 8] += gi[k] * gj[k];
            }
        }
        t3s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        if constexpr (D == 16) {
            if (d < 16) {    // d = 9 .. 15: the remainder follows the eight lanes one by one
#pragma unroll
                for (int k = 8; k < 15; ++k)
                    if (k < d) t3s += gi[k] * gj[k];
            }
        }
    }
    return t3s;
}

// Row r of L for the pair being evaluated: the same address behind an offset the compiler cannot see
// through, tied to a value of this pair (the previous rows' t1s).  Without it the loop-invariant loads
// of L are hoisted out of the loop over pairs into D * D live registers (D = 8: 250 VGPRs, D = 16:
// scratch); with it a row is loaded next to its use -- scalar loads (UNIFORM: the caller's array) or
// LDS broadcast reads (the padded copy) -- and at most a row or two of L is live.  Not volatile: the
// chains of different pairs stay independent for the scheduler.
// UNIFORM reads go through the constant address space (L is never written while a kernel runs), which is
// what lets a uniform address next to the kernel's own stores be a scalar load.
typedef const __attribute__((address_space(4))) double* ConstF64Ptr;

template <bool UNIFORM>
__device__ __forceinline__ auto dense_linv_row(const double* Lrow, double dep) {
    int off = 0;
    if constexpr (UNIFORM) {   // a wave-uniform tie, so the address stays scalar
        const int u = __builtin_amdgcn_readfirstlane((int)__double_as_longlong(dep));
        asm("" : "+s"(off) : "s"(u));
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        return (ConstF64Ptr)(Lrow + off);
#pragma clang diagnostic pop
    } else {
        asm("" : "+v"(off) : "v"(dep));
        return Lrow + off;
    }
}

// xi, gi, xj, gj: D registers each, entries k >= d zero.  Lp: D x D doubles, row-major, block-uniform:
// the caller's d x d array itself for D <= 8 (D == d); for the padded width the kernel's zero-padded
// LDS copy (stage_dense_linv) -- rows r >= d and columns k >= d are zero, so y_r = 0 there and every
// padded product adds an exact zero
template <int D, bool UNIFORM>
__device__ __forceinline__ double pair_dense(const double (&xi)[D], const double (&gi)[D],
                                             const double (&xj)[D], const double (&gj)[D],
                                             const double* __restrict__ Lp, int d, double tr) {
    static_assert(D <= 8 || D == kMaxDenseDim, "dense widths: 1 .. 8 and 16");
    double dx[D], ds[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        dx[k] = xi[k] - xj[k];
        ds[k] = gi[k] - gj[k];
    }
    double qs = 0.0, t1s = 0.0, t2s = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        const auto Lr = dense_linv_row<UNIFORM>(Lp + r * D, r == 0 ? dx[0] : t1s);
        double y = Lr[0] * dx[0];
#pragma unroll
        for (int k = 1; k < D; ++k) y = __builtin_fma(Lr[k], dx[k], y);
        if (r == 0) {
            qs = y * dx[0]; t1s = y * y; t2s = y * ds[0];
        } else {
            qs = __builtin_fma(y, dx[r], qs);
            t1s = __builtin_fma(y, y, t1s);
            t2s = __builtin_fma(y, ds[r], t2s);
        }
    }
    return finish_pair(qs, t1s, t2s, dense_t3<D>(gi, gj, d), tr);
}

// zero-padded 16 x 16 copy of the d x d array L in LDS (one per block; the caller synchronises)
__device__ __forceinline__ void stage_dense_linv(const double* __restrict__ L, int d, double* s_L) {
    for (int e = threadIdx.x; e < kMaxDenseDim * kMaxDenseDim; e += blockDim.x) {
        const int r = e / kMaxDenseDim, k = e % kMaxDenseDim;
        s_L[e] = (r < d && k < d) ? L[r * d + k] : 0.0;
    }
}

// row i of an SoA (d, ld) array into D registers, zero beyond d
template <int D>
__device__ __forceinline__ void load_row_padded(const double* __restrict__ col, int64_t ld, int d,
                                                double (&out)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if constexpr (D <= 8) out[k] = col[k * ld];
        else out[k] = k < d ? col[k * ld] : 0.0;
    }
}

}  // namespace st
