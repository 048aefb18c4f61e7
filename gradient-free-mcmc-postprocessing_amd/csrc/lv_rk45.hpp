// scipy's RK45 (Dormand-Prince) for the Lotka-Volterra systems, one integration per thread: the only copy
// of the integrator that lv.hip (gradient, log density) and lv_mcmc.hip (sampler) run.  Step for step
// scipy's algorithm: initial step selection (common.select_initial_step), the accept / reject loop of
// RungeKutta._step_impl (SAFETY 0.9, factors in [0.2, 10], error exponent -1/5, RMS error norm), the tableau
// as scipy holds it (rk45_tableau.hpp, generated), and dense output y = h Q p(x) + y_old per accepted step
// with OdeSolution's segment rule (t in (t_j, t_j+1] -> segment j).  Every function is inlined into its
// kernel; the order of the operations is part of the contract (the build has -ffp-contract=off and the only
// fused multiply-adds are the explicit ones of the Horner form).
#pragma once

#include <hip/hip_runtime.h>

#include "rk45_tableau.hpp"
#include "stein_internal.hpp"

namespace st {

// NS = 2: the system itself; NS = 10: with the forward sensitivities du/dtheta (2 x 4, row-major)
template <int NS>
__device__ __forceinline__ void lv_rhs(const double th[4], const double* y, double* f) {
    const double th1 = th[0], th2 = th[1], th3 = th[2], th4 = th[3];
    const double u1 = y[0], u2 = y[1];
    f[0] = th1 * u1 - th2 * u1 * u2;
    f[1] = th4 * u1 * u2 - th3 * u2;
    if constexpr (NS == 10) {
        const double w1 = y[2], w2 = y[3], w3 = y[4], w4 = y[5];
        const double w5 = y[6], w6 = y[7], w7 = y[8], w8 = y[9];
        f[2] = u1 + (th1 - th2 * u2) * w1 - th2 * u1 * w5;
        f[3] = -u1 * u2 + (th1 - th2 * u2) * w2 - th2 * u1 * w6;
        f[4] = (th1 - th2 * u2) * w3 - th2 * u1 * w7;
        f[5] = (th1 - th2 * u2) * w4 - th2 * u1 * w8;
        f[6] = th4 * u2 * w1 + (th4 * u1 - th3) * w5;
        f[7] = th4 * u2 * w2 + (th4 * u1 - th3) * w6;
        f[8] = -u2 + th4 * u2 * w3 + (th4 * u1 - th3) * w7;
        f[9] = u1 * u2 + th4 * u2 * w4 + (th4 * u1 - th3) * w8;
    }
}

// scipy common.norm: np.linalg.norm(x) / x.size ** 0.5
template <int NS>
__device__ __forceinline__ double rms(const double* v) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) s += v[i] * v[i];
    return sqrt(s) / sqrt((double)NS);
}

// common.select_initial_step (order = error estimator order 4, max_step = inf, direction +1); f = rhs(y)
template <int NS>
__device__ __forceinline__ double select_initial_step(const double th[4], const double* y, const double* f,
                                                      double interval, double rtol, double atol) {
    double sc[NS], v[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) sc[c] = atol + fabs(y[c]) * rtol;
#pragma unroll
    for (int c = 0; c < NS; ++c) v[c] = y[c] / sc[c];
    const double d0 = rms<NS>(v);
#pragma unroll
    for (int c = 0; c < NS; ++c) v[c] = f[c] / sc[c];
    const double d1 = rms<NS>(v);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h0 = fmin(h0, interval);
    double y1[NS], f1[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) y1[c] = y[c] + h0 * 1.0 * f[c];
    lv_rhs<NS>(th, y1, f1);
#pragma unroll
    for (int c = 0; c < NS; ++c) v[c] = (f1[c] - f[c]) / sc[c];
    const double d2 = rms<NS>(v) / h0;
    double h1;
    if (d1 <= 1e-15 && d2 <= 1e-15) h1 = fmax(1e-6, h0 * 1e-3);
    else h1 = pow(0.01 / fmax(d1, d2), 1.0 / (rk45::kOrder + 1));
    return fmin(fmin(100 * h0, h1), interval);   // max_step = inf
}

// the dense output of one accepted step at x = (t - t_old) / h, p = (x, x^2, x^3, x^4) in Horner form
template <int NS>
__device__ __forceinline__ void lv_horner(double x, const double* y_old, const double (*Q)[rk45::kDenseOrder],
                                          double* u) {
    static_assert(rk45::kDenseOrder == 4, "Horner form below is written for RK45's quartic");
#pragma unroll
    for (int c = 0; c < NS; ++c)
        u[c] = __builtin_fma(x, __builtin_fma(x, __builtin_fma(x, __builtin_fma(x, Q[c][3], Q[c][2]), Q[c][1]),
                                              Q[c][0]), y_old[c]);
}

// Integrates u' = lv_rhs(u) from p.u0 (sensitivities from 0) over [p.t0, p.t1] and calls
//   on_step(t_old, t_new, inv_hd, y_old, Q, last) -> int
// after every accepted step: y(t) = lv_horner(x = (t - t_old) * inv_hd, y_old, Q) on (t_old, t_new]; `last`
// marks the step that reaches p.t1 (it takes every point that is left).  A non-zero return ends the
// integration with that status.  Returns the status: 0 finished, 1 step size below min_step, 2 p.max_steps
// accepted steps taken without reaching p.t1 (scipy would go on), or on_step's.
template <int NS, class OnStep>
__device__ __forceinline__ int lv_integrate(const double th[4], const LvProblem& p, OnStep&& on_step) {
    const double rtol = p.rtol, atol = p.atol;
    double y[NS], f[NS], K[rk45::kStages + 1][NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) y[c] = c < 2 ? p.u0[c] : 0.0;
    double t = p.t0;
    const double t_bound = p.t1;
    lv_rhs<NS>(th, y, f);
    double h_abs = select_initial_step<NS>(th, y, f, fabs(t_bound - t), rtol, atol);
    int status = 0;
    for (int64_t step = 0;; ++step) {
        if (t == t_bound) break;      // OdeSolver.step: finished
        if (__builtin_expect(step >= p.max_steps, 0)) { status = 2; break; }
        const double min_step = 10 * fabs(nextafter(t, INFINITY) - t);
        if (h_abs < min_step) h_abs = min_step;   // (h_abs > max_step = inf never)
        bool rejected = false;
        double t_new, h, y_new[NS], f_new[NS];
        for (;;) {
            if (__builtin_expect(h_abs < min_step, 0)) { status = 1; break; }
            h = h_abs;
            t_new = t + h;
            if (t_new - t_bound > 0) t_new = t_bound;
            h = t_new - t;
            h_abs = fabs(h);
            // rk_step
#pragma unroll
            for (int c = 0; c < NS; ++c) K[0][c] = f[c];
#pragma unroll
            for (int s = 1; s < rk45::kStages; ++s) {
                double ys[NS];
#pragma unroll
                for (int c = 0; c < NS; ++c) {
                    double dy = K[0][c] * rk45::A[s][0];
#pragma unroll
                    for (int j = 1; j < s; ++j) dy += K[j][c] * rk45::A[s][j];
                    ys[c] = y[c] + dy * h;
                }
                lv_rhs<NS>(th, ys, K[s]);
            }
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double bsum = K[0][c] * rk45::B[0];
#pragma unroll
                for (int j = 1; j < rk45::kStages; ++j) bsum += K[j][c] * rk45::B[j];
                y_new[c] = y[c] + h * bsum;
            }
            lv_rhs<NS>(th, y_new, f_new);
#pragma unroll
            for (int c = 0; c < NS; ++c) K[rk45::kStages][c] = f_new[c];
            double ev[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double e = K[0][c] * rk45::E[0];
#pragma unroll
                for (int j = 1; j <= rk45::kStages; ++j) e += K[j][c] * rk45::E[j];
                const double scale = atol + fmax(fabs(y[c]), fabs(y_new[c])) * rtol;
                ev[c] = e * h / scale;
            }
            const double error_norm = rms<NS>(ev);
            if (error_norm < 1) {
                double factor = error_norm == 0 ? rk45::kMaxFactor
                                                : fmin(rk45::kMaxFactor, rk45::kSafety * pow(error_norm, rk45::kErrorExponent));
                if (rejected) factor = fmin(1.0, factor);
                h_abs *= factor;
                break;
            }
            h_abs *= fmax(rk45::kMinFactor, rk45::kSafety * pow(error_norm, rk45::kErrorExponent));
            rejected = true;
        }
        if (status) break;
        // dense output of this step: Q = K^T P.  scipy evaluates h Q p(x) + y_old with p = (x, x^2, x^3, x^4);
        // here hQ is formed once per step and p is applied in Horner form, x = (t - t_old) * (1 / h): the
        // dense output feeds nothing back into the step sequence, so these roundings only move the result
        // within the 1e-8 tolerance of the BLAS-ordered reference (tests/test_gpu_lv.py), at ~45 instead of
        // ~110 fp64 instructions per observation point
        const double t_old = t;
        const double hd = t_new - t_old;
        const double inv_hd = 1.0 / hd;
        double Q[NS][rk45::kDenseOrder];
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int q = 0; q < rk45::kDenseOrder; ++q) {
                double s = K[0][c] * rk45::P[0][q];
#pragma unroll
                for (int j = 1; j <= rk45::kStages; ++j) s += K[j][c] * rk45::P[j][q];
                Q[c][q] = hd * s;
            }
        const bool last = t_new - t_bound >= 0;
        status = on_step(t_old, t_new, inv_hd, y, Q, last);
        if (status) break;
        t = t_new;
#pragma unroll
        for (int c = 0; c < NS; ++c) { y[c] = y_new[c]; f[c] = f_new[c]; }
    }
    return status;
}

// The observation points of one accepted step, consumed in time order while the integration proceeds:
// on_point(k, u) with u = y(p.t_eval[k]) for every k from kk on that lies in (t_old, t_new]; kk moves on.
// Branch hints: this loop usually goes on (t_n / accepted steps points per step, ~80 in the reference's
// setting) and the two failure exits of lv_integrate are rare.  They change no value; without them the
// register allocator reloads spilled scalars (U, c_log) inside this loop in some kernels and not in
// others, depending on the caller's source form (measured: DESIGN.md section 16).
template <int NS, class OnPoint>
__device__ __forceinline__ void lv_observe(const LvProblem& p, int& kk, double t_old, double t_new, double inv_hd,
                                           const double* y_old, const double (*Q)[rk45::kDenseOrder], bool last,
                                           OnPoint&& on_point) {
    while (__builtin_expect(kk < p.t_n, 1) && (last || p.t_eval[kk] <= t_new)) {
        const double x = (p.t_eval[kk] - t_old) * inv_hd;
        double u[NS];
        lv_horner<NS>(x, y_old, Q, u);
        on_point(kk, u);
        ++kk;
    }
}

// lv_observe for one of `stride` lanes that share an integration: the lane owns the points k, k + stride, ...
// (its cursor k starts at its lane index) and tk holds p.t_eval[k] while k < p.t_n, loaded when the cursor
// moves, so the test of the next step starts without a load.  The segment rule per point is lv_observe's,
// x is formed from the same t_eval[k], so on_point sees the values lv_observe would hand it; with ascending
// t_eval the lanes together consume exactly lv_observe's points of the step, each lane its own in increasing
// k, and the lanes' trip counts differ by at most one.  No cross-lane operation.
template <int NS, class OnPoint>
__device__ __forceinline__ void lv_observe_strided(const LvProblem& p, int& k, double& tk, int stride, double t_old,
                                                   double t_new, double inv_hd, const double* y_old,
                                                   const double (*Q)[rk45::kDenseOrder], bool last,
                                                   OnPoint&& on_point) {
    while (k < p.t_n && (last || tk <= t_new)) {
        const double x = (tk - t_old) * inv_hd;
        double u[NS];
        lv_horner<NS>(x, y_old, Q, u);
        on_point(k, u);
        k = p.t_n - k > stride ? k + stride : p.t_n;     // (no overflow for t_n near INT_MAX)
        if (k < p.t_n) tk = p.t_eval[k];
    }
}

// mvn.logpdf(y_k - u, 0, C) of observation k: -0.5 (c_log + |r U|^2)
__device__ __forceinline__ double lv_loglik_term(const LvProblem& p, int k, const double* u) {
    const double r0 = p.y_obs[2 * k] - u[0], r1 = p.y_obs[2 * k + 1] - u[1];
    const double z0 = r0 * p.U[0] + r1 * p.U[2];
    const double z1 = r0 * p.U[1] + r1 * p.U[3];
    return -0.5 * (p.c_log + (z0 * z0 + z1 * z1));
}

// the gradient's term of observation k, added to acc: acc[j] += (J_k^T C^-1 (y_k - u))_j with J_k = du/dtheta
// = u[2 ..] (2 x 4, row-major) and cinv = inv(C) row-major -- the per-point expression of lv_kernel<10>
// (lv.hip), operation for operation
__device__ __forceinline__ void lv_grad_term(const LvProblem& p, const double cinv[4], int k, const double* u,
                                             double acc[4]) {
    const double r0 = p.y_obs[2 * k] - u[0], r1 = p.y_obs[2 * k + 1] - u[1];
    const double g0 = cinv[0] * r0 + cinv[1] * r1;
    const double g1 = cinv[2] * r0 + cinv[3] * r1;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += u[2 + j] * g0 + u[6 + j] * g1;
}

// log_prior = np.sum(norm.logpdf(log_theta))
__device__ __forceinline__ double lv_log_prior(const double* log_theta, double norm_logc) {
    double lp = -0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double x = log_theta[j];
        lp += -(x * x) / 2.0 - norm_logc;
    }
    return 0.0 + lp;
}

}  // namespace st
