// Cholesky factor and both triangular solves of one d x d system held in LDS, for a 256-thread block (als.hip, exposure.hip).
// Every sum has a fixed order, so the result is bit-identical from run to run.
#pragma once

#include "common.h"

namespace qrec {

__device__ inline double chol_readlane_f64(double v, int lane) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Right-looking Cholesky of the lower triangle of A (row stride lda): L overwrites the strict lower triangle, its diagonal
// goes to s_diag.  Called by all 256 threads of the block; returns false, uniformly over the block (every thread reads the
// same pivot), at the first non-positive (or NaN) pivot.
__device__ inline bool chol_factor_lds(double *A, int lda, int d, double *s_diag) {
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    for (int k = 0; k < d; ++k) {
        const double piv = A[k * lda + k];
        if (!(piv > 0.0)) return false;
        const double lkk = sqrt(piv);
        if (tid == 0) s_diag[k] = lkk;
        for (int i = k + 1 + tid; i < d; i += 256) A[i * lda + k] = A[i * lda + k] / lkk;
        __syncthreads();
        for (int i = k + 1 + ty; i < d; i += 16) {
            const double lik = A[i * lda + k];
            for (int j = k + 1 + tx; j <= i; j += 16) A[i * lda + j] = fma(-lik, A[j * lda + k], A[i * lda + j]);
        }
        __syncthreads();
    }
    return true;
}

// L y = b, then L^T x = y, on the factor of chol_factor_lds; called by the first wave only (lane l holds entries l and l + 64,
// d <= 128).  Writes out[0 .. ld), zero past d.
__device__ inline void chol_solve_wave(const double *A, int lda, int d, int ld, const double *s_b, const double *s_diag,
                                       double *out) {
    const int i0 = threadIdx.x, i1 = threadIdx.x + 64;
    double v0 = i0 < d ? s_b[i0] : 0.0, v1 = i1 < d ? s_b[i1] : 0.0;
    for (int k = 0; k < d; ++k) {
        const double yk = chol_readlane_f64(k < 64 ? v0 : v1, k & 63) / s_diag[k];
        if (i0 > k && i0 < d) v0 = fma(-A[i0 * lda + k], yk, v0); else if (i0 == k) v0 = yk;
        if (i1 > k && i1 < d) v1 = fma(-A[i1 * lda + k], yk, v1); else if (i1 == k) v1 = yk;
    }
    for (int k = d - 1; k >= 0; --k) {
        const double xk = chol_readlane_f64(k < 64 ? v0 : v1, k & 63) / s_diag[k];
        if (i0 < k) v0 = fma(-A[k * lda + i0], xk, v0); else if (i0 == k) v0 = xk;
        if (i1 < k) v1 = fma(-A[k * lda + i1], xk, v1); else if (i1 == k) v1 = xk;
    }
    if (i0 < ld) out[i0] = i0 < d ? v0 : 0.0;
    if (i1 < ld) out[i1] = i1 < d ? v1 : 0.0;
}

}  // namespace qrec
