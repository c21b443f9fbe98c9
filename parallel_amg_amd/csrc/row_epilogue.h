// row_epilogue.h — what a row kernel does with a finished row sum (SPEC §S3, §S9): shared by the row
// kernels of kernels.hip and the multi-column block-row kernel of bsr_multi.hip, so that both round alike.
// Device code only (included inside a unit's own anonymous namespace of namespace pamg).
#pragma once

// OP_JACOBI and OP_CHEB capture the row's diagonal on the way (the in-tile / in-row search).
template <int OP>
constexpr bool kDiagOp = OP == OP_JACOBI || OP == OP_CHEB;

// The Chebyshev step k >= 1 (SPEC §S9) from the row's residual u = b_i - s: seven roundings, none
// fused (-ffp-contract=off). xo is xold_i, +0.0 where the step follows a zero guess.
__device__ __forceinline__ double cheb_step(double u, double xi, double xo, double d, double c1, double c2) {
    const double v = c2 * u;
    const double w = v / d;
    const double e = xi - xo;
    const double q = c1 * e;
    const double t = q + w;
    return xi + t;
}

template <int OP>
__device__ __forceinline__ void epilogue(int r, double s, const double* __restrict__ x,
                                         const double* __restrict__ b, double* __restrict__ y,
                                         double omega, double d, double c1 = 0.0,
                                         const double* __restrict__ xold = nullptr) {
    if constexpr (OP == OP_SPMV) {
        y[r] = s;
    } else if constexpr (OP == OP_RESID) {
        y[r] = b[r] - s;
    } else if constexpr (OP == OP_JACOBI) {
        const double u = b[r] - s;
        const double v = omega * u;
        const double w = v / d;
        y[r] = x[r] + w;
    } else if constexpr (OP == OP_CHEB) {
        y[r] = cheb_step(b[r] - s, x[r], xold ? xold[r] : 0.0, d, c1, omega);
    } else {
        y[r] = y[r] + s;
    }
}

// The BS entries of x that block column c of a block-row operator reads (k_rows_bsr, k_rows_bsr_mc):
// adjacent doubles; 16-byte loads for BS 2 and 4 where x16 says x is 16-byte aligned.
template <int BS>
__device__ __forceinline__ void bsr_load_x(const double* __restrict__ x, int c, bool x16, double (&xe)[BS]) {
    const double* p = x + (int64_t)c * BS;
    if constexpr (BS == 3) {
        xe[0] = p[0];
        xe[1] = p[1];
        xe[2] = p[2];
    } else {
        if (x16) {
#pragma unroll
            for (int e = 0; e < BS; e += 2) {
                const double2 v = *reinterpret_cast<const double2*>(p + e);
                xe[e] = v.x;
                xe[e + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int e = 0; e < BS; ++e) xe[e] = p[e];
        }
    }
}
