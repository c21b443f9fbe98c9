// bsr_multi.hip — the block-row kernel on several right-hand sides (SPEC §S13; gfx950).
//
// k_rows_bsr (kernels.hip) streams 8 + 4 / bs^2 bytes of matrix per stored nonzero and 2 to 7 % as many
// bytes of vectors, so a second right-hand side costs the whole stream again. k_rows_bsr_mc walks the same
// slices with the same lanes and loads each block slot — its column and its BS^2 values — once for NV
// columns: per column the lane loads the block's BS entries of x and adds s[c][d] = s[c][d] + v_de x_ce
// in e order, each product and each add rounded once (-ffp-contract=off), which is k_rows_bsr's sum for
// that column alone. Nothing is summed across columns, and a padded slot is skipped whole. The epilogues
// are epilogue<OP>'s and the fused block sweeps k_rows_bsr's, per column, with the diagonal entries and
// the lane's d_binv block loaded once. No LDS, no barrier.
// A unit of its own: kernels.hip's code object stays as it is ("Several right-hand sides").
// Values stored in binary32 (SPEC §S15; BsrSet::d_val32): the kernels' VT = float instantiations load the same
// slots as 4-byte values — 4 + 4 / bs^2 bytes per nonzero — and widen each exactly, (double)v, before the fp64
// product, so the sums are those of an fp64 upload of the rounded values.

#include "multi_cols.h"
#include "pamg_device.h"

namespace pamg {
namespace {

#include "row_epilogue.h"

// The columns of one launch, by value in the kernel's arguments: any subset of a multi-vector's columns
template <int NV>
struct McIn {
    const double* p[NV];
};
template <int NV>
struct McOut {
    double* p[NV];
};

// VT: the stored value type (SPEC §S15: float values are widened exactly before the fp64 product)
template <int BS, int OP, int FUSE, int NV, typename VT = double>
__global__ __launch_bounds__(kBlock) void k_rows_bsr_mc(int nb, int ns, const int64_t* __restrict__ soff,
                                                        const int* __restrict__ bcol, const VT* __restrict__ val,
                                                        const double* __restrict__ diag,
                                                        const double* __restrict__ binv, int x16, McIn<NV> x,
                                                        McIn<NV> b, McOut<NV> y, double omega, double c1,
                                                        McIn<NV> xold) {
    const int lane = threadIdx.x & (kEllW - 1);
    const int sl = blockIdx.x * kBsrSlices + (threadIdx.x >> 6);
    if (sl >= ns) return;
    const int64_t k0 = soff[sl], k1 = soff[sl + 1];
    const int m = sl * kEllW + lane;
    double s[NV][BS];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
#pragma unroll
        for (int d = 0; d < BS; ++d) s[c][d] = 0.0;
    }
    const int* cp = bcol + k0 * kEllW + lane;
    const VT* vp = val + k0 * (BS * BS) * kEllW + lane;
    for (int64_t k = k0; k < k1; ++k, cp += kEllW, vp += BS * BS * kEllW) {
        const int col = *cp;
        if (col < 0) continue;
        double v[BS * BS];
#pragma unroll
        for (int j = 0; j < BS * BS; ++j) v[j] = (double)vp[j * kEllW];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            double xe[BS];
            bsr_load_x<BS>(x.p[c], col, x16 != 0, xe);
#pragma unroll
            for (int d = 0; d < BS; ++d) {
#pragma unroll
                for (int e = 0; e < BS; ++e) {
                    const double p = v[d * BS + e] * xe[e];
                    s[c][d] = s[c][d] + p;
                }
            }
        }
    }
    if (m >= nb) return;
    const int64_t r0 = (int64_t)m * BS;
    if constexpr (FUSE == 0) {
#pragma unroll
        for (int d = 0; d < BS; ++d) {
            double dg = 1.0;
            if constexpr (kDiagOp<OP>) dg = diag[r0 + d];
#pragma unroll
            for (int c = 0; c < NV; ++c)
                epilogue<OP>((int)(r0 + d), s[c][d], x.p[c], b.p[c], y.p[c], omega, dg, c1, xold.p[c]);
        }
    } else {
        double di[BS * BS];
#pragma unroll
        for (int j = 0; j < BS * BS; ++j) di[j] = binv[r0 * BS + j];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const double* __restrict__ xc = x.p[c];
            const double* __restrict__ bc = b.p[c];
            const double* __restrict__ xo = xold.p[c];
            double* __restrict__ yc = y.p[c];
            double u[BS];
#pragma unroll
            for (int d = 0; d < BS; ++d) u[d] = bc[r0 + d] - s[c][d];
#pragma unroll
            for (int d = 0; d < BS; ++d) {
                double w = 0.0;
#pragma unroll
                for (int j = 0; j < BS; ++j) {
                    const double p = di[d * BS + j] * u[j];
                    w = w + p;
                }
                const int64_t r = r0 + d;
                if constexpr (FUSE == 1) {
                    const double vv = omega * w;
                    yc[r] = xc[r] + vv;
                } else {
                    const double xi = xc[r];
                    const double vv = omega * w;
                    const double e = xi - (xo ? xo[r] : 0.0);
                    const double q = c1 * e;
                    const double t = q + vv;
                    yc[r] = xi + t;
                }
            }
        }
    }
}

template <int OP, int FUSE, int NV>
void launch_chunk(const pamg_mat& A, const double* const* x, const double* const* b, const double* const* xold,
                  double* const* y, double omega, double c1, hipStream_t s) {
    const BsrSet& B = A.bsr;
    McIn<NV> xa, ba, oa;
    McOut<NV> ya;
    int x16 = 1;  // the 16-byte x loads only where every column of the launch allows them
    for (int c = 0; c < NV; ++c) {
        xa.p[c] = x[c];
        ba.p[c] = b ? b[c] : nullptr;
        oa.p[c] = xold ? xold[c] : nullptr;
        ya.p[c] = y[c];
        if ((reinterpret_cast<uintptr_t>(x[c]) & 15) != 0) x16 = 0;
    }
    auto go = [&](auto kern, auto* val) {
        kern<<<B.grid, kBlock, 0, s>>>((int)B.nb, (int)B.nslices, B.d_soff, B.d_bcol, val, A.d_diag, A.d_binv, x16,
                                       xa, ba, ya, omega, c1, oa);
    };
    if (B.d_val32) {
        switch (B.bs) {
            case 2: go(k_rows_bsr_mc<2, OP, FUSE, NV, float>, B.d_val32); break;
            case 3: go(k_rows_bsr_mc<3, OP, FUSE, NV, float>, B.d_val32); break;
            default: go(k_rows_bsr_mc<4, OP, FUSE, NV, float>, B.d_val32); break;
        }
        return;
    }
    switch (B.bs) {
        case 2: go(k_rows_bsr_mc<2, OP, FUSE, NV>, B.d_val); break;
        case 3: go(k_rows_bsr_mc<3, OP, FUSE, NV>, B.d_val); break;
        default: go(k_rows_bsr_mc<4, OP, FUSE, NV>, B.d_val); break;
    }
}

template <int NV>
void launch_chunk_op(const pamg_mat& A, int op, int fuse, const double* const* x, const double* const* b,
                     const double* const* xold, double* const* y, double omega, double c1, hipStream_t s) {
    if (fuse == 1) return launch_chunk<OP_RESID, 1, NV>(A, x, b, nullptr, y, omega, 0.0, s);
    if (fuse == 2) return launch_chunk<OP_RESID, 2, NV>(A, x, b, xold, y, omega, c1, s);
    switch (op) {
        case OP_SPMV: launch_chunk<OP_SPMV, 0, NV>(A, x, b, nullptr, y, omega, 0.0, s); break;
        case OP_RESID: launch_chunk<OP_RESID, 0, NV>(A, x, b, nullptr, y, omega, 0.0, s); break;
        case OP_JACOBI: launch_chunk<OP_JACOBI, 0, NV>(A, x, b, nullptr, y, omega, 0.0, s); break;
        case OP_CHEB: launch_chunk<OP_CHEB, 0, NV>(A, x, b, xold, y, omega, c1, s); break;
        default: launch_chunk<OP_PROLONG, 0, NV>(A, x, b, nullptr, y, omega, 0.0, s); break;
    }
}

// ------------------------------------------------------------------ the row-per-lane form (BsrSet::row_lanes)
// k_rows_bsr_r: one lane per SCALAR row of a restriction-shaped block-row operator (SPEC §S14: R has few,
// long block rows — about 125 blocks per coarse node on a 27-point grid and nb / 27 nodes — so a lane per node
// leaves most of the machine idle). One slice of kEllW rows per wave, kBsrSlices slices per workgroup; the BS
// rows of a node sit in BS adjacent lanes. Per slot a lane loads the block column, its own row's BS values
// (adjacent doubles, 16-byte loads for BS 2 and 4: the wave reads one contiguous run of 512 BS bytes) and,
// per column of the launch, the block's BS entries of x — the lanes of a node read the same line — and adds
// s = s + v_e x_e in e order, each product and each add rounded once: row BS m + d's stored order, so §S3's
// bits. Row sums are never split over lanes. Slots go four at a time, the columns and values of a group
// loaded before its first product (a padded slot holds column -1 and zeros: its loads are in bounds, its
// products are skipped), so four dependent x loads are in flight per lane instead of one. No LDS, no barrier.
// OP_SPMV, OP_RESID and OP_PROLONG only: the form is built for operators that are not square.
// (binary32 values, SPEC §S15: BS adjacent floats, one 8- or 16-byte load for BS 2 or 4, widened exactly)
template <int BS>
__device__ __forceinline__ void bsr_r_load_v(const float* __restrict__ p, double (&v)[BS]) {
    if constexpr (BS == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = (double)t.x;
        v[1] = (double)t.y;
    } else if constexpr (BS == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = (double)t.x;
        v[1] = (double)t.y;
        v[2] = (double)t.z;
        v[3] = (double)t.w;
    } else {
        v[0] = (double)p[0];
        v[1] = (double)p[1];
        v[2] = (double)p[2];
    }
}

template <int BS>
__device__ __forceinline__ void bsr_r_load_v(const double* __restrict__ p, double (&v)[BS]) {
    if constexpr (BS == 3) {
        v[0] = p[0];
        v[1] = p[1];
        v[2] = p[2];
    } else {
#pragma unroll
        for (int e = 0; e < BS; e += 2) {
            const double2 t = *reinterpret_cast<const double2*>(p + e);
            v[e] = t.x;
            v[e + 1] = t.y;
        }
    }
}

template <int BS, int OP, int NV, typename VT = double>
__global__ __launch_bounds__(kBlock) void k_rows_bsr_r(int nrows, int ns, const int64_t* __restrict__ soff,
                                                       const int* __restrict__ bcol, const VT* __restrict__ val,
                                                       int x16, McIn<NV> x, McIn<NV> b, McOut<NV> y) {
    constexpr int U = 4;
    const int lane = threadIdx.x & (kEllW - 1);
    const int sl = blockIdx.x * kBsrSlices + (threadIdx.x >> 6);
    if (sl >= ns) return;
    const int64_t k0 = soff[sl], k1 = soff[sl + 1];
    const int r = sl * kEllW + lane;
    double s[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) s[c] = 0.0;
    const int* cp = bcol + k0 * kEllW + lane;
    const VT* vp = val + (k0 * kEllW + lane) * BS;
    auto slot = [&](int col, const double (&v)[BS]) {
        if (col < 0) return;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            double xe[BS];
            bsr_load_x<BS>(x.p[c], col, x16 != 0, xe);
#pragma unroll
            for (int e = 0; e < BS; ++e) {
                const double p = v[e] * xe[e];
                s[c] = s[c] + p;
            }
        }
    };
    int64_t k = k0;
    for (; k + U <= k1; k += U, cp += U * kEllW, vp += U * kEllW * BS) {
        int col[U];
        double v[U][BS];
#pragma unroll
        for (int u = 0; u < U; ++u) col[u] = cp[u * kEllW];
#pragma unroll
        for (int u = 0; u < U; ++u) bsr_r_load_v<BS>(vp + u * kEllW * BS, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) slot(col[u], v[u]);
    }
    for (; k < k1; ++k, cp += kEllW, vp += kEllW * BS) {
        double v[BS];
        bsr_r_load_v<BS>(vp, v);
        slot(*cp, v);
    }
    if (r >= nrows) return;
#pragma unroll
    for (int c = 0; c < NV; ++c) epilogue<OP>(r, s[c], x.p[c], b.p[c], y.p[c], 0.0, 1.0);
}

template <int OP, int NV>
void launch_rows_chunk(const pamg_mat& A, const double* const* x, const double* const* b, double* const* y,
                       hipStream_t s) {
    const BsrSet& B = A.bsr;
    McIn<NV> xa, ba;
    McOut<NV> ya;
    int x16 = 1;
    for (int c = 0; c < NV; ++c) {
        xa.p[c] = x[c];
        ba.p[c] = b ? b[c] : nullptr;
        ya.p[c] = y[c];
        if ((reinterpret_cast<uintptr_t>(x[c]) & 15) != 0) x16 = 0;
    }
    auto go = [&](auto kern, auto* val) {
        kern<<<B.grid, kBlock, 0, s>>>((int)A.nrows, (int)B.nslices, B.d_soff, B.d_bcol, val, x16, xa, ba, ya);
    };
    if (B.d_val32) {
        switch (B.bs) {
            case 2: go(k_rows_bsr_r<2, OP, NV, float>, B.d_val32); break;
            case 3: go(k_rows_bsr_r<3, OP, NV, float>, B.d_val32); break;
            default: go(k_rows_bsr_r<4, OP, NV, float>, B.d_val32); break;
        }
        return;
    }
    switch (B.bs) {
        case 2: go(k_rows_bsr_r<2, OP, NV>, B.d_val); break;
        case 3: go(k_rows_bsr_r<3, OP, NV>, B.d_val); break;
        default: go(k_rows_bsr_r<4, OP, NV>, B.d_val); break;
    }
}

template <int NV>
void launch_rows_chunk_op(const pamg_mat& A, int op, const double* const* x, const double* const* b, double* const* y,
                          hipStream_t s) {
    switch (op) {
        case OP_SPMV: launch_rows_chunk<OP_SPMV, NV>(A, x, b, y, s); break;
        case OP_RESID: launch_rows_chunk<OP_RESID, NV>(A, x, b, y, s); break;
        case OP_PROLONG: launch_rows_chunk<OP_PROLONG, NV>(A, x, b, y, s); break;
        default: break;  // (the diagonal ops are refused before: the operator is not square)
    }
}

}  // namespace

void launch_bsr_rows(const pamg_mat& A, int op, int ncols, const double* const* x, const double* const* b,
                     double* const* y, hipStream_t s) {
    if (!A.bsr.row_lanes || A.nrows <= 0) return;
    int first[mc::kMaxCols], width[mc::kMaxCols];
    const int n = mc::chunks(ncols, first, width);
    for (int i = 0; i < n; ++i) {
        const int c = first[i];
        const double* const* bc = b ? b + c : nullptr;
        if (width[i] == 4) launch_rows_chunk_op<4>(A, op, x + c, bc, y + c, s);
        else if (width[i] == 2) launch_rows_chunk_op<2>(A, op, x + c, bc, y + c, s);
        else launch_rows_chunk_op<1>(A, op, x + c, bc, y + c, s);
    }
}

void launch_bsr_multi(const pamg_mat& A, int op, int fuse, int ncols, const double* const* x, const double* const* b,
                      const double* const* xold, double* const* y, double omega, double c1, hipStream_t s) {
    if (A.interior.bsr_r) return launch_bsr_rows(A, op, ncols, x, b, y, s);
    if (A.bsr.nb <= 0) return;
    int first[mc::kMaxCols], width[mc::kMaxCols];
    const int n = mc::chunks(ncols, first, width);
    for (int i = 0; i < n; ++i) {
        const int c = first[i];
        const double* const* bc = b ? b + c : nullptr;
        const double* const* oc = xold ? xold + c : nullptr;
        if (width[i] == 4) {
            launch_chunk_op<4>(A, op, fuse, x + c, bc, oc, y + c, omega, c1, s);
        } else if (width[i] == 2) {
            launch_chunk_op<2>(A, op, fuse, x + c, bc, oc, y + c, omega, c1, s);
        } else if (fuse) {  // one column: today's launchers
            launch_bsr_block(A, fuse == 1 ? BM_JACOBI : BM_CHEB, x[c], b[c], oc ? oc[0] : nullptr, y[c], c1, omega, s);
        } else {
            const double* xo = op == OP_CHEB ? (oc ? oc[0] : nullptr) : x[c];
            launch_set(A, A.interior, op, x[c], bc ? bc[0] : nullptr, xo, y[c], omega, s, c1);
        }
    }
}

}  // namespace pamg
