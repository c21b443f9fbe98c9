/* div_rn.h — the quotient of the Jacobi / Chebyshev steps of k_sym_zm, k_sym_zc (kernels.hip).
 * One text for the device (hipcc: __host__ __device__) and for tools/div_check.c (plain C), so
 * the tool checks what ships.
 *
 * RN(w / d) given r = RN(1 / d): q0 = RN(w r) and two residual corrections through exact FMA
 * residuals (Markstein: q1 is within one ulp of w / d, so q2 = RN(q1 + (w - q1 d) r) is the
 * correctly rounded quotient) — 5 f64 operations instead of the ~11 of the IEEE division
 * sequence. That argument needs every one of the five results to be a normal number: an
 * overflowing q0 turns the residuals into inf - inf = NaN where w / d is +-inf, and a subnormal
 * quotient is rounded at 2^-1074 instead of at its own last place, where r < 1 / d pushes an
 * almost-tie the wrong way (div_rn(9 2^-875, 3 2^200) would give 2^-1074 for 3 2^-1075, which
 * ties to even, 2^-1073). So the fast path is taken only for |w| and |r| in [2^-500, 2^500]:
 * then |q| lies in [2^-1000, 2^1000], normal with room to spare, |d| in [2^-501, 2^501] (r is
 * within a rounding of 1 / d), q d is about w and cannot overflow, and the residuals
 * e = w - q d are exact: multiples of ulp(q) ulp(d) >= 2^-106 |w| >= 2^-606, far above
 * 2^-1074, and no larger than 2^-51 |w|. Everything else — zeros (whose sign the sequence
 * could lose), subnormals, tiny and huge values, inf, NaN, and a d whose reciprocal is tiny,
 * huge or not finite — takes the division itself.
 * Bitwise the same as w / d for every w, d with r = RN(1 / d); two NaNs count as the same.
 * Checked by tools/div_check.c (tests/test_div_rn.py): operands over the whole range 2^-1074 ..
 * 2^1023 with +-0 and subnormals, both guard edges, near-midpoint quotients, overflowing
 * quotients and quotients built onto subnormal ties. */
#ifndef PAMG_DIV_RN_H
#define PAMG_DIV_RN_H

#if defined(__HIPCC__)
#define PAMG_DIV_RN_FN __host__ __device__ __forceinline__
#else
#define PAMG_DIV_RN_FN static inline
#endif

PAMG_DIV_RN_FN double div_rn(double w, double d, double r) {
    const double aw = __builtin_fabs(w), ar = __builtin_fabs(r);
    if (aw >= 0x1p-500 && aw <= 0x1p500 && ar >= 0x1p-500 && ar <= 0x1p500) {
        const double q0 = w * r;
        const double e0 = __builtin_fma(-q0, d, w);
        const double q1 = __builtin_fma(e0, r, q0);
        const double e1 = __builtin_fma(-q1, d, w);
        return __builtin_fma(e1, r, q1);
    }
    return w / d;
}

#endif
