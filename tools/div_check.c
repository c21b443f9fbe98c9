/* div_check.c — div_rn (parallel_amg_amd/csrc/div_rn.h, the text kernels.hip compiles) against
 * IEEE division on the host, bit for bit (two NaNs count as equal), with r = RN(1 / d):
 *   - random operands over 2^-60 .. 2^60 and near-midpoint quotients (w = q d and its
 *     neighbours) for the diagonals of the SPEC grids (6, 4 + 2 eps, ...): the fast path;
 *   - w and d over the whole range 2^-1074 .. 2^1023, subnormals and +-0 among them: both
 *     branches, overflowing and underflowing quotients;
 *   - |w| and |r| at and next to the guard's edges 2^-500 and 2^500;
 *   - the two cases the [2^-900, 2^900] guard got wrong: 2^600 / 2^-500 (inf, was NaN) and
 *     9 2^-875 / (3 2^200) (a subnormal tie);
 *   - quotients built onto subnormal ties: d = m 2^k, w = m (2j+1) 2^(k-1075).
 * Dev tool, not part of libpamg; tests/test_div_rn.py runs it at a small count.
 *   gcc -O2 -ffp-contract=off -o /tmp/div_check tools/div_check.c -lm && /tmp/div_check [cases]
 * cases (default 2e8): the number of random 2^+-60 draws; the other classes scale with it. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../parallel_amg_amd/csrc/div_rn.h"

static uint64_t s = 88172645463325252ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double rexp(int span) {
    uint64_t u = rnd();
    double d;
    u = (u & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - span + (rnd() % (2 * span))) << 52);
    memcpy(&d, &u, 8);
    return d;
}
/* any finite double, the exponent field uniform over 0 .. 2046 (0: subnormals); 1 in 64 is +-0 */
static double rfull(void) {
    uint64_t u = rnd();
    double d;
    u = (u & 0x800FFFFFFFFFFFFFull) | ((rnd() % 2047) << 52);
    if (rnd() % 64 == 0) u &= 0x8000000000000000ull;
    memcpy(&d, &u, 8);
    return d;
}
static double step(double v, int k) {  /* k representable values up (k > 0) or down */
    for (int j = 0; j < abs(k); ++j) v = nextafter(v, k > 0 ? INFINITY : -INFINITY);
    return v;
}
static long n = 0, bad = 0;
static void check(double w, double d) {
    const double got = div_rn(w, d, 1.0 / d), want = w / d;
    ++n;
    if (got != got && want != want) return;
    bad += memcmp(&got, &want, 8) != 0;
}
int main(int argc, char** argv) {
    const double ds[8] = {6.0, 4.002, 3.0, 7.0, 0.1, 1.0 / 3.0, 6.000000000000001, 5.999999999999999};
    const double ms[4] = {3.0, 5.0, 7.0, 6.000000000000001};
    const long cases = argc > 1 ? atol(argv[1]) : 200000000;
    long at[5];
    if (cases <= 0) {
        fprintf(stderr, "usage: div_check [cases > 0]\n");
        return 2;
    }
    for (long i = 0; i < cases; ++i) {  /* random operands */
        const double d = (i % 3 == 0) ? ds[i % 8] : fabs(rexp(60)), w = rexp(60);
        check(w, d);
    }
    at[0] = bad;
    for (long i = 0; i < cases / 2; ++i) {  /* quotients at / next to representable values */
        const double d = ds[i % 8];
        check(step(rexp(30) * d, (int)(rnd() % 5) - 2), d);
    }
    at[1] = bad;
    for (long i = 0; i < cases; ++i) check(rfull(), rfull());  /* the whole range */
    at[2] = bad;
    for (long i = 0; i < cases / 8; ++i) {  /* the guard's edges, |w| and |r| independently */
        const double e[2] = {0x1p-500, 0x1p500};
        const double w = step(e[rnd() % 2], (int)(rnd() % 7) - 3) * ((rnd() & 1) ? -1.0 : 1.0);
        const double d = step(1.0 / e[rnd() % 2], (int)(rnd() % 7) - 3) * ((rnd() & 1) ? -1.0 : 1.0);
        check(w, (i % 4 == 0) ? rfull() : d);
        check((i % 4 == 1) ? rfull() : w, d);
    }
    at[3] = bad;
    check(0x1p600, 0x1p-500);
    check(-0x1p600, 0x1p-500);
    check(9 * 0x1p-875, 3 * 0x1p200);
    for (int m = 0; m < 4; ++m)  /* subnormal ties */
        for (int k = 150; k <= 300; ++k)
            for (int j = 0; j < 16; ++j)
                for (int t = -1; t <= 1; ++t) {
                    const double w = step(ldexp(ms[m] * (2 * j + 1), k - 1075), t);
                    check(w, ldexp(ms[m], k));
                    check(-w, ldexp(ms[m], k));
                }
    at[4] = bad;
    printf("{\"cases\": %ld, \"mismatches\": %ld, \"by_class\": {\"random\": %ld, \"midpoint\": %ld, "
           "\"full_range\": %ld, \"guard_edges\": %ld, \"constructed_ties\": %ld}}\n",
           n, bad, at[0], at[1] - at[0], at[2] - at[1], at[3] - at[2], at[4] - at[3]);
    return bad != 0;
}
