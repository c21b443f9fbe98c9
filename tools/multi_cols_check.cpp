// The two layout rules of several right-hand sides (csrc/multi_cols.h, SPEC §S13) on the CPU: for every
// column count 1 .. 8 the launch chunks are 4, then 2, then 1 wide, cover each column exactly once and
// number at most two wide ones plus a single; a column count outside 1 .. 8 gives no chunk; the column
// stride of a multi-vector is a multiple of 32 doubles, at least n_own + n_ghost, and less than 32 more.
// Prints one JSON line {"bad": 0, "cases": n}; exit status 1 on any violation.
//
//   g++ -std=c++17 -Wall tools/multi_cols_check.cpp -o multi_cols_check && ./multi_cols_check
#include <cstdint>
#include <cstdio>

#include "../parallel_amg_amd/csrc/multi_cols.h"

namespace mc = pamg::mc;

static int bad = 0, cases = 0;

static void expect(bool ok, const char* what, long long a, long long b) {
    ++cases;
    if (ok) return;
    ++bad;
    std::fprintf(stderr, "violated: %s (%lld, %lld)\n", what, a, b);
}

int main() {
    for (int k = -1; k <= mc::kMaxCols + 2; ++k) {
        int first[mc::kMaxCols], width[mc::kMaxCols];
        const int n = mc::chunks(k, first, width);
        if (k < 1 || k > mc::kMaxCols) {
            expect(n == 0, "no chunk outside 1..8", k, n);
            continue;
        }
        int seen[mc::kMaxCols] = {};
        int next = 0, wide = 0, single = 0;
        for (int i = 0; i < n; ++i) {
            expect(width[i] == 4 || width[i] == 2 || width[i] == 1, "chunk width in {4, 2, 1}", k, width[i]);
            expect(first[i] == next, "chunks are consecutive", k, first[i]);
            expect(i == 0 || width[i] <= width[i - 1], "widths never grow", k, i);
            // the preference: no chunk where a wider one would have fitted the columns left
            expect(!(width[i] < 4 && k - first[i] >= 4) && !(width[i] < 2 && k - first[i] >= 2), "widest chunk first", k, i);
            for (int c = first[i]; c < first[i] + width[i] && c < mc::kMaxCols; ++c) ++seen[c];
            next = first[i] + width[i];
            (width[i] > 1 ? wide : single) += 1;
        }
        expect(next == k, "chunks end at k", k, next);
        for (int c = 0; c < mc::kMaxCols; ++c) expect(seen[c] == (c < k ? 1 : 0), "each column exactly once", k, c);
        expect(wide <= 2 && single <= 1, "at most two wide chunks and one single", k, n);
    }
    const int64_t sizes[] = {0, 1, 2, 31, 32, 33, 63, 64, 81, 243, 4095, 4096, 4097, 1536000, (int64_t)1 << 31};
    for (int64_t n_own : sizes)
        for (int64_t n_ghost : {(int64_t)0, (int64_t)1, (int64_t)17, (int64_t)32}) {
            const int64_t s = mc::col_stride(n_own, n_ghost), n = n_own + n_ghost;
            expect(s % mc::kColAlign == 0, "stride is a multiple of 32", n, s);
            expect(s >= n && s >= mc::kColAlign, "stride holds a column", n, s);
            expect(s - n < mc::kColAlign || n == 0, "stride pads less than 32", n, s);
            expect((s * 8) % 256 == 0, "every column starts 256-byte aligned", n, s);
        }
    std::printf("{\"bad\": %d, \"cases\": %d}\n", bad, cases);
    return bad ? 1 : 0;
}
