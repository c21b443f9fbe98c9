// multi_cols.h — the two layout rules of several right-hand sides (SPEC §S13), in plain C++ so that
// tools/multi_cols_check.cpp can check them on the CPU: how the columns of a multi-column operation are
// cut into kernel launches, and where the columns of a multi-vector start.
#pragma once
#include <cstdint>
#include <initializer_list>

namespace pamg {
namespace mc {

constexpr int kMaxCols = 8;    // columns of one multi-column operation: 1 .. kMaxCols
constexpr int kColAlign = 32;  // a column starts on a multiple of this many doubles (256 bytes)

// Columns 0 .. k - 1 in chunks of 4, then 2, then 1 (the widths the multi-column kernels exist in; a
// chunk of 1 is the single-column launcher): width[i] columns from first[i] on. Returns the chunks, 0
// for k outside 1 .. kMaxCols.
inline int chunks(int k, int first[kMaxCols], int width[kMaxCols]) {
    if (k < 1 || k > kMaxCols) return 0;
    int n = 0, c = 0;
    for (int w : {4, 2, 1})
        while (k - c >= w) {
            first[n] = c;
            width[n] = w;
            ++n;
            c += w;
        }
    return n;
}

// Doubles from one column of a multi-vector to the next: n_own + n_ghost rounded up to a multiple of
// kColAlign (at least one), so that every column starts 256-byte aligned like a vector of its own.
inline int64_t col_stride(int64_t n_own, int64_t n_ghost) {
    const int64_t n = n_own + n_ghost;
    return n <= 0 ? kColAlign : (n + kColAlign - 1) / kColAlign * kColAlign;
}

}  // namespace mc
}  // namespace pamg
