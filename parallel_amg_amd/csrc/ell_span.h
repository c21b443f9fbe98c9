// Group pairs of the windowed sliced ELL (Options::ell_xwin 1 | 2; pamg_device.h EllSet::npairs):
// the host pass that couples windowed groups whose x windows overlap, and the union window of a
// pair. Plain C++ over the groups' column runs, no device call: matrix.hip's build_ell_xwin runs it
// after the groups are formed, tools/ell_span_check.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <utility>
#include <vector>

namespace pamg {

// a window's runs of consecutive columns: (first column — even —, end, LDS slot of the first), by column
using EllRuns = std::vector<std::array<int, 3>>;

// The union window of two groups: their runs merged by the rule a group's own are built with (runs
// up to 16 columns apart share one), slots assigned in column order. Returns the slots; `chunks`:
// the loads of <= 128 doubles that stage it.
inline int ell_span_union(const EllRuns& a, const EllRuns& b, EllRuns& out, int& chunks) {
    out.clear();
    size_t i = 0, j = 0;
    while (i < a.size() || j < b.size()) {
        const bool ta = j == b.size() || (i < a.size() && a[i][0] <= b[j][0]);
        const std::array<int, 3>& r = ta ? a[i++] : b[j++];
        if (!out.empty() && r[0] <= out.back()[1] + 16) out.back()[1] = std::max(out.back()[1], r[1]);
        else out.push_back({r[0], r[1], 0});
    }
    int slots = 0;
    chunks = 0;
    for (auto& r : out) {
        r[2] = slots;
        slots += r[1] - r[0];
        chunks += (r[1] - r[0] + 127) / 128;
    }
    return slots;
}

// the columns two windows share
inline int ell_span_overlap(const EllRuns& a, const EllRuns& b) {
    int n = 0;
    size_t i = 0, j = 0;
    while (i < a.size() && j < b.size()) {
        n += std::max(0, std::min(a[i][1], b[j][1]) - std::max(a[i][0], b[j][0]));
        if (a[i][1] <= b[j][1]) ++i;
        else ++j;
    }
    return n;
}

// A group's lof word (slot of the pair's column at lane 0, + 64; `lmin`: the first lane that reads
// it, whose slot lies inside a run) carried from the group's own window into the union's
inline uint16_t ell_span_relof(uint16_t word, int lmin, const EllRuns& own, const EllRuns& uni) {
    const int slot = (int)word - 64 + lmin;
    size_t r = 0;
    while (r + 1 < own.size() && own[r + 1][2] <= slot) ++r;
    const int col = own[r][0] + slot - own[r][2];
    size_t u = 0;
    while (u + 1 < uni.size() && uni[u + 1][0] <= col) ++u;
    return (uint16_t)(uni[u][2] + col - uni[u][0] - lmin + 64);
}

// The greedy pass, the slices' rule one level up: the lowest unassigned windowed group, then the
// unassigned windowed group sharing the most window columns with it (ties: the lower group) among
// the best six of the groups that hold its window's columns as rows (sgroup: slice -> group, w the
// slice width); a candidate is taken where the union fits `cap` doubles and `max_chunks` chunks and
// is at most `share` percent of the two windows together. runs[g] empty: no window (a gather group).
// Returns the pairs (lower group first), by first group.
inline std::vector<std::pair<int, int>> ell_span_pairs(const std::vector<EllRuns>& runs, const std::vector<int>& gwin,
                                                       const std::vector<int>& sgroup, int w, int cap,
                                                       int max_chunks, int share) {
    const int ng = (int)runs.size(), ns = (int)sgroup.size();
    std::vector<std::pair<int, int>> pairs;
    std::vector<char> done(ng, 0);
    std::vector<int> cand, score(ng, 0);
    EllRuns uni;
    for (int a = 0; a < ng; ++a) {
        if (done[a] || runs[a].empty()) continue;
        done[a] = 1;
        cand.clear();
        for (const auto& r : runs[a])
            for (int q = std::max(r[0], 0) / w; q <= (r[1] - 1) / w && q < ns; ++q) {
                const int b = sgroup[q];
                if (b >= 0 && !done[b] && !runs[b].empty() && score[b] == 0) {
                    score[b] = 1 + ell_span_overlap(runs[a], runs[b]);
                    cand.push_back(b);
                }
            }
        const size_t top = std::min<size_t>(6, cand.size());
        std::partial_sort(cand.begin(), cand.begin() + top, cand.end(),
                          [&](int p, int q) { return score[p] != score[q] ? score[p] > score[q] : p < q; });
        int take = -1;
        for (size_t c = 0; c < top && take < 0; ++c) {
            int nch = 0;
            const int slots = ell_span_union(runs[a], runs[cand[c]], uni, nch);
            if (slots <= cap && nch <= max_chunks && (int64_t)slots * 100 <= (int64_t)share * (gwin[a] + gwin[cand[c]]))
                take = cand[c];
        }
        for (int b : cand) score[b] = 0;
        if (take >= 0) {
            done[take] = 1;
            pairs.push_back({a, take});
        }
    }
    return pairs;
}

}  // namespace pamg
