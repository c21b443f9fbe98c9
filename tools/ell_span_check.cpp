// Stand-alone check of the windowed ELL's group-pair pass (parallel_amg_amd/csrc/ell_span.h), meant to
// be built with -fsanitize=address,undefined (tests/test_ell_span_host.py): windows of generated band
// operators — groups of 4 consecutive 64-row slices, the columns of rows r .. r + 255 at the given
// offsets, merged into runs as build_ell_xwin merges them — are paired, and every pair's union window
// and carried lof words are checked against the columns they stand for. Prints one JSON line.
//   ell_span_check <rows> <cap> <offset>...
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../parallel_amg_amd/csrc/ell_span.h"

using pamg::EllRuns;

static EllRuns runs_of(const std::set<int>& cols) {
    EllRuns runs;
    for (int c : cols) {
        const int s = c & ~1, e = (c + 2) & ~1;
        if (!runs.empty() && s <= runs.back()[1] + 16) runs.back()[1] = std::max(runs.back()[1], e);
        else runs.push_back({s, e, 0});
    }
    int slots = 0;
    for (auto& r : runs) {
        r[2] = slots;
        slots += r[1] - r[0];
    }
    return runs;
}

static int slot_of(const EllRuns& runs, int col) {
    for (const auto& r : runs)
        if (col >= r[0] && col < r[1]) return r[2] + col - r[0];
    return -1;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int n = std::atoi(argv[1]), cap = std::atoi(argv[2]), w = 64;
    std::vector<int> offs;
    for (int a = 3; a < argc; ++a) offs.push_back(std::atoi(argv[a]));
    const int ns = (n + w - 1) / w, ng = (ns + 3) / 4;
    std::vector<EllRuns> runs(ng);
    std::vector<int> gwin(ng, 0), sgroup(ns);
    for (int q = 0; q < ns; ++q) sgroup[q] = q / 4;
    for (int g = 0; g < ng; ++g) {
        std::set<int> cols;
        for (int i = g * 256; i < std::min(n, (g + 1) * 256); ++i)
            for (int o : offs)
                if (i + o >= 0 && i + o < n) cols.insert(i + o);
        runs[g] = runs_of(cols);
        for (const auto& r : runs[g]) gwin[g] += r[1] - r[0];
        if (gwin[g] > cap) {  // a gather group
            runs[g].clear();
            gwin[g] = 0;
        }
    }
    const auto pairs = pamg::ell_span_pairs(runs, gwin, sgroup, w, cap, 512, 90);
    std::vector<char> seen(ng, 0);
    long usum = 0;
    int bad = 0;
    EllRuns uni;
    for (const auto& p : pairs) {
        const int a = p.first, b = p.second;
        if (a >= b || seen[a] || seen[b] || runs[a].empty() || runs[b].empty()) ++bad;
        seen[a] = seen[b] = 1;
        int nch = 0;
        const int slots = pamg::ell_span_union(runs[a], runs[b], uni, nch);
        if (slots > cap || nch > 512 || slots * 100L > 90L * (gwin[a] + gwin[b])) ++bad;
        if (slots < std::max(gwin[a], gwin[b]) || slots > gwin[a] + gwin[b] + 16 * (int)uni.size()) ++bad;
        usum += slots;
        // a lof word of either group (the column c0 + lmin of a pair read from lane lmin on) names the
        // same column in the union window
        for (int g : {a, b})
            for (const auto& r : runs[g])
                for (int lmin : {0, 1, 37, 63})
                    for (int col : {r[0], (r[0] + r[1]) / 2, r[1] - 1}) {
                        const uint16_t word = (uint16_t)(slot_of(runs[g], col) - lmin + 64);
                        const uint16_t got = pamg::ell_span_relof(word, lmin, runs[g], uni);
                        if ((int)got - 64 + lmin != slot_of(uni, col)) ++bad;
                    }
    }
    std::printf("{\"groups\": %d, \"pairs\": %d, \"union_mean\": %ld, \"bad\": %d}\n", ng, (int)pairs.size(),
                pairs.empty() ? 0L : usum / (long)pairs.size(), bad);
    return bad ? 1 : 0;
}
