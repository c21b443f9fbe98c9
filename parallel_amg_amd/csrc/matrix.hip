// matrix.hip — from a caller's CSR arrays to a finished pamg_mat: the threaded host passes and
// staged copies of the upload, the detector and builder of every layout family (sym, rpat, ell,
// pnc, bsr, tiles) with its four contract functions, and the pamg_mat_* entry points of include/pamg.h
// that drive them. The rest of the runtime (runtime.hip) reaches this unit through those entry
// points only; everything else here is file-local.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "pamg_device.h"
#include "pamg_host.h"
#include "ell_span.h"

namespace {

// ---- host side of the upload: threads for the per-nonzero passes, pinned staging for copies
// Threads: OMP_NUM_THREADS if set (16 on the GPU box), else the hardware count, at most 64.
int host_threads() {
    static const int n = [] {
        const char* e = std::getenv("OMP_NUM_THREADS");
        int v = e ? std::atoi(e) : 0;
        if (v <= 0) v = (int)std::thread::hardware_concurrency();
        return std::max(1, std::min(v, 64));
    }();
    return n;
}

// f(begin, end) over [0, n) in contiguous chunks, one per thread (each chunk's work is
// independent of the others; results are the same for any thread count)
template <class F>
void par_for(int64_t n, F&& f) {
    const int nt = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, n / 16384));
    if (nt <= 1) {
        if (n > 0) f((int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int t = 0; t < nt; ++t) {
        const int64_t a = n * t / nt, b = n * (t + 1) / nt;
        th.emplace_back([&f, a, b] { f(a, b); });
    }
    for (auto& x : th) x.join();
}

// Host-to-device copy of a large pageable buffer through two pinned 64 MiB staging buffers:
// threads copy chunk k into one while the DMA engine moves chunk k-1 out of the other.
int h2d(pamg_ctx* ctx, void* dst, const void* src, size_t bytes) {
    constexpr size_t kChunk = size_t(64) << 20;
    if (bytes == 0) return PAMG_OK;
    if (bytes < (size_t(4) << 20)) {
        HIPC(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return PAMG_OK;
    }
    // per context (one host thread per context, pamg.h): the events belong to ctx's device
    char** stage = ctx->stage;
    hipEvent_t* done = ctx->stage_done;
    for (int k = 0; k < 2; ++k) {
        if (!stage[k]) HIPC(hipHostMalloc(reinterpret_cast<void**>(&stage[k]), kChunk, hipHostMallocPortable));
        if (!done[k]) HIPC(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    }
    hipStream_t s = ctx->s_comp;
    size_t off = 0;
    for (int k = 0; off < bytes; k ^= 1) {
        const size_t m = std::min(kChunk, bytes - off);
        HIPC(hipEventSynchronize(done[k]));  // the DMA out of this buffer has finished
        const char* from = static_cast<const char*>(src) + off;
        char* to = stage[k];
        par_for((int64_t)((m + 4095) / 4096), [&](int64_t a, int64_t b) {
            const size_t lo = (size_t)a * 4096, hi = std::min(m, (size_t)b * 4096);
            std::memcpy(to + lo, from + lo, hi - lo);
        });
        HIPC(hipMemcpyAsync(static_cast<char*>(dst) + off, to, m, hipMemcpyHostToDevice, s));
        HIPC(hipEventRecord(done[k], s));
        off += m;
    }
    HIPC(hipStreamSynchronize(s));
    return PAMG_OK;
}

// std::vector storage whose sizing constructor leaves the elements uninitialised: the upload's
// column and row-pointer copies (up to 3.75 GB at 512^3) are filled by parallel loops, not zeroed
// first on one thread
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) {}
    template <class U, class... Args>
    void construct(U* p, Args&&... args) {
        if constexpr (sizeof...(Args) == 0)
            ::new ((void*)p) U;
        else
            ::new ((void*)p) U(std::forward<Args>(args)...);
    }
};
using IdxVec = std::vector<int, NoInitAlloc<int>>;
using PtrVec = std::vector<int64_t, NoInitAlloc<int64_t>>;

// PAMG_TRACE_UPLOAD=1: per-phase host times of each matrix upload on stderr
struct UploadTrace {
    bool on = std::getenv("PAMG_TRACE_UPLOAD") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    int64_t nnz = 0;
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pamg upload nnz=%lld] %-14s %8.3f s\n", (long long)nnz, what,
                     std::chrono::duration<double>(now - t).count());
        t = now;
    }
};

// ------------------------------------------------------------------ shared by the layout families

// Compute units of the current device (256 on MI355X), for occupancy-keyed layout rules
int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return 256;
    return cus;
}

// Per own column: the largest gap between consecutive rows that read it (0 if fewer than two
// do). Row chunks in parallel, each over the column range its rows touch (first / last reader
// and the largest gap inside the chunk), then merged per column in chunk order: the values of
// one sequential pass. A matrix whose chunks together span more than ~2x the columns (no band
// structure) takes the sequential pass.
std::vector<int> column_reuse_gaps(const PtrVec& rp, const IdxVec& ci, int64_t nrows,
                                   int64_t ncols) {
    std::vector<int> gap(ncols, 0);
    const int nch = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, nrows / 65536));
    std::vector<int64_t> r0(nch + 1);
    for (int t = 0; t <= nch; ++t) r0[t] = nrows * t / nch;
    // one thread per chunk (par_for would keep a handful of items on one thread)
    auto each_chunk = [nch](const std::function<void(int)>& f) {
        std::vector<std::thread> th;
        for (int t = 0; t < nch; ++t) th.emplace_back([&f, t] { f(t); });
        for (auto& x : th) x.join();
    };
    std::vector<int> lo(nch, INT32_MAX), hi(nch, -1);
    each_chunk([&](int t) {
        int a = INT32_MAX, b = -1;
        for (int64_t k = rp[r0[t]]; k < rp[r0[t + 1]]; ++k)
            if (ci[k] < ncols) {
                a = std::min(a, ci[k]);
                b = std::max(b, ci[k]);
            }
        lo[t] = a;
        hi[t] = b;
    });
    int64_t span = 0;
    for (int t = 0; t < nch; ++t) span += hi[t] >= lo[t] ? (int64_t)hi[t] - lo[t] + 1 : 0;
    if (nch == 1 || span > 2 * ncols + 65536) {
        std::vector<int> last(ncols, -1);
        for (int64_t i = 0; i < nrows; ++i)
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                const int c = ci[k];
                if (c < ncols) {
                    if (last[c] >= 0) gap[c] = std::max(gap[c], (int)i - last[c]);
                    last[c] = (int)i;
                }
            }
        return gap;
    }
    // per chunk, over [lo, hi]: first reader, last reader, largest gap inside the chunk
    std::vector<std::vector<int>> first(nch), last(nch), cgap(nch);
    each_chunk([&](int t) {
        if (hi[t] < lo[t]) return;
        const int64_t w = (int64_t)hi[t] - lo[t] + 1;
        first[t].assign(w, -1);
        last[t].assign(w, -1);
        cgap[t].assign(w, 0);
        int* f = first[t].data();
        int* l = last[t].data();
        int* g = cgap[t].data();
        for (int64_t i = r0[t]; i < r0[t + 1]; ++i)
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                const int c = ci[k];
                if (c >= ncols) continue;
                const int j = c - lo[t];
                if (l[j] >= 0) g[j] = std::max(g[j], (int)i - l[j]);
                else f[j] = (int)i;
                l[j] = (int)i;
            }
    });
    par_for(ncols, [&](int64_t a, int64_t b) {
        for (int64_t c = a; c < b; ++c) {
            int g = 0, prev = -1;
            for (int t = 0; t < nch; ++t) {
                if (c < lo[t] || c > hi[t]) continue;
                const int64_t j = c - lo[t];
                if (first[t][j] < 0) continue;
                if (prev >= 0) g = std::max(g, first[t][j] - prev);
                g = std::max(g, cgap[t][j]);
                prev = last[t][j];
            }
            gap[c] = g;
        }
    });
    return gap;
}

// a copy of the context's registered grids (pamg_ctx::grids)
std::vector<std::array<int64_t, 4>> grids_of(pamg_ctx* ctx) {
    std::lock_guard<std::mutex> lk(ctx->grids_mu);
    return ctx->grids;
}

// a 7-point grid operator's grid, for a later prolongation / restriction over it (pnc, ELL group order)
void register_grid(pamg_ctx* ctx, int64_t n, int64_t nx, int64_t ny, int64_t nz) {
    const std::array<int64_t, 4> gk{n, nx, ny, nz};
    std::lock_guard<std::mutex> lk(ctx->grids_mu);
    auto& gs = ctx->grids;
    if (std::find(gs.begin(), gs.end(), gk) == gs.end()) gs.push_back(gk);
}

// A restriction over a registered grid (Options::ell_yblock > 0; its columns are the grid's points):
// the groups of kEllGroup rows of each XCD's eighth (kernels.hip k_rows_ell / k_rows_rpat) in
// (y / yblock, z, y) order of their first row's anchor, so the window of groups in flight is a
// compact (y, z) block of the grid, not whole planes. *d_order stays null otherwise.
int blocked_group_order(pamg_ctx* ctx, const std::vector<int>& anc, int64_t ng, int64_t own_cols, int** d_order) {
    using pamg::kEllGroup;
    const int yb = pamg::options().ell_yblock;
    for (const auto& gr : grids_of(ctx))
        if (yb > 0 && gr[0] == own_cols) {
            const int64_t gnx = gr[1], gny = gr[2], gM = gr[1] * gr[2];
            std::vector<int64_t> key(ng);
            par_for(ng, [&](int64_t a, int64_t b) {
                for (int64_t g = a; g < b; ++g) {
                    const int64_t c = anc[g * kEllGroup];
                    const int64_t y = (c / gnx) % gny, z = c / gM;
                    key[g] = ((y / yb) << 40) | (z << 20) | y;
                }
            });
            const int64_t per = (ng + 7) / 8;
            std::vector<int> order(ng);
            for (int64_t g = 0; g < ng; ++g) order[g] = (int)g;
            for (int64_t e = 0; e < 8; ++e) {
                const int64_t lo = std::min(ng, e * per), hi = std::min(ng, (e + 1) * per);
                std::stable_sort(order.begin() + lo, order.begin() + hi, [&](int p, int q) { return key[p] < key[q]; });
            }
            CHECK(dalloc(d_order, ng));
            CHECK(h2d(ctx, *d_order, order.data(), sizeof(int) * ng));
            break;
        }
    return PAMG_OK;
}

// ---- the layout families' interfaces
// What pamg_mat_upload hands to each family in turn. A->ctx, the shapes, nnz and the plan are
// set; `inner` lists the interior rows no family has taken yet (ascending).
struct Upload {
    pamg_mat* A;
    const PtrVec& rp;                // row pointers, base 0
    const IdxVec& ci;                // columns, base 0 (own columns first, then ghosts)
    const double* val;
    int64_t n_own_cols;
    bool has_all_diag;               // square with a nonzero diagonal in every row
    std::vector<int>& inner;
    const std::vector<int>& bnd;     // the rows with ghost columns (always tiles)
    const std::function<int64_t()>& band;  // the banded tile order's row distance, computed on first use
    UploadTrace& tr;
    int bs = 1;                      // > 1: uploaded through pamg_mat_upload_blocked (bsr_try)
    bool rect = false;               // with bs > 1: through pamg_mat_upload_block_rows (any shape, no diagonal asked)
};
// Every family provides four functions. X_try holds the family's eligibility rule and its
// builder: where it takes the rows it sets its TileSet flag on A->interior and clears
// u.inner; where it declines it leaves both; PAMG_OK either way, an error only for a failed
// allocation or copy. X_free releases the family's device arrays and resets its struct. X_bytes
// is its share of pamg_mat_stream_bytes (0 where it holds no rows). X_report writes its slots and
// bits of pamg_mat_layout's out[10] for tile set t (nothing where t is not its).

// ------------------------------------------------------------------ sym

// Symmetric diagonal-class layout of the interior rows (pamg::SymDia, k_rows_sym), when they
// qualify: <= 2*kSymMaxU+1 distinct row-relative offsets forming a symmetric set with 0, every
// interior row's entries in strictly ascending offset order (so the kernel's ascending sum is
// the storage-order sum of SPEC §S3), and every lower entry bit-identical to its mirror
// a(i-o, i) in row i-o. Otherwise nothing is built and the rows keep their tiles.
int build_sym_dia(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val,
                  const std::vector<int>& inner, const std::function<int64_t()>& get_band) {
    using pamg::kSymMaxU;
    const int64_t n = A->nrows;
    constexpr int kMaxOff = 2 * kSymMaxU + 1;
    // distinct offsets of the interior rows (per thread, merged)
    std::mutex mu;
    std::vector<int> offs;
    std::atomic<bool> too_many{false};
    par_for((int64_t)inner.size(), [&](int64_t a, int64_t b) {
        std::vector<int> loc;
        for (int64_t q = a; q < b && !too_many; ++q) {
            const int i = inner[q];
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                const int o = ci[k] - i;
                if (std::find(loc.begin(), loc.end(), o) == loc.end()) {
                    loc.push_back(o);
                    if ((int)loc.size() > kMaxOff) {
                        too_many = true;
                        return;
                    }
                }
            }
        }
        std::lock_guard<std::mutex> g(mu);
        for (int o : loc)
            if (std::find(offs.begin(), offs.end(), o) == offs.end()) offs.push_back(o);
    });
    if (too_many || (int)offs.size() > kMaxOff) return PAMG_OK;
    std::sort(offs.begin(), offs.end());
    const int no = (int)offs.size();
    if (no % 2 == 0 || offs[no / 2] != 0) return PAMG_OK;
    for (int k = 0; k < no; ++k)
        if (offs[k] != -offs[no - 1 - k]) return PAMG_OK;
    const int nu = no / 2;
    if (nu < 1) return PAMG_OK;  // diagonal-only rows: the tile path (no class to mirror)
    pamg::SymDia sd;
    sd.nu = nu;
    for (int c = 0; c < nu; ++c) sd.off[c] = offs[nu + 1 + c];
    sd.ld = (n + 63) / 64 * 64 + 64;
    const int mb = 2 * nu + 1 <= 7 ? 1 : 2;  // mask bytes per row (kernels.hip SymMask)
    const uint32_t in_flag = mb == 1 ? 0x80u : 0x8000u;
    // (zeroed by parallel loops: 5 GB at 512^3)
    std::vector<uint16_t, NoInitAlloc<uint16_t>> mask(n + kVecPad);
    std::vector<double, NoInitAlloc<double>> dg(n + kVecPad), up((size_t)nu * sd.ld);
    std::vector<char, NoInitAlloc<char>> in_set(n);
    par_for(n + kVecPad, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) {
            mask[i] = 0;
            dg[i] = 0.0;
            if (i < n) in_set[i] = 0;
        }
    });
    par_for((int64_t)up.size(), [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) up[i] = 0.0;
    });
    par_for((int64_t)inner.size(), [&](int64_t a, int64_t b) {
        for (int64_t q = a; q < b; ++q) in_set[inner[q]] = 1;
    });
    auto cls = [&](int o) { return (int)(std::lower_bound(offs.begin(), offs.end(), o) - offs.begin()); };
    std::atomic<bool> bad{false};
    par_for(n, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b && !bad; ++i) {
            // every own row: diagonal and upper values (the mirrors interior rows read)
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                const int o = ci[k] - (int)i;
                if (ci[k] >= n) continue;  // ghost column (boundary rows)
                if (o == 0) dg[i] = val[k];
                else if (o > 0) {
                    const int c = cls(o);
                    if (c < no && offs[c] == o) up[(size_t)(c - nu - 1) * sd.ld + i] = val[k];
                }
            }
            if (!in_set[i]) continue;
            uint32_t m = in_flag;
            int last = -1;
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                const int o = ci[k] - (int)i;
                const int c = cls(o);
                if (c <= last) {  // not strictly ascending
                    bad = true;
                    break;
                }
                last = c;
                m |= 1u << c;
                if (o < 0) {  // the mirror a(i+o, i) must exist with the same bits
                    const int64_t j = i + o;
                    bool found = false;
                    for (int64_t kk = rp[j]; kk < rp[j + 1]; ++kk)
                        if (ci[kk] == (int)i) {
                            found = std::memcmp(&val[kk], &val[k], sizeof(double)) == 0;
                            break;
                        }
                    if (!found) {
                        bad = true;
                        break;
                    }
                }
            }
            mask[i] = (uint16_t)m;
        }
    });
    if (bad) return PAMG_OK;
    // A part of several (a z-slab of whole planes, SymDia::tb_part): the set must be exactly its
    // planes 1 .. nz-2 (the first and last plane read ghosts); its bands are whole planes, so
    // the separate sweeps can run on plane windows (launch_sym_planes)
    const int64_t Mp = nu == 3 ? sd.off[2] : 0;
    const bool whole = A->ncols == n && (int64_t)inner.size() == n;
    bool part = false;
    int plo = 0, phi = 0;
    if (!whole && nu == 3 && Mp > 0 && n % Mp == 0 && n / Mp >= 6 && !inner.empty() && inner.size() % Mp == 0 &&
        inner.front() % Mp == 0) {
        const int nzp = (int)(n / Mp);
        plo = (int)(inner.front() / Mp);
        phi = plo + (int)(inner.size() / Mp);
        part = (plo == 0 || plo == 1) && (phi == nzp || phi == nzp - 1) && phi - plo < nzp;
        for (size_t q = 0; q < inner.size() && part; ++q) part = inner[q] == inner.front() + (int64_t)q;
    }
    // XCD-banded block order (natural order: one band)
    // (a 7-point grid's column reuse gap is one plane less one line, M - nx: no need to measure it —
    // column_reuse_gaps over 938M nonzeros took 0.6 s of the 512^3 upload)
    const bool grid7 = nu == 3 && sd.off[0] == 1 && sd.off[2] % sd.off[1] == 0;
    const int64_t band = grid7 ? (int64_t)sd.off[2] - sd.off[1] : get_band();
    int64_t bd = (pamg::options().tile_order == 1 && band >= 8 * pamg::kBlock) ? band : n;
    if (part && Mp >= 8 * pamg::kBlock) bd = Mp;
    sd.band = (int)bd;
    sd.rpl = pamg::options().sym_rows;
    const int64_t rows_per_block = (int64_t)pamg::kBlock * sd.rpl;
    sd.band_blocks = (int)((bd + rows_per_block - 1) / rows_per_block);
    sd.eighth = (sd.band_blocks + 7) / 8;
    sd.nbands = (int)((n + bd - 1) / bd);
    sd.mask_bytes = mb;
    // Row-class dictionary (Options::sym_vd, two rows per lane): the distinct (mask, D, U_0 ..
    // U_{nu-1}) bit tuples of the own rows in first-occurrence order (chunks scanned in
    // parallel, merged in chunk order — the table one sequential pass builds); a constant-
    // coefficient stencil has one per boundary case (512^3 Poisson: 27)
    std::vector<uint8_t> tid;
    std::vector<double> vtab;
    std::vector<uint32_t> mtab;
    if (pamg::options().sym_vd && sd.rpl == 2) {
        using Key = std::array<uint64_t, 2 + kSymMaxU>;
        auto key_of = [&](int64_t i) {
            Key k{};
            k[0] = mask[i];
            std::memcpy(&k[1], &dg[i], 8);
            for (int c = 0; c < nu; ++c) std::memcpy(&k[2 + c], &up[(size_t)c * sd.ld + i], 8);
            return k;
        };
        const int nch = std::max(1, std::min<int>(host_threads(), (int)(n / 65536)));
        std::vector<std::vector<Key>> firsts(nch);
        std::atomic<bool> over{false};
        {
            std::vector<std::thread> th;
            for (int c = 0; c < nch; ++c)
                th.emplace_back([&, c] {
                    std::vector<Key>& f = firsts[c];
                    int last = -1;
                    for (int64_t i = n * c / nch, e = n * (c + 1) / nch; i < e && !over; ++i) {
                        const Key k = key_of(i);
                        if (last >= 0 && f[last] == k) continue;
                        last = -1;
                        for (int q = 0; q < (int)f.size() && last < 0; ++q)
                            if (f[q] == k) last = q;
                        if (last >= 0) continue;
                        if ((int)f.size() == pamg::kSymVdMax) {
                            over = true;
                            break;
                        }
                        f.push_back(k);
                        last = (int)f.size() - 1;
                    }
                });
            for (auto& x : th) x.join();
        }
        std::vector<Key> tab;
        for (int c = 0; c < nch && !over; ++c)
            for (const Key& k : firsts[c]) {
                if (std::find(tab.begin(), tab.end(), k) != tab.end()) continue;
                if ((int)tab.size() == pamg::kSymVdMax) {
                    over = true;
                    break;
                }
                tab.push_back(k);
            }
        if (!over && !tab.empty()) {
            tid.assign(n + kVecPad, 0);
            par_for(n, [&](int64_t a, int64_t b) {
                int last = 0;
                for (int64_t i = a; i < b; ++i) {
                    const Key k = key_of(i);
                    if (tab[last] != k) last = (int)(std::find(tab.begin(), tab.end(), k) - tab.begin());
                    tid[i] = (uint8_t)last;
                }
            });
            const int nv = (int)tab.size();
            vtab.assign((size_t)nv * (nu + 1) + kVecPad, 0.0);
            mtab.assign(nv + kVecPad, 0u);
            for (int e = 0; e < nv; ++e) {
                mtab[e] = (uint32_t)tab[e][0];
                for (int c = 0; c <= nu; ++c) std::memcpy(&vtab[(size_t)e * (nu + 1) + c], &tab[e][1 + c], 8);
            }
            sd.vd_n = nv;
            // the most frequent class (a grid's interior rows): k_rows_symd's register fast path
            std::vector<int64_t> cnt(nv, 0);
            {
                std::mutex mu;
                par_for(n, [&](int64_t a, int64_t b) {
                    std::vector<int64_t> c(nv, 0);
                    for (int64_t i = a; i < b; ++i) ++c[tid[i]];
                    std::lock_guard<std::mutex> lk(mu);
                    for (int e = 0; e < nv; ++e) cnt[e] += c[e];
                });
            }
            sd.vd_main = (int)(std::max_element(cnt.begin(), cnt.end()) - cnt.begin());
        }
    }
    if (sd.vd_n) {
        CHECK(dalloc(&sd.d_tid, (int64_t)tid.size()));
        CHECK(h2d(A->ctx, sd.d_tid, tid.data(), tid.size()));
        CHECK(dalloc(&sd.d_vtab, (int64_t)vtab.size()));
        CHECK(h2d(A->ctx, sd.d_vtab, vtab.data(), sizeof(double) * vtab.size()));
        CHECK(dalloc(&sd.d_mtab, (int64_t)mtab.size()));
        CHECK(h2d(A->ctx, sd.d_mtab, mtab.data(), sizeof(uint32_t) * mtab.size()));
    } else {
        CHECK(dalloc(&sd.d_mask, (n + kVecPad) * mb));
        CHECK(dalloc(&sd.d_diag, n + kVecPad));
        CHECK(dalloc(&sd.d_upper, (int64_t)nu * sd.ld));
        if (mb == 1) {
            std::vector<uint8_t> m8(mask.begin(), mask.end());
            CHECK(h2d(A->ctx, sd.d_mask, m8.data(), m8.size()));
        } else {
            CHECK(h2d(A->ctx, sd.d_mask, mask.data(), sizeof(uint16_t) * mask.size()));
        }
        CHECK(h2d(A->ctx, sd.d_diag, dg.data(), sizeof(double) * dg.size()));
        CHECK(h2d(A->ctx, sd.d_upper, up.data(), sizeof(double) * up.size()));
    }
    // temporally blocked sweeps (kernels.hip k_sym_tb): one part with every row in the set, a
    // 7-point grid stencil in natural order (classes 1, nx, nx*ny; n = nx*ny*nz) whose rows
    // never reach across a grid line (the -1 / +1 / -nx / +nx classes absent at x = 0 / nx-1 /
    // y = 0 / ny-1), tiles of kTbX x kTbY
    const bool slab = part;  // (a slab of whole planes registers its grid whatever its bands)
    part = part && sd.band == Mp;
    if (nu == 3 && mb == 1 && (whole || slab) && sd.off[0] == 1 && sd.off[2] % sd.off[1] == 0 && n % sd.off[2] == 0) {
        const int nx = sd.off[1], ny = sd.off[2] / sd.off[1];
        const int nz = (int)(n / sd.off[2]);
        // (ok: the blocked sweeps' tiles; reg: the grid registers for a later prolongation / restriction —
        // the neighbour-coded march's tiles, which every kTbX x kTbY grid cuts into as well)
        const bool ok = nx % pamg::kTbX == 0 && ny % pamg::kTbY == 0, reg = ok || pamg::pnc_tiled(nx, ny);
        std::atomic<bool> cross{false};
        if (reg)
            par_for(n, [&](int64_t a0, int64_t b0) {
                for (int64_t i = a0; i < b0 && !cross; ++i) {
                    const int x = (int)(i % nx), y = (int)((i / nx) % ny);
                    const uint32_t m = mask[i];  // ascending classes -M, -nx, -1, 0, 1, nx, M
                    if (((m & 4u) && x == 0) || ((m & 16u) && x == nx - 1) || ((m & 2u) && y == 0) ||
                        ((m & 32u) && y == ny - 1))
                        cross = true;
                }
            });
        if (ok && !cross && (whole || part)) {
            pamg::TbGeom& g = sd.tb;
            g.nx = nx;
            g.ny = ny;
            g.nz = nz;
            g.tiles_x = nx / pamg::kTbX;
            g.tiles_y = ny / pamg::kTbY;
            // about one workgroup per CU (one fits: registers), planes split when a plane has
            // fewer tiles than the chip has CUs
            const int tiles = g.tiles_x * g.tiles_y;
            const int want = std::max(1, (device_cus() + tiles - 1) / tiles);
            g.zchunks = std::max(1, std::min(want, nz / 4 > 0 ? nz / 4 : 1));
            g.zlen = (nz + g.zchunks - 1) / g.zchunks;
            g.zchunks = (nz + g.zlen - 1) / g.zlen;
            g.zlo = 0;
            g.zhi = nz;
            sd.tb_ok = whole;
            sd.tb_part = part;
            sd.part_lo = part ? plo : 0;
            sd.part_hi = part ? phi : nz;
        }
        if (reg && !cross) register_grid(A->ctx, n, nx, ny, nz);
    } else if (nu == 2 && mb == 1 && whole && sd.off[0] == 1 && n % sd.off[1] == 0) {
        // one plane of such a grid (a 5-point stencil: classes -nx, -1, 0, 1, nx): registered alone
        const int nx = sd.off[1], ny = (int)(n / sd.off[1]);
        std::atomic<bool> cross{false};
        if (pamg::pnc_tiled(nx, ny)) {
            par_for(n, [&](int64_t a0, int64_t b0) {
                for (int64_t i = a0; i < b0 && !cross; ++i) {
                    const int x = (int)(i % nx), y = (int)(i / nx);
                    const uint32_t m = mask[i];
                    if (((m & 2u) && x == 0) || ((m & 8u) && x == nx - 1) || ((m & 1u) && y == 0) ||
                        ((m & 16u) && y == ny - 1))
                        cross = true;
                }
            });
            if (!cross) register_grid(A->ctx, n, nx, ny, 1);
        }
    }
    A->sym = sd;
    A->interior.sym = true;
    A->interior.rows_short = (int64_t)inner.size();
    return PAMG_OK;
}

int sym_try(Upload& u) {
    pamg_mat* A = u.A;
    if (pamg::options().sym_dia && u.n_own_cols == A->nrows && u.has_all_diag && !u.inner.empty())
        CHECK(build_sym_dia(A, u.rp, u.ci, u.val, u.inner, u.band));
    if (A->interior.sym) u.inner.clear();  // the interior rows run in k_rows_sym, not in tiles
    u.tr.mark("sym dia");
    return PAMG_OK;
}

void sym_free(pamg::SymDia& S) {
    dfree(S.d_mask);
    dfree(S.d_diag);
    dfree(S.d_upper);
    dfree(S.d_tid);
    dfree(S.d_vtab);
    dfree(S.d_mtab);
    S = pamg::SymDia{};
}

// 8/16-bit mask, diagonal and nu upper values per row (the mirrored lower values are the same
// lines, re-read from cache)
int64_t sym_bytes(const pamg_mat* A) {
    if (!A->interior.sym) return 0;
    const int64_t nrows = A->nrows;
    return A->sym.vd_n ? nrows + (int64_t)A->sym.vd_n * (8 * (A->sym.nu + 1) + 4)
                       : nrows * (A->sym.mask_bytes + 8 + 8 * (int64_t)A->sym.nu);
}

void sym_report(const pamg_mat* A, const pamg::TileSet& t, int out[10]) {
    if (!t.sym) return;
    out[4] = A->sym.nu;  // upper classes, k_rows_sym's grid
    out[8] = A->sym.nbands * 8 * A->sym.eighth;
    out[9] |= 8 | (A->sym.rpl == 2 ? 16 : 0) | (A->sym.tb_ok || A->sym.tb_part ? 32 : 0) | (A->sym.vd_n ? 128 : 0);
}

// ------------------------------------------------------------------ rpat

// Pattern-dictionary rows (Options::rpat, pamg::RpatSet): a restriction whose rows, as (column - first
// column, value bits) sequences, repeat at most kRpatMax patterns (<= kRpatEnt entries, <= 256 values,
// offsets < 2^24, rows of 1 .. kRpatMaxLen entries). Declines (leaves ELL / tiles to the caller)
// otherwise. The patterns are numbered in first-appearance order (chunks scanned in parallel, merged
// in chunk order: the numbering one sequential pass gives).
int build_rpat(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val, const std::vector<int>& inner) {
    using pamg::kRpatEnt;
    using pamg::kRpatMax;
    using pamg::kRpatMaxLen;
    using pamg::kRpatSkip;
    const int64_t n = A->nrows;
    if (n <= 0) return PAMG_OK;
    std::vector<char> in_set;
    if ((int64_t)inner.size() != n) {
        in_set.assign(n, 0);
        for (int i : inner) in_set[i] = 1;
    }
    auto member = [&](int64_t i) { return in_set.empty() || in_set[i]; };
    // a row's pattern key: length, offsets, value bits
    auto row_hash = [&](int64_t i) {
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(rp[i + 1] - rp[i]);
        const int64_t c0 = ci[rp[i]];
        for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
            uint64_t u;
            std::memcpy(&u, &val[k], 8);
            h = (h ^ (uint64_t)(ci[k] - c0)) * 0x100000001B3ull;
            h = (h ^ u) * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
        }
        return h;
    };
    auto same = [&](int64_t i, int64_t j) {
        const int64_t L = rp[i + 1] - rp[i];
        if (L != rp[j + 1] - rp[j]) return false;
        const int64_t ci0 = ci[rp[i]], cj0 = ci[rp[j]];
        for (int64_t k = 0; k < L; ++k) {
            if (ci[rp[i] + k] - ci0 != ci[rp[j] + k] - cj0) return false;
            if (std::memcmp(&val[rp[i] + k], &val[rp[j] + k], 8) != 0) return false;
        }
        return true;
    };
    // pass 1: each chunk's distinct patterns (hash, representative row) in first-appearance order
    const int nch = std::max(1, std::min<int>(host_threads() * 4, (int)(n / 65536)));
    std::vector<std::vector<std::pair<uint64_t, int64_t>>> firsts(nch);
    std::atomic<bool> ok{true};
    {
        std::vector<std::thread> th;
        const int nt = std::min(nch, host_threads());
        std::atomic<int> next{0};
        for (int t = 0; t < nt; ++t)
            th.emplace_back([&] {
                for (int c; ok && (c = next.fetch_add(1)) < nch;) {
                    auto& f = firsts[c];
                    int last = -1;
                    for (int64_t i = n * c / nch, e = n * (c + 1) / nch; i < e && ok; ++i) {
                        if (!member(i)) continue;
                        const int64_t L = rp[i + 1] - rp[i];
                        if (L < 1 || L > kRpatMaxLen) {
                            ok = false;
                            break;
                        }
                        for (int64_t k = rp[i] + 1; k < rp[i + 1]; ++k)
                            if (ci[k] <= ci[k - 1] || (int64_t)ci[k] - ci[rp[i]] >= (int64_t(1) << 24)) ok = false;
                        const uint64_t h = row_hash(i);
                        if (last >= 0 && f[last].first == h && same(f[last].second, i)) continue;
                        last = -1;
                        for (int q = 0; q < (int)f.size() && last < 0; ++q)
                            if (f[q].first == h && same(f[q].second, i)) last = q;
                        if (last >= 0) continue;
                        if ((int)f.size() == kRpatMax) {
                            ok = false;
                            break;
                        }
                        f.emplace_back(h, i);
                        last = (int)f.size() - 1;
                    }
                }
            });
        for (auto& x : th) x.join();
    }
    if (!ok) return PAMG_OK;
    std::vector<std::pair<uint64_t, int64_t>> pats;  // (hash, representative row)
    for (int c = 0; c < nch; ++c)
        for (const auto& e : firsts[c]) {
            bool seen = false;
            for (const auto& q : pats) seen = seen || (q.first == e.first && same(q.second, e.second));
            if (seen) continue;
            if ((int)pats.size() == kRpatMax) return PAMG_OK;
            pats.push_back(e);
        }
    if (pats.empty()) return PAMG_OK;
    // the entries and the value table
    std::vector<int2> pmeta(pats.size());
    std::vector<uint32_t> pent;
    std::vector<uint64_t> vals;
    for (size_t p = 0; p < pats.size(); ++p) {
        const int64_t r = pats[p].second;
        pmeta[p] = make_int2((int)pent.size(), (int)(rp[r + 1] - rp[r]));
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
            uint64_t u;
            std::memcpy(&u, &val[k], 8);
            size_t vi = std::find(vals.begin(), vals.end(), u) - vals.begin();
            if (vi == vals.size()) {
                if (vals.size() == 256) return PAMG_OK;
                vals.push_back(u);
            }
            pent.push_back((uint32_t)(ci[k] - ci[rp[r]]) | ((uint32_t)vi << 24));
        }
        if ((int)pent.size() > kRpatEnt) return PAMG_OK;
    }
    // pass 2: every row's pattern id (hash lookup, full compare) and first column
    std::vector<std::pair<uint64_t, int>> byhash(pats.size());
    for (size_t p = 0; p < pats.size(); ++p) byhash[p] = {pats[p].first, (int)p};
    std::sort(byhash.begin(), byhash.end());
    std::vector<uint8_t> pid(n + kVecPad, (uint8_t)kRpatSkip);
    std::vector<int> anc(n + kVecPad, 0);
    par_for(n, [&](int64_t a, int64_t b) {
        int last = -1;
        for (int64_t i = a; i < b; ++i) {
            anc[i] = rp[i + 1] > rp[i] ? ci[rp[i]] : 0;
            if (!member(i)) continue;
            if (last >= 0 && same(pats[last].second, i)) {
                pid[i] = (uint8_t)last;
                continue;
            }
            const uint64_t h = row_hash(i);
            last = -1;
            for (auto it = std::lower_bound(byhash.begin(), byhash.end(), std::make_pair(h, -1));
                 it != byhash.end() && it->first == h && last < 0; ++it)
                if (same(pats[it->second].second, i)) last = it->second;
            if (last < 0) {  // (cannot happen: every row's pattern was collected in pass 1)
                ok = false;
                return;
            }
            pid[i] = (uint8_t)last;
        }
    });
    if (!ok) return PAMG_OK;
    std::vector<double> vtab(vals.size());
    for (size_t e = 0; e < vals.size(); ++e) std::memcpy(&vtab[e], &vals[e], 8);
    pamg::RpatSet& R = A->rpat;
    pamg_ctx* ctx = A->ctx;
    R.ngroups = (n + pamg::kEllGroup - 1) / pamg::kEllGroup;
    R.npat = (int)pats.size();
    R.nent = (int)pent.size();
    R.nval = (int)vals.size();
    CHECK(dalloc(&R.d_anc, n + kVecPad));
    CHECK(dalloc(&R.d_pid, n + kVecPad));
    CHECK(dalloc(&R.d_pmeta, R.npat));
    CHECK(dalloc(&R.d_pent, R.nent));
    CHECK(dalloc(&R.d_vtab, R.nval));
    CHECK(h2d(ctx, R.d_anc, anc.data(), sizeof(int) * anc.size()));
    CHECK(h2d(ctx, R.d_pid, pid.data(), pid.size()));
    CHECK(h2d(ctx, R.d_pmeta, pmeta.data(), sizeof(int2) * pmeta.size()));
    CHECK(h2d(ctx, R.d_pent, pent.data(), sizeof(uint32_t) * pent.size()));
    CHECK(h2d(ctx, R.d_vtab, vtab.data(), sizeof(double) * vtab.size()));
    CHECK(blocked_group_order(ctx, anc, R.ngroups, A->plan ? A->plan->n_own : A->ncols, &R.d_gorder));
    A->interior.rpat = true;
    return PAMG_OK;
}

// restrictions whose rows repeat few patterns (an aggregate shape each); several parts: the interior
// rows, when they are >= 3/4 of the operator — a 512^3 z-slab part's level 1
int rpat_try(Upload& u) {
    pamg_mat* A = u.A;
    const int64_t nrows = A->nrows;
    if (pamg::options().rpat && !A->interior.sym && u.n_own_cols > nrows && nrows > 0 &&
        (int64_t)u.inner.size() * 4 >= (int64_t)nrows * 3) {
        CHECK(build_rpat(A, u.rp, u.ci, u.val, u.inner));
        if (A->interior.rpat) u.inner.clear();  // the rows run in k_rows_rpat, not in tiles
        u.tr.mark("rpat");
    }
    return PAMG_OK;
}

// the first column and the pattern id per row, the tables
int64_t rpat_bytes(const pamg_mat* A) {
    if (!A->interior.rpat) return 0;
    return 5 * A->nrows + 8 * A->rpat.npat + 4 * A->rpat.nent + 8 * A->rpat.nval;
}

void rpat_report(const pamg_mat* A, const pamg::TileSet& t, int out[10]) {
    if (!t.rpat) return;
    out[3] = A->rpat.nval;  // the pattern and value tables, k_rows_rpat's grid
    out[4] = A->rpat.npat;
    out[8] = (int)A->rpat.ngroups;
    out[9] |= 2048;
}

void rpat_free(pamg::RpatSet& R) {
    dfree(R.d_anc);
    dfree(R.d_pid);
    dfree(R.d_pmeta);
    dfree(R.d_pent);
    dfree(R.d_vtab);
    dfree(R.d_gorder);
    R = pamg::RpatSet{};
}

// ------------------------------------------------------------------ ell

// Windowed sliced ELL (Options::ell_xwin, pamg::EllSet::win; k_rows_ellw): the whole of a square
// one-part operator. The slices and their index streams are build_ell's; a workgroup's 4 slices are
// chosen by coupling instead of 4g .. 4g+3, so that their rows read a compact set of columns (the
// 512^3 A1: 64 x 2 x 2 aggregates, 3.1 nonzeros per window entry against 1.9 for 256 consecutive
// rows), and that set — runs of consecutive columns — is what the kernel loads into LDS in place of
// the per-nonzero gathers. Greedy grouping: the lowest unassigned slice, then three times the
// unassigned slice holding the most columns of the group's nonzeros (ties: the lower slice) among
// the best six whose pairs keep the group's (offset, value) dictionary within 256; none of the six
// fits: the group closes short. Declines (build_ell goes on with consecutive groups) where a slice
// alone holds more than 256 pairs or the operator misses the acceptance thresholds (pamg_device.h).
int build_ell_xwin(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val,
                   const std::vector<int2>& smeta, int64_t words) {
    using pamg::kEllW;
    const int64_t n = A->nrows, ns = (n + kEllW - 1) / kEllW;
    const int cap = std::min(pamg::options().ell_xwin_max, pamg::kEllWinCap);
    auto pair_key = [](int off, uint64_t u) {
        uint64_t h = (u ^ (u >> 29)) * 0x9E3779B97F4A7C15ull + (uint64_t)(uint32_t)off * 0xC2B2AE3D27D4EB4Full;
        return h ^ (h >> 32);
    };
    // per slice: its distinct pairs (64-bit keys, sorted) and the slices its columns fall in
    std::vector<std::vector<uint64_t>> spair(ns);
    std::vector<std::vector<std::pair<int, int>>> scoup(ns);
    std::atomic<bool> ok{true};
    par_for(ns, [&](int64_t a, int64_t b) {
        std::vector<uint64_t> h;
        std::vector<int> t;
        for (int64_t q = a; q < b && ok; ++q) {
            h.clear();
            t.clear();
            for (int64_t i = q * kEllW; i < std::min(n, (q + 1) * kEllW); ++i)
                for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                    uint64_t u;
                    std::memcpy(&u, &val[k], 8);
                    h.push_back(pair_key(ci[k] - (int)i, u));
                    t.push_back(ci[k] / kEllW);
                }
            std::sort(h.begin(), h.end());
            h.erase(std::unique(h.begin(), h.end()), h.end());
            if (h.size() > 256) ok = false;
            spair[q] = h;
            std::sort(t.begin(), t.end());
            for (size_t e = 0; e < t.size();) {
                size_t f = e;
                while (f < t.size() && t[f] == t[e]) ++f;
                if (t[e] != q) scoup[q].push_back({t[e], (int)(f - e)});
                e = f;
            }
        }
    });
    if (!ok) return PAMG_OK;
    // the greedy pass (serial: a few candidates per slice)
    std::vector<std::array<int, 4>> grp;
    grp.reserve(ns / 4 + 1);
    {
        std::vector<char> done(ns, 0);
        std::vector<int> score(ns, 0), touched, cand;
        std::vector<uint64_t> un, tmp;
        auto couple = [&](int q) {
            for (const auto& c : scoup[q])
                if (!done[c.first]) {
                    if (score[c.first] == 0) touched.push_back(c.first);
                    score[c.first] += c.second;
                }
        };
        for (int64_t first = 0; first < ns; ++first) {
            if (done[first]) continue;
            std::array<int, 4> g = {(int)first, -1, -1, -1};
            done[first] = 1;
            un = spair[first];
            touched.clear();
            couple((int)first);
            for (int m = 1; m < 4; ++m) {
                cand.clear();
                for (int t : touched)
                    if (!done[t]) cand.push_back(t);
                if (cand.empty()) {  // nothing coupled is left: the next slice in row order
                    int64_t t = first + 1;
                    while (t < ns && done[t]) ++t;
                    if (t < ns) cand.push_back((int)t);
                }
                const size_t top = std::min<size_t>(6, cand.size());
                std::partial_sort(cand.begin(), cand.begin() + top, cand.end(), [&](int p, int q) {
                    return score[p] != score[q] ? score[p] > score[q] : p < q;
                });
                int take = -1;
                for (size_t c = 0; c < top && take < 0; ++c) {
                    tmp.clear();
                    std::set_union(un.begin(), un.end(), spair[cand[c]].begin(), spair[cand[c]].end(),
                                   std::back_inserter(tmp));
                    if (tmp.size() <= 256) take = cand[c];
                }
                if (take < 0) break;
                un.swap(tmp);
                g[m] = take;
                done[take] = 1;
                couple(take);
            }
            for (int t : touched) score[t] = 0;
            grp.push_back(g);
        }
    }
    std::vector<std::vector<std::pair<int, int>>>().swap(scoup);
    std::vector<std::vector<uint64_t>>().swap(spair);
    const int64_t ng = (int64_t)grp.size();
    // per group: the pair table and the index bytes (as build_ell), the window's runs, chunks and lof words
    std::vector<std::vector<int>> goff(ng);
    std::vector<std::vector<uint64_t>> gval(ng);
    std::vector<std::vector<int2>> gchunk(ng);
    std::vector<std::vector<uint16_t>> glof(ng);
    std::vector<int> gwin(ng, 0), gruns(ng, 0);
    std::vector<int64_t> gnnz(ng, 0);
    // (group pairs, below: every windowed group's runs and, per lof word, the first lane that reads it)
    const bool span2 = pamg::options().ell_xwin <= 2;  // (3, 4: single groups only)
    std::vector<pamg::EllRuns> gwruns(span2 ? ng : 0);
    std::vector<std::vector<uint8_t>> glmin(span2 ? ng : 0);
    std::vector<uint32_t> cw(words + 1, 0u);
    std::vector<uint8_t> len(n + kVecPad, 0), dpos(n + kVecPad, (uint8_t)255);
    par_for(ng, [&](int64_t a, int64_t b) {
        constexpr int kSlots = 1024;
        std::vector<int> pid(kSlots), pstamp(kSlots, -1), pkey_o(kSlots);
        std::vector<uint64_t> pkey_v(kSlots);
        std::vector<int> o, lmin(4 * 256), lmax(4 * 256);
        std::vector<uint64_t> v;
        std::vector<std::array<int, 2>> rng;
        std::vector<std::array<int, 3>> runs;  // (first column, end, slot)
        for (int64_t g = a; g < b && ok; ++g) {
            const int stamp = (int)(g - a);
            o.clear();
            v.clear();
            for (int w = 0; w < 4 && ok; ++w) {
                const int64_t q = grp[g][w];
                if (q < 0) continue;
                for (int64_t i = q * kEllW; i < std::min(n, (q + 1) * kEllW) && ok; ++i) {
                    len[i] = (uint8_t)(rp[i + 1] - rp[i]);
                    gnnz[g] += rp[i + 1] - rp[i];
                    const int lane = (int)(i % kEllW);
                    for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                        const int kk = (int)(k - rp[i]);
                        const int off = ci[k] - (int)i;
                        if (off == 0) dpos[i] = (uint8_t)kk;
                        uint64_t u;
                        std::memcpy(&u, &val[k], 8);
                        uint32_t h = (uint32_t)((((uint64_t)(uint32_t)off * 0x9E3779B1u) ^ u ^ (u >> 29)) *
                                                0x9E3779B97F4A7C15ull >> 54);
                        while (pstamp[h] == stamp && (pkey_o[h] != off || pkey_v[h] != u)) h = (h + 1) & (kSlots - 1);
                        if (pstamp[h] != stamp) {
                            if (o.size() == 256) {  // (two pairs with one 64-bit key in the greedy's count)
                                ok = false;
                                break;
                            }
                            pstamp[h] = stamp;
                            pkey_o[h] = off;
                            pkey_v[h] = u;
                            pid[h] = (int)o.size();
                            for (int x = 0; x < 4; ++x) {
                                lmin[x * 256 + pid[h]] = kEllW;
                                lmax[x * 256 + pid[h]] = -1;
                            }
                            o.push_back(off);
                            v.push_back(u);
                        }
                        const int p = pid[h];
                        lmin[w * 256 + p] = std::min(lmin[w * 256 + p], lane);
                        lmax[w * 256 + p] = std::max(lmax[w * 256 + p], lane);
                        const int64_t wd = smeta[q].x + (int64_t)(kk / 4) * kEllW + lane;
                        cw[wd] |= (uint32_t)p << (8 * (kk % 4));
                    }
                }
            }
            if (!ok) break;
            goff[g] = o;
            gval[g] = v;
            const int np = (int)o.size();
            // the column ranges the waves read per pair, merged into runs that start on 16 bytes
            // (ranges up to a cache line apart share a run)
            rng.clear();
            for (int w = 0; w < 4; ++w)
                for (int p = 0; p < np; ++p)
                    if (grp[g][w] >= 0 && lmax[w * 256 + p] >= 0) {
                        const int c0 = grp[g][w] * kEllW + o[p];
                        rng.push_back({c0 + lmin[w * 256 + p], c0 + lmax[w * 256 + p]});
                    }
            std::sort(rng.begin(), rng.end());
            runs.clear();
            for (const auto& r : rng) {
                const int s = r[0] & ~1, e = (r[1] + 2) & ~1;
                if (!runs.empty() && s <= runs.back()[1] + 16) runs.back()[1] = std::max(runs.back()[1], e);
                else runs.push_back({s, e, 0});
            }
            int slots = 0, nch = 0;
            for (auto& r : runs) {
                r[2] = slots;
                slots += r[1] - r[0];
                nch += (r[1] - r[0] + 127) / 128;
            }
            if (slots == 0 || slots > cap || nch > pamg::kEllWinChunks) continue;  // a gather group
            // (every load stays inside x and its pad: real columns, rounded to pairs)
            if (runs.front()[0] < 0 || runs.back()[1] > ((int)A->ncols + 1)) continue;
            gwin[g] = slots;
            gruns[g] = (int)runs.size();
            for (const auto& r : runs)
                for (int c = r[0]; c < r[1]; c += 128)
                    gchunk[g].push_back(make_int2(c, (r[2] + c - r[0]) | (std::min(128, r[1] - c) / 2) << 16));
            glof[g].assign((size_t)4 * np, (uint16_t)64);
            if (span2) {
                gwruns[g] = runs;
                glmin[g].assign((size_t)4 * np, (uint8_t)255);
            }
            for (int w = 0; w < 4; ++w)
                for (int p = 0; p < np; ++p) {
                    uint16_t word = 64;
                    if (grp[g][w] >= 0 && lmax[w * 256 + p] >= 0) {
                        const int c0 = grp[g][w] * kEllW + o[p], c = c0 + lmin[w * 256 + p];
                        size_t r = 0;
                        while (r + 1 < runs.size() && runs[r + 1][0] <= c) ++r;
                        word = (uint16_t)(runs[r][2] + c0 - runs[r][0] + 64);
                        if (span2) glmin[g][(size_t)w * np + p] = (uint8_t)lmin[w * 256 + p];
                    }
                    glof[g][(size_t)w * np + p] = word;
                }
        }
    });
    if (!ok) return PAMG_OK;
    // Occupancy: a workgroup's LDS is the operator's largest window + 4 KB of tables, and the kernel
    // lives on the waves in flight (512^3 A1, windows up to 3552: 4 workgroups per CU 0.42 ms, capped
    // at 2816 — 6 per CU, 14 % of the groups gathering — 0.38 ms). So the largest window is lowered to
    // what k workgroups per CU allow, for the largest k <= 8 that keeps kEllWinKeep percent of the
    // windowed groups; the groups above it gather.
    {
        int64_t have = 0;
        for (int64_t g = 0; g < ng; ++g) have += gwin[g] > 0;
        for (int k = 8; k >= 2 && have > 0; --k) {
            const int fit = ((pamg::kEllLdsPerCu / k - 2048) / 8 - 256) & ~1;
            int64_t keep = 0;
            for (int64_t g = 0; g < ng; ++g) keep += gwin[g] > 0 && gwin[g] <= fit;
            if (keep * 100 < pamg::kEllWinKeep * have) continue;
            for (int64_t g = 0; g < ng; ++g)
                if (gwin[g] > fit) {
                    gwin[g] = 0;
                    gchunk[g].clear();
                    glof[g].clear();
                    if (span2) gwruns[g].clear();
                }
            break;
        }
    }
    pamg::EllSet& E = A->ell;
    int64_t win_nnz = 0, win_slots = 0, win_runs = 0, win_pairs = 0;
    for (int64_t g = 0; g < ng; ++g) {
        E.max_pairs = std::max(E.max_pairs, (int)goff[g].size());
        bool contig = true;
        for (int w = 1; w < 4; ++w) contig = contig && (grp[g][w] < 0 || grp[g][w] == grp[g][0] + w);
        if (gwin[g] > 0) {
            ++E.win_groups;
            win_nnz += gnnz[g];
            win_slots += gwin[g];
            E.max_window = std::max(E.max_window, gwin[g]);
            E.max_chunks = std::max(E.max_chunks, (int)gchunk[g].size());
            if (!contig) ++E.noncontig_groups;
            win_runs += gruns[g];
            win_pairs += (int64_t)goff[g].size();
            E.max_runs = std::max(E.max_runs, gruns[g]);
            if (grp[g][3] >= 0) ++E.full_groups;
        } else {
            ++E.gather_groups;
        }
    }
    if ((int64_t)E.win_groups * 100 < pamg::kEllWinMinShare * ng || win_nnz * 100 < pamg::kEllWinMinRatio100 * win_slots) {
        E = pamg::EllSet{};
        return PAMG_OK;
    }
    {
        std::vector<int> ws;
        for (int64_t g = 0; g < ng; ++g)
            if (gwin[g] > 0) ws.push_back(gwin[g]);
        std::sort(ws.begin(), ws.end());
        E.p95_window = ws[(ws.size() - 1) * 95 / 100];
        E.mean_window = (int)(win_slots / E.win_groups);
        E.mean_runs = (int)(win_runs / E.win_groups);
        E.mean_pairs = (int)(win_pairs / E.win_groups);
    }
    // Group pairs (Options::ell_xwin 1 | 2; pamg_device.h, ell_span.h): windowed groups coupled two
    // and two where their union window pays, the groups renumbered pairs first — pair p = groups 2p,
    // 2p + 1, then the rest in their order (no pair: nothing moves, the layout is span 1's) —; a pair's
    // chunks are its union window's, stored with its first group, and both groups' lof words point
    // into that window.
    std::vector<int> gunion(ng, 0);  // per renumbered group: its pair's union window (0: single)
    if (span2) {
        std::vector<int> sgroup(ns, -1);
        for (int64_t g = 0; g < ng; ++g)
            for (int w = 0; w < 4; ++w)
                if (grp[g][w] >= 0) sgroup[grp[g][w]] = (int)g;
        const std::vector<std::pair<int, int>> prs =
            pamg::ell_span_pairs(gwruns, gwin, sgroup, kEllW, std::min(cap, pamg::kEllSpanWin), pamg::kEllSpanChunks,
                                 pamg::kEllSpanShare);
        E.npairs = (int)prs.size();
        if (E.npairs > 0) {
            std::vector<int> order;
            std::vector<char> paired(ng, 0);
            order.reserve(ng);
            for (const auto& pr : prs) {
                order.push_back(pr.first);
                order.push_back(pr.second);
                paired[pr.first] = paired[pr.second] = 1;
            }
            for (int64_t g = 0; g < ng; ++g)
                if (!paired[g]) order.push_back((int)g);
            auto permute = [&](auto& v) {
                std::remove_reference_t<decltype(v)> t(v.size());
                for (int64_t g = 0; g < ng; ++g) t[g] = std::move(v[order[g]]);
                v.swap(t);
            };
            permute(grp);
            permute(goff);
            permute(gval);
            permute(gchunk);
            permute(glof);
            permute(gwin);
            permute(gwruns);
            permute(glmin);
            std::vector<int> usz(E.npairs);
            int64_t usum = 0, upct = 0;
            par_for(E.npairs, [&](int64_t a, int64_t b) {
                pamg::EllRuns uni;
                for (int64_t p = a; p < b; ++p) {
                    int nch = 0;
                    usz[p] = pamg::ell_span_union(gwruns[2 * p], gwruns[2 * p + 1], uni, nch);
                    gchunk[2 * p].clear();
                    gchunk[2 * p + 1].clear();
                    for (const auto& r : uni)
                        for (int c = r[0]; c < r[1]; c += 128)
                            gchunk[2 * p].push_back(make_int2(c, (r[2] + c - r[0]) | (std::min(128, r[1] - c) / 2) << 16));
                    for (int64_t g = 2 * p; g < 2 * p + 2; ++g) {
                        for (size_t e = 0; e < glof[g].size(); ++e)  // (255: no lane of the wave reads the pair)
                            if (glmin[g][e] != 255)
                                glof[g][e] = pamg::ell_span_relof(glof[g][e], glmin[g][e], gwruns[g], uni);
                        gunion[g] = usz[p];
                    }
                }
            });
            for (int p = 0; p < E.npairs; ++p) {
                usum += usz[p];
                upct += (int64_t)usz[p] * 100 / (gwin[2 * p] + gwin[2 * p + 1]);
                E.max_union = std::max(E.max_union, usz[p]);
            }
            std::sort(usz.begin(), usz.end());
            E.p95_union = usz[(usz.size() - 1) * 95 / 100];
            E.mean_union = (int)(usum / E.npairs);
            E.union_pct = (int)(upct / E.npairs);
        }
        std::vector<pamg::EllRuns>().swap(gwruns);
        std::vector<std::vector<uint8_t>>().swap(glmin);
    }
    std::vector<int4> gmeta(ng), wmeta(ng), gsl(ng);
    int64_t on = 0, cn = 0, ln = 0;
    for (int64_t g = 0; g < ng; ++g) {
        const int np = (int)goff[g].size();
        gmeta[g] = make_int4((int)on, np, (int)on, np);
        // (a paired group: .y 0 — alone, where x is not 16-byte aligned, it gathers — and .w its pair's window)
        wmeta[g] = make_int4((int)cn, gunion[g] ? 0 : (int)gchunk[g].size(), (int)ln, gunion[g] ? gunion[g] : gwin[g]);
        gsl[g] = make_int4(grp[g][0], grp[g][1], grp[g][2], grp[g][3]);
        on += np;
        cn += (int64_t)gchunk[g].size();
        ln += (int64_t)glof[g].size();
    }
    if (ln >= INT32_MAX || cn >= INT32_MAX) {
        E = pamg::EllSet{};
        return PAMG_OK;
    }
    std::vector<int4> prec((size_t)4 * E.npairs);
    for (int p = 0; p < E.npairs; ++p) {
        const int a = 2 * p, b = a + 1;
        prec[4 * p] = gsl[a];
        prec[4 * p + 1] = gsl[b];
        prec[4 * p + 2] = make_int4(gmeta[a].x, gmeta[a].y, gmeta[b].x, gmeta[b].y);
        prec[4 * p + 3] = make_int4(wmeta[a].x, (int)gchunk[a].size() | gunion[a] << 16, wmeta[a].z, wmeta[b].z);
    }
    std::vector<int> otab(on + 1, 0);
    std::vector<double> vtab(on + 1, 0.0);
    std::vector<int2> chunks(cn + 1, make_int2(0, 0));
    std::vector<uint16_t> lof(ln + 2, (uint16_t)0);
    par_for(ng, [&](int64_t a, int64_t b) {
        for (int64_t g = a; g < b; ++g) {
            std::copy(goff[g].begin(), goff[g].end(), otab.begin() + gmeta[g].x);
            for (size_t e = 0; e < gval[g].size(); ++e) std::memcpy(&vtab[gmeta[g].x + e], &gval[g][e], 8);
            std::copy(gchunk[g].begin(), gchunk[g].end(), chunks.begin() + wmeta[g].x);
            std::copy(glof[g].begin(), glof[g].end(), lof.begin() + wmeta[g].z);
        }
    });
    // Row classes (Options::ell_xwin 1 | 3 — 2 | 4 keep the per-row stream —, EllSet::cls): the rows of a slice in classes of equal length,
    // diagonal position and pair bytes (the stream's padding bytes are 0, so equal dwords and equal
    // lengths are equal rows), numbered by first appearance; the slice then stores one padded row per
    // class, class-interleaved, and a class byte per row. Taken where that is at most half of the
    // per-row stream's bytes (the 512^3 A1: ~6 classes per slice of 64 rows).
    std::vector<int2> smeta_c;
    std::vector<uint32_t> ccw;
    std::vector<uint8_t> cid;
    if (pamg::options().ell_xwin == 1 || pamg::options().ell_xwin == 3) {
        std::vector<int> snc(ns, 0), smin(ns, 0);
        cid.assign(n + kVecPad, 0);
        par_for(ns, [&](int64_t a, int64_t b) {
            int rep[kEllW];
            for (int64_t q = a; q < b; ++q) {
                const int nq = (smeta[q].y + 3) / 4;
                const int64_t r0 = q * kEllW, s0 = smeta[q].x;
                const int rows = (int)std::min<int64_t>(n - r0, kEllW);
                int nc = 0;
                for (int l = 0; l < rows; ++l) {
                    int c = 0;
                    for (; c < nc; ++c) {
                        const int m = rep[c];
                        bool same = len[r0 + l] == len[r0 + m] && dpos[r0 + l] == dpos[r0 + m];
                        for (int k = 0; k < nq && same; ++k) same = cw[s0 + (int64_t)k * kEllW + l] == cw[s0 + (int64_t)k * kEllW + m];
                        if (same) break;
                    }
                    if (c == nc) rep[nc++] = l;
                    cid[r0 + l] = (uint8_t)c;
                }
                snc[q] = nc;
                // the slice's shortest row (a partial slice: 0 — its idle lanes hold no row)
                int lmin = rows == kEllW ? 255 : 0;
                for (int l = 0; l < rows; ++l) lmin = std::min<int>(lmin, len[r0 + l]);
                smin[q] = lmin;
            }
        });
        smeta_c.resize(ns);
        int64_t cwords = 0;
        for (int64_t q = 0; q < ns; ++q) {
            smeta_c[q] = make_int2((int)cwords, smeta[q].y | smin[q] << 8 | snc[q] << 16);
            cwords += (int64_t)snc[q] * ((smeta[q].y + 3) / 4);
            E.cls_total += snc[q];
            E.cls_max = std::max(E.cls_max, snc[q]);
        }
        if (2 * (4 * cwords + n) <= 4 * words) {
            E.cls = true;
            E.cls_words = cwords;
            ccw.assign(cwords + 1, 0u);
            par_for(ns, [&](int64_t a, int64_t b) {
                for (int64_t q = a; q < b; ++q) {
                    const int nq = (smeta[q].y + 3) / 4, nc = snc[q];
                    const int64_t r0 = q * kEllW, s0 = smeta[q].x;
                    const int rows = (int)std::min<int64_t>(n - r0, kEllW);
                    for (int l = 0; l < rows; ++l)  // (every row of a class writes the same dwords)
                        for (int k = 0; k < nq; ++k)
                            ccw[smeta_c[q].x + (int64_t)k * nc + cid[r0 + l]] = cw[s0 + (int64_t)k * kEllW + l];
                }
            });
            std::vector<uint32_t>().swap(cw);
        } else {
            E.cls_total = 0;
            E.cls_max = 0;
        }
    }
    const std::vector<int2>& sm_up = E.cls ? smeta_c : smeta;
    const std::vector<uint32_t>& cw_up = E.cls ? ccw : cw;
    const int64_t up_words = E.cls ? E.cls_words : words;
    pamg_ctx* ctx = A->ctx;
    E.nslices = ns;
    E.ngroups = ng;
    E.words = words;
    E.otab_n = on;
    E.vtab_n = on;
    E.paired = true;
    E.win = true;
    E.nchunks = cn;
    E.lof_n = ln;
    CHECK(dalloc(&E.d_smeta, ns));
    CHECK(dalloc(&E.d_ci, up_words + 1));
    if (E.cls) {
        CHECK(dalloc(&E.d_cid, n + kVecPad));
        CHECK(h2d(ctx, E.d_cid, cid.data(), cid.size()));
    }
    CHECK(dalloc(&E.d_len, n + kVecPad));
    CHECK(dalloc(&E.d_gmeta, ng));
    CHECK(dalloc(&E.d_otab, on + 1));
    CHECK(dalloc(&E.d_vtab, on + 1));
    CHECK(dalloc(&E.d_gslices, ng));
    CHECK(dalloc(&E.d_wmeta, ng));
    CHECK(dalloc(&E.d_chunks, cn + 1));
    CHECK(dalloc(&E.d_lof, ln + 2));
    CHECK(dalloc(&E.d_dpos, n + kVecPad));
    CHECK(h2d(ctx, E.d_dpos, dpos.data(), dpos.size()));
    CHECK(h2d(ctx, E.d_smeta, sm_up.data(), sizeof(int2) * ns));
    CHECK(h2d(ctx, E.d_ci, cw_up.data(), sizeof(uint32_t) * (up_words + 1)));
    CHECK(h2d(ctx, E.d_len, len.data(), len.size()));
    CHECK(h2d(ctx, E.d_gmeta, gmeta.data(), sizeof(int4) * ng));
    CHECK(h2d(ctx, E.d_otab, otab.data(), sizeof(int) * (on + 1)));
    CHECK(h2d(ctx, E.d_vtab, vtab.data(), sizeof(double) * (on + 1)));
    CHECK(h2d(ctx, E.d_gslices, gsl.data(), sizeof(int4) * ng));
    CHECK(h2d(ctx, E.d_wmeta, wmeta.data(), sizeof(int4) * ng));
    CHECK(h2d(ctx, E.d_chunks, chunks.data(), sizeof(int2) * (cn + 1)));
    CHECK(h2d(ctx, E.d_lof, lof.data(), sizeof(uint16_t) * (ln + 2)));
    if (E.npairs > 0) {
        CHECK(dalloc(&E.d_pairs, prec.size()));
        CHECK(h2d(ctx, E.d_pairs, prec.data(), sizeof(int4) * prec.size()));
    }
    A->interior.ell = true;
    return PAMG_OK;
}

// Sliced ELL with per-group dictionaries (Options::ell, pamg::EllSet): a square operator whose
// rows are all interior, in slices of kEllW rows padded to the slice's longest row, kEllGroup
// rows sharing one table of column offsets (col - row) and one of values (bit patterns), each of
// <= 256 entries. Declines (leaves the tile layouts to the caller) where a table would be larger or
// a row longer than 255. Rows keep their storage order, so the kernel sums every row's products in
// the SPEC §S3 order.
// Rectangular operators (anchored: a restriction) take their offsets from each row's first column
// (col - col_first(row)), the anchors stored per row.
// Several parts: the set is the interior rows only (`inner`, ascending); the slices still span every
// row index, the boundary rows marked skipped (length byte kEllSkip: no load, no store — the
// boundary tiles compute them after the exchange).
int build_ell(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val,
              bool anchored, const std::vector<int>& inner) {
    using pamg::kEllGroup;
    using pamg::kEllSkip;
    using pamg::kEllW;
    const int64_t n = A->nrows;
    std::vector<char> in_set;
    if ((int64_t)inner.size() != n) {
        in_set.assign(n, 0);
        for (int i : inner) in_set[i] = 1;
    }
    auto member = [&](int64_t i) { return in_set.empty() || in_set[i]; };
    auto base_of = [&](int64_t i) -> int { return anchored ? (rp[i + 1] > rp[i] ? ci[rp[i]] : 0) : (int)i; };
    const int64_t ns = (n + kEllW - 1) / kEllW, ng = (n + kEllGroup - 1) / kEllGroup;
    std::vector<int> slen(ns, 0);
    std::atomic<bool> ok{true};
    par_for(ns, [&](int64_t a, int64_t b) {
        for (int64_t q = a; q < b; ++q) {
            int m = 0;
            for (int64_t i = q * kEllW; i < std::min(n, (q + 1) * kEllW); ++i)
                if (member(i)) m = std::max<int>(m, (int)(rp[i + 1] - rp[i]));
            if (m >= kEllSkip) ok = false;
            slen[q] = m;
        }
    });
    if (!ok) return PAMG_OK;
    std::vector<int2> smeta(ns);
    int64_t words = 0;
    for (int64_t q = 0; q < ns; ++q) {
        smeta[q] = make_int2((int)words, slen[q]);
        words += (int64_t)kEllW * ((slen[q] + 3) / 4);
        if (words >= INT32_MAX) return PAMG_OK;
    }
    // the whole of a square one-part operator: coupled groups with their x windows in LDS, where that pays
    if (!anchored && in_set.empty() && !A->plan && pamg::options().ell_pair && pamg::options().ell_xwin) {
        CHECK(build_ell_xwin(A, rp, ci, val, smeta, words));
        if (A->interior.ell) return PAMG_OK;
    }
    // per group, one pass: an entry's offset and value take the index of their first appearance in
    // the group (open addressing over 512 slots, stamped per group instead of cleared), and the index
    // bytes go straight into the slice streams (a slice lies in one group: no two threads share a word)
    // Paired dictionaries (Options::ell_pair, round 6): where every group has <= 256 distinct (offset,
    // value) pairs — the 512^3 A1: a regular 27-point-like stencil over the aggregates — one index byte
    // per nonzero names the pair (the offset and value tables then run in parallel); otherwise one byte
    // each into separate offset and value tables.
    std::vector<std::vector<int>> goff(ng);
    std::vector<std::vector<uint64_t>> gval(ng);
    std::vector<uint32_t> cw(words + 1, 0u), vw;
    std::vector<uint8_t> len(n + kVecPad, 0);
    bool paired = pamg::options().ell_pair != 0;
    if (paired) {
        std::atomic<bool> fits{true};
        par_for(ng, [&](int64_t a, int64_t b) {
            constexpr int kSlots = 1024;
            std::vector<int> pid(kSlots), pstamp(kSlots, -1), pkey_o(kSlots);
            std::vector<uint64_t> pkey_v(kSlots);
            std::vector<int> o;
            std::vector<uint64_t> v;
            for (int64_t g = a; g < b && fits; ++g) {
                const int stamp = (int)(g - a);
                o.clear();
                v.clear();
                const int64_t r1 = std::min(n, (g + 1) * kEllGroup);
                for (int64_t i = g * kEllGroup; i < r1 && fits; ++i) {
                    if (!member(i)) {
                        len[i] = (uint8_t)kEllSkip;
                        continue;
                    }
                    len[i] = (uint8_t)(rp[i + 1] - rp[i]);
                    const int64_t q = i / kEllW, lane = i % kEllW;
                    const int base = base_of(i);
                    for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                        const int kk = (int)(k - rp[i]);
                        const int off = ci[k] - base;
                        uint64_t u;
                        std::memcpy(&u, &val[k], 8);
                        uint32_t h = (uint32_t)((((uint64_t)(uint32_t)off * 0x9E3779B1u) ^ u ^ (u >> 29)) *
                                                0x9E3779B97F4A7C15ull >> 54);
                        while (pstamp[h] == stamp && (pkey_o[h] != off || pkey_v[h] != u)) h = (h + 1) & (kSlots - 1);
                        if (pstamp[h] != stamp) {
                            pstamp[h] = stamp;
                            pkey_o[h] = off;
                            pkey_v[h] = u;
                            pid[h] = (int)o.size();
                            o.push_back(off);
                            v.push_back(u);
                            if (o.size() > 256) {
                                fits = false;
                                break;
                            }
                        }
                        const int64_t w = smeta[q].x + (int64_t)(kk / 4) * kEllW + lane;
                        cw[w] |= (uint32_t)pid[h] << (8 * (kk % 4));
                    }
                }
                goff[g] = o;
                gval[g] = v;
            }
        });
        if (!fits) {  // back to separate tables: start over
            paired = false;
            std::fill(cw.begin(), cw.end(), 0u);
        }
    }
    if (!paired) vw.assign(words + 1, 0u);
    if (!paired) par_for(ng, [&](int64_t a, int64_t b) {
        constexpr int kSlots = 512;
        std::vector<int> okey(kSlots), oid(kSlots), ostamp(kSlots, -1), vid(kSlots), vstamp(kSlots, -1);
        std::vector<uint64_t> vkey(kSlots);
        std::vector<int> o;
        std::vector<uint64_t> v;
        for (int64_t g = a; g < b && ok; ++g) {
            const int stamp = (int)(g - a);
            o.clear();
            v.clear();
            const int64_t r1 = std::min(n, (g + 1) * kEllGroup);
            for (int64_t i = g * kEllGroup; i < r1; ++i) {
                if (!member(i)) {
                    len[i] = (uint8_t)kEllSkip;
                    continue;
                }
                len[i] = (uint8_t)(rp[i + 1] - rp[i]);
                const int64_t q = i / kEllW, lane = i % kEllW;
                const int base = base_of(i);
                for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                    const int kk = (int)(k - rp[i]);
                    const int off = ci[k] - base;
                    uint32_t h = ((uint32_t)off * 0x9E3779B1u) >> 23;
                    while (ostamp[h] == stamp && okey[h] != off) h = (h + 1) & (kSlots - 1);
                    if (ostamp[h] != stamp) {
                        ostamp[h] = stamp;
                        okey[h] = off;
                        oid[h] = (int)o.size();
                        o.push_back(off);
                    }
                    uint64_t u;
                    std::memcpy(&u, &val[k], 8);
                    uint32_t hv = (uint32_t)((u ^ (u >> 29)) * 0x9E3779B97F4A7C15ull >> 55);
                    while (vstamp[hv] == stamp && vkey[hv] != u) hv = (hv + 1) & (kSlots - 1);
                    if (vstamp[hv] != stamp) {
                        vstamp[hv] = stamp;
                        vkey[hv] = u;
                        vid[hv] = (int)v.size();
                        v.push_back(u);
                    }
                    if (o.size() > 256 || v.size() > 256) {
                        ok = false;
                        return;
                    }
                    const int64_t w = smeta[q].x + (int64_t)(kk / 4) * kEllW + lane;
                    cw[w] |= (uint32_t)oid[h] << (8 * (kk % 4));
                    vw[w] |= (uint32_t)vid[hv] << (8 * (kk % 4));
                }
            }
            goff[g] = o;
            gval[g] = v;
        }
    });
    if (!ok) return PAMG_OK;
    std::vector<int4> gmeta(ng);
    int64_t on = 0, vn = 0;
    for (int64_t g = 0; g < ng; ++g) {
        gmeta[g] = make_int4((int)on, (int)goff[g].size(), (int)vn, (int)gval[g].size());
        on += (int64_t)goff[g].size();
        vn += (int64_t)gval[g].size();
    }
    std::vector<int> otab(on + 1, 0);
    std::vector<double> vtab(vn + 1, 0.0);
    par_for(ng, [&](int64_t a, int64_t b) {
        for (int64_t g = a; g < b; ++g) {
            std::copy(goff[g].begin(), goff[g].end(), otab.begin() + gmeta[g].x);
            for (size_t e = 0; e < gval[g].size(); ++e) std::memcpy(&vtab[gmeta[g].z + e], &gval[g][e], 8);
        }
    });
    pamg::EllSet& E = A->ell;
    pamg_ctx* ctx = A->ctx;
    E.nslices = ns;
    E.ngroups = ng;
    E.words = words;
    E.otab_n = on;
    E.vtab_n = vn;
    E.paired = paired;
    CHECK(dalloc(&E.d_smeta, ns));
    CHECK(dalloc(&E.d_ci, words + 1));
    if (!paired) CHECK(dalloc(&E.d_vi, words + 1));
    CHECK(dalloc(&E.d_len, n + kVecPad));
    CHECK(dalloc(&E.d_gmeta, ng));
    CHECK(dalloc(&E.d_otab, on + 1));
    CHECK(dalloc(&E.d_vtab, vn + 1));
    CHECK(h2d(ctx, E.d_smeta, smeta.data(), sizeof(int2) * ns));
    CHECK(h2d(ctx, E.d_ci, cw.data(), sizeof(uint32_t) * (words + 1)));
    if (!paired) CHECK(h2d(ctx, E.d_vi, vw.data(), sizeof(uint32_t) * (words + 1)));
    CHECK(h2d(ctx, E.d_len, len.data(), len.size()));
    CHECK(h2d(ctx, E.d_gmeta, gmeta.data(), sizeof(int4) * ng));
    CHECK(h2d(ctx, E.d_otab, otab.data(), sizeof(int) * (on + 1)));
    CHECK(h2d(ctx, E.d_vtab, vtab.data(), sizeof(double) * (vn + 1)));
    if (anchored) {
        std::vector<int> anc(n + kVecPad, 0);
        par_for(n, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) anc[i] = base_of(i);
        });
        CHECK(dalloc(&E.d_anc, n + kVecPad));
        CHECK(h2d(ctx, E.d_anc, anc.data(), sizeof(int) * anc.size()));
        CHECK(blocked_group_order(ctx, anc, ng, A->plan ? A->plan->n_own : A->ncols, &E.d_gorder));
    }
    A->interior.ell = true;
    return PAMG_OK;
}

// square operators (offsets from the row) and restrictions (fewer rows than columns; offsets from
// each row's first column); several parts: the interior rows, when they are >= 3/4 of the operator
int ell_try(Upload& u) {
    pamg_mat* A = u.A;
    const int64_t nrows = A->nrows, n_own_cols = u.n_own_cols;
    if (pamg::options().ell && !A->interior.sym && !A->interior.rpat && n_own_cols >= nrows && nrows > 0 &&
        (int64_t)u.inner.size() * 4 >= (int64_t)nrows * 3 && nrows >= pamg::options().ell_min_rows &&
        (n_own_cols == nrows || pamg::options().ell_restrict)) {
        CHECK(build_ell(A, u.rp, u.ci, u.val, n_own_cols != nrows, u.inner));
        if (A->interior.ell) u.inner.clear();  // the rows run in k_rows_ell, not in tiles
        u.tr.mark("ell");
    }
    return PAMG_OK;
}

// two index bytes per padded nonzero, a length byte per row, the slice and group descriptors and
// the group tables
int64_t ell_bytes(const pamg_mat* A) {
    if (!A->interior.ell) return 0;
    const int64_t nrows = A->nrows;
    // (row classes: the class records and a class byte per row in place of the per-row stream)
    const int64_t index = A->ell.cls ? 4 * A->ell.cls_words + nrows : (A->ell.paired ? 4 : 8) * A->ell.words;
    return index + nrows + 8 * A->ell.nslices + 16 * A->ell.ngroups + 4 * A->ell.otab_n +
           8 * A->ell.vtab_n + (A->ell.d_anc ? 4 * nrows : 0) +
           (A->ell.win ? 32 * A->ell.ngroups + 8 * A->ell.nchunks + 2 * A->ell.lof_n + nrows : 0) -
           // (a pair's workgroup reads its 64-byte record in place of two groups' 48 bytes of descriptors)
           32 * (int64_t)A->ell.npairs;
}

void ell_report(const pamg_mat* A, const pamg::TileSet& t, int out[10]) {
    if (!t.ell) return;
    out[8] = (int)A->ell.ngroups;  // k_rows_ell's grid
    out[9] |= 512 | (A->ell.paired ? 8192 : 0);
}

void ell_window(const pamg_mat* A, int out[16]) {
    const pamg::EllSet& E = A->ell;
    const bool w = A->interior.ell && E.win;
    out[0] = w ? 1 : 0;
    out[1] = w ? E.win_groups : 0;
    out[2] = w ? E.gather_groups : 0;
    out[3] = w ? E.max_window : 0;
    out[4] = w ? E.noncontig_groups : 0;
    out[5] = w ? E.max_pairs : 0;
    out[6] = w ? E.max_chunks : 0;
    out[7] = w ? (int)E.ngroups : 0;
    out[8] = w ? E.mean_window : 0;
    out[9] = w ? E.p95_window : 0;
    out[10] = w ? E.mean_runs : 0;
    out[11] = w ? E.max_runs : 0;
    out[12] = w ? E.mean_pairs : 0;
    out[13] = w ? E.full_groups : 0;
    out[14] = out[15] = 0;
}

// the group pairs of a windowed operator (pamg_mat_ell_span)
void ell_span(const pamg_mat* A, int out[8]) {
    const pamg::EllSet& E = A->ell;
    const bool w = A->interior.ell && E.win;
    out[0] = w ? E.npairs : 0;
    out[1] = w ? E.win_groups - 2 * E.npairs : 0;
    out[2] = w ? E.mean_union : 0;
    out[3] = w ? E.p95_union : 0;
    out[4] = w ? E.union_pct : 0;
    out[5] = w ? E.max_union : 0;
    out[6] = out[7] = 0;
}

// the row classes of a windowed operator (pamg_mat_ell_classes)
void ell_classes(const pamg_mat* A, int64_t out[8]) {
    const pamg::EllSet& E = A->ell;
    const bool c = A->interior.ell && E.cls;
    out[0] = c ? 1 : 0;
    out[1] = c ? E.nslices : 0;
    out[2] = c ? E.cls_total : 0;
    out[3] = c ? E.cls_max : 0;
    out[4] = c ? 4 * E.cls_words : 0;
    out[5] = c ? A->nrows : 0;
    out[6] = c ? 4 * E.words : 0;
    out[7] = 0;
}

void ell_free(pamg::EllSet& E) {
    dfree(E.d_cid);
    dfree(E.d_gorder);
    dfree(E.d_smeta);
    dfree(E.d_ci);
    dfree(E.d_vi);
    dfree(E.d_len);
    dfree(E.d_gmeta);
    dfree(E.d_otab);
    dfree(E.d_vtab);
    dfree(E.d_anc);
    dfree(E.d_gslices);
    dfree(E.d_wmeta);
    dfree(E.d_chunks);
    dfree(E.d_lof);
    dfree(E.d_dpos);
    dfree(E.d_pairs);
    E = pamg::EllSet{};
}

// ------------------------------------------------------------------ pnc

// Neighbour-coded prolongation (Options::pnc, pamg::PncSet): every row's columns named by the
// grid neighbours whose anchors they are. Declines (leaves the tile layouts to the caller) where a
// row is longer than kPncMaxLen, a column is no neighbour's anchor, or a table would overflow.
int build_pnc(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val,
              const std::array<int64_t, 4>& grid, const std::vector<int>& inner) {
    using pamg::kPncMaxLen;
    using pamg::kPncSkip;
    const int64_t n = A->nrows;
    // several parts: the interior rows only (the boundary rows — ghost columns — run in their tiles
    // after the exchange; their records carry the skip pattern id)
    std::vector<char> in_set;
    if ((int64_t)inner.size() != n) {
        in_set.assign(n, 0);
        for (int i : inner) in_set[i] = 1;
    }
    auto member = [&](int64_t i) { return in_set.empty() || in_set[i]; };
    const int64_t nx = grid[1], ny = grid[2], nz = grid[3], M = nx * ny;
    if (n != nx * ny * nz || n <= 0 || M % 256 != 0) return PAMG_OK;  // (k_rows_pnc / k_rows_pnct: 256-point blocks of a plane)
    std::vector<int> anc(n + kVecPad, 0);
    std::atomic<bool> ok{true};
    par_for(n, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b && ok; ++i) {
            if (member(i) && rp[i + 1] - rp[i] > kPncMaxLen) {
                ok = false;
                return;
            }
            int64_t best = rp[i];
            for (int64_t k = rp[i] + 1; k < rp[i + 1]; ++k)
                if (val[k] > val[best]) best = k;
            anc[i] = rp[i + 1] > rp[i] ? ci[best] : 0;
        }
    });
    if (!ok) return PAMG_OK;
    // pass 1: each row's pattern word (length, codes) and the distinct patterns and values
    std::vector<uint32_t> pw(n);
    std::mutex mu;
    std::vector<uint32_t> pats;
    std::vector<uint64_t> vals;
    const int64_t d[7] = {0, -1, 1, -nx, nx, -M, M};
    par_for(n, [&](int64_t a, int64_t b) {
        // this chunk's distinct patterns and values (open addressing; the tables' limits are far below
        // the slot counts, so a chunk past them stops)
        constexpr int kPS = 4096, kVS = 1024;
        std::vector<uint32_t> pkey(kPS, 0xffffffffu);
        std::vector<uint64_t> vkey(kVS);
        std::vector<char> vused(kVS, 0);
        std::vector<uint32_t> lp;
        std::vector<uint64_t> lv;
        for (int64_t i = a; i < b && ok; ++i) {
            if (!member(i)) continue;
            const int64_t x = i % nx, y = (i / nx) % ny, z = i / M;
            const bool in[7] = {true, x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1};
            uint32_t w = (uint32_t)(rp[i + 1] - rp[i]);
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                int c = 0;
                while (c < 7 && !(in[c] && anc[i + d[c]] == ci[k])) ++c;
                if (c == 7) {
                    ok = false;
                    return;
                }
                w |= (uint32_t)c << (3 + 3 * (k - rp[i]));
                uint64_t u;
                std::memcpy(&u, &val[k], 8);
                uint32_t h = (uint32_t)((u ^ (u >> 29)) * 0x9E3779B97F4A7C15ull >> 54);
                while (vused[h] && vkey[h] != u) h = (h + 1) & (kVS - 1);
                if (!vused[h]) {
                    vused[h] = 1;
                    vkey[h] = u;
                    lv.push_back(u);
                    if (lv.size() > (size_t)pamg::kPncValMax) {
                        ok = false;
                        return;
                    }
                }
            }
            pw[i] = w;
            uint32_t h = (w * 0x9E3779B1u) >> 20;
            while (pkey[h] != 0xffffffffu && pkey[h] != w) h = (h + 1) & (kPS - 1);
            if (pkey[h] == 0xffffffffu) {
                pkey[h] = w;
                lp.push_back(w);
                if (lp.size() > (size_t)kPncSkip) {
                    ok = false;
                    return;
                }
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        pats.insert(pats.end(), lp.begin(), lp.end());
        vals.insert(vals.end(), lv.begin(), lv.end());
        std::sort(pats.begin(), pats.end());
        pats.erase(std::unique(pats.begin(), pats.end()), pats.end());
        std::sort(vals.begin(), vals.end());
        vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    });
    if (!ok || pats.size() > (size_t)kPncSkip || vals.size() > (size_t)pamg::kPncValMax) return PAMG_OK;
    // pass 2: the records (pattern id, value indices)
    std::vector<uint2> rec(n + kVecPad, make_uint2(0u, 0u));
    par_for(n, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) {
            if (!member(i)) {
                rec[i] = make_uint2((uint32_t)kPncSkip, 0u);
                continue;
            }
            uint64_t r = (uint64_t)(std::lower_bound(pats.begin(), pats.end(), pw[i]) - pats.begin());
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                uint64_t u;
                std::memcpy(&u, &val[k], 8);
                const uint64_t vi = (uint64_t)(std::lower_bound(vals.begin(), vals.end(), u) - vals.begin());
                r |= vi << (10 + 7 * (k - rp[i]));
            }
            rec[i] = make_uint2((uint32_t)r, (uint32_t)(r >> 32));
        }
    });
    std::vector<double> vtab(vals.size());
    for (size_t e = 0; e < vals.size(); ++e) std::memcpy(&vtab[e], &vals[e], 8);
    // compact records: the distinct (pattern word, value indices) combinations, numbered in sorted order
    std::vector<std::pair<uint32_t, uint64_t>> combs;
    if (pamg::options().pnc_compact) {
        std::atomic<bool> fits{true};
        par_for(n, [&](int64_t a, int64_t b) {
            std::vector<std::pair<uint32_t, uint64_t>> lc;
            std::pair<uint32_t, uint64_t> last{0xffffffffu, 0};
            for (int64_t i = a; i < b && fits; ++i) {
                if (!member(i)) continue;
                const uint64_t r = ((uint64_t)rec[i].y << 32) | rec[i].x;
                const std::pair<uint32_t, uint64_t> c{pats[r & 1023u], r >> 10};
                if (c == last) continue;
                last = c;
                if (std::find(lc.begin(), lc.end(), c) == lc.end()) {
                    lc.push_back(c);
                    if (lc.size() > (size_t)pamg::kPncCombMax) fits = false;
                }
            }
            std::lock_guard<std::mutex> lk(mu);
            combs.insert(combs.end(), lc.begin(), lc.end());
            std::sort(combs.begin(), combs.end());
            combs.erase(std::unique(combs.begin(), combs.end()), combs.end());
            if (combs.size() > (size_t)pamg::kPncCombMax) fits = false;
        });
        if (!fits) combs.clear();
    }
    pamg::PncSet& P = A->pnc;
    pamg_ctx* ctx = A->ctx;
    P.nx = (int)nx;
    P.ny = (int)ny;
    P.nz = (int)nz;
    P.npat = (int)pats.size();
    P.nval = (int)vals.size();
    // the grid of k_rows_pnct and k_rows_pnc (pamg_mat_layout out[8]): one workgroup per 256 points of a
    // plane — a tile or a piece of a line — and 32-plane chunk (kernels.hip launch_pnc)
    {
        const int64_t zlen = std::min<int64_t>(32, nz);
        P.grid = (int)((M / 256 * ((nz + zlen - 1) / zlen) + 7) / 8 * 8);
    }
    CHECK(dalloc(&P.d_anc, n + kVecPad));
    CHECK(dalloc(&P.d_vtab, (int64_t)vals.size()));
    CHECK(h2d(ctx, P.d_anc, anc.data(), sizeof(int) * anc.size()));
    CHECK(h2d(ctx, P.d_vtab, vtab.data(), sizeof(double) * vtab.size()));
    if (!combs.empty()) {
        std::vector<uint16_t> cid(n + kVecPad, (uint16_t)pamg::kPncCombSkip);
        par_for(n, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) {
                if (!member(i)) continue;
                const uint64_t r = ((uint64_t)rec[i].y << 32) | rec[i].x;
                const std::pair<uint32_t, uint64_t> c{pats[r & 1023u], r >> 10};
                cid[i] = (uint16_t)(std::lower_bound(combs.begin(), combs.end(), c) - combs.begin());
            }
        });
        std::vector<uint32_t> cw(combs.size());
        std::vector<uint64_t> cv(combs.size());
        for (size_t e = 0; e < combs.size(); ++e) {
            cw[e] = combs[e].first;
            cv[e] = combs[e].second;
        }
        P.npat = (int)combs.size();
        CHECK(dalloc(&P.d_cid, n + kVecPad));
        CHECK(dalloc(&P.d_ptab, (int64_t)cw.size()));
        CHECK(dalloc(&P.d_pvals, (int64_t)cv.size()));
        CHECK(h2d(ctx, P.d_cid, cid.data(), sizeof(uint16_t) * cid.size()));
        CHECK(h2d(ctx, P.d_ptab, cw.data(), sizeof(uint32_t) * cw.size()));
        CHECK(h2d(ctx, P.d_pvals, cv.data(), sizeof(uint64_t) * cv.size()));
    } else {
        CHECK(dalloc(&P.d_rec, n + kVecPad));
        CHECK(dalloc(&P.d_ptab, (int64_t)pats.size()));
        CHECK(h2d(ctx, P.d_rec, rec.data(), sizeof(uint2) * rec.size()));
        CHECK(h2d(ctx, P.d_ptab, pats.data(), sizeof(uint32_t) * pats.size()));
    }
    A->interior.pnc = true;
    return PAMG_OK;
}

// a prolongation over a 7-point grid uploaded earlier on this context
int pnc_try(Upload& u) {
    pamg_mat* A = u.A;
    const int64_t nrows = A->nrows;
    if (pamg::options().pnc && u.n_own_cols < nrows && (int64_t)u.inner.size() * 4 >= (int64_t)nrows * 3) {
        // (every registered grid of this row count, the latest first: grids of one size but other
        // shapes may be registered too, and the neighbour check decides)
        const auto grids = grids_of(A->ctx);
        for (auto g = grids.rbegin(); g != grids.rend() && !A->interior.pnc; ++g)
            if ((*g)[0] == nrows) CHECK(build_pnc(A, u.rp, u.ci, u.val, *g, u.inner));
        if (A->interior.pnc) u.inner.clear();  // the rows run in k_rows_pnc, not in tiles
        u.tr.mark("pnc");
    }
    return PAMG_OK;
}

// the anchor and the record per row, the two tables
int64_t pnc_bytes(const pamg_mat* A) {
    if (!A->interior.pnc) return 0;
    return (A->pnc.d_cid ? 6 : 12) * A->nrows + (A->pnc.d_cid ? 12 : 4) * A->pnc.npat + 8 * A->pnc.nval;
}

void pnc_report(const pamg_mat* A, const pamg::TileSet& t, int out[10]) {
    if (!t.pnc) return;
    out[3] = A->pnc.nval;  // the pattern and value tables, the grid of the march Options::pnc == 1 launches
    out[4] = A->pnc.npat;
    out[8] = A->pnc.grid;
    out[9] |= 1024 | (A->pnc.d_cid ? 4096 : 0) | (pamg::pnc_tiled(A->pnc.nx, A->pnc.ny) ? 16384 : 0);
}

void pnc_free(pamg::PncSet& P) {
    dfree(P.d_anc);
    dfree(P.d_rec);
    dfree(P.d_cid);
    dfree(P.d_pvals);
    dfree(P.d_ptab);
    dfree(P.d_vtab);
    P = pamg::PncSet{};
}

// ------------------------------------------------------------------ bsr

// Block-row layout (pamg::BsrSet, k_rows_bsr) of a matrix uploaded through pamg_mat_upload_blocked or
// pamg_mat_upload_block_rows (shared: the operator may be rectangular, a block row may be empty), when it
// qualifies: the bs rows of every node store the same block columns c_0 < c_1 < ..., row bs m + d as the
// entries bs c_0, bs c_0 + 1, ..., bs c_0 + bs - 1, bs c_1, ... in that storage order — every touched block
// whole, and the kernel's walk "blocks in order, e = 0 .. bs - 1 inside" the row's stored order (SPEC §S3).
// Otherwise nothing is built.
// row_lanes: the row-per-lane form (BsrSet::row_lanes, TileSet::bsr_r) instead of one lane per node.
// f32 (SPEC §S15): val holds values exact in binary32, and the slots are stored as float in d_val32.
int build_bsr_rows(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val, int bs, bool f32);
// the slot values on the device: as they are, or narrowed (exactly) to binary32
int bsr_put_values(pamg_ctx* ctx, pamg::BsrSet& B, const std::vector<double>& bval, int64_t min_count, bool f32) {
    const int64_t n = std::max<int64_t>((int64_t)bval.size(), min_count);
    if (!f32) {
        CHECK(dalloc(&B.d_val, n));
        return h2d(ctx, B.d_val, bval.data(), sizeof(double) * bval.size());
    }
    std::vector<float> v32(bval.size());
    par_for((int64_t)bval.size(), [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) v32[i] = (float)bval[i];
    });
    CHECK(dalloc(&B.d_val32, n));
    return h2d(ctx, B.d_val32, v32.data(), sizeof(float) * v32.size());
}
int build_bsr(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val, int bs, bool row_lanes = false,
              bool f32 = false) {
    using pamg::kEllW;
    pamg_ctx* ctx = A->ctx;
    const int64_t nb = A->nrows / bs, ns = (nb + kEllW - 1) / kEllW;
    std::atomic<bool> ok{true};
    par_for(nb, [&](int64_t a, int64_t b) {
        for (int64_t m = a; m < b && ok.load(std::memory_order_relaxed); ++m) {
            const int64_t k0 = rp[m * bs], len = rp[m * bs + 1] - k0;
            bool good = len % bs == 0;
            for (int d = 0; d < bs && good; ++d) good = rp[m * bs + d + 1] - rp[m * bs + d] == len;
            for (int64_t j = 0; j < len && good; j += bs) {
                const int c0 = ci[k0 + j];
                good = c0 % bs == 0 && (j == 0 || c0 > ci[k0 + j - bs]);
                for (int d = 0; d < bs && good; ++d)
                    for (int e = 0; e < bs && good; ++e) good = ci[rp[m * bs + d] + j + e] == c0 + e;
            }
            if (!good) ok = false;
        }
    });
    if (!ok) return PAMG_OK;
    if (row_lanes) return build_bsr_rows(A, rp, ci, val, bs, f32);
    pamg::BsrSet& B = A->bsr;
    std::vector<int64_t> soff(ns + 1, 0);
    for (int64_t s = 0; s < ns; ++s) {
        int64_t w = 0;
        for (int64_t m = s * kEllW; m < std::min(nb, (s + 1) * kEllW); ++m)
            w = std::max(w, (rp[m * bs + 1] - rp[m * bs]) / bs);
        soff[s + 1] = soff[s] + w;
    }
    const int64_t slots = soff[ns] * kEllW, b2 = (int64_t)bs * bs;
    if (slots >= INT32_MAX) return PAMG_OK;  // (pamg_mat_layout reports the slots as an int)
    std::vector<int> bcol((size_t)slots, -1);
    std::vector<double> bval((size_t)(slots * b2), 0.0);
    par_for(nb, [&](int64_t a, int64_t b) {
        for (int64_t m = a; m < b; ++m) {
            const int64_t s = m / kEllW, l = m % kEllW, nblk = (rp[m * bs + 1] - rp[m * bs]) / bs;
            for (int64_t k = 0; k < nblk; ++k) {
                bcol[(soff[s] + k) * kEllW + l] = ci[rp[m * bs] + k * bs] / bs;
                for (int d = 0; d < bs; ++d)
                    for (int e = 0; e < bs; ++e)
                        bval[((soff[s] + k) * b2 + d * bs + e) * kEllW + l] = val[rp[m * bs + d] + k * bs + e];
            }
        }
    });
    CHECK(dalloc(&B.d_soff, ns + 1));
    CHECK(dalloc(&B.d_bcol, std::max<int64_t>(slots, 1)));
    CHECK(h2d(ctx, B.d_soff, soff.data(), sizeof(int64_t) * (ns + 1)));
    CHECK(h2d(ctx, B.d_bcol, bcol.data(), sizeof(int) * bcol.size()));
    CHECK(bsr_put_values(ctx, B, bval, 1, f32));
    B.bs = bs;
    B.nb = nb;
    B.nslices = ns;
    B.slots = slots;
    B.grid = (int)((ns + pamg::kBsrSlices - 1) / pamg::kBsrSlices);
    A->interior.bsr = true;
    return PAMG_OK;
}

// The row-per-lane form of a matrix build_bsr has checked: a sliced ELL over scalar rows, a block column and
// the row's bs entries of the block per slot (pamg_device.h, BsrSet).
int build_bsr_rows(pamg_mat* A, const PtrVec& rp, const IdxVec& ci, const double* val, int bs, bool f32) {
    using pamg::kEllW;
    pamg_ctx* ctx = A->ctx;
    const int64_t n = A->nrows, ns = (n + kEllW - 1) / kEllW;
    pamg::BsrSet& B = A->bsr;
    std::vector<int64_t> soff(ns + 1, 0);
    for (int64_t s = 0; s < ns; ++s) {
        int64_t w = 0;
        for (int64_t i = s * kEllW; i < std::min(n, (s + 1) * kEllW); ++i) w = std::max(w, (rp[i + 1] - rp[i]) / bs);
        soff[s + 1] = soff[s] + w;
    }
    const int64_t slots = soff[ns] * kEllW;
    if (slots >= INT32_MAX) return PAMG_OK;  // (pamg_mat_layout reports the slots as an int)
    std::vector<int> bcol((size_t)slots, -1);
    std::vector<double> bval((size_t)(slots * bs), 0.0);
    par_for(n, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) {
            const int64_t s = i / kEllW, l = i % kEllW, nblk = (rp[i + 1] - rp[i]) / bs;
            for (int64_t k = 0; k < nblk; ++k) {
                const int64_t at = (soff[s] + k) * kEllW + l;
                bcol[at] = ci[rp[i] + k * bs] / bs;
                for (int e = 0; e < bs; ++e) bval[at * bs + e] = val[rp[i] + k * bs + e];
            }
        }
    });
    CHECK(dalloc(&B.d_soff, ns + 1));
    CHECK(dalloc(&B.d_bcol, std::max<int64_t>(slots, 1)));
    CHECK(h2d(ctx, B.d_soff, soff.data(), sizeof(int64_t) * (ns + 1)));
    CHECK(h2d(ctx, B.d_bcol, bcol.data(), sizeof(int) * bcol.size()));
    CHECK(bsr_put_values(ctx, B, bval, 4, f32));
    B.bs = bs;
    B.nb = n / bs;
    B.nslices = ns;
    B.slots = slots;
    B.grid = (int)((ns + pamg::kBsrSlices - 1) / pamg::kBsrSlices);
    B.row_lanes = true;
    A->interior.bsr_r = true;
    return PAMG_OK;
}

// Which form a restriction-shaped operator of pamg_mat_upload_block_rows takes: the row-per-lane one (the
// measured choice, DESIGN.md "Nodal hierarchy"), unless PAMG_BSR_ROW_LANES=0 in the environment asks for a
// lane per node (=1: the row-per-lane form; read at every upload; for A/B measurements and the tests).
constexpr bool kBsrRowLanes = true;
bool bsr_row_lanes() {
    const char* e = std::getenv("PAMG_BSR_ROW_LANES");
    if (e && (e[0] == '0' || e[0] == '1') && e[1] == 0) return e[0] == '1';
    return kBsrRowLanes;
}

// a square operator with a nonzero diagonal in every row and no ghost column, in whole nodes; through
// pamg_mat_upload_block_rows (u.rect) any shape between two node-major spaces, no diagonal asked for
int bsr_try(Upload& u) {
    pamg_mat* A = u.A;
    const bool shape = u.rect ? u.n_own_cols % u.bs == 0 : u.n_own_cols == A->nrows && u.has_all_diag;
    if (u.bs > 1 && shape && u.bnd.empty() && A->nrows > 0 && A->nrows % u.bs == 0) {
        // (few, long block rows: a lane per scalar row where that form is wanted)
        const bool row_lanes = u.rect && A->nrows < u.n_own_cols && bsr_row_lanes();
        CHECK(build_bsr(A, u.rp, u.ci, u.val, u.bs, row_lanes, A->value_bits == 32));
        if (pamg::bsr_any(*A)) u.inner.clear();  // the rows run in k_rows_bsr / k_rows_bsr_r, not in tiles
        u.tr.mark("bsr");
    }
    return PAMG_OK;
}

// the padded stream: a column and bs^2 values per block slot, the slice offsets
int64_t bsr_bytes(const pamg_mat* A) {
    if (!pamg::bsr_any(*A)) return 0;
    const int64_t per_slot = A->bsr.row_lanes ? A->bsr.bs : (int64_t)A->bsr.bs * A->bsr.bs;
    const int64_t vbytes = A->bsr.d_val32 ? 4 : 8;  // (SPEC §S15: binary32 slots)
    return A->bsr.slots * (4 + vbytes * per_slot) + 8 * (A->bsr.nslices + 1);
}

void bsr_report(const pamg_mat* A, const pamg::TileSet& t, int out[10]) {
    if (!t.bsr && !t.bsr_r) return;
    out[3] = A->bsr.bs;  // the block size, the padded block slots, k_rows_bsr's grid
    out[4] = (int)A->bsr.slots;
    out[6] = t.bsr_r ? 1 : 0;  // the row-per-lane form: the slots are per scalar row (bs values each)
    out[8] = A->bsr.grid;
    out[9] |= 32768;
    if (A->bsr.d_val32) out[9] |= 65536;  // the set stores 4-byte values (SPEC §S15)
}

void bsr_free(pamg::BsrSet& B) {
    dfree(B.d_soff);
    dfree(B.d_bcol);
    dfree(B.d_val);
    dfree(B.d_val32);
    B = pamg::BsrSet{};
}

// ------------------------------------------------------------------ tiles (every row no other family took)

// tile_order 1 (banded XCD-blocked order) for a square matrix of half-bandwidth `band`:
// cut the rows into super-rows of `band` rows (one grid plane for the stencils), give XCD k
// the k-th eighth of every super-row, and interleave the 8 sequences so block b (XCD b % 8,
// as dispatch is observed to deal blocks) walks its eighth plane after plane. The x lines of
// rows z-1, z, z+1 of one eighth then stay in that XCD's L2. Speed only: any order is correct.
// (Cutting each eighth into sub-slabs walked one after another was measured slower on every
// operator and removed: DESIGN.md "Measured and rejected".)
static std::vector<int4> xcd_band_order(const std::vector<int4>& tiles, int64_t band) {
    std::vector<std::vector<int4>> bucket(8);
    for (const auto& t : tiles) bucket[((int64_t)(t.x % band) * 8) / band].push_back(t);
    size_t m = 0;
    for (auto& b : bucket) m = std::max(m, b.size());
    std::vector<int4> out;
    out.reserve(8 * m);
    for (size_t i = 0; i < m; ++i)
        for (int k = 0; k < 8; ++k) out.push_back(i < bucket[k].size() ? bucket[k][i] : make_int4(0, 0, 0, 0));
    return out;
}

// Value dictionaries of a 24-bit tile set: every tile holds <= 16 distinct values (bit
// patterns, so -0.0 / NaN payloads survive); indices go to vidx (4 bits per entry). Tiles are
// independent (tables in parallel); the indices go through a byte per nonzero and are packed by
// byte afterwards, since two tiles can share the byte of an odd boundary.
int build_value_dict(const std::vector<int4>& tiles, const double* val, pamg::TileSet* ts,
                     std::vector<uint8_t>* vidx, size_t nslots) {
    const int64_t nt = (int64_t)tiles.size();
    std::vector<double> tab(tiles.size() * 16, 0.0);
    std::atomic<bool> over{false};
    par_for(nt, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b && !over; ++t) {
            uint64_t key[16];
            int nk = 0;
            for (int k = tiles[t].z; k < tiles[t].w; ++k) {
                uint64_t u;
                std::memcpy(&u, &val[k], 8);
                int j = 0;
                while (j < nk && key[j] != u) ++j;
                if (j == nk) {
                    if (nk == 16) {  // does not fit: plain values for this set
                        over = true;
                        return;
                    }
                    key[nk++] = u;
                    tab[t * 16 + j] = val[k];
                }
            }
        }
    });
    if (over) return PAMG_OK;
    std::vector<uint8_t> one(2 * nslots, 0);  // nonzeros outside every tile (long rows) keep 0
    par_for(nt, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b; ++t) {
            const double* tt = &tab[t * 16];
            for (int k = tiles[t].z; k < tiles[t].w; ++k) {
                int j = 0;
                while (std::memcmp(&tt[j], &val[k], 8) != 0) ++j;
                one[k] = (uint8_t)j;
            }
        }
    });
    if (vidx->empty()) vidx->assign(nslots, 0);
    par_for((int64_t)nslots, [&](int64_t a, int64_t b) {
        for (int64_t q = a; q < b; ++q) (*vidx)[q] |= (uint8_t)(one[2 * q] | (one[2 * q + 1] << 4));
    });
    CHECK(dalloc(&ts->d_vtab, (int64_t)tab.size()));
    HIPC(hipMemcpy(ts->d_vtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    ts->vd = true;
    return PAMG_OK;
}

// Greedy tiling of the rows listed in `rows` (ascending) into runs of consecutive rows with
// <= kTileRows rows and <= tile_nnz nonzeros; rows above the budget become "long" rows.
int build_tiles(const PtrVec& rp, const std::vector<int>& rows, bool square,
                pamg::TileSet* ts, int64_t band, const IdxVec& ci,
                std::vector<uint16_t>* lo, std::vector<uint8_t>* hi, const double* val,
                std::vector<uint8_t>* vidx, std::vector<int4>* tiles_out, bool tall = false) {
    const auto& opt = pamg::options();
    int tnnz = opt.tile_nnz;
    const int trows = pamg::kTileRows;
    // long_tiles: operators with long rows (coarse A_l, R_l: >= 48 nonzeros per row on
    // average) take 4096-nonzero tiles instead of the default 1024 — their time goes into the
    // in-order add chain of each row (SPEC §S3), and a tile of 4x the rows runs 4x the chains
    // side by side (512^3: A2 0.139 -> 0.110 ms, R1 0.458 -> 0.439 ms,
    // profiles/r01_kbench_512_tnnz.jsonl); the 7- and 27-point levels keep 1024. Square
    // operators only: the long-row restriction R1 (188 nonzeros per row, tile-major) is 9 %
    // faster with 1024 (profiles/r02_exp/kbench512_level12_tiles.jsonl), A2 13 % slower.
    if (opt.long_tiles && square && tnnz == 1024 && !rows.empty()) {
        int64_t nz = 0;
        for (int r : rows) nz += rp[r + 1] - rp[r];
        // >= 48 per row always; from long_tiles_min (24) per row when the set is large enough
        // to keep the chip full with 4096-nonzero tiles: >= 32 of them per CU (512^3 A1, 31 per
        // row, ~500 tiles per CU on one GPU and ~60 on each of 8: residual -3 %, Jacobi -2 %;
        // the 6 M-nonzero A1 of 128^3, 6 per CU, is 9 % slower with them,
        // profiles/r02_exp/bench_long_tiles_min_ab/). Keyed on the CU count, not on a fixed
        // nonzero count, so a part of an 8-GPU run takes the layout one GPU takes.
        // Round 3 (8-bit per-tile value dictionaries): the set under the second rule (512^3 A1)
        // takes 2048-nonzero tiles — residual + Jacobi 1.85 -> 1.80 ms on one box; 3072 1.83
        // (profiles/r03_jdiag/kb.jsonl) — A2 (>= 48 per row) stays at 4096 (2048: Jacobi +5 %).
        const int64_t nr = (int64_t)rows.size();
        if (nz >= 48 * nr)
            tnnz = 4096;
        else if (nz >= (int64_t)opt.long_tiles_min * nr && nz >= int64_t(32) * 4096 * device_cus())
            tnnz = 2048;
    } else if (opt.long_tiles && !square && !tall && tnnz == 1024 && !rows.empty()) {
        // Round 4: a restriction with 24 .. 47 nonzeros per row on a set large enough for the
        // rule above (512^3 R0: 32 per row, anchored dictionary in tile-major slots) takes
        // 2048-nonzero tiles: 1.09-1.10 -> 1.03 ms (4096: 1.03), profiles/r04_p/kbench_tn.jsonl;
        // the long-row R1 (~150 per row) stays at 1024 (2048 / 4096: +14-16 %, r03)
        int64_t nz = 0;
        for (int r : rows) nz += rp[r + 1] - rp[r];
        const int64_t nr = (int64_t)rows.size();
        if (nz >= (int64_t)opt.long_tiles_min * nr && nz < 48 * nr && nz >= int64_t(32) * 4096 * device_cus())
            tnnz = 2048;
    }
    ts->tile_nnz = tnnz;
    std::vector<int4> tiles;
    std::vector<int> longr;
    size_t i = 0;
    while (i < rows.size()) {
        const int r = rows[i];
        const int64_t len = rp[r + 1] - rp[r];
        // the kernel streams [rp[r] & ~3, end): the alignment head counts against the budget
        const int64_t head = rp[r] & 3;
        if (head + len > tnnz) {
            longr.push_back(r);
            ++i;
            continue;
        }
        int end = r + 1;
        int64_t nz = head + len;
        size_t j = i + 1;
        while (j < rows.size() && rows[j] == end && end - r < trows) {
            const int64_t l2 = rp[end + 1] - rp[end];
            if (nz + l2 > tnnz) break;
            nz += l2;
            ++end;
            ++j;
        }
        tiles.push_back(make_int4(r, end, (int)rp[r], (int)rp[end]));
        ts->nnz_short += rp[end] - rp[r];
        ts->rows_short += end - r;
        for (int q = r; q < end; ++q) ts->max_short_len = std::max(ts->max_short_len, (int)(rp[q + 1] - rp[q]));
        i = j;
    }
    for (int r : longr) ts->nnz_long += rp[r + 1] - rp[r];
    if (opt.tile_order == 1 && band >= 64 && tiles.size() >= 64) tiles = xcd_band_order(tiles, band);
    ts->n_short = (int)tiles.size();
    ts->n_long = (int)longr.size();
    CHECK(dalloc(&ts->d_short, ts->n_short));
    CHECK(dalloc(&ts->d_long, ts->n_long));
    // 24-bit column stream: usable when every tile's columns span < 2^24 (banded matrices;
    // not for tiles that reach the ghost columns of a large part)
    ts->c24 = false;
    if (opt.col24 && !tiles.empty()) {
        const int64_t nt = (int64_t)tiles.size();
        std::vector<int> base(nt, 0);
        std::vector<char> fit(nt, 1);
        par_for(nt, [&](int64_t a, int64_t b) {
            for (int64_t t = a; t < b; ++t) {
                const int4 d = tiles[t];
                int mn = INT32_MAX, mx = 0;
                for (int k = d.z; k < d.w; ++k) {
                    mn = std::min(mn, ci[k]);
                    mx = std::max(mx, ci[k]);
                }
                if (d.w == d.z) mn = mx = 0;
                base[t] = mn;
                fit[t] = (int64_t)mx - mn < (int64_t(1) << 24);
            }
        });
        if (std::all_of(fit.begin(), fit.end(), [](char f) { return f != 0; })) {
            if (lo->empty()) {
                lo->assign(ci.size(), 0);
                hi->assign(ci.size(), 0);
            }
            par_for(nt, [&](int64_t a, int64_t b) {
                for (int64_t t = a; t < b; ++t)
                    for (int k = tiles[t].z; k < tiles[t].w; ++k) {
                        const uint32_t dlt = (uint32_t)(ci[k] - base[t]);
                        (*lo)[k] = (uint16_t)(dlt & 0xffffu);
                        (*hi)[k] = (uint8_t)(dlt >> 16);
                    }
            });
            CHECK(dalloc(&ts->d_base, (int64_t)tiles.size()));
            HIPC(hipMemcpy(ts->d_base, base.data(), sizeof(int) * base.size(), hipMemcpyHostToDevice));
            ts->c24 = true;
        }
    }
    // 4-bit per-tile value dictionaries for the prolongations (more rows than columns: P0
    // 1.21 ms vs 1.40 with 8-bit column dictionaries, 512^3, profiles/r03_r0/); the other
    // operators keep their column dictionaries in tile-major slots with 8-bit value
    // dictionaries there (build_tile_major: R0 1.06 vs 1.12 ms, elastic3d 80^3 A0 0.206 vs
    // 0.237 ms, profiles/r03_r0/, profiles/r03_e80/)
    ts->vd = false;
    if (opt.value_dict == 1 && ts->c24 && val && tall)
        CHECK(build_value_dict(tiles, val, ts, vidx, (ci.size() + 1) / 2 + 8));
    ts->rl8 = opt.row_len8 && ts->c24 && ts->max_short_len <= 255 && ts->n_short > 0 &&
              ts->nnz_short <= 16 * ts->rows_short;
    // ^ short rows only: the 3 B/row saved are 3-8 % of a 4-7-nonzero row (A0 SpMV -2 %, P0
    //   -5..-8 %) but ~1 % of a 30-nonzero row, where the scan's latency costs more (R0, A1
    //   +2..3 %; profiles/r01_kbench_512_rl8.jsonl); with the value dictionaries too (P0)
    if (ts->n_short)
        HIPC(hipMemcpy(ts->d_short, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice));
    if (ts->n_long)
        HIPC(hipMemcpy(ts->d_long, longr.data(), sizeof(int) * longr.size(), hipMemcpyHostToDevice));
    tiles_out->swap(tiles);
    return PAMG_OK;
}

// Per-tile column dictionaries (Options::col_dict_tile) for tile sets no global table fits:
// every tile carries its own table of <= 256 offsets (capacity ctab_n = the largest tile's
// count rounded up to a power of two >= 16, so 4-bit indices where every tile has <= 16),
// row-relative (col - row: the coarse operators, 33 offsets per tile on average for A1 at
// 512^3 against ~10^4 in the whole matrix) or anchored (col - the row's middle column, stored
// as a 16-bit delta from a per-tile base: the prolongators, a few per tile). The form
// with fewer bytes is taken, and only if it streams less than the 24-bit columns; it runs in
// the descriptor kernel (k_rows_tile2), not in tile-major slots.
int build_tile_dicts(pamg_mat* A, const PtrVec& rp, const IdxVec& ci,
                     const std::vector<int4>& tiles, pamg::TileSet* ts, std::vector<uint8_t>* idx,
                     std::vector<int>* tab, std::vector<uint16_t>* anc16) {
    const int64_t nt = (int64_t)tiles.size();
    if (nt == 0) return PAMG_OK;
    // anchor of a row: its middle column (for a prolongator row, its own aggregate's
    // neighbourhood), so one tile's anchors stay within a 16-bit span
    auto mid_col = [&](int r) { return rp[r + 1] > rp[r] ? ci[rp[r] + (rp[r + 1] - rp[r] - 1) / 2] : 0; };
    int64_t nz = 0, rows = 0;
    for (const int4& t : tiles) {
        nz += t.w - t.z;
        rows += t.y - t.x;
    }
    // per tile: distinct offsets in first-occurrence order (count only), both forms
    std::vector<int> cnt_rel(nt), cnt_anc(nt), base(nt, 0);
    std::vector<char> span_ok(nt, 1);
    auto distinct = [&](const int4& t, bool anchored, int* out_tab, int cap) {
        constexpr int kCells = 2048;
        int key[kCells], slot[kCells];
        std::fill(slot, slot + kCells, -1);
        int n = 0;
        for (int r = t.x; r < t.y; ++r) {
            const int an = anchored ? mid_col(r) : r;
            for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
                const int o = ci[k] - an;
                uint32_t h = ((uint32_t)o * 0x9E3779B1u) >> 21;
                while (slot[h] >= 0 && key[h] != o) h = (h + 1) & (kCells - 1);
                if (slot[h] < 0) {
                    if (n == cap) return cap + 1;
                    key[h] = o;
                    slot[h] = n;
                    if (out_tab) out_tab[n] = o;
                    ++n;
                }
                if (idx && out_tab) (*idx)[k] = (uint8_t)slot[h];
            }
        }
        return n;
    };
    par_for(nt, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b; ++t) {
            const int4 d = tiles[t];
            cnt_rel[t] = distinct(d, false, nullptr, 256);
            cnt_anc[t] = distinct(d, true, nullptr, 256);
            int mn = INT32_MAX, mx = INT32_MIN;
            for (int r = d.x; r < d.y; ++r)
                if (rp[r + 1] > rp[r]) {
                    mn = std::min(mn, mid_col(r));
                    mx = std::max(mx, mid_col(r));
                }
            base[t] = mn == INT32_MAX ? 0 : mn;
            span_ok[t] = mn == INT32_MAX || (int64_t)mx - mn < 65536;
        }
    });
    auto cap_of = [](int m) {
        int c = 16;
        while (c < m) c <<= 1;
        return c;
    };
    const int mrel = *std::max_element(cnt_rel.begin(), cnt_rel.end());
    const int manc = *std::max_element(cnt_anc.begin(), cnt_anc.end());
    const bool anc_ok = manc <= 256 && std::all_of(span_ok.begin(), span_ok.end(), [](char c) { return c != 0; });
    auto bytes = [&](int m, bool anchored) -> double {
        const int c = cap_of(m);
        return (c <= 16 ? 0.5 : 1.0) * (double)nz + 4.0 * c * nt + (anchored ? 2.0 * rows : 0.0);
    };
    const double b24 = 3.0 * (double)nz + 4.0 * nt;  // the 24-bit stream it would replace
    bool use_anc = false;
    double best = b24;
    if (mrel <= 256 && bytes(mrel, false) < best) best = bytes(mrel, false);
    if (anc_ok && bytes(manc, true) < best) {
        best = bytes(manc, true);
        use_anc = true;
    }
    if (std::getenv("PAMG_TRACE_UPLOAD"))
        std::fprintf(stderr, "[pamg upload] per-tile dictionaries: %lld tiles, max offsets/tile row-relative %d, "
                     "anchored %d (16-bit span %s) -> %s\n", (long long)nt, mrel, manc, anc_ok ? "ok" : "no",
                     best >= b24 ? "24-bit kept" : use_anc ? "anchored" : "row-relative");
    if (best >= b24) return PAMG_OK;
    const int cap = cap_of(use_anc ? manc : mrel);
    tab->assign((size_t)nt * cap, 0);
    if (use_anc && anc16->empty()) anc16->assign((size_t)A->nrows + kVecPad, 0);
    par_for(nt, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b; ++t) {
            distinct(tiles[t], use_anc, tab->data() + (size_t)t * cap, cap);
            if (use_anc)
                for (int r = tiles[t].x; r < tiles[t].y; ++r)
                    (*anc16)[r] = rp[r + 1] > rp[r] ? (uint16_t)(mid_col(r) - base[t]) : 0;
        }
    });
    if (use_anc) {
        CHECK(dalloc(&ts->d_abase, nt));
        HIPC(hipMemcpy(ts->d_abase, base.data(), sizeof(int) * nt, hipMemcpyHostToDevice));
    }
    ts->pt = true;
    ts->anc = use_anc;
    ts->ctab_n = cap;
    return PAMG_OK;
}

// Column dictionaries (Options::col_dict). A tile set whose short-tile nonzeros have at most
// 256 distinct row-relative offsets col - row (the fine-grid stencils: 7 for the 7-point
// Poisson, 5 in 2D, 99 for elastic3d) stores each column as an index into the set's offset
// table: 4 bits where every such set of the matrix has <= 16 offsets, else 8 bits (one width
// per matrix, so the interior and boundary sets share d_cidx). The kernel rebuilds the
// column as row + table[index] (exact); its rows come from the 8-bit row lengths, so a
// dictionary set also turns rl8 on. Against the 24-bit stream this saves 2.5 B/nonzero
// (4-bit) or 2 B/nonzero (8-bit) of the 11-12 B a nonzero streams.
int build_col_dicts(pamg_mat* A, const PtrVec& rp, const IdxVec& ci,
                    const std::vector<int4>& t_in, const std::vector<int4>& t_bd,
                    std::vector<uint8_t>* idx8) {
    const auto& opt = pamg::options();
    pamg::TileSet* sets[2] = {&A->interior, &A->boundary};
    const std::vector<int4>* tl[2] = {&t_in, &t_bd};
    std::vector<uint8_t> idx;  // 8-bit index per nonzero (packed to 4 bits below if they fit)
    std::vector<int> tab[2];   // global table, or (per-tile sets) nt x ctab_n tables
    std::vector<uint16_t> anc16;  // per-tile anchored sets: each row's first column - tile base
    for (int q = 0; q < 2; ++q) {
        pamg::TileSet* ts = sets[q];
        if (!opt.col_dict || ts->n_short == 0 || ts->max_short_len > 255)
            continue;
        // a set with 4-bit value dictionaries (the prolongators) keeps its 24-bit columns
        // (per-tile column dictionaries there measured 8 % slower)
        if (ts->vd) continue;
        if (idx.empty()) idx.assign((size_t)A->nnz + kVecPad, 0);
        const std::vector<int4>& tiles = *tl[q];
        const int64_t nt = (int64_t)tiles.size();
        // Offset of a nonzero: col - row (row-relative: stencils), or col - the row's first
        // column (anchored: rows of a repeated shape whose columns do not follow the row
        // index, e.g. a restriction's 5x5x5 neighbourhoods of an aggregate root: 75 offsets).
        // Anchored sets are read only by the tile-major kernel (the row anchors live in its
        // slots), so they need tile_major on.
        auto try_dict = [&](bool anchored) -> bool {
            auto anchor = [&](int r) { return anchored ? (rp[r + 1] > rp[r] ? ci[rp[r]] : 0) : r; };
            // Distinct offsets in first-occurrence order (tile order, then storage order):
            // every chunk of tiles lists its own (<= 257) in parallel, the lists are merged in
            // chunk order — the same table a single sequential pass builds.
            const int nch = std::max(1, std::min<int>(host_threads(), (int)(nt / 64)));
            std::vector<std::vector<int>> firsts(nch);
            auto scan = [&](int64_t a, int64_t b, std::vector<int>& out) {
                constexpr int kCells = 1024;  // open addressing: offset -> seen
                int key[kCells];
                bool used[kCells] = {};
                for (int64_t t = a; t < b && out.size() <= 256; ++t)
                    for (int r = tiles[t].x; r < tiles[t].y; ++r) {
                        const int an = anchor(r);
                        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
                            const int o = ci[k] - an;
                            uint32_t h = ((uint32_t)o * 0x9E3779B1u) >> 22;
                            while (used[h] && key[h] != o) h = (h + 1) & (kCells - 1);
                            if (!used[h]) {
                                used[h] = true;
                                key[h] = o;
                                out.push_back(o);
                                if (out.size() > 256) return;
                            }
                        }
                    }
            };
            {
                std::vector<std::thread> th;
                for (int c = 0; c < nch; ++c)
                    th.emplace_back([&, c] { scan(nt * c / nch, nt * (c + 1) / nch, firsts[c]); });
                for (auto& x : th) x.join();
            }
            constexpr int kCells = 1024;
            int key[kCells], slot[kCells];
            std::fill(slot, slot + kCells, -1);
            auto find = [&](int o) {
                uint32_t h = ((uint32_t)o * 0x9E3779B1u) >> 22;
                while (slot[h] >= 0 && key[h] != o) h = (h + 1) & (kCells - 1);
                return h;
            };
            tab[q].clear();
            for (int c = 0; c < nch; ++c)
                for (int o : firsts[c]) {
                    const uint32_t h = find(o);
                    if (slot[h] >= 0) continue;
                    if (tab[q].size() == 256) {
                        tab[q].clear();
                        return false;
                    }
                    key[h] = o;
                    slot[h] = (int)tab[q].size();
                    tab[q].push_back(o);
                }
            par_for(nt, [&](int64_t a, int64_t b) {
                for (int64_t t = a; t < b; ++t)
                    for (int r = tiles[t].x; r < tiles[t].y; ++r) {
                        const int an = anchor(r);
                        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) idx[k] = (uint8_t)slot[find(ci[k] - an)];
                    }
            });
            return true;
        };
        ts->anc = false;
        ts->pt = false;
        if (try_dict(false)) continue;
        if (opt.col_dict_anchor && opt.tile_major && try_dict(true)) {
            ts->anc = true;
            continue;
        }
        if (opt.col_dict_tile) CHECK(build_tile_dicts(A, rp, ci, tiles, ts, &idx, &tab[q], &anc16));
    }
    int width = 0;
    for (int q = 0; q < 2; ++q) {
        if (tab[q].empty()) continue;
        const size_t entries = sets[q]->pt ? (size_t)sets[q]->ctab_n : tab[q].size();
        width = std::max(width, entries <= 16 ? 4 : 8);
    }
    if (width == 0) return PAMG_OK;
    for (int q = 0; q < 2; ++q) {
        if (tab[q].empty()) continue;
        pamg::TileSet* ts = sets[q];
        if (ts->pt) {  // nt x ctab_n per-tile tables (+ 256 so any index of the last tile stays inside)
            tab[q].resize(tab[q].size() + 256, 0);
            CHECK(dalloc(&ts->d_ctab, (int64_t)tab[q].size()));
            CHECK(h2d(A->ctx, ts->d_ctab, tab[q].data(), sizeof(int) * tab[q].size()));
        } else {
            std::vector<int> tab256(256, 0);  // any 8-bit index stays inside the allocation
            std::copy(tab[q].begin(), tab[q].end(), tab256.begin());
            CHECK(dalloc(&ts->d_ctab, (int64_t)tab256.size()));
            HIPC(hipMemcpy(ts->d_ctab, tab256.data(), sizeof(int) * tab256.size(), hipMemcpyHostToDevice));
            ts->ctab_n = (int)tab[q].size();
        }
        ts->cd = width;
        ts->rl8 = true;
    }
    if (!anc16.empty()) {
        CHECK(dalloc(&A->d_anc16, (int64_t)anc16.size()));
        CHECK(h2d(A->ctx, A->d_anc16, anc16.data(), sizeof(uint16_t) * anc16.size()));
    }
    if (width == 4) {
        std::vector<uint8_t> nib(((size_t)A->nnz + 1) / 2 + kVecPad, 0);
        const int64_t nb = (A->nnz + 1) / 2;
        par_for(nb, [&](int64_t a, int64_t b) {
            for (int64_t j = a; j < b; ++j) {
                const int64_t k = 2 * j;
                nib[j] = (uint8_t)((idx[k] & 15) | (k + 1 < A->nnz ? (idx[k + 1] & 15) << 4 : 0));
            }
        });
        CHECK(dalloc(&A->d_cidx, (int64_t)nib.size()));
        CHECK(h2d(A->ctx, A->d_cidx, nib.data(), nib.size()));
    } else {
        CHECK(dalloc(&A->d_cidx, (int64_t)idx.size()));
        CHECK(h2d(A->ctx, A->d_cidx, idx.data(), idx.size()));
    }
    idx8->swap(idx);
    return PAMG_OK;
}

// x staging (Options::x_stage; pamg::XStage) for a tile-major set with a set-wide row-relative
// dictionary: cluster the sorted offsets (a new run where the gap exceeds kXsGap), and when
// the runs of the widest tile fit (<= kXsMaxClusters runs, rows + run width <= 256 lanes,
// all runs in kXsCap doubles) write each offset's LDS position into the table at kXsIoff.
int build_x_stage(pamg_mat* A, pamg::TileSet* ts, int rs) {
    using pamg::kXsCap;
    using pamg::kXsGap;
    using pamg::kXsIoff;
    using pamg::kXsMaxClusters;
    ts->xs = false;
    if (!pamg::options().x_stage || !ts->cd || ts->anc || ts->pt || ts->ctab_n > kXsIoff || ts->ctab_n == 0)
        return PAMG_OK;
    std::vector<int> tab(256);
    HIPC(hipMemcpy(tab.data(), ts->d_ctab, sizeof(int) * 256, hipMemcpyDeviceToHost));
    std::vector<int> off(tab.begin(), tab.begin() + ts->ctab_n);
    std::vector<int> srt(off);
    std::sort(srt.begin(), srt.end());
    std::vector<int> cmin, cmax;
    for (int o : srt) {
        if (cmin.empty() || (int64_t)o - cmax.back() > kXsGap) {
            cmin.push_back(o);
            cmax.push_back(o);
        } else {
            cmax.back() = o;
        }
    }
    const int ncl = (int)cmin.size();
    int wmax = 0;
    for (int c = 0; c < ncl; ++c) wmax = std::max(wmax, cmax[c] - cmin[c]);
    const int stride = rs + wmax;
    if (ncl > kXsMaxClusters || stride > 256 || ncl * stride > kXsCap) return PAMG_OK;
    pamg::XStage& x = ts->xst;
    x = pamg::XStage{};
    x.ncl = ncl;
    x.stride = stride;
    x.ncols = (int)A->ncols;
    for (int c = 0; c < ncl; ++c) {
        x.omin[c] = cmin[c];
        x.wid[c] = cmax[c] - cmin[c];
    }
    for (int i = 0; i < ts->ctab_n; ++i) {
        int c = 0;
        while (off[i] > cmax[c]) ++c;
        tab[kXsIoff + i] = c * stride + (off[i] - cmin[c]);
        if (off[i] == 0) x.zix = i;
    }
    HIPC(hipMemcpy(ts->d_ctab, tab.data(), sizeof(int) * 256, hipMemcpyHostToDevice));
    ts->xs = true;
    return PAMG_OK;
}

// Tile-major copies (Options::tile_major, kernel variant 4 k_rows_tm): for a tile set with
// one row per lane (<= 256 rows per tile, rows <= 255 nonzeros) and 24-bit or dictionary
// columns, tile t's values, column stream and row lengths are copied to fixed, zero-padded
// slots (t * tile_nnz, t * tm_rs), so the kernel addresses every pre-gather load from its
// block index. The CSR arrays stay resident for the other variants and the long rows.
int build_tile_major(pamg_mat* A, int64_t n_own_cols, const PtrVec& rp,
                     const IdxVec& ci, const double* val,
                     const std::vector<int4>& t_in, const std::vector<int4>& t_bd,
                     const std::vector<uint16_t>& lo, const std::vector<uint8_t>& hi,
                     const std::vector<uint8_t>& idx8) {
    const auto& opt = pamg::options();
    pamg::TileSet* sets[2] = {&A->interior, &A->boundary};
    const std::vector<int4>* tl[2] = {&t_in, &t_bd};
    for (int q = 0; q < 2; ++q) {
        pamg::TileSet* ts = sets[q];
        ts->tm = false;
        // per-tile dictionaries run in the descriptor kernel, row-relative ones in tile-major
        // slots with tm_tile_dicts
        if (ts->pt && (ts->anc || !opt.tm_tile_dicts)) continue;
        if (!opt.tile_major || ts->vd || ts->n_short == 0 || ts->max_short_len > 255 ||
            !(ts->cd || (ts->c24 && !lo.empty())) || (ts->cd && idx8.empty()) || !val) {
            if (ts->anc) return fail(PAMG_E_STATE, "upload: anchored column dictionary without tile-major slots");
            continue;
        }
        // tile_major 1 (default): the sets where it measured faster at 512^3
        // (profiles/r01_kbench_512_tm_*.jsonl) — column-dictionary sets (A0: Jacobi -9 %,
        // residual -7 %, SpMV -5 %) and the non-square operators whose tiles fill >= 97 % of
        // their slots (R0 -5..-7 %, P1 -3 %); P0's row-limited tiles leave ~8 % of each slot as
        // padding (+5 %) and the square coarse A1 gains nothing (Jacobi +3 %): variant 1.
        // tile_major 2: every eligible set (A/B, tests).
        if (opt.tile_major == 1 && !ts->cd) {
            const double fill = (double)ts->nnz_short / ((double)ts->n_short * (double)ts->tile_nnz);
            if (n_own_cols == A->nrows || fill < 0.97) continue;
        }
        const std::vector<int4>& tiles = *tl[q];
        const int64_t nt = (int64_t)tiles.size(), tn = ts->tile_nnz;
        // k_rows_tm keeps per-tile tables of <= kTmSmallTab entries in LDS for 2048-nonzero tiles:
        // a set with longer per-tile column tables stays in the descriptor kernel
        if (ts->pt && tn == 2048 && ts->ctab_n > pamg::kTmSmallTab) {
            if (UploadTrace{}.on)
                std::fprintf(stderr, "[pamg upload nnz=%lld] set %d: per-tile column tables of %d > %d entries on "
                             "2048-nonzero tiles: descriptor kernel instead of tile-major slots\n",
                             (long long)A->nnz, q, ts->ctab_n, pamg::kTmSmallTab);
            continue;
        }
        int rs = 0;
        for (const int4& t : tiles) rs = std::max(rs, t.y - t.x);
        rs = (rs + 3) & ~3;
        // every slot is written whole (nonzeros, then zero padding) by the thread that owns its
        // tile, so the buffers need no serial zero fill
        const int cdw = ts->cd;
        // 8-bit per-tile value dictionaries (value_dict): every tile <= 256 distinct values
        // (bit patterns: +0.0 and -0.0 stay distinct)
        int vt = 0;
        if (opt.value_dict) {
            std::atomic<int> vmax{0};
            std::atomic<bool> over{false};
            par_for(nt, [&](int64_t a, int64_t b) {
                std::vector<uint64_t> u;
                for (int64_t i = a; i < b && !over; ++i) {
                    const int4 t = tiles[i];
                    u.assign(reinterpret_cast<const uint64_t*>(val) + t.z, reinterpret_cast<const uint64_t*>(val) + t.w);
                    std::sort(u.begin(), u.end());
                    const int d = (int)(std::unique(u.begin(), u.end()) - u.begin());
                    if (d > 256) over = true;
                    int m = vmax.load();
                    while (d > m && !vmax.compare_exchange_weak(m, d)) {
                    }
                }
            });
            if (!over) vt = std::max(4, (vmax.load() + 3) & ~3);
            if (tn == 2048 && vt > pamg::kTmSmallTab) {  // (the kernel's LDS table, see above)
                if (UploadTrace{}.on)
                    std::fprintf(stderr, "[pamg upload nnz=%lld] set %d: a 2048-nonzero tile has %d > %d distinct "
                                 "values: 8-B values instead of the 8-bit value dictionary\n",
                                 (long long)A->nnz, q, vmax.load(), pamg::kTmSmallTab);
                vt = 0;
            }
            if (over && UploadTrace{}.on)
                std::fprintf(stderr, "[pamg upload nnz=%lld] set %d: a tile has > 256 distinct values: 8-B values\n",
                             (long long)A->nnz, q);
        }
        std::unique_ptr<double[]> tv(vt ? nullptr : new double[nt * tn + kVecPad]);
        std::unique_ptr<uint8_t[]> tvi(vt ? new uint8_t[nt * tn + kVecPad] : nullptr);
        std::unique_ptr<double[]> tvt(vt ? new double[nt * vt + kVecPad] : nullptr);
        std::unique_ptr<uint8_t[]> trl(new uint8_t[nt * rs + kVecPad]);
        const int64_t ncb = cdw == 4 ? tn / 2 : tn;  // column-stream bytes per slot (cd / chi)
        std::unique_ptr<uint8_t[]> tci(new uint8_t[nt * ncb + kVecPad]);
        std::unique_ptr<uint16_t[]> tcl(cdw ? nullptr : new uint16_t[nt * tn + kVecPad]);
        std::unique_ptr<int[]> tan(ts->anc ? new int[nt * rs + kVecPad] : nullptr);
        par_for(nt, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) {
                const int4 t = tiles[i];
                const int cnt = t.w - t.z;
                uint8_t* rl = &trl[i * rs];
                for (int r = 0; r < rs; ++r) rl[r] = t.x + r < t.y ? (uint8_t)(rp[t.x + r + 1] - rp[t.x + r]) : 0;
                if (tan)  // row anchors: each row's first column (anchored column dictionary)
                    for (int r = 0; r < rs; ++r) {
                        const int row = t.x + r;
                        tan[i * rs + r] = row < t.y && rp[row + 1] > rp[row] ? ci[rp[row]] : 0;
                    }
                if (vt) {  // the tile's table in first-occurrence order, indices per nonzero
                    double* tab = &tvt[i * vt];
                    uint8_t* vi = &tvi[i * tn];
                    uint64_t hk[512];
                    int16_t hv[512];
                    std::fill(hv, hv + 512, (int16_t)-1);
                    int nd = 0;
                    for (int k = 0; k < cnt; ++k) {
                        uint64_t key;
                        std::memcpy(&key, &val[t.z + k], sizeof(key));
                        uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 55);  // 9 bits
                        while (hv[h] >= 0 && hk[h] != key) h = (h + 1) & 511;
                        if (hv[h] < 0) {
                            hk[h] = key;
                            hv[h] = (int16_t)nd;
                            std::memcpy(&tab[nd++], &key, sizeof(key));
                        }
                        vi[k] = (uint8_t)hv[h];
                    }
                    std::fill(tab + nd, tab + vt, 0.0);
                    std::fill(vi + cnt, vi + tn, (uint8_t)0);
                } else {
                    double* v = &tv[i * tn];
                    std::memcpy(v, val + t.z, sizeof(double) * cnt);
                    std::fill(v + cnt, v + tn, 0.0);
                }
                uint8_t* c = &tci[i * ncb];
                if (cdw == 4) {
                    std::fill(c, c + ncb, (uint8_t)0);
                    for (int k = 0; k < cnt; ++k) c[k >> 1] |= (uint8_t)((idx8[t.z + k] & 15) << (4 * (k & 1)));
                } else if (cdw == 8) {
                    std::memcpy(c, &idx8[t.z], cnt);
                    std::fill(c + cnt, c + tn, (uint8_t)0);
                } else {
                    uint16_t* l = &tcl[i * tn];
                    std::memcpy(l, &lo[t.z], sizeof(uint16_t) * cnt);
                    std::fill(l + cnt, l + tn, (uint16_t)0);
                    std::memcpy(c, &hi[t.z], cnt);
                    std::fill(c + cnt, c + tn, (uint8_t)0);
                }
            }
        });
        if (tv) std::fill(&tv[nt * tn], &tv[nt * tn] + kVecPad, 0.0);
        std::fill(&trl[nt * rs], &trl[nt * rs] + kVecPad, (uint8_t)0);
        std::fill(&tci[nt * ncb], &tci[nt * ncb] + kVecPad, (uint8_t)0);
        if (tcl) std::fill(&tcl[nt * tn], &tcl[nt * tn] + kVecPad, (uint16_t)0);
        if (tan) {
            std::fill(&tan[nt * rs], &tan[nt * rs] + kVecPad, 0);
            CHECK(dalloc(&ts->d_tm_anc, nt * rs + kVecPad));
            CHECK(h2d(A->ctx, ts->d_tm_anc, tan.get(), sizeof(int) * (nt * rs + kVecPad)));
        }
        if (vt) {
            std::fill(&tvi[nt * tn], &tvi[nt * tn] + kVecPad, (uint8_t)0);
            std::fill(&tvt[nt * vt], &tvt[nt * vt] + kVecPad, 0.0);
            CHECK(dalloc(&ts->d_tm_vidx, nt * tn + kVecPad));
            CHECK(h2d(A->ctx, ts->d_tm_vidx, tvi.get(), nt * tn + kVecPad));
            CHECK(dalloc(&ts->d_tm_vtab, nt * vt + kVecPad));
            CHECK(h2d(A->ctx, ts->d_tm_vtab, tvt.get(), sizeof(double) * (nt * vt + kVecPad)));
        } else {
            CHECK(dalloc(&ts->d_tm_val, nt * tn + kVecPad));
            CHECK(h2d(A->ctx, ts->d_tm_val, tv.get(), sizeof(double) * (nt * tn + kVecPad)));
        }
        ts->tm_vt = vt;
        CHECK(dalloc(&ts->d_tm_rlen, nt * rs + kVecPad));
        CHECK(h2d(A->ctx, ts->d_tm_rlen, trl.get(), nt * rs + kVecPad));
        if (cdw) {
            CHECK(dalloc(&ts->d_tm_cidx, nt * ncb + kVecPad));
            CHECK(h2d(A->ctx, ts->d_tm_cidx, tci.get(), nt * ncb + kVecPad));
        } else {
            CHECK(dalloc(&ts->d_tm_clo, nt * tn + kVecPad));
            CHECK(dalloc(&ts->d_tm_chi, nt * tn + kVecPad));
            CHECK(h2d(A->ctx, ts->d_tm_clo, tcl.get(), sizeof(uint16_t) * (nt * tn + kVecPad)));
            CHECK(h2d(A->ctx, ts->d_tm_chi, tci.get(), nt * tn + kVecPad));
        }
        ts->tm_rs = rs;
        ts->tm = true;
        CHECK(build_x_stage(A, ts, rs));
    }
    return PAMG_OK;
}

int tiles_try(Upload& u) {
    pamg_mat* A = u.A;
    pamg_ctx* ctx = A->ctx;
    const PtrVec& rp = u.rp;
    const IdxVec& ci = u.ci;
    const int64_t nrows = A->nrows, nnz = A->nnz, n_own_cols = u.n_own_cols;
    std::vector<uint16_t> lo;
    std::vector<uint8_t> hi, vidx;
    {
        std::vector<int4> t_in, t_bd;
        const bool square = n_own_cols == nrows;
        const bool tall = n_own_cols < nrows;  // a prolongation's shape
        const int64_t tb = u.inner.empty() && u.bnd.empty() ? 0 : u.band();
        CHECK(build_tiles(rp, u.inner, square, &A->interior, tb, ci, &lo, &hi, u.val, &vidx, &t_in, tall));
        CHECK(build_tiles(rp, u.bnd, square, &A->boundary, tb, ci, &lo, &hi, u.val, &vidx, &t_bd, tall));
        u.tr.mark("tiles");
        std::vector<uint8_t> idx8;
        CHECK(build_col_dicts(A, rp, ci, t_in, t_bd, &idx8));
        u.tr.mark("col dicts");
        CHECK(build_tile_major(A, n_own_cols, rp, ci, u.val, t_in, t_bd, lo, hi, idx8));
        u.tr.mark("tile-major");
    }
    if (A->interior.rl8 || A->boundary.rl8) {
        std::vector<uint8_t> rl(nrows + kVecPad, 0);
        par_for(nrows, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) rl[i] = (uint8_t)std::min<int64_t>(255, rp[i + 1] - rp[i]);
        });
        CHECK(dalloc(&A->d_rlen, nrows + kVecPad));
        CHECK(h2d(ctx, A->d_rlen, rl.data(), rl.size()));
    }
    if (!vidx.empty()) {
        CHECK(dalloc(&A->d_vidx, (int64_t)vidx.size()));
        CHECK(h2d(ctx, A->d_vidx, vidx.data(), vidx.size()));
    }
    if (!lo.empty()) {  // padded like d_col
        lo.resize(nnz + kVecPad, 0);
        hi.resize(nnz + kVecPad, 0);
        CHECK(dalloc(&A->d_clo, nnz + kVecPad));
        CHECK(dalloc(&A->d_chi, nnz + kVecPad));
        CHECK(h2d(ctx, A->d_clo, lo.data(), sizeof(uint16_t) * lo.size()));
        CHECK(h2d(ctx, A->d_chi, hi.data(), sizeof(uint8_t) * hi.size()));
    }
    u.tr.mark("rest");  // (before the index streams above are freed, as the trace always timed it)
    return PAMG_OK;
}

// the bytes one apply streams, per tile set: long rows (row pointer, 12 B/nonzero, list
// entry) + short tiles in their layout — row bounds (1 B/row with 8-bit lengths, else 4-B
// row pointers), columns (4 B; 3 B 24-bit; cd/8 B with a dictionary + its 4-B offsets),
// values (8 B; or a 4-bit index + the tile's 128-B table), 16-B descriptors (+ a 4-B
// column base with 24-bit columns); a tile-major set streams whole padded slots
// (tile_nnz values and column entries, tm_rs row lengths per tile).
int64_t tiles_bytes(const pamg_mat* A) {
    int64_t sum = 0;
    for (const pamg::TileSet* t : {&A->interior, &A->boundary}) {
        if (t->sym || t->ell || t->pnc || t->rpat || t->bsr || t->bsr_r) continue;  // counted by their families
        const int64_t ns = t->n_short, nz = t->nnz_short;
        int64_t b = 8 * (int64_t)t->n_long + 12 * t->nnz_long;
        const bool base = t->c24 && !t->cd;
        if (t->tm) {  // whole padded slots: tile_nnz values + column entries + tm_rs lengths
            const int64_t tn = t->tile_nnz;
            const int64_t rowb = t->tm_rs;
            const int64_t valb = t->tm_vt ? tn + 8 * (int64_t)t->tm_vt : 8 * tn;  // 8-bit indices + table
            b += ns * (rowb * (t->anc ? 5 : 1) + valb + (t->cd ? t->cd * tn / 8 : 3 * tn) + 16 + (base ? 4 : 0)) +
                 (t->cd ? 4 * t->ctab_n * (t->pt ? ns : 1) : 0);
        } else {
            b += (t->rl8 ? 1 : 4) * t->rows_short;
            b += t->cd ? (t->cd * nz + 7) / 8 + 4 * t->ctab_n * (t->pt ? ns : 1) : (t->c24 ? 3 : 4) * nz;
            if (t->pt && t->anc) b += 2 * t->rows_short + 4 * ns;  // 16-bit anchors + tile bases
            b += t->vd ? nz / 2 + 128 * ns : 8 * nz;
            b += (16 + (base ? 4 : 0)) * ns;
        }
        sum += b;
    }
    return sum;
}

void tiles_report(const pamg_mat* A, const pamg::TileSet& t, int out[10]) {
    out[0] = t.c24;
    out[1] = t.vd;
    out[2] = t.rl8;
    out[3] = t.cd;
    out[4] = t.ctab_n;
    out[5] = t.tm;
    out[6] = t.tm_rs;
    out[7] = t.tile_nnz;
    out[8] = t.n_short;
    out[9] = (t.anc ? 1 : 0) | (t.pt ? 2 : 0) | (t.xs ? 4 : 0) | (t.tm && t.tm_vt ? 64 : 0);
}

void tiles_free(pamg::TileSet& ts) {
    dfree(ts.d_short);
    dfree(ts.d_long);
    dfree(ts.d_base);
    dfree(ts.d_vtab);
    dfree(ts.d_ctab);
    ts.cd = ts.ctab_n = 0;
    dfree(ts.d_tm_val);
    dfree(ts.d_tm_cidx);
    dfree(ts.d_tm_clo);
    dfree(ts.d_tm_chi);
    dfree(ts.d_tm_rlen);
    dfree(ts.d_tm_anc);
    dfree(ts.d_tm_vidx);
    dfree(ts.d_tm_vtab);
    ts.tm_vt = 0;
    dfree(ts.d_abase);
    ts.anc = ts.pt = ts.xs = false;
    ts.tm = false;
    ts.tm_rs = 0;
    ts.c24 = ts.vd = ts.rl8 = false;
    ts.max_short_len = 0;
    ts.rows_short = 0;
    ts.n_short = ts.n_long = 0;
}

// pamg_mat_upload (bs = 1), pamg_mat_upload_blocked and pamg_mat_upload_block_rows (bs > 1, their arguments
// checked; rect: the latter): the block-row family is tried first for those two alone; where it declines the
// matrix goes on exactly as bs = 1 does
int mat_upload(pamg_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* rowptr, const void* col, int col_is_64,
               const double* val, int index_base, const pamg_plan* plan, int bs, pamg_mat** out, bool rect = false,
               int value_bits = 64) {
    if (!ctx || !out || nrows < 0 || ncols < 0 || !rowptr || (index_base != 0 && index_base != 1))
        return fail(PAMG_E_ARG, "mat_upload: bad args");
    const int64_t nnz = rowptr[nrows] - index_base;
    if (nnz < 0 || (nnz > 0 && (!col || !val))) return fail(PAMG_E_ARG, "mat_upload: bad arrays");
    if (nnz >= INT32_MAX - 16 || nrows >= INT32_MAX || ncols >= INT32_MAX)
        return fail(PAMG_E_OVERFLOW, "mat_upload: nnz/rows/cols exceed the int32 device layout");
    const int64_t n_own_cols = plan ? plan->n_own : ncols;
    if (plan && plan->n_own + plan->n_ghost != ncols)
        return fail(PAMG_E_ARG, "mat_upload: ncols %lld != plan own+ghost %lld", (long long)ncols,
                    (long long)(plan->n_own + plan->n_ghost));
    CHECK(set_device(ctx));
    UploadTrace tr;
    tr.nnz = nnz;
    PtrVec rp(nrows + 1);
    IdxVec ci(nnz + kVecPad);
    {
        std::atomic<int64_t> bad_row{INT64_MAX};
        par_for(nrows + 1, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) {
                rp[i] = rowptr[i] - index_base;
                if (i > 0 && rowptr[i] < rowptr[i - 1]) {
                    int64_t cur = bad_row.load();
                    while (i - 1 < cur && !bad_row.compare_exchange_weak(cur, i - 1)) {
                    }
                }
            }
        });
        if (bad_row.load() != INT64_MAX)
            return fail(PAMG_E_ARG, "mat_upload: rowptr not monotone at %lld", (long long)bad_row.load());
    }
    if (rp[0] != 0) return fail(PAMG_E_ARG, "mat_upload: rowptr[0] != index_base");
    for (int k = 0; k < kVecPad; ++k) ci[nnz + k] = 0;
    {
        std::atomic<int64_t> bad_at{INT64_MAX};
        par_for(nnz, [&](int64_t a, int64_t b) {
            for (int64_t k = a; k < b; ++k) {
                const int64_t c = (col_is_64 ? static_cast<const int64_t*>(col)[k]
                                             : (int64_t) static_cast<const int32_t*>(col)[k]) - index_base;
                if (c < 0 || c >= ncols) {
                    int64_t cur = bad_at.load();
                    while (k < cur && !bad_at.compare_exchange_weak(cur, k)) {
                    }
                    return;
                }
                ci[k] = (int)c;
            }
        });
        if (bad_at.load() != INT64_MAX) {
            const int64_t k = bad_at.load();
            const int64_t c = (col_is_64 ? static_cast<const int64_t*>(col)[k]
                                         : (int64_t) static_cast<const int32_t*>(col)[k]) - index_base;
            return fail(PAMG_E_ARG, "mat_upload: column %lld out of range", (long long)c);
        }
    }
    tr.mark("columns");
    // SPEC §S15: the operator is A~, a~_ij = (double)RN32(a_ij) — rounded here, before any family sees a value,
    // so every layout, diagonal and block is A~'s; the block-row layouts store the floats themselves. A finite
    // value that rounds to an infinity is refused before anything is allocated.
    std::vector<double> rounded;
    if (value_bits == 32 && nnz > 0) {
        rounded.resize(nnz);
        std::atomic<int64_t> bad_at{INT64_MAX};
        par_for(nnz, [&](int64_t a, int64_t b) {
            for (int64_t k = a; k < b; ++k) {
                const float f = (float)val[k];  // round to nearest even; subnormals and signed zeros kept
                if (std::isinf(f) && std::isfinite(val[k])) {
                    int64_t cur = bad_at.load();
                    while (k < cur && !bad_at.compare_exchange_weak(cur, k)) {
                    }
                }
                rounded[k] = (double)f;
            }
        });
        if (bad_at.load() != INT64_MAX) {
            const int64_t k = bad_at.load();
            const int64_t row = std::upper_bound(rp.begin(), rp.end(), k) - rp.begin() - 1;
            return fail(PAMG_E_ARG,
                        "mat_upload_f32: the value %a of row %lld, column %lld (index base %d) rounds to an infinite "
                        "binary32",
                        val[k], (long long)(row + index_base), (long long)(ci[k] + index_base), index_base);
        }
        val = rounded.data();
        tr.mark("round32");
    }
    // released through pamg_mat_destroy on every error path (no device memory leaks)
    std::unique_ptr<pamg_mat, int (*)(pamg_mat*)> A(new pamg_mat, pamg_mat_destroy);
    A->ctx = ctx;
    ctx_ref(ctx);  // (before the first failure point: the deleter drops it)
    A->nrows = nrows;
    A->ncols = ncols;
    A->nnz = nnz;
    A->plan = plan;
    A->value_bits = value_bits;
    // classify rows: interior (own columns only) or boundary (>= 1 ghost column), and find
    // the diagonal (threads over row ranges)
    std::vector<int> inner, bnd;
    std::vector<double> diag(n_own_cols == nrows ? nrows : 0, 0.0);  // (square operators only)
    std::vector<char> ghost_row(nrows, 0);
    std::atomic<bool> has_all_diag{n_own_cols == nrows};
    // (no ghost columns and no diagonal to find — a one-part prolongation or restriction: nothing
    // to scan)
    const bool scan = n_own_cols == nrows || ncols != n_own_cols;
    if (scan) par_for(nrows, [&](int64_t a, int64_t b) {
        bool all = true;
        for (int64_t i = a; i < b; ++i) {
            bool g = false, d = false;
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
                const int c = ci[k];
                g |= c >= n_own_cols;
                if (c == i && n_own_cols == nrows) {
                    diag[i] = val[k];
                    d = true;
                }
            }
            if (!d || diag[i] == 0.0) all = false;
            ghost_row[i] = g;
        }
        if (!all) has_all_diag = false;
    });
    std::atomic<int64_t> n_ghost_rows{0};
    par_for(nrows, [&](int64_t a, int64_t b) {
        int64_t c = 0;
        for (int64_t i = a; i < b; ++i) c += ghost_row[i];
        n_ghost_rows += c;
    });
    if (n_ghost_rows.load() == 0) {  // (one part: every row interior, listed in parallel)
        inner.resize(nrows);
        par_for(nrows, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) inner[i] = (int)i;
        });
    } else {
        for (int64_t i = 0; i < nrows; ++i) (ghost_row[i] ? bnd : inner).push_back((int)i);
    }
    std::vector<char>().swap(ghost_row);
    tr.mark("classify");
    // The row distance at which rows share x entries, for the banded tile order: per own
    // column the largest gap between consecutive rows that read it (one grid plane for a
    // stencil, one aggregate layer for a restriction); band = its 90th percentile over the
    // columns. (Sequential: the gaps depend on the row order.) Computed when a layout that
    // uses it is tried (the symmetric layout, tiles): not for rows that all go to ELL / pnc.
    int64_t band = -1;
    const std::function<int64_t()> get_band = [&]() -> int64_t {
        if (band >= 0) return band;
        band = 0;
        std::vector<int> max_gap = column_reuse_gaps(rp, ci, nrows, n_own_cols);
        auto end = std::remove(max_gap.begin(), max_gap.end(), 0);
        const size_t m = (size_t)(end - max_gap.begin());
        if (m > 0) {
            auto q = max_gap.begin() + (ptrdiff_t)((m * 9) / 10);
            std::nth_element(max_gap.begin(), q, end);
            band = *q;
            // restriction-shaped operators (fewer rows than columns: R0 reads the fine vector
            // through 5x5x5 root neighbourhoods) walk half-layer bands: each XCD's window
            // of fine lines between reuses halves (512^3 R0 -3 % in kbench,
            // profiles/r02_exp/kbench512_band_pct_r0_p0.jsonl; in the bench R0 -1 %, R1 -2.5 %,
            // the cycle within noise: bench_band_pct_restrict_ab/)
            const int pct = nrows < n_own_cols ? pamg::options().band_pct_restrict : pamg::options().band_pct;
            if (pct != 100) band = std::max<int64_t>(1, band * pct / 100);
        }
        tr.mark("band");
        return band;
    };
    // the layout families in their fixed order: each takes the interior rows left (and clears the
    // list) or declines
    Upload u{A.get(), rp, ci, val, n_own_cols, has_all_diag, inner, bnd, get_band, tr, bs, rect};
    CHECK(bsr_try(u));
    if (!pamg::bsr_any(*A)) {
        CHECK(sym_try(u));
        CHECK(rpat_try(u));
        CHECK(ell_try(u));
        CHECK(pnc_try(u));
    }
    // the CSR copies: read by the tile and long-row kernels only, so not uploaded when every row
    // runs in the symmetric, ELL or neighbour-coded layout (the 512^3 A0, A1, R0, P0: 29 GB less)
    if (!inner.empty() || !bnd.empty()) {
        std::vector<int> rp32(nrows + 1);
        par_for(nrows + 1, [&](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) rp32[i] = (int)rp[i];
        });
        CHECK(dalloc(&A->d_rowptr, nrows + 1));
        CHECK(dalloc(&A->d_col, nnz + kVecPad));
        CHECK(dalloc(&A->d_val, nnz + kVecPad));
        CHECK(h2d(ctx, A->d_rowptr, rp32.data(), sizeof(int) * (nrows + 1)));
        CHECK(h2d(ctx, A->d_col, ci.data(), sizeof(int) * (nnz + kVecPad)));
        CHECK(dzero(ctx, A->d_val, sizeof(double) * (nnz + kVecPad)));
        if (nnz) CHECK(h2d(ctx, A->d_val, val, sizeof(double) * nnz));
    }
    if (has_all_diag && nrows > 0) {
        CHECK(dalloc(&A->d_diag, nrows));
        CHECK(h2d(ctx, A->d_diag, diag.data(), sizeof(double) * nrows));
    }
    tr.mark("csr copies");
    CHECK(tiles_try(u));
    // the bytes one apply streams: every family's share + the closing pointer
    A->stream_bytes = 4 + sym_bytes(A.get()) + ell_bytes(A.get()) + pnc_bytes(A.get()) + rpat_bytes(A.get()) +
                      bsr_bytes(A.get()) + tiles_bytes(A.get());
    *out = A.release();
    return PAMG_OK;
}

// The argument checks of the block uploads (`who` names the entry point): bs in 1..4 and, with bs > 1, whole
// blocks of rows, and a square operator (rect false) or whole blocks of own columns (rect true).
int check_block_args(const char* who, const pamg_ctx* ctx, int64_t nrows, int64_t ncols, const pamg_plan* plan, int bs,
                     bool rect) {
    if (bs < 1 || bs > 4) return fail(PAMG_E_ARG, "%s: block size %d outside 1..4", who, bs);
    if (bs > 1 && ctx && nrows >= 0 && ncols >= 0) {
        const int64_t n_own_cols = plan ? plan->n_own : ncols;
        if (!rect && nrows != n_own_cols)
            return fail(PAMG_E_ARG, "%s: the operator must be square (%lld rows, %lld own columns)", who, (long long)nrows,
                        (long long)n_own_cols);
        if (nrows % bs != 0) return fail(PAMG_E_ARG, "%s: %lld rows are not whole blocks of %d", who, (long long)nrows, bs);
        if (rect && n_own_cols % bs != 0)
            return fail(PAMG_E_ARG, "%s: %lld own columns are not whole blocks of %d", who, (long long)n_own_cols, bs);
    }
    return PAMG_OK;
}

}  // namespace

// ------------------------------------------------------------------ C-ABI: pamg_mat_*

extern "C" {

int pamg_mat_upload(pamg_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* rowptr,
                    const void* col, int col_is_64, const double* val, int index_base,
                    const pamg_plan* plan, pamg_mat** out) {
    return mat_upload(ctx, nrows, ncols, rowptr, col, col_is_64, val, index_base, plan, 1, out);
}

int pamg_mat_upload_blocked(pamg_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* rowptr,
                            const void* col, int col_is_64, const double* val, int index_base,
                            const pamg_plan* plan, int bs, pamg_mat** out) {
    CHECK(check_block_args("mat_upload_blocked", ctx, nrows, ncols, plan, bs, false));
    return mat_upload(ctx, nrows, ncols, rowptr, col, col_is_64, val, index_base, plan, bs, out);
}

int pamg_mat_upload_block_rows(pamg_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* rowptr,
                               const void* col, int col_is_64, const double* val, int index_base,
                               const pamg_plan* plan, int bs, pamg_mat** out) {
    CHECK(check_block_args("mat_upload_block_rows", ctx, nrows, ncols, plan, bs, true));
    return mat_upload(ctx, nrows, ncols, rowptr, col, col_is_64, val, index_base, plan, bs, out, bs > 1);
}

// SPEC §S15: either block upload, or the plain one, of the values rounded to binary32 (mat_upload rounds them
// after its own checks and marks the matrix).
int pamg_mat_upload_f32(pamg_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* rowptr, const void* col,
                        int col_is_64, const double* val, int index_base, const pamg_plan* plan, int bs, int rect,
                        pamg_mat** out) {
    if (rect != 0 && rect != 1) return fail(PAMG_E_ARG, "mat_upload_f32: rect is %d, not 0 or 1", rect);
    CHECK(check_block_args("mat_upload_f32", ctx, nrows, ncols, plan, bs, rect != 0));
    return mat_upload(ctx, nrows, ncols, rowptr, col, col_is_64, val, index_base, plan, bs, out, bs > 1 && rect, 32);
}

int pamg_mat_value_bits(const pamg_mat* A, int* bits) {
    if (!A || !bits) return fail(PAMG_E_ARG, "mat_value_bits: bad args");
    *bits = A->value_bits;
    return PAMG_OK;
}

// Locality permutation inside the device layout: device row i = caller row row_perm[i], own
// column c of the caller = device column inv(col_perm)[c] (ghost columns stay). Each row keeps
// its entries in the caller's storage order, so every row sum (SPEC §S3) keeps its bits; only
// the rows' places and the x entries they gather move.
static int check_perm(const int64_t* p, int64_t n, const char* what) {
    std::vector<char> seen(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (p[i] < 0 || p[i] >= n || seen[p[i]])
            return fail(PAMG_E_ARG, "mat_upload_perm: %s is not a permutation of 0..%lld", what, (long long)(n - 1));
        seen[p[i]] = 1;
    }
    return PAMG_OK;
}

int pamg_mat_upload_perm(pamg_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* rowptr,
                         const void* col, int col_is_64, const double* val, int index_base,
                         const pamg_plan* plan, const int64_t* row_perm, const int64_t* col_perm,
                         pamg_mat** out) {
    if (!ctx || !out || nrows < 0 || ncols < 0 || !rowptr || (index_base != 0 && index_base != 1))
        return fail(PAMG_E_ARG, "mat_upload_perm: bad args");
    const int64_t nnz = rowptr[nrows] - index_base;
    if (nnz < 0 || rowptr[0] != index_base || (nnz > 0 && (!col || !val)))
        return fail(PAMG_E_ARG, "mat_upload_perm: bad arrays");
    if (nnz >= INT32_MAX - 16 || nrows >= INT32_MAX || ncols >= INT32_MAX)
        return fail(PAMG_E_OVERFLOW, "mat_upload_perm: nnz/rows/cols exceed the int32 device layout");
    const int64_t n_own_cols = plan ? plan->n_own : ncols;
    if (n_own_cols > ncols) return fail(PAMG_E_ARG, "mat_upload_perm: plan has more own columns than the matrix");
    if (row_perm) CHECK(check_perm(row_perm, nrows, "row_perm"));
    std::vector<int> cinv;
    if (col_perm) {
        CHECK(check_perm(col_perm, n_own_cols, "col_perm"));
        cinv.resize(n_own_cols);
        for (int64_t k = 0; k < n_own_cols; ++k) cinv[col_perm[k]] = (int)k;
    }
    std::vector<int64_t> rp(nrows + 1, 0);
    for (int64_t i = 0; i < nrows; ++i) {
        const int64_t r = row_perm ? row_perm[i] : i;
        const int64_t len = rowptr[r + 1] - rowptr[r];
        if (len < 0) return fail(PAMG_E_ARG, "mat_upload_perm: rowptr not monotone at %lld", (long long)r);
        rp[i + 1] = rp[i] + len;
    }
    std::vector<int> ci(nnz);
    std::vector<double> va(nnz);
    std::atomic<bool> bad{false};
    par_for(nrows, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) {
            const int64_t r = row_perm ? row_perm[i] : i;
            const int64_t s = rowptr[r] - index_base;
            for (int64_t k = 0; k < rp[i + 1] - rp[i]; ++k) {
                const int64_t c = (col_is_64 ? static_cast<const int64_t*>(col)[s + k]
                                             : (int64_t) static_cast<const int32_t*>(col)[s + k]) - index_base;
                if (c < 0 || c >= ncols) {
                    bad = true;
                    return;
                }
                ci[rp[i] + k] = (c < n_own_cols && col_perm) ? cinv[c] : (int)c;
                va[rp[i] + k] = val[s + k];
            }
        }
    });
    if (bad) return fail(PAMG_E_ARG, "mat_upload_perm: column out of range");
    CHECK(pamg_mat_upload(ctx, nrows, ncols, rp.data(), ci.data(), 0, va.data(), 0, plan, out));
    (*out)->permuted = row_perm || col_perm;
    return PAMG_OK;
}

// SPEC §S12: the node blocks of the own rows and their inverses (pamg_setup_block_diag's arrays, nrows * bs
// doubles each), kept beside d_diag. Device rows must be the caller's rows: a permuted upload scatters the
// nodes' rows, so it is refused.
int pamg_mat_set_block_diag(pamg_ctx* ctx, pamg_mat* A, int bs, const double* blocks, const double* inv) {
    if (!ctx || !A || A->ctx != ctx) return fail(PAMG_E_ARG, "mat_set_block_diag: bad context or matrix");
    (void)hipSetDevice(ctx->device);
    if (bs == 1 || !blocks || !inv) {
        if (bs != 1 && (bs < 2 || bs > 4)) return fail(PAMG_E_ARG, "mat_set_block_diag: block size %d outside 1..4", bs);
        HIPC(hipStreamSynchronize(ctx->s_comp));  // (a sweep still in flight reads the arrays)
        dfree(A->d_bdiag);
        dfree(A->d_binv);
        A->d_bdiag = A->d_binv = nullptr;
        A->bs = 1;
        return PAMG_OK;
    }
    if (bs < 2 || bs > 4) return fail(PAMG_E_ARG, "mat_set_block_diag: block size %d outside 1..4", bs);
    const int64_t n_own_cols = A->plan ? A->plan->n_own : A->ncols;
    if (A->nrows != n_own_cols)
        return fail(PAMG_E_ARG, "mat_set_block_diag: the operator must be square (%lld rows, %lld own columns)",
                    (long long)A->nrows, (long long)n_own_cols);
    if (A->nrows % bs != 0)
        return fail(PAMG_E_ARG, "mat_set_block_diag: %lld rows are not whole blocks of %d", (long long)A->nrows, bs);
    if (A->permuted)
        return fail(PAMG_E_STATE, "mat_set_block_diag: the matrix was uploaded with a permutation (its rows are not "
                    "in node order)");
    HIPC(hipStreamSynchronize(ctx->s_comp));
    dfree(A->d_bdiag);
    dfree(A->d_binv);
    A->d_bdiag = A->d_binv = nullptr;
    A->bs = 1;
    if (A->nrows == 0) {
        A->bs = bs;
        return PAMG_OK;
    }
    const size_t cnt = (size_t)A->nrows * bs;
    CHECK(dalloc(&A->d_bdiag, cnt));
    CHECK(dalloc(&A->d_binv, cnt));
    CHECK(h2d(ctx, A->d_bdiag, blocks, sizeof(double) * cnt));
    CHECK(h2d(ctx, A->d_binv, inv, sizeof(double) * cnt));
    A->bs = bs;
    return PAMG_OK;
}

int pamg_mat_block_size(const pamg_mat* A, int* bs) {
    if (!A || !bs) return fail(PAMG_E_ARG, "mat_block_size: bad args");
    *bs = A->bs;
    return PAMG_OK;
}

int pamg_mat_destroy(pamg_mat* A) {
    if (!A) return PAMG_OK;
    (void)hipSetDevice(A->ctx->device);
    (void)hipStreamSynchronize(A->ctx->s_comp);
    dfree(A->d_rowptr);
    dfree(A->d_col);
    dfree(A->d_clo);
    dfree(A->d_rlen);
    dfree(A->d_chi);
    dfree(A->d_vidx);
    dfree(A->d_cidx);
    dfree(A->d_anc16);
    dfree(A->d_val);
    dfree(A->d_diag);
    dfree(A->d_bdiag);
    dfree(A->d_binv);
    sym_free(A->sym);
    tiles_free(A->interior);
    tiles_free(A->boundary);
    ell_free(A->ell);
    pnc_free(A->pnc);
    rpat_free(A->rpat);
    bsr_free(A->bsr);
    pamg_ctx* owner = A->ctx;
    delete A;
    ctx_unref(owner);
    return PAMG_OK;
}

int pamg_mat_info(const pamg_mat* A, int64_t* nrows, int64_t* ncols, int64_t* nnz) {
    if (!A) return fail(PAMG_E_ARG, "mat_info: NULL");
    if (nrows) *nrows = A->nrows;
    if (ncols) *ncols = A->ncols;
    if (nnz) *nnz = A->nnz;
    return PAMG_OK;
}

int pamg_mat_stream_bytes(const pamg_mat* A, int64_t* bytes) {
    if (!A || !bytes) return fail(PAMG_E_ARG, "mat_stream_bytes: bad args");
    *bytes = A->stream_bytes;
    return PAMG_OK;
}

int pamg_mat_layout(const pamg_mat* A, int set, int out[10]) {
    if (!A || !out || set < 0 || set > 1) return fail(PAMG_E_ARG, "mat_layout: bad args");
    const pamg::TileSet& t = set == 0 ? A->interior : A->boundary;
    tiles_report(A, t, out);  // every slot; the family that holds the set overrides its own
    ell_report(A, t, out);
    rpat_report(A, t, out);
    pnc_report(A, t, out);
    sym_report(A, t, out);
    bsr_report(A, t, out);
    return PAMG_OK;
}

int pamg_mat_ell_window(const pamg_mat* A, int out[16]) {
    if (!A || !out) return fail(PAMG_E_ARG, "mat_ell_window: bad args");
    ell_window(A, out);
    return PAMG_OK;
}

int pamg_mat_ell_span(const pamg_mat* A, int out[8]) {
    if (!A || !out) return fail(PAMG_E_ARG, "mat_ell_span: bad args");
    ell_span(A, out);
    return PAMG_OK;
}

int pamg_mat_ell_classes(const pamg_mat* A, int64_t out[8]) {
    if (!A || !out) return fail(PAMG_E_ARG, "mat_ell_classes: bad args");
    ell_classes(A, out);
    return PAMG_OK;
}

}  // extern "C"
