// pamg_device.h — device-side objects of libpamg (context, plans, vectors, matrices,
// hierarchy) and the kernel launchers of kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cstdint>
#include <array>
#include <mutex>
#include <vector>

#include "pamg_common.h"

namespace pamg {

// Row tiles of the LDS-staged CSR kernels (kernels.hip): each tile is a run of <= kTileRows
// consecutive rows (one per lane of the 256-thread workgroup) holding <= tile_nnz nonzeros;
// a row longer than the budget is a tile of its own in the "long" list.
constexpr int kBlock = 256;
constexpr int kTileRows = 256;

// x staging of row-relative dictionary tiles (TileSet::xs, k_rows_tm<..., XS>): the x values a
// tile reads are the runs [r0 + omin_c, r0 + nr - 1 + omin_c + wid_c] of its offset clusters c
// (offsets within kXsGap of each other share a run); they are loaded coalesced at kernel entry
// into LDS segments of `stride` doubles and the products read them there — no dependent x
// gathers. The dictionary table holds, at kXsIoff + index, each offset's LDS position
// c * stride + offset - omin_c.
constexpr int kXsMaxClusters = 12;
// tile-major sets of 2048-nonzero tiles: per-tile column / value tables of <= this many entries
constexpr int kTmSmallTab = 128;
constexpr int kXsCap = 1088;   // LDS doubles (8.5 KiB; 512^3 7-point: 5 runs x 210)
constexpr int kXsIoff = 128;   // table entries [128, 256): the LDS positions of offsets [0, 128)
constexpr int kXsGap = 48;
struct XStage {
    int ncl = 0, stride = 0, zix = -1, ncols = 0;
    int omin[kXsMaxClusters] = {}, wid[kXsMaxClusters] = {};
};
enum RowOp : int {
    OP_SPMV = 0,     // y = A x
    OP_RESID = 1,    // y = b - A x
    OP_JACOBI = 2,   // y = x + (omega (b - A x)) / a_ii
    OP_PROLONG = 3,  // y = y + A x      (x += P e)
    // (4, 5: the temporally blocked passes of pamg_bench_rowop)
    OP_CHEB = 6,     // y = x + (c1 (x - xold) + (c2 (b - A x)) / a_ii): Chebyshev step k >= 1 (SPEC §S9);
                     // c2 travels in the omega argument, a null xold stands for a zero vector
};

struct TileSet {
    int4* d_short = nullptr;  // (row_begin, row_end, nnz_begin, nnz_end)
    int n_short = 0;
    int* d_long = nullptr;  // single rows
    int n_long = 0;
    int tile_nnz = 1024;  // nonzero budget the tiles were cut with
    // 24-bit column stream: every tile's columns lie in [base, base + 2^24), so a column is
    // stored as base (per tile) + 16-bit low part (pamg_mat::d_clo) + 8-bit high part (d_chi)
    int* d_base = nullptr;  // per short tile (same order as d_short), when c24
    bool c24 = false;
    // value dictionary (opt-in, Options::value_dict): every tile has <= 16 distinct values;
    // a value is a 4-bit index (pamg_mat::d_vidx) into the tile's 16-entry table
    double* d_vtab = nullptr;  // 16 per short tile
    bool vd = false;
    // 8-bit row lengths (pamg_mat::d_rlen) instead of row pointers: every row of a short tile
    // has <= 255 nonzeros (one row per lane, 24-bit columns, plain values)
    bool rl8 = false;
    // column dictionary (Options::col_dict; needs rl8): every nonzero of the short tiles has
    // column = row + d_ctab[i] for one of the set's <= 16 (cd = 4 bits) / <= 256 (cd = 8)
    // offsets; i is stored in pamg_mat::d_cidx (4 or 8 bits per nonzero)
    int cd = 0;
    int* d_ctab = nullptr;
    int ctab_n = 0;
    // anchored dictionary (Options::col_dict_anchor; tile-major sets only): column = the row's
    // first column + d_ctab[i]; the row anchors sit in the tile-major slots (d_tm_anc)
    bool anc = false;
    // per-tile dictionaries (Options::col_dict_tile; anchored: descriptor kernel, row-relative: tile-major slots): d_ctab holds
    // n_short tables of ctab_n entries; anchored ones take pamg_mat::d_anc16 + d_abase[tile]
    bool pt = false;
    int* d_abase = nullptr;
    // x staging (Options::x_stage): see XStage
    bool xs = false;
    XStage xst;
    // tile-major copies (Options::tile_major; kernels.hip k_rows_tm): tile t's values and
    // column stream at t * tile_nnz, its row lengths at t * tm_rs, zero-padded
    bool tm = false;
    int tm_rs = 0;                 // row-length slot per tile (>= its rows, multiple of 4)
    double* d_tm_val = nullptr;
    uint8_t* d_tm_cidx = nullptr;  // column dictionary indices (cd bits each)
    uint16_t* d_tm_clo = nullptr;  // or 24-bit columns: low 16 bits
    uint8_t* d_tm_chi = nullptr;   //   high 8 bits
    uint8_t* d_tm_rlen = nullptr;
    int* d_tm_anc = nullptr;       // anchored dictionary: each row's first column (tm_rs per tile)
    // 8-bit per-tile value dictionaries in tile-major slots (Options::value_dict, where every
    // tile of the set has <= 256 distinct values and the 4-bit ones do not fit): value = tile
    // t's table d_tm_vtab[t * tm_vt + index], index d_tm_vidx[t * tile_nnz + k]; d_tm_val unused
    int tm_vt = 0;                 // table entries per tile (0: plain values)
    uint8_t* d_tm_vidx = nullptr;
    double* d_tm_vtab = nullptr;
    // symmetric diagonal-class layout (Options::sym_dia; interior set of a square operator,
    // pamg_mat::sym): the set's rows run in k_rows_sym instead of tiles
    bool sym = false;
    // sliced-ELL layout (pamg_mat::ell; the whole interior set of a square operator): the set's rows run in
    // k_rows_ell instead of tiles
    bool ell = false;
    // neighbour-coded prolongation (pamg_mat::pnc; the whole set of a prolongation over a registered grid):
    // the rows run in k_rows_pnc instead of tiles
    bool pnc = false;
    // pattern-dictionary rows (pamg_mat::rpat; the whole interior set of a restriction): the rows run in
    // k_rows_rpat instead of tiles
    bool rpat = false;
    // block-row layout (pamg_mat::bsr; the whole of a square node-major operator uploaded through
    // pamg_mat_upload_blocked): the rows run in k_rows_bsr instead of tiles
    bool bsr = false;
    // the block-row layout's row-per-lane form (pamg_mat::bsr with BsrSet::row_lanes; a restriction-shaped
    // operator uploaded through pamg_mat_upload_block_rows): the rows run in k_rows_bsr_r (bsr_multi.hip)
    // through launch_set, never in launch_rows
    bool bsr_r = false;
    int max_short_len = 0;    // longest row in a short tile
    int64_t rows_short = 0;   // rows covered by the short tiles
    int64_t nnz_short = 0, nnz_long = 0;  // nonzeros covered by the tiles / the long rows
};

// Tuning knobs (pamg_set_option): kernel variant and tile budget used by later uploads.
struct Options {
    // defaults = fastest measured on MI355X at 512^3 (profiles/r01_kbench_*.jsonl):
    // 1024-nonzero / 256-row tiles
    int tile_nnz = 1024;       // 1024 / 2048 / 4096 (tiles always hold <= kTileRows rows)
    int tile_order = 1;        // 1: banded XCD-blocked tile order (see build_tiles)
    int col24 = 1;             // 1: 3-byte column stream where every tile's span fits 2^24
    int long_tiles = 1;        // 1: 4096-nonzero tiles for square operators with long rows (build_tiles)
    int long_tiles_min = 24;   // nonzeros per row from which sets of >= 32 x 4096 nonzeros per CU take 2048-nonzero tiles
    int row_len8 = 1;          // 1: 8-bit row lengths instead of 32-bit row pointers where they fit
    int value_dict = 1;        // 1: per-tile value dictionaries (4-bit for rectangular operators where a tile has
                               //    <= 16 distinct values, 8-bit in tile-major slots); 2: 8-bit ones only
    int col_dict = 1;          // 1: row-relative column dictionaries (4/8-bit) where they fit
    int tile_major = 1;        // tile-major padded copies (variant 4): 1 where measured faster, 2 all eligible
    int col_dict_tile = 1;     // 1: per-tile column dictionaries where no global table fits (and they beat 24-bit)
    int tm_tile_dicts = 1;     // 1: row-relative per-tile dictionary sets in tile-major slots (512^3 A1: -1..-3 %)
    int band_pct = 100;        // scale of the measured band of the XCD-blocked tile order (percent)
    int band_pct_restrict = 50;  // the same for operators with fewer rows than columns (restrictions)
    int x_stage = 1;           // 1: stage x runs in LDS for row-relative dictionary tile-major sets (no x gathers)
    int col_dict_anchor = 1;   // 1: anchored column dictionaries (col - row's first column) where row-relative ones do not fit
    int poison_ghosts = 0;     // 1 (debug): NaN-fill ghost slots before each exchange
    int sym_dia = 1;           // 1: symmetric diagonal-class layout for stencil-shaped symmetric operators
    int sym_rows = 2;          // rows per lane of its kernel (1 | 2)
    int jr_fuse = 1;           // 1: temporally blocked level-0 Jacobi -> residual / cross-cycle pipeline where the
                               //    operator is a grid stencil (k_sym_tb)
    int symd_chunks = 2;       // 512-row units per block of k_rows_symd (1, 2 or 4; 2: SpMV -2 %, residual and
                               // Jacobi -4..-5 %, 4: -1..-2 %; same-box A/B profiles/r04_g_c2/, r04_g_c4/)
    int chain_store_x = 0;     // 1: the pipelined chain also stores its post-smoothed iterate (never read)
    int tb_xfast = 1;          // blocked passes: tiles x-fastest (an XCD takes whole rows of tiles; chain -0.9 %,
                               // S = 2 pass -1.1 %, same-box A/B profiles/r05_l/) or y-fastest (0)
    int sym_zm = 1;            // 1: one-sweep ops of a whole one-part row-class grid operator march along z
                               //    (k_sym_zm); 0: k_rows_symd
    int zm_chunks = 0;         // z chunks per tile column of k_sym_zm (0: ~4 workgroups per CU)
    int ell = 1;               // 1: sliced ELL with per-group 8-bit dictionaries for square operators whose every row
                               //    is interior, where the tables fit (EllSet; the level-1 operator)
    int ell_min_rows = 65536;  // ... with at least this many rows
    int ell_restrict = 1;      // 1: also restrictions (fewer rows than columns), offsets from each row's first column
    int ell_yblock = 16;       // restrictions over a grid: groups processed in (y-block of this many lines, z, y)
                               //    order within each XCD's eighth (0: row order; 512^3 R0 0.81 -> 0.745 ms for any
                               //    block of 2..64 lines, profiles/r05_r/); read at upload
    int rpat = 1;              // 1: pattern-dictionary rows for restrictions whose rows repeat few patterns (RpatSet)
    int ell_pair = 1;          // 1: one index byte per ELL nonzero naming an (offset, value) pair where they fit
    int ell_xwin = 1;          // 1: windowed ELL for whole square one-part operators with pair tables (EllSet::win):
                               //    groups of 4 coupled slices whose x neighbourhood is staged in LDS. Taken where
                               //    >= kEllWinMinShare percent of the groups are windowed and their nonzeros per
                               //    window entry are >= kEllWinMinRatio100 / 100 (below: the thresholds). With 1
                               //    a windowed operator also stores each slice's distinct rows once, and a class
                               //    byte per row, where that at least halves its index bytes (EllSet::cls);
                               //    2: windowed, always the per-row index stream. With 1 and 2 windowed groups whose
                               //    windows overlap are coupled into pairs that share one workgroup and one staged
                               //    window (EllSet::npairs; k_rows_ellw's SPAN 2); 3 and 4: as 1 and 2 without pairs
    int ell_xwin_max = 7168;   // window capacity in doubles (<= kEllWinCap, the kernel's: 56 KB of its 60 KB of LDS)
    int pnc_compact = 1;       // 1: 16-bit combination ids instead of 64-bit records where <= kPncCombMax fit
    int pnc = 1;               // != 0: neighbour-coded prolongations over a grid registered on the context (PncSet);
                               //    read per launch, where the plane cuts into tiles: 1 the tiled march with the coarse
                               //    values in LDS, 3 the one with the anchors in LDS; 2 (and other planes) the line blocks
    int sym_vd = 1;            // 1: row-class dictionary for the symmetric layout where the rows take <= kSymVdMax
                               //    distinct (mask, diagonal, upper values) tuples (SymDia::vd_n)
};

// Symmetric diagonal-class layout (k_rows_sym): a square operator whose interior rows use at
// most 2*kSymMaxU+1 row-relative offsets {-o_NU..-o_1, 0, o_1..o_NU} (a symmetric set), each
// row in ascending offset order, with bitwise-symmetric values a_ij == a_ji. Per own row i:
// the diagonal D[i], the upper values U_c[i] = a(i, i+o_c) (0 where absent), and a 16-bit
// mask (bit k: the k-th offset in ascending order is present; bit 15: the row belongs to the
// set). A lower value a(i, i-o_c) is read from its mirror U_c[i-o_c], so the matrix streams
// NU+1 values per row instead of 2*NU+1, with no column stream at all. (Where 2*NU+1 <= 7 the
// mask is one byte, the set flag in bit 7.)
constexpr int kSymMaxU = 7;
// Row-class dictionary of the symmetric layout (Options::sym_vd): at most this many distinct
// (mask, D, U_0 .. U_{nu-1}) bit tuples over the own rows; each row then stores its class id
// (1 byte) instead of mask + diagonal + nu upper values, the table sits in LDS
constexpr int kSymVdMax = 64;
// Temporal blocking of S dependent row sweeps (kernels.hip k_sym_tb): the operator is a 7-point
// grid stencil in natural order — classes {1, nx, nx*ny}, n = nx*ny*nz, and no row reaching
// across a grid line or plane (checked at upload) — so a workgroup owns a kTbX x kTbY column of
// the grid over a range of planes and streams it along z, computing the earlier sweeps on a
// halo it recomputes itself. No data passes between workgroups inside a launch.
struct TbGeom {
    int nx = 0, ny = 0, nz = 0;
    int tiles_x = 0, tiles_y = 0;   // kTbX x kTbY tiles of a plane
    int zchunks = 1, zlen = 0;      // planes per workgroup (the last chunk may be shorter)
    int zlo = 0, zhi = 0;           // output planes [zlo, zhi) of a launch (set by launch_sym_tb)
    int xfast = 0;                  // tile order: 0 y-fastest, 1 x-fastest (kernels.hip tb_ctx_init)
};
// Sliced ELL with per-group dictionaries (Options::ell; round 5, the level-1 operator and R0 of one
// part; on several parts the interior rows of a part's operator, its boundary rows carrying the length
// byte kEllSkip and running in tiles after the exchange): rows in
// slices of kEllW consecutive rows (one per lane of a wave), kEllGroup rows (a workgroup) sharing
// two tables of <= 256 entries — the rows' column offsets (col - row) and values (bit patterns).
// A slice stores its padded nonzeros k = 0 .. maxlen-1 as one column-index byte and one value-index
// byte per row, 4 consecutive k of a row packed in a dword, lanes interleaved: dword (k / 4, lane) at
// start + (k / 4) * kEllW + lane. Rows keep their storage order (the products are summed in it).
constexpr int kEllW = 64;
constexpr int kEllGroup = 256;
constexpr int kEllSkip = 255;  // length byte of a row outside the set (several parts: a boundary row)
// Windowed ELL (Options::ell_xwin; k_rows_ellw): a workgroup's 4 slices are chosen by coupling, not
// consecutive (d_gslices, -1: none), the x entries their rows read are runs of consecutive columns
// loaded once into LDS in chunks of <= 64 x 16 bytes (d_chunks: first column — even —, LDS slot |
// double2 count << 16), and the x of a nonzero of wave w naming pair p is lx[lof[w][p] + lane]
// (d_lof: 16-bit words per group in [wave][pair] order: lof + 64); d_dpos is each row's diagonal
// position (the entry with offset 0; 255: none), for Jacobi. A group whose window exceeds ell_xwin_max or kEllWinChunks chunks gathers as k_rows_ell
// does (d_wmeta .y == 0). Acceptance: the operator takes the layout where at least kEllWinMinShare
// percent of its groups are windowed and those groups hold at least kEllWinMinRatio100 / 100 nonzeros
// per window entry (a 7-point grid's 4-line groups hold 2.0, the 512^3 A1 3.1; at 1.0 every entry
// would be loaded for one use, the gathers' own traffic).
constexpr int kEllWinCap = 7168;
constexpr int kEllWinChunks = 256;  // (a wave reads its <= 64 chunk words with one load)
constexpr int kEllLdsPerCu = 160 * 1024;
constexpr int kEllWinKeep = 85;  // percent of the windowed groups kept when the largest window is lowered for occupancy
constexpr int kEllWinMinShare = 50;
constexpr int kEllWinMinRatio100 = 150;
// Group pairs (Options::ell_xwin 1 and 2, not 3 and 4; ell_span.h, k_rows_ellw's SPAN 2): two windowed groups whose
// windows overlap run in one workgroup of 2 * kEllGroup threads behind one barrier, their union
// window staged once. The groups are renumbered so that pair p holds groups 2p and 2p + 1 and the
// groups left single follow; d_pairs holds 4 int4 per pair: the slices of group 2p, of group 2p + 1,
// (table start and entries of either), (first chunk, chunks | window doubles << 16, first d_lof word
// of either). A CU holds 2,048 threads, so at most 4 such workgroups, whatever their LDS; fewer would
// be the single groups' 24 waves or less. So the union's capacity is what 4 per CU leave of the LDS
// after either group's tables (2 x 4 KB): kEllSpanWin doubles. 8 waves read the chunk words, lane k
// of wave w chunk w + 8k: kEllSpanChunks. A pair is kept where the union is at most kEllSpanShare
// percent of the two windows together: the workgroup's barrier waits for the whole union, the longer
// staging chain of the two, and that is paid for by what is staged less — below a tenth of two
// windows (~600 doubles at 512^3) the saving is less than one group's tables and lof words (4 KB).
constexpr int kEllSpanWin = (kEllLdsPerCu / 4 - 2 * 4096) / 8;
constexpr int kEllSpanChunks = 2 * kEllWinChunks;
constexpr int kEllSpanShare = 90;
struct EllSet {
    int64_t nslices = 0, ngroups = 0;
    int2* d_smeta = nullptr;     // per slice: (first dword of its index streams, maxlen)
    uint32_t* d_ci = nullptr;    // column-index stream
    uint32_t* d_vi = nullptr;    // value-index stream
    uint8_t* d_len = nullptr;    // per row: its length
    int4* d_gmeta = nullptr;     // per group: (offset-table start, entries, value-table start, entries)
    int* d_otab = nullptr;       // the groups' offset tables, concatenated
    double* d_vtab = nullptr;    // the groups' value tables, concatenated
    int* d_anc = nullptr;        // anchored (rectangular operators): per row the column its offsets start from
    // a restriction over a registered grid (its columns are the grid's points): the groups in a
    // processing order whose in-flight window is a compact (y, z) block of the grid instead of whole
    // planes (Options::ell_yblock; kernels.hip k_rows_ell), null otherwise
    int* d_gorder = nullptr;
    int64_t words = 0, otab_n = 0, vtab_n = 0;
    // paired dictionaries (Options::ell_pair): one index byte per nonzero names an (offset, value)
    // pair of the group (d_otab / d_vtab entries in parallel, gmeta .x == .z, .y == .w); d_vi null
    bool paired = false;
    // windowed (Options::ell_xwin; then paired, d_anc and d_gorder null, ngroups = the coupled groups)
    bool win = false;
    int4* d_gslices = nullptr;   // per group: its waves' slices (-1: none)
    int4* d_wmeta = nullptr;     // per group: (first chunk, chunks — 0: gather —, first d_lof word, window doubles);
                                 // a paired group: chunks 0 (alone it gathers), window = its pair's union
    int2* d_chunks = nullptr;
    uint16_t* d_lof = nullptr;
    uint8_t* d_dpos = nullptr;
    int64_t nchunks = 0, lof_n = 0;
    int win_groups = 0, gather_groups = 0, noncontig_groups = 0;
    int max_window = 0, max_pairs = 0, max_chunks = 0;  // over the windowed groups (max_pairs: all groups)
    // census of the upload (pamg_mat_ell_window): windows, runs and pairs per windowed group, 4-slice groups
    int mean_window = 0, p95_window = 0, mean_runs = 0, max_runs = 0, mean_pairs = 0, full_groups = 0;
    // group pairs (Options::ell_xwin 1 | 2; above): groups 0 .. 2 npairs - 1 run pairwise, the rest alone
    int4* d_pairs = nullptr;
    int npairs = 0;
    int max_union = 0, mean_union = 0, p95_union = 0;  // the pairs' union windows (doubles)
    int union_pct = 0;                                  // mean of union / (the two windows), percent
    // row classes (Options::ell_xwin 1 | 3; windowed operators): two rows of a slice are one class where their
    // length, diagonal position and pair bytes are equal. d_ci then holds every slice's classes once, padded
    // to the slice's dwords and class-interleaved — dword q of class c at start + q * nc + c, d_smeta .y =
    // maxlen | minlen << 8 | nc << 16 (minlen: the slice's shortest row, 0 for a partial slice: the dwords
    // below minlen / 4 hold no padding, and the kernel walks them without its selects) — and d_cid each
    // row's class within its slice. Taken where the class records and the id bytes are at most half of
    // the per-row stream (below that the kernel's loads are the same in number, their lines fewer);
    // `words` stays the per-row stream's size, for the census.
    bool cls = false;
    uint8_t* d_cid = nullptr;
    int64_t cls_words = 0;
    int cls_max = 0;             // most classes of a slice
    int64_t cls_total = 0;       // classes over all slices
};

// Neighbour-coded prolongation (Options::pnc; round 5, the 512^3 P0): a prolongation (more rows than
// columns) whose rows are the points of a 7-point grid uploaded earlier on the same context — on one
// part all of them; on several parts a part's interior rows, its boundary rows (ghost columns) carrying
// the pattern id kPncSkip and running in tiles after the exchange (the grids: pamg_ctx::grids).
// Each column of row i is the anchor of one of the points i, i-1, i+1, i-nx, i+nx, i-M, i+M (codes 0..6) — the anchor of a row being the column of its largest
// value (in smoothed aggregation: the point's own aggregate; P = (I - w D^-1 A) P_tent reaches
// the aggregates of the point's stencil neighbours). Per row: the anchor (4 B) and a 64-bit record:
// bits 0-9 a pattern id (a global table of <= kPncPatMax words: bits 0-2 the row length, 3 + 3k
// the k-th entry's neighbour code), bits 10 + 7k the k-th entry's value index (a global table of
// <= kPncValMax bit patterns). 12 B per row against 3.5 B per nonzero + 1 B per row in tiles. Rows
// keep their storage order (SPEC S3 sums).
constexpr int kPncPatMax = 1024, kPncValMax = 128, kPncMaxLen = 7;
constexpr int kPncSkip = kPncPatMax - 1;  // pattern id of a row outside the set (several parts: a boundary row)
// Compact records (round 6): where the rows take at most kPncCombMax distinct (pattern word, value
// indices) combinations — 428 for the 512^3 P0, whose aggregates are nearly all alike — a row stores
// a 16-bit combination id (kPncCombSkip: outside the set) instead of the 64-bit record: 6 B per row
// with the anchor instead of 12. Then d_ptab holds the combinations' pattern words and d_pvals their
// value indices (7 bits per entry from bit 0), npat = the combinations, d_rec = null.
constexpr int kPncCombMax = 1024;
constexpr int kPncCombSkip = 0xffff;
// The tiled march (Options::pnc == 1: k_rows_pncv, the tile's coarse values in LDS; == 3:
// k_rows_pnct, its anchors in LDS): a workgroup's 256 rows are a kPncTx x kPncTy tile of a plane,
// where the plane cuts into whole tiles; else, and under Options::pnc == 2, 256 consecutive points
// of a line (k_rows_pnc). The PncSet arrays and the grid are the same for all three. A 7-point
// grid registers on the context where its planes cut into these tiles (matrix.hip).
constexpr int kPncTx = 64, kPncTy = 4;
constexpr bool pnc_tiled(int nx, int ny) { return nx % kPncTx == 0 && ny % kPncTy == 0; }
struct PncSet {
    int nx = 0, ny = 0, nz = 0;
    int* d_anc = nullptr;       // nrows (+ pad)
    uint2* d_rec = nullptr;     // nrows (+ pad): the 64-bit records as (low, high) dwords
    uint16_t* d_cid = nullptr;  // compact records: nrows (+ pad) combination ids
    uint64_t* d_pvals = nullptr;
    uint32_t* d_ptab = nullptr;
    double* d_vtab = nullptr;
    int npat = 0, nval = 0;
    int grid = 0;               // workgroups of k_rows_pnct / k_rows_pnc
};

// Pattern-dictionary rows (Options::rpat; round 6, the 512^3 R0): a restriction (fewer rows than columns)
// whose rows, read as (column - the row's first column, value bits) sequences in storage order, are
// copies of at most kRpatMax patterns of at most kRpatEnt entries in all. In smoothed aggregation a
// row of R = P^T is one aggregate's dilated shape, so the patterns are the aggregate shapes: 58 of
// them, 1,249 entries, for the 16.8M rows of the 512^3 R0 (the sliced ELL, 2 index bytes per padded
// nonzero, streamed 59 B per row). Per row: its first column (4 B) and pattern id (1 B; kRpatSkip: a
// row outside the set, several parts' boundary rows). Pattern p's entries at d_pent[start_p ..
// start_p + len_p): column offset in bits 0-23, value index (into d_vtab, <= 256 bit patterns) in
// bits 24-31. Rows keep their storage order (SPEC S3 sums); the groups of kEllGroup rows run in the
// ELL's blocked order over the registered grid of the columns (d_gorder) where there is one.
constexpr int kRpatMax = 255, kRpatEnt = 4096, kRpatMaxLen = 128;
constexpr int kRpatSkip = 255;
struct RpatSet {
    int64_t ngroups = 0;
    int* d_anc = nullptr;        // nrows (+ pad): the first column of each row
    uint8_t* d_pid = nullptr;    // nrows (+ pad): the pattern id of each row
    int2* d_pmeta = nullptr;     // per pattern: (first entry, entries)
    uint32_t* d_pent = nullptr;  // the patterns' entries, concatenated
    double* d_vtab = nullptr;    // the values' bit patterns
    int* d_gorder = nullptr;     // the groups' processing order (as EllSet::d_gorder), or null
    int npat = 0, nent = 0, nval = 0;
};

// Block-row layout (pamg_mat_upload_blocked; k_rows_bsr): a square one-part operator in node-major order
// whose rows bs m .. bs m + bs - 1 (node m) store the same block columns, every touched bs x bs block
// whole (explicit zeros stored) and each row's entries in ascending column order. A sliced ELL over
// block rows in natural order: slice s holds the kEllW block rows from kEllW s, one per lane of a wave,
// padded to the slice's own width (the most blocks of any of its rows); its slots start at block slot
// d_soff[s] (64-bit) and number d_soff[s + 1] - d_soff[s]. Slot k of slice s, lane l: the block column at
// d_bcol[(d_soff[s] + k) * kEllW + l] (-1: padding — skipped, no x read, no product, SPEC §S3), the
// block's entry (d, e) at d_val[((d_soff[s] + k) * bs * bs + d * bs + e) * kEllW + l]. One column index per
// block: 8 + 4 / bs^2 bytes per stored nonzero; x is gathered once per block as bs adjacent doubles; a
// lane holds its node's bs row sums in registers (the fused block smoothers of SPEC §S12).
//
// Through pamg_mat_upload_block_rows the operator may be rectangular (a block column c reads x[bs c ..
// bs c + bs - 1] of the column space; an empty block row is all padding), and a restriction-shaped one —
// fewer rows than own columns: few, long block rows — takes the row-per-lane form (row_lanes; k_rows_bsr_r):
// a sliced ELL over SCALAR rows, slice s the kEllW rows from kEllW s, so the bs rows of a node sit in bs
// adjacent lanes and every row sum is still one lane's (SPEC §S3). Slot k of slice s, lane l: the block
// column at d_bcol[(d_soff[s] + k) * kEllW + l] (-1: padding), the row's bs entries of that block at
// d_val[((d_soff[s] + k) * kEllW + l) * bs + e] — bs adjacent doubles per lane, contiguous over the wave.
// 8 + 4 / bs bytes per stored nonzero, bs times the lanes of the node-per-lane form.
//
// Through pamg_mat_upload_f32 (SPEC §S15) either form holds its values as binary32 in d_val32, the same slots
// in the same order (d_val stays null): 4 + 4 / bs^2 and 4 + 4 / bs bytes per stored nonzero. The kernels widen
// each value exactly before the fp64 product.
constexpr int kBsrSlices = kBlock / kEllW;  // slices (waves) per workgroup
struct BsrSet {
    int bs = 0;
    int64_t nb = 0, nslices = 0;  // block rows, slices
    int64_t slots = 0;            // padded block slots: d_soff[nslices] * kEllW
    int64_t* d_soff = nullptr;    // nslices + 1
    int* d_bcol = nullptr;        // slots
    double* d_val = nullptr;      // slots * bs * bs
    float* d_val32 = nullptr;     // SPEC §S15 (pamg_mat_upload_f32): the same slots as binary32, d_val null
    int grid = 0;                 // workgroups of k_rows_bsr
    bool row_lanes = false;       // the row-per-lane form: nslices, slots and the arrays are per scalar row
};

struct SymDia {
    int nu = 0;                     // upper offset classes
    int off[kSymMaxU] = {};         // ascending positive offsets
    int64_t ld = 0;                 // leading dimension of the U arrays
    int band = 0, band_blocks = 0, eighth = 0, nbands = 0;  // XCD-banded block order
    int rpl = 1;                    // rows per lane (k_rows_sym / k_rows_sym2)
    // temporally blocked sweeps (Options::jr_fuse; one part, every row in the set, nu = 3)
    bool tb_ok = false;
    // one part of several (z-slab of whole planes; a plane next to another part reads ghosts,
    // the set is the other planes): the blocked passes run on the planes whose halo stays inside
    // the set (S planes from a neighbour part) and the separate sweeps (with their exchanges) on
    // the rest (runtime.hip jr_part)
    bool tb_part = false;
    int part_lo = 0, part_hi = 0;   // the set's planes [part_lo, part_hi) (the others read ghosts)
    int plane0 = 0;                 // first plane of a plane-range launch of k_rows_sym / sym2
    int gap_at = 1 << 30, gap = 0;  // ... whose planes from gap_at on are shifted by gap (a second window)
    TbGeom tb;
    uint8_t* d_mask = nullptr;      // nrows (+ pad) masks of 1 byte (2 nu + 1 <= 7) or 2 bytes
    int mask_bytes = 2;
    double* d_diag = nullptr;       // nrows (+ pad)
    double* d_upper = nullptr;      // nu * ld
    // row-class dictionary (vd_n > 0; then d_mask / d_diag / d_upper are not allocated): row i's
    // class d_tid[i]; class e's values d_vtab[e * (nu + 1) + {0: D, 1 + c: U_c}], mask d_mtab[e]
    // (the in-set flag included); the lower value a(i, i - o_c) is U_c of class d_tid[i - o_c]
    int vd_n = 0;
    int vd_main = 0;                // the most frequent class (k_rows_symd's register fast path)
    uint8_t* d_tid = nullptr;       // nrows (+ pad)
    double* d_vtab = nullptr;
    uint32_t* d_mtab = nullptr;
};
Options& options();

}  // namespace pamg

struct pamg_ctx {
    int device = 0;
    // references: the caller's handle + one per plan / vector / matrix / hierarchy on it
    // (runtime.hip ctx_ref / ctx_unref); the context is torn down when the last one is dropped
    std::atomic<int> refs{1};
    hipStream_t s_comp = nullptr;  // compute stream
    hipStream_t s_comm = nullptr;  // ghost exchange stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    pamg_host_comm_fn host_fn = nullptr;  // debug transport (pamg_comm_init_host)
    void* host_user = nullptr;
    pamg_world* world = nullptr;           // in-process transport (pamg_comm_init_local)
    hipEvent_t ev_ready = nullptr;         //   "the vector I posted is written" (on s_comp / s_comm)
    std::vector<double> h_send, h_recv;   // staging for the debug transport
    double* d_red = nullptr;  // reduction workspace (partials + result)
    int red_cap = 0;
    double* h_red = nullptr;  // pinned host scalar
    // the reductions of a multi-column step (SPEC §S13; allocated by the first multi-column call): column
    // c's partials at d_redk + c * 1024, the results behind them; h_redk: the pinned results
    double* d_redk = nullptr;
    double* h_redk = nullptr;
    // upload staging (matrix.hip h2d): two pinned 64 MiB buffers and their DMA-done events,
    // created on first use on this context's device and owned by the context
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_done[2] = {nullptr, nullptr};
    // 7-point grids of the square operators uploaded on this context in the temporally blocked
    // layout (SymDia::tb_ok): (rows, nx, ny, nz) — a later prolongation with as many rows may take
    // the neighbour-coded layout over one of them (pamg::PncSet)
    std::vector<std::array<int64_t, 4>> grids;
    std::mutex grids_mu;  // (uploads on one context from several host threads)
};

void ctx_ref(pamg_ctx* ctx);
void ctx_unref(pamg_ctx* ctx);

struct pamg_plan {
    pamg_ctx* ctx = nullptr;
    int64_t n_own = 0, n_ghost = 0;
    std::vector<int> nbr;
    std::vector<int64_t> recv_off, send_off;  // n_nbr + 1
    int* d_send_idx = nullptr;
    double* d_sendbuf = nullptr;
    // per neighbour: first own index if its send list is one contiguous run (the boundary
    // planes of a slab partition), else -1; all_contig: no pack kernel is needed at all
    std::vector<int64_t> send_run;
    bool all_contig = false;
    // split exchange (pamg_exchange_begin / _end): completion event on the comm stream
    hipEvent_t ev_done = nullptr;
    const void* in_flight = nullptr;  // the vector of the exchange begun and not yet ended
    // identity of the index space the plan describes, the same on every part (pamg_plan_set_tag;
    // 0 = untagged): the in-process world refuses to pair two parts' exchanges whose tags differ
    int64_t tag = 0;
};

struct pamg_vec {
    pamg_ctx* ctx = nullptr;
    int64_t n_own = 0, n_ghost = 0;
    double* d = nullptr;  // n_own + n_ghost (+ padding)
    // several right-hand sides (SPEC §S13; pamg_mvec_create): ncols columns of n_own + n_ghost doubles,
    // column c at d + c * stride (pamg::mc::col_stride); the single-column entry points see column 0
    int ncols = 1;
    int64_t stride = 0;
    bool owns = true;  // false: a column view (pamg_mvec_column) — d belongs to the multi-vector
};

struct pamg_mat {
    pamg_ctx* ctx = nullptr;
    int64_t nrows = 0, ncols = 0, nnz = 0;
    int* d_rowptr = nullptr;
    int* d_col = nullptr;
    uint16_t* d_clo = nullptr;  // 24-bit column stream (TileSet::c24): low 16 bits
    uint8_t* d_chi = nullptr;   //   and high 8 bits of (column - tile base)
    uint8_t* d_vidx = nullptr;  // value dictionary indices, two per byte (TileSet::vd)
    uint8_t* d_rlen = nullptr;  // row lengths, when a tile set uses them (TileSet::rl8)
    uint8_t* d_cidx = nullptr;  // column dictionary indices (TileSet::cd; 4 or 8 bits each)
    uint16_t* d_anc16 = nullptr;  // per-tile anchored dictionaries: row's first column - tile base
    double* d_val = nullptr;
    double* d_diag = nullptr;  // a_ii for square matrices (zero-guess Jacobi), else null
    // point blocks (SPEC §S12; pamg_mat_set_block_diag): bs = 1 none; else row i's bs entries of its node
    // block D_m at d_bdiag[i * bs ..] and of D_m^-1 at d_binv[i * bs ..], beside d_diag
    bool permuted = false;  // uploaded through pamg_mat_upload_perm with a row or column permutation
    int value_bits = 64;    // 32: uploaded through pamg_mat_upload_f32 (SPEC §S15; the values are RN32's)
    int bs = 1;
    double* d_bdiag = nullptr;
    double* d_binv = nullptr;
    const pamg_plan* plan = nullptr;
    pamg::SymDia sym;        // the interior set's symmetric diagonal-class layout (TileSet::sym)
    pamg::TileSet interior;  // rows with own columns only (overlap with the exchange)
    pamg::TileSet boundary;  // rows with >= 1 ghost column
    pamg::EllSet ell;        // the interior set's sliced-ELL layout (TileSet::ell)
    pamg::PncSet pnc;        // the neighbour-coded prolongation layout (TileSet::pnc)
    pamg::RpatSet rpat;      // the pattern-dictionary restriction layout (TileSet::rpat)
    pamg::BsrSet bsr;        // the block-row layout (TileSet::bsr)
    int64_t stream_bytes = 0;  // matrix bytes one apply reads (values, columns, row pointers, tiles)
};

namespace pamg {

// kernels.hip launchers (all asynchronous on `s`).
// (c1 and xold: OP_CHEB only — its c2 is `omega`; square operators only, never the pnc / rpat sets)
void launch_rows(const pamg_mat& A, const TileSet& ts, int op, const double* x, const double* b,
                 const double* xold, double* y, double omega, hipStream_t s, double c1 = 0.0);
// y[i] = x[i] + (c1 (x[i] - xold[i]) + (c2 y[i]) / diag[i]) in place, y holding the residual b - A x: the
// Chebyshev step of the layouts without a native OP_CHEB (k_rows_sym / sym2 / symd), the same seven
// roundings. Rows outside the symmetric set (a part's boundary rows) keep their y.
void launch_cheb_update(const pamg_mat& A, const double* x, const double* xold, double* y, double c1, double c2,
                        hipStream_t s);
void launch_jacobi_zero(int64_t n, const double* b, const double* diag, double omega, double* y,
                        hipStream_t s);
void launch_dense_gemv(int64_t n_rows, int64_t n_cols, int64_t row0, const double* ainv_rm,
                       const double* b, double* y, hipStream_t s);
void launch_pack(int64_t n, const int* idx, const double* x, double* out, hipStream_t s);
void launch_fill(int64_t n, double v, double* y, hipStream_t s);
// S (2 | 3) dependent sweeps in one temporally blocked launch (k_sym_tb; A.sym.tb_ok): stage 0
// is a weighted-Jacobi sweep from in0 into out[0]; stage s > 0 reads stage s-1's result, a
// Jacobi sweep into out[s], the last one the residual b - A t when last_resid.
struct TbArgs {
    int nstages = 0;
    bool last_resid = false;
    const double* in0 = nullptr;
    double* out[3] = {nullptr, nullptr, nullptr};
    const double* b = nullptr;
    double omega = 0.0;
};
constexpr int kTbX = 64, kTbY = 16;  // output tile of a workgroup (grid points in x, y)
void launch_sym_tb(const pamg_mat& A, const TbArgs& ta, hipStream_t s);
// a row operation of the symmetric set on the grid planes [p0, p1) and [p2, p3) only (band = one
// plane; p1 <= p2), one launch
void launch_sym_planes(const pamg_mat& A, int op, int p0, int p1, const double* x, const double* b, double* y,
                       double omega, hipStream_t s, int p2 = 0, int p3 = 0);
// dst[i] = src[perm[i]] (gather), or dst[perm[i]] = src[i] (scatter)
void launch_permute(int64_t n, const int* perm, const double* src, double* dst, bool scatter, hipStream_t s);
void launch_axpby(int64_t n, double a, const double* x, double b, double* y, hipStream_t s);
// Deterministic two-pass dot: writes the local sum to *out (device).
void launch_dot(int64_t n, const double* x, const double* y, double* partials, int nparts,
                double* out, hipStream_t s);
int dot_partials(int64_t n);
// x += alpha p; r -= alpha q; out = r.r (bit-identical to two launch_axpby + launch_dot)
void launch_cg_update(int64_t n, double alpha, const double* p, const double* q, double* x, double* r,
                      double* partials, int np, double* out, hipStream_t s);
// y[k] = the SPEC §S2 generator value of index i0 + k (the bits of pamg_gen_xstar)
void launch_fill_xstar(int64_t n, int64_t i0, uint64_t seed, double* y, hipStream_t s);
// SPEC §S10 step after y = A v: out[0] = v.y, out[1] = (diag v).v (each with launch_dot's bits),
// v <- y / diag. partials holds 2 np doubles, np = dot_partials(n).
void launch_lmax_step(int64_t n, const double* y, const double* diag, double* v, double* partials, int np,
                      double* out, hipStream_t s);
// SPEC §S12, the second pass of a point-block sweep (k_block_update; A carries block data): u holds the
// residual b - A x of the own rows (mode BM_ZERO: b itself) and may be y; w = D_b^-1 u per block, then
// BM_JACOBI y = x + c2 w, BM_ZERO y = 0.0 + c2 w, BM_CHEB y = x + (c1 (x - xold) + c2 w) (null xold:
// zeros), BM_SOLVE y = w. Own rows only.
enum BlockMode : int { BM_JACOBI = 0, BM_ZERO = 1, BM_CHEB = 2, BM_SOLVE = 3 };
void launch_block_update(const pamg_mat& A, int mode, const double* u, const double* x, const double* xold, double* y,
                         double c1, double c2, hipStream_t s);
// SPEC §S12, a whole point-block sweep in one launch on a block-row operator (A.interior.bsr, A.bs ==
// A.bsr.bs, block data attached; bsr_fused below): the lane that holds node m's row sums forms u = b - s
// and w = D_m^-1 u in registers, then BM_JACOBI or BM_CHEB as launch_block_update writes them — the same
// roundings in the same order, so the bits of the two passes. y differs from x and xold.
inline bool bsr_fused(const pamg_mat& A) {
    return A.interior.bsr && A.bs > 1 && A.bs == A.bsr.bs && A.d_binv != nullptr;
}
void launch_bsr_block(const pamg_mat& A, int mode, const double* x, const double* b, const double* xold, double* y,
                      double c1, double c2, hipStream_t s);
// bsr_multi.hip, SPEC §S13: one row operation of a block-row operator (A.interior.bsr) on ncols columns (1 ..
// mc::kMaxCols), column c reading x[c], b[c], xold[c] and writing y[c] with the bits of the single-column
// launch on those four. fuse 0: the RowOp `op` (omega, c1 and xold as launch_rows takes them); fuse 1 / 2:
// the fused block Jacobi / block Chebyshev sweep (bsr_fused(A); omega is c2). The columns are cut into
// launches of 4, then 2 (k_rows_bsr_mc), then 1 (launch_rows / launch_bsr_block). b and xold may be null
// where the operation reads none; an entry of xold may be null (zeros).
void launch_bsr_multi(const pamg_mat& A, int op, int fuse, int ncols, const double* const* x, const double* const* b,
                      const double* const* xold, double* const* y, double omega, double c1, hipStream_t s);
// bsr_multi.hip: OP_SPMV, OP_RESID or OP_PROLONG of an operator in the row-per-lane block-row form
// (A.interior.bsr_r; never square, so no other op reaches it) on ncols columns, cut like launch_bsr_multi's.
void launch_bsr_rows(const pamg_mat& A, int op, int ncols, const double* const* x, const double* const* b,
                     double* const* y, hipStream_t s);
inline bool bsr_any(const pamg_mat& A) { return A.interior.bsr || A.interior.bsr_r; }
// The rows of one set of A, whatever their layout: launch_rows, or k_rows_bsr_r for the row-per-lane form.
inline void launch_set(const pamg_mat& A, const TileSet& ts, int op, const double* x, const double* b,
                       const double* xold, double* y, double omega, hipStream_t s, double c1 = 0.0) {
    if (ts.bsr_r) launch_bsr_rows(A, op, 1, &x, b ? &b : nullptr, &y, s);
    else launch_rows(A, ts, op, x, b, xold, y, omega, s, c1);
}
// SPEC §S12 estimate step after y = A v: out[0] = v.y, out[1] = (D_b v).v (launch_lmax_step's order and
// trees), then v <- D_b^-1 y in a pass of its own. partials holds 2 np doubles.
void launch_lmax_step_block(const pamg_mat& A, const double* y, double* v, double* partials, int np, double* out,
                            hipStream_t s);
// The scalars of a device-resident PCG solve (SPEC §S11; pamg_pcg_resident), one block in device
// memory: rz = (r, z), pq = (p, q), rr = r.r of iteration k; done is set by the first iteration
// whose rr <= rr_max and never cleared during a solve.
struct PcgScalars {
    double rz, pq, alpha, beta, rr, rr_max;
    int k, done;
};
// First half of a §S11 iteration after q = A p: (p, q), alpha = rz / (p, q), x += alpha p,
// r -= alpha q, rr = r.r, k += 1, rr_hist[k] = rr, done = (rr <= rr_max) — launch_dot's and
// launch_cg_update's bits with the scalars read from and written to S. Nothing but the
// partials is touched once S->done is set.
void launch_pcg_half_a(int64_t n, PcgScalars* S, const double* p, const double* q, double* x, double* r,
                       double* partials, int np, double* rr_hist, hipStream_t s);
// Second half after z = M^-1 r: beta = (r, z) / rz, rz = (r, z), p = z + beta p (launch_axpby's
// bits); the same predicate.
void launch_pcg_half_b(int64_t n, PcgScalars* S, const double* r, const double* z, double* p, double* partials,
                       int np, hipStream_t s);

}  // namespace pamg
