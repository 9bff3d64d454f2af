// Internal declarations shared by the translation units of libmlvdb_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mlvdb_hip.h"
#include "../../include/mlvdb_where.h"
#include "../../include/mlvdb_where_each.h"
#include "../../include/mlvdb_where_each_range.h"
#include "../../include/mlvdb_distinct.h"
#include "../../include/mlvdb_grouped.h"
#include "../../include/mlvdb_facet.h"
#include "../../include/mlvdb_stats.h"
#include "../../include/mlvdb_order.h"
#include "../../include/mlvdb_mmr.h"
#include "../../include/mlvdb_like.h"
#include "../../include/mlvdb_maxsim.h"
#include "../../include/mlvdb_mutate.h"
#include "../../include/mlvdb_list.h"
#include "../../include/mlvdb_sparse.h"
#include "../../include/mlvdb_bits.h"
#include "../../include/mlvdb_hybrid.h"
#include "../../include/mlvdb_geo.h"
#include "../../include/mlvdb_score.h"
#include "../../include/mlvdb_examples.h"
#include "../../include/mlvdb_join.h"
#include "../../include/mlvdb_cluster.h"
#include "layout.h"
#include "wave_topk.h"
#include "wave_topk_distinct.h"
#include "examples_plan.h"
#include "cluster_plan.h"

namespace mlvdb {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is bound per device: one bit per device ordinal per call site, so a
// second index on another GPU of the same process (Index(devices=[...])) configures its own copy of the kernel, and
// host threads serving different handles do not race on a plain bool (setting the attribute twice is harmless).
inline hipError_t ensure_dynamic_lds(std::atomic<uint64_t>& done, const void* kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

// The same for one kernel instance (one instantiation, hence one flag per device, per kernel): a launch with `lds` above the
// 48 KiB every kernel may use configures the instance once for `max_bytes`, the most any later launch of it may ask for --
// the attribute holds for the rest of the process.
template <auto Kernel>
inline hipError_t ensure_instance_lds(size_t lds, int max_bytes) {
    static std::atomic<uint64_t> lds_set{0};
    return lds > 48 * 1024 ? ensure_dynamic_lds(lds_set, reinterpret_cast<const void*>(Kernel), max_bytes) : hipSuccess;
}

// f(SPACE) with the space as a compile-time constant: f is a generic lambda, `constexpr int SPACE = decltype(sp)::value` inside it.
template <class F>
inline hipError_t with_space(int32_t space, F&& f) {
    switch (space) {
        case kSpaceL2: return f(std::integral_constant<int, kSpaceL2>{});
        case kSpaceCosine: return f(std::integral_constant<int, kSpaceCosine>{});
        default: return f(std::integral_constant<int, kSpaceIp>{});
    }
}

// f(SPACE, QT): the same with the queries per tile (1, 2, otherwise 4) of a gathered launch as a second constant.
template <class F>
inline hipError_t with_space_qt(int32_t space, int32_t qt, F&& f) {
    return with_space(space, [&](auto sp) {
        switch (qt) {
            case 1: return f(sp, std::integral_constant<int, 1>{});
            case 2: return f(sp, std::integral_constant<int, 2>{});
            default: return f(sp, std::integral_constant<int, 4>{});
        }
    });
}

// The tiles of the exact scan and of the scans that keep its geometry (distinct, maxsim): queries per tile, panels of 16
// rows per wave step, waves per block.  plan_exact picks the tile and sizes the grid by it; with_exact_tile instantiates it.
struct ExactTile {
    int qt, pw, nw;
};
constexpr ExactTile kExactTiles[4] = {{1, 2, 16}, {2, 2, 16}, {4, 4, 8}, {8, 2, 8}};
constexpr int exact_tile_index(int qt) { return qt == 1 ? 0 : qt == 2 ? 1 : qt == 4 ? 2 : 3; }

// f(SPACE, QT, PW, NW): the space and the tile of `qt` queries as compile-time constants.
template <class F>
inline hipError_t with_exact_tile(int32_t space, int32_t qt, F&& f) {
    return with_space(space, [&](auto sp) {
        auto tile = [&](auto i) {
            constexpr ExactTile t = kExactTiles[decltype(i)::value];
            return f(sp, std::integral_constant<int, t.qt>{}, std::integral_constant<int, t.pw>{},
                     std::integral_constant<int, t.nw>{});
        };
        switch (exact_tile_index(qt)) {
            case 0: return tile(std::integral_constant<int, 0>{});
            case 1: return tile(std::integral_constant<int, 1>{});
            case 2: return tile(std::integral_constant<int, 2>{});
            default: return tile(std::integral_constant<int, 3>{});
        }
    });
}

// The most dynamic LDS a kernel that stages fp64 query images by plan_exact's rule may ask for: an image of one query is
// ld x 8 B <= 64 KiB (ld <= 8192: mlvdb_index_create refuses a wider row), a tile of more queries is halved until its
// image fits 64 KiB, and the block merges' lists stay below that (at most 8 x 8 x 64 x 12 B = 48 KiB for the exact scan,
// 16 x 2 x 64 x 20 B = 40 KiB for the distinct scan).
constexpr int kQueryImageMaxLds = 64 * 1024;

// ---------------------------------------------------------------- tuning state (per handle)
// Every knob the kernels' launchers and the pass orchestration consult.  Filled ONCE, by mlvdb_index_create, from the
// MLVDB_* environment variables of that moment (tuning_from_env, api.hip: the library's only getenv loop), and changed
// afterwards only through mlvdb_index_set_tuning(h, "KEY=VAL") -- nothing on the search path reads the environment, so
// host threads that serve different handles (MultiDeviceEngine: one per shard) never race a setenv in glibc.
#define MLVDB_TUNING_FIELDS(X)                                                                                          \
    X(i8, "I8", 1)                     /* 0: bf16 bodies on an index that keeps a bf16 shadow */                       \
    X(no_shadow, "NO_SHADOW", 0)       /* creation: no shadow at all (the filter converts fp32 rows in registers) */   \
    X(shadow_bf16, "SHADOW_BF16", 0)   /* creation: keep the bf16 shadow beside the int8 one (MLVDB_SHADOW=bf16) */    \
    X(i8_pad, "I8_PAD", 1)             /* creation: int8 shadow zero-padded to a multiple of 256 columns for any dim */\
    X(i8_err_l2, "I8_ERR_L2", 1100)    /* l2: largest relative row error (thousandths) of the FEW odd groups an int8 index may hold (30: none; a row quantised to all zeros has 1.0) */ \
    X(i8_err_ip, "I8_ERR_IP", 30)      /* ip: largest index-wide relative row error (thousandths) the int8 bounds are used with */ \
    X(small_batch, "SMALL_BATCH", 1)   /* one query on a small corpus: ONE scan round after an 11,520-row exact prefix (0: the rounds) */ \
    X(small_seed, "SMALL_SEED", 1)     /* 1-2 queries: exact prefix seed */                                             \
    X(small_finish, "SMALL_FINISH", 1) /* 1-2 queries: fused last refine + rescoring + ranking */                       \
    X(small_nq, "SMALL_NQ", 2)                                                                                          \
    X(seed_rows, "SEED_ROWS", 5)       /* dense seeding pass, units of 768 rows */                                      \
    X(round1, "ROUND1", 85)            /* ends of the first / second scan round, units of 768 rows */                   \
    X(round2, "ROUND2", 2048)                                                                                           \
    X(refine_picks, "REFINE_PICKS", 0) /* 0 = 1.5 k, at least 16 */                                                     \
    X(range_l2, "RANGE_L2", 1)         /* range passes: fp16 second-level bound before the exact gather */             \
    X(bigk, "BIGK", 1)                 /* top_k in (64, 1024] on the filter path (0: paged exact scan) */              \
    X(bigk_budget, "BIGK_BUDGET", 400000) /* entries one scan launch of a big-k pass may append (sizes its rounds) */ \
    X(l2_shadow, "L2_SHADOW", 1)       /* fp16 row-major shadow for second-level bounds (built lazily; 0: never) */    \
    X(debug_entries, "DEBUG_ENTRIES", 0)                                                                                \
    X(scan_narrow, "SCAN_NARROW", 1)                                                                                    \
    X(scan_l2c, "SCAN_L2C", 1)         /* l2: the int8 bodies (one query quantisation step per pass, per-row integer offsets: cosine's one-constant test); 0: l2 off the int8 shadow */ \
    X(scan_nqt, "SCAN_NQT", 0)         /* query tiles of the int8 body: 0 = by batch size, else 4 / 8 / 16 */          \
    X(l2_offset_cache, "L2_OFFSET_CACHE", 1) /* l2: keep the offsets plane across passes of the same scale (0: recompute per pass) */ \
    X(where_gather, "WHERE_GATHER", 150) /* per-query filters: gather a program's rows when matches x query tiles x 1000 <= live x this (0: never; tools/where_each_ab.py) */ \
    X(distinct_oversample, "DISTINCT_OVERSAMPLE", 4) /* distinct kNN: the list pass ranks min(1024, max(64, this x k)) rows per query (0: no list pass, every query takes the grouped exact scan; tools/distinct_ab.py) */ \
    X(maxsim_ws_mb, "MAXSIM_WS_MB", 1024) /* late interaction: MiB of the [token, document] workspace one chunk of queries may take (always at least one query; every setting returns the same bytes) */ \
    X(examples_ws_mb, "EXAMPLES_WS_MB", 1024) /* recommend / discover: MiB of the per-(query, row) state one chunk of queries may take for its bags of more than one tile (always at least one query; every setting returns the same bytes) */

struct Tuning {
#define X(field, name, dflt) int field = dflt;
    MLVDB_TUNING_FIELDS(X)
#undef X
};

// ---------------------------------------------------------------- layout kernels (kernels_layout.hip)
// stage: row-major [n, dim] on the device -> panels; rows first_row..first_row+n-1
hipError_t launch_scatter_rows(const float* stage, float* X, int64_t first_row, int64_t n, int32_t dim, int32_t ld,
                               hipStream_t s);
// Xb (bf16 shadow, layout_offset_b) for the same rows, from the fp32 panels
hipError_t launch_shadow_rows(const float* X, void* Xb, int64_t first_row, int64_t n, int32_t ld, hipStream_t s);
// rn[row] = (float)|x_row| for the same rows (fp64 sum of squares); *rel_err_max = max(*rel_err_max, |x - bf16(x)| / |x|)
// as float bits (rounded up); rel_err_max[1] / [2] = the largest / smallest norm of a non-zero row so far, as float bits
// (+inf for a row whose norm is no float): the index's side of the magnitude window below
hipError_t launch_row_norms(const float* X, float* rn, int64_t first_row, int64_t n, int32_t ld, unsigned int* rel_err_max,
                            hipStream_t s);
// stats[1] / [2] (as launch_row_norms keeps them) from the stored norms of rows [0, n): max / min over the live non-zero rows
hipError_t launch_norm_range(const float* rn, int64_t n, unsigned int* stats, hipStream_t s);
// panels -> row-major [n, dim]
hipError_t launch_gather_rows(const float* X, float* out, int64_t first_row, int64_t n, int32_t dim, int32_t ld,
                              hipStream_t s);
// labelled rows -> row-major [n, dim] (labels on the device, all within [0, total))
hipError_t launch_gather_rows_at(const float* X, float* out, const int64_t* labels, int64_t n, int32_t dim, int32_t ld,
                                 hipStream_t s);
// rn[label] = NaN for each valid, live label; *changed += number of rows that changed state
hipError_t launch_tombstone(float* rn, const int64_t* labels, int64_t n, int64_t total, unsigned long long* changed,
                            hipStream_t s);
// compaction: old_of_new[new label] = old label of the live rows (rn == rn) in order, *live = their count;
// block_scratch holds ceil(total / 1024) words
hipError_t launch_compact_map(const float* rn, int64_t total, uint32_t* block_scratch, unsigned long long* live,
                              int32_t* old_of_new, hipStream_t s);
// gather the live rows (fp32 panels, bf16 shadow when Xb != nullptr, norms) into freshly zeroed / NaN-filled buffers
hipError_t launch_compact_rows(const float* X, float* nX, const void* Xb, void* nXb, const float* rn, float* nrn,
                               const int32_t* old_of_new, int64_t live, int32_t ld, hipStream_t s);
// out[i] = mask[i] ? rn[i] : NaN (i < total), NaN up to capacity: a masked-out row looks tombstoned to every scan
hipError_t launch_mask_norms(const float* rn, const uint8_t* mask, float* out, int64_t total, int64_t capacity, hipStream_t s);
// the same for the int8 shadow's row pairs [rows][2]
hipError_t launch_mask_pairs(const float* rp8, const uint8_t* mask, float* out, int64_t total, int64_t capacity, int l2,
                             hipStream_t s);
// Qpad[q][0..ld) = queries[q][0..dim) zero padded; qaux[q] = 1/(|q|+1e-30) (cosine) or |q| (l2, ip)
// qerr (optional): |q^ - bf16 image of q^| per query, rounded up
hipError_t launch_query_prep(const float* queries, int32_t nq, int32_t dim, int32_t ld, int32_t space, float* Qpad,
                             double* qaux, float* qerr, hipStream_t s);

// ---------------------------------------------------------------- exact scan (kernels_exact.hip)
struct ExactPlan {
    int qt;        // queries per block tile (1, 2, 4, 8)
    int nblk;      // blocks along the corpus
    int nqtiles;   // blocks along the query batch
    int threads;   // block size
    size_t lds_bytes;
};
ExactPlan plan_exact(int64_t nrows, int32_t ld, int32_t nq_sel, int32_t k);

struct ExactArgs {
    const float* X;
    const float* rn;
    int64_t row_end;     // rows [0, row_end) are scanned (<= total)
    int32_t ld;
    int32_t space;
    const float* Qpad;   // [nq][ld]
    const double* qaux;  // [nq]
    const int32_t* qsel; // [nq_sel] query indices to process, or nullptr for 0..nq_sel-1
    int32_t nq_sel;
    const int32_t* nq_sel_dev;  // optional: the actual count lives on the device (<= nq_sel); blocks beyond it exit
    int32_t k;
    const double* cursor_d;   // optional paging cursor per query (nullptr = none):
    const int32_t* cursor_l;  //   only rows strictly after (cursor_d, cursor_l) in rank order are admitted
    TopEntry* partial;        // [nq_sel][nblk][k]
};
hipError_t launch_exact_scan(const ExactArgs& a, const ExactPlan& p, hipStream_t s);
// merge partial lists -> final outputs at the original query index
hipError_t launch_exact_merge(const TopEntry* partial, int32_t nq_sel, const int32_t* nq_sel_dev, const int32_t* qsel,
                              int32_t nblk, int32_t k,
                              int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64,
                              hipStream_t s);

// exact fp64 distances of rows 0..m-1 to every query (tombstoned rows: +inf): d64 = [nq][m]
hipError_t launch_prefix_exact(const float* X, const float* rn, const float* Qpad, const double* qaux, int32_t nq, int32_t m,
                               int32_t ld, int32_t space, double* d64, hipStream_t s);
// exact fp64 distances of given pairs: out[q][j] = d(query q, row labels[q][j]) (labels on the device, each < total or < 0 = +inf)
hipError_t launch_pair_distances(const float* X, const float* Qpad, const double* qaux, const int64_t* labels, int32_t nq,
                                 int32_t m, int32_t ld, int32_t space, double* out64, float* out32, hipStream_t s);

// ---------------------------------------------------------------- filter path (kernels_filter.hip)
// The magnitude window of the filter path (DESIGN "Magnitudes").  Its bounds, thresholds and shadows are fp32, and a threshold
// beyond +-1e30 counts as a sentinel; the window is where that arithmetic neither overflows nor loses a normal float:
//   cosine  2^-100 .. 2^120  scores lie in [-1, 1]; above, a norm or a bf16 component nears +inf; below, |x| + 1e-30 is all
//                            regulariser and the shadows' scales turn subnormal
//   ip      2^-63 .. 2^90    scores reach |x| (in units of |q|)
//   l2      2^-63 .. 2^48    scores reach |q|^2 + 2 |q| |x| + |x|^2: 4 x 2^96 = 3.2e29; a squared norm of 2^-126 is still normal
// An index holding a non-zero row whose norm lies outside the window is served by the exact scans (use_filter, api.hip); a
// non-zero query outside it is flagged for the exact fallback by the pass's prep kernel (query_leaves_window,
// kernels_filter.hip).  Zero rows and zero queries are inside.
__host__ __device__ constexpr float norm_window_lo(int space) { return space == kSpaceCosine ? 0x1p-100f : 0x1p-63f; }
__host__ __device__ constexpr float norm_window_hi(int space) {
    return space == kSpaceCosine ? 0x1p120f : (space == kSpaceIp ? 0x1p90f : 0x1p48f);
}
constexpr int kRowErrWords = 4;       // the index's device scalars behind FilterArgs::row_err: {bf16 error, largest norm, smallest norm, -}
constexpr int kFilterQueries = 256;   // queries per filter pass
constexpr int kFilterChunkK = 64;     // columns per Q chunk staged in LDS
constexpr int kCandCap = 8192;        // candidate slots per query (kNN passes; also the most range hits sorted in LDS)
constexpr int kRangeCandCap = 65536;  // candidate slots per query of a range pass: true hits + the bound's band
constexpr int kFilterTile = 768;      // scan ranges start on multiples of it (common multiple of the kernels' 192/128/256-row tiles)
constexpr int kScanMaxGrid = 512;     // most workgroups any scan launch uses
constexpr int kWgCap = 16384;         // append slots per workgroup and launch (assembly scan: split evenly over its waves)

struct CandEntry {
    float u;      // upper bound of the row's score (higher = nearer)
    int32_t row;
};

struct RangeHit {
    double d;
    int32_t l;
    int32_t pad;
};

// What a workgroup of the assembly scan appends to its private buffer; the scatter kernel then moves
// the entries into the per-query lists (the scan itself never waits for a device-scope atomic).
struct WgEntry {
    float u;
    int32_t row;
    uint32_t q;
    uint32_t pad;
};

bool filter_supported(int32_t ld);
size_t filter_qimg_bytes(int32_t ld);   // bf16 query image for one pass of kFilterQueries

// The body that serves every scan of a pass -- what its kernels stream, hence which query image the prep writes and in which
// k-order: the fp32 rows converted in registers, the bf16 shadow, or the int8 shadow.  Decided once per pass (filter_set_body).
enum ScanBody : int32_t { kBodyFp32 = 0, kBodyBf16 = 1, kBodyI8 = 2 };

struct FilterArgs {
    const Tuning* tn;       // host only: the handle's tuning state (never dereferenced on the device)
    ScanBody body;          // set by filter_set_body; the prep and the scan launchers read it instead of X8 / Xb
    const float* X;
    const void* Xb;         // bf16 shadow of X (layout_offset_b) or nullptr: the scan then converts fp32 in registers
    const float* rn;
    int64_t total;
    int32_t ld;
    int32_t ld8;            // columns of the int8 shadow and of the int8 query image: round_up(ld, 256), zero padded (0: no int8 shadow)
    int32_t space;
    const float* Qpad;      // [nq][ld] raw queries of this pass (q0..q0+nq)
    const double* qaux;
    const float* qerr;      // [nq] rounding error of the bf16 query image, |q^ - q^_b| (rounded up)
    const float* row_err;   // device scalars: [0] max over rows of |x - bf16(x)| / |x| (rounded up), [1] the largest row norm
    int32_t nq;             // <= kFilterQueries
    // workspace (per pass)
    void* qimg;             // bf16 image, filter_qimg_bytes
    float* qscale;          // [256] per-query multiplier of the dot product in score units
    float* thr;             // [256] admission threshold (lower bound of the k-th best score)
    float* ke;              // [256] per-query error term of the bound: cosine E1q + 2 slack, ip / l2 E1q + slack (x |x|)
    uint32_t* cnt;          // [256] candidates appended
    uint32_t* overflow;     // [256] nonzero = list overflowed, query must be re-run exactly
    CandEntry* cand;        // [256][cand_cap]
    int32_t cand_cap;       // kCandCap (kNN passes) or kRangeCandCap (range passes: their own, larger lists)
    struct RangeHit* rhits; // range passes: [256][kCandCap] exact hits (fp64 distance, row) found by range_score_flat_kernel
    uint32_t* rhit_cnt;     // [256] exact hit count per query (may exceed kCandCap: the excess is counted, not stored)
    // int8 shadow (cosine, ld % 256 == 0; MLVDB_I8=0 disables): all null / unused otherwise
    const void* X8;         // int8 rows, per-row scale: panels of 16 rows, 64-column groups of 1 KiB (layout_offset_i8)
    const float* rp8;       // [rows][2] cosine {scale/(|x|+1e-30), row error}, l2 / ip {scale, |x|}; NaN = tombstoned
    int64_t rp8_cap;        // l2: rows the rp8 array was allocated for; behind its pairs (float index 2 * rp8_cap) lies the plane of
                            // per-row int32 offsets of the folded l2 admission test (filter_l2_offsets_kernel).  0 = none
    int32_t l2c;            // l2, common query scale for the pass: 0 = off
    float* l2c_out;         // l2: {SQ, KEq, KEr} of the pass, written by filter_l2_offsets_kernel, read by the l2c scan bodies
    uint32_t* l2tag;        // l2: {pass scale the offsets plane behind rp8 holds (float bits), its rows, block counter, -} or nullptr
    float* rmaxq;           // l2: [256] largest raw component of each query of the pass (fused prep -> filter_prep8_l2c_kernel)
    const float* row_err8;  // device scalar: max over rows of |x - scale * x8| / |x| (rounded up)
    void* qimg8;            // int8 query image
    float* sq8;             // [256] scale of the query image
    float* ke8;             // [257] cosine: the query's own int8 error term (row errors are per row); [256] = K = (1 + max eq8)/min sq8
    unsigned int* sqmin;    // two device scalars: bits of the smallest sq8 / of the largest query error of the pass's queries
    struct RangeHit* rs;    // kNN passes: [256][kCandCap] exact (distance, label) of every rescored candidate (filter_rescore_score_kernel -> _rank_kernel)
    WgEntry* wgbuf;         // [kScanMaxGrid][kWgCap] append buffers of one scan launch, one slice per wave
    uint32_t* wgcnt;        // [kScanMaxGrid * 8] entries appended per wave (may exceed the slice: the excess was flagged as overflow)
    int32_t scan_q4;        // host only: a k <= 64 kNN pass (run_filter_pass sets it, nobody else) -- its scans append few entries
                            // per wave and may take the four-buffer int8 body, whose LDS staging area is small (launch_scan_space)
};
// a.body from the shadows the pass was given (X8 attached: int8; else Xb: bf16; else fp32).  The one place that refuses a pass
// without a body: only the int8 one takes an ld that is no multiple of 64 (hipErrorInvalidValue).
hipError_t filter_set_body(FilterArgs& a);
// The per-query state alone (scale, bf16 error term, threshold, empty list) from a.qaux / a.qerr as launch_query_prep left
// them: one block, no image -- the exact range scan reads Qpad.
hipError_t launch_filter_state(const FilterArgs& a, hipStream_t s);
// Everything a pass needs of its queries in one launch (+ the one-block fin or the l2 image kernel of an int8 pass):
// `queries` = the pass's raw [a.nq][dim] rows on the device; writes Qpad / qaux / qerr (= a.Qpad / a.qaux / a.qerr), the
// per-query state and the query image of a.body.
// a.sqmin[] must hold {0x7f7f7f7f, 0} on entry (set when the workspace is allocated, restored by every fin kernel).
hipError_t launch_filter_prep_fused(const FilterArgs& a, const float* queries, int32_t dim, float* Qpad, double* qaux, float* qerr,
                                    hipStream_t s);
// seed thresholds from exact kNN distances of a prefix of the corpus: seed_d64[q][k]
// thr[q] from the k-th smallest of d64[q][0..m) (m <= 3 kSeedRows; fewer than k finite values: thr stays as it is)
hipError_t launch_filter_prefix_thr(const FilterArgs& a, const double* d64, int32_t m, int32_t k, hipStream_t s);
hipError_t launch_filter_seed_thr(const FilterArgs& a, const double* seed_d64, int32_t k, hipStream_t s);
// int8 shadow: (re)build the panels covering rows [row_begin, row_end) (also rp8 and the index-wide error)
hipError_t launch_shadow8_rows(const float* X, const float* rn, void* X8, float* rp8, float* row_err8, int64_t row_begin,
                               int64_t row_end, int32_t ld, int32_t ld8, int32_t space, hipStream_t s);
// l2, once per pass (after the prep kernels): the integer offsets e_j of rows [0, rows) that fold the row term -|x|^2 of the l2
// score into the scan's accumulators (tools/gen_scan_asm.py, l2e): needs a.rp8_cap > 0
hipError_t launch_filter_l2_offsets(const FilterArgs& a, int64_t rows, hipStream_t s);
bool filter_refine_can_fuse(const FilterArgs& a);
bool filter_narrow_ok(const FilterArgs& a);  // the pass's scans run on the narrow kernel (bf16 shadow, <= 64 queries, image resident in LDS)
// What follows every scan launch of a k <= 64 pass: lists -> thresholds, entries below them dropped (cnt[q] = survivors).  An
// int8 pass, whose bounds are loose, first takes its thresholds from the exact scores of the best bounds; that kernel prunes
// too where the lists fit in LDS beside the query (filter_refine_can_fuse), and the update kernel is then not launched.
// forced_cnt >= 0: every list holds that many entries (after the dense pass); -1: cnt[q]
hipError_t launch_filter_refine_update(const FilterArgs& a, int32_t k, int32_t forced_cnt, hipStream_t s);
// batches of <= 8 queries: the last refine + exact rescoring + ranking + output in one launch (needs filter_refine_can_fuse)
hipError_t launch_filter_finish_small(const FilterArgs& a, int32_t k, int32_t q0, int64_t* out_labels, float* out_dist,
                                      int32_t* out_counts, double* out_d64, unsigned long long* rescored, int32_t* qsel,
                                      int32_t* nflag, hipStream_t s);
hipError_t launch_filter_scan(const FilterArgs& a, int64_t row_begin, int64_t row_end, hipStream_t s);
// dense seeding pass over rows [0,row_end), row_end <= kSeedRows: all bounds -> candidate lists -> thresholds (update)
constexpr int kSeedRows = 3840;  // a multiple of every scan tile (128, 192) and <= kCandCap
hipError_t launch_filter_seed_scan(const FilterArgs& a, int64_t row_end, int32_t k, hipStream_t s);
// rescored[0] += rescored pairs; qsel != nullptr: also compacts the overflowed queries of the pass, qsel[0..*nflag) = their
// indices, rescored[1] += *nflag (the device-decided exact fallback that follows reads them)
hipError_t launch_filter_rescore(const FilterArgs& a, int32_t k, int32_t q0, int64_t* out_labels, float* out_dist,
                                 int32_t* out_counts, double* out_d64, unsigned long long* rescored, int32_t* qsel,
                                 int32_t* nflag, hipStream_t s);
// range variant: fixed per-query threshold from the radius, then exact rescoring with emit
hipError_t launch_filter_range_thr(const FilterArgs& a, float radius, hipStream_t s);
// exact candidate generator for range queries (any dim): appends every live row with dist <= radius
// qsel/nsel: restrict to these queries of the pass (nullptr = all a.nq); cnt[q] ends as the exact hit count
hipError_t launch_exact_range_scan(const FilterArgs& a, float radius, const int32_t* qsel, int32_t nsel, hipStream_t s);
hipError_t launch_range_rescore(const FilterArgs& a, float radius, int32_t q0, int64_t capacity, int64_t* out_labels,
                                float* out_dist, int64_t* out_counts, hipStream_t s);
// the ranking alone, over hit arrays another kernel filled (a.rhits / a.rhit_cnt / a.overflow of a.nq <= 256 queries; range
// mode): ranked hits and exact counts at rows q0.. of the outputs; more than kCandCap hits flag the query (overflow = 2)
hipError_t launch_range_rank(const FilterArgs& a, int32_t q0, int64_t capacity, int64_t* out_labels, float* out_dist,
                             int64_t* out_counts, hipStream_t s);
// The dense pass alone: every (query, row) bound of rows [0, rows) -> slot `row` of the query's list (rows a multiple of 128,
// <= a.cand_cap).  launch_filter_seed_scan = this + the first refine / update; big-k passes seed up to 65,280 rows with it.
hipError_t launch_filter_dense_scan(const FilterArgs& a, int64_t rows, hipStream_t s);
// kNN ending on the range kernels (big-k passes): exact fp64 distance of every list entry (range_score_flat_kernel with an
// infinite radius), then the ranking kernel in kNN mode: the k nearest by (distance, label), int32 counts, padded tails,
// optional fp64 distances; more than kCandCap live entries flag the query (overflow = 2) for the paged exact scan.
hipError_t launch_knn_rescore_rank(const FilterArgs& a, int32_t k, int32_t q0, int64_t* out_labels, float* out_dist,
                                   int32_t* out_counts, double* out_d64, unsigned long long* rescored, hipStream_t s);

// ---------------------------------------------------------------- mid bounds + big-k candidate lists (kernels_refine.hip)
constexpr uint32_t kRefinedBit = 0x80000000u;  // CandEntry::row bit 31: u is the entry's mid (fp16) upper bound, not the scan's
constexpr int kBigKMax = 1024;                 // largest top_k of a filter pass (beyond: paged exact scan)
constexpr int kBigSeedRows = 65280;            // dense seeding pass of a big-k pass: 85 x 768 rows (<= kRangeCandCap)
constexpr int kPicksCap = 2048;                // pick-list slots per query (>= kBigKMax + kBigKMax / 4 + 32)

struct MidArgs {
    const _Float16* X16;     // row-major fp16 shadow [rows][ld16]: x ~ s16[row] * h
    const float* s16;        // [rows] scale of the row
    const float* row_err16;  // device scalar: max over rows of |x - s16 h| / |x| (rounded up)
    int32_t ld16;            // round_up(dim, 64): 128 bytes per row and step
    const uint32_t* picks;   // [256][picks_cap] list indices to refine, or nullptr: every entry without a mid bound
    const uint32_t* npicks;  // [256]
    int32_t picks_cap;
};
hipError_t launch_shadow16_rows(const float* X, void* X16, float* s16, float* row_err16, int64_t row_begin, int64_t row_end,
                                int32_t ld, int32_t ld16, hipStream_t s);
hipError_t launch_mid_score(const FilterArgs& a, const MidArgs& m, hipStream_t s);
hipError_t launch_bigk_select(const FilterArgs& a, int32_t want, int32_t forced_cnt, uint32_t* picks, uint32_t* npicks,
                              int32_t picks_cap, hipStream_t s);
// k > 0: threshold from the k-th largest mid lower bound, then prune; k == 0: prune only (range passes)
hipError_t launch_bigk_thr_prune(const FilterArgs& a, const MidArgs& m, int32_t k, int32_t forced_cnt, hipStream_t s);

// ---------------------------------------------------------------- metadata filters (kernels_where.hip)
constexpr int kWhereMaxOps = MLVDB_WHERE_MAX_OPS;
// One op of a validated program as the device reads it: the column resolved to its pointer and type on the host
// (no per-row lookup of the attribute table, no dynamic indexing of kernel arguments)
struct WhereOp {
    int32_t op;
    int32_t type;      // MLVDB_ATTR_* of the column (0 for TRUE / AND / OR / NOT)
    int64_t a, b;      // list ops (mlvdb_list.h): b = the pool's device address, a = the value (HAS) or set offset << 32 | count
                       // (HAS_ANY / HAS_ALL); LEN keeps its bounds in a, b
    const void* col;   // the column's capacity values (int64, float64 bits or list slots)
};
// mask[i] = row i is live and matches, for i < total; *matches += their count
hipError_t launch_where_eval(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, int64_t total,
                             uint8_t* mask, unsigned long long* matches, hipStream_t s);
hipError_t launch_attr_fill(int64_t* col, int64_t value, int64_t first, int64_t n, hipStream_t s);
hipError_t launch_attr_gather(const int64_t* col, int64_t* ncol, const int32_t* old_of_new, int64_t live, hipStream_t s);

// ---------------------------------------------------------------- attribute updates, filtered deletes (kernels_mutate.hip)
// One assignment of a validated mlvdb_attr_update_where call as the device reads it (the column resolved on the host)
struct MutateSet {
    int64_t* col;
    int64_t a;
    int32_t type;  // MLVDB_ATTR_* of the column
    int32_t op;    // MLVDB_SET_*
};
// col[labels[j]] = values[j] for the live rows among n distinct labels in [0, total) (all three on the device);
// *updated += rows written
hipError_t launch_attr_scatter(int64_t* col, const int64_t* labels, const int64_t* values, int64_t n, const float* rn,
                               unsigned long long* updated, hipStream_t s);
// counters[0] += live rows the program matches, counters[1] += those of them for which an ADD of `sets` cannot be stored;
// store: every storable value of those rows is written (all of them, when the counting pass before found counters[1] == 0)
hipError_t launch_attr_update(const WhereOp* prog, int32_t n_ops, const int64_t* set, const MutateSet* sets, int32_t n_sets,
                              const float* rn, int64_t total, bool store, unsigned long long* counters, hipStream_t s);
// ---------------------------------------------------------------- list columns (kernels_list.hip, include/mlvdb_list.h)
constexpr int kListBlock = 256;  // rows per block of the three kernels below: one row per thread
// sums[b] = summed list lengths of rows [b * kListBlock, ...) of the n slots (rn != nullptr: of the live ones among them)
hipError_t launch_list_block_sums(const int64_t* slots, const float* rn, int64_t n, int64_t* sums, hipStream_t s);
// sums[0 .. nblocks) -> their exclusive prefix sums in place, sums[nblocks] = the total
hipError_t launch_list_scan_sums(int64_t* sums, int64_t nblocks, hipStream_t s);
// The lists of the n slots copied back to back into out_pool in row order (offsets from the scanned block sums);
// out_slots[i] (may be `slots` itself) = the row's slot into out_pool, out_offsets[0 .. n] its CSR offsets,
// out_present[i] = 0 for an absent row -- each of the three may be null
hipError_t launch_list_move(const int64_t* slots, int64_t n, const int64_t* sums, const int64_t* pool, int64_t* out_pool,
                            int64_t* out_slots, int64_t* out_offsets, uint8_t* out_present, hipStream_t s);

// ---------------------------------------------------------------- sparse vector columns (kernels_sparse.hip, include/mlvdb_sparse.h)
constexpr int kSparseQT = 8;            // queries per tile
constexpr int kSparseMaxUnion = 1024;   // terms in a tile's union (= MLVDB_SPARSE_MAX_QUERY_TERMS: a query alone always fits)
constexpr int kSparseMaxBlocks = 1024;  // blocks per tile: beyond 16 * kSparseMaxBlocks rows the blocks stride
constexpr int kSparseChunk = 256;       // queries per pass
// queries [q0, q0 + nq) of the pass; their sorted term union U[u0, u0 + nu) and weights W[(u0 + u) * kSparseQT + i]
struct SparseTile {
    int32_t q0, nq, u0, nu;
};
int32_t sparse_scan_blocks(int64_t total, int64_t nq, int32_t k);
// partial[(q * nblk + block) * k ..] = the block's k best (-score, row) of query q over the live rows with a present slot
// (mask != nullptr: whose mask byte is set too)
hipError_t launch_sparse_scan(const int64_t* slots, const int64_t* pool, const float* rn, const uint8_t* mask, int64_t total,
                              const SparseTile* tiles, int32_t ntiles, const int32_t* U, const float* W, int32_t k,
                              int32_t nblk, TopEntry* partial, hipStream_t s);
// ... folded: labels (-1), scores (float and double, -inf) and counts of nq queries
hipError_t launch_sparse_merge(const TopEntry* partial, int32_t nq, int32_t nblk, int32_t k, int64_t* out_labels,
                               float* out_score, int32_t* out_counts, double* out_s64, hipStream_t s);

// ---------------------------------------------------------------- hybrid search (kernels_hybrid.hip, include/mlvdb_hybrid.h)
constexpr int kHybridMaxFetchDense = MLVDB_HYBRID_MAX_FETCH_DENSE;
constexpr int kHybridMaxUnion = kHybridMaxFetchDense + kWave;  // |C| <= fetch_dense + fetch_sparse
// One block per query over its ranked lists (d_lab: [nq][fd], s_lab: [nq][fs], d_cnt / s_cnt valid entries): the union in
// [nq][fd + fs] arrays -- D's entries in order, then S's that D lacks, in order; u_rd / u_rs the member's position in D / S
// (-1: not in it); need_d / need_s the member's label where it lacks a distance / a score, -1 elsewhere; the tails all -1
hipError_t launch_hybrid_union(const int64_t* d_lab, const int32_t* d_cnt, int32_t fd, const int64_t* s_lab,
                               const int32_t* s_cnt, int32_t fs, int32_t nq, int64_t* u_lab, int32_t* u_rd, int32_t* u_rs,
                               int64_t* need_d, int64_t* need_s, int32_t* u_cnt, hipStream_t s);
// The gathered scorer: out[q][p] = the sparse score of (query q, row labels[q][p]) for p < min(cnt[q], m), the bits
// launch_sparse_scan gives the pair; +0.0 for a label < 0 and for a row without a vector.  The queries are a CSR on the
// device (q_off[0 .. nq], <= kSparseMaxUnion terms each); labels < total.
hipError_t launch_sparse_pair_score(const int64_t* slots, const int64_t* pool, int64_t total, const int64_t* q_off,
                                    const int32_t* q_terms, const float* q_weights, const int64_t* labels, const int32_t* cnt,
                                    int32_t nq, int32_t m, double* out, hipStream_t s);
// One block per query: the members' components (the lists' own d_d64 / s_d64 where u_rd / u_rs >= 0, else comp_d / comp_s;
// both null: an RRF call that reports no component), the fused score of `method` and the top k by (fused descending, label
// ascending) to the outputs [nq][k] with padded tails; out_d64 / out_s64 / out_rd / out_rs may be null
hipError_t launch_hybrid_fuse(const int64_t* u_lab, const int32_t* u_rd, const int32_t* u_rs, const int32_t* u_cnt, int32_t nq,
                              int32_t m, const double* d_d64, int32_t fd, const double* s_d64, int32_t fs, const double* comp_d,
                              const double* comp_s, int32_t method, double w_dense, double w_sparse, double rrf_c, int32_t k,
                              int64_t* out_labels, double* out_fused, int32_t* out_counts, double* out_d64, double* out_s64,
                              int32_t* out_rd, int32_t* out_rs, hipStream_t s);

// ---------------------------------------------------------------- binary vector columns (kernels_bits.hip, include/mlvdb_bits.h)
constexpr int kBitsQT = 16;           // queries per tile
constexpr int kBitsMaxBlocks = 512;   // blocks over all tiles of a pass (two per CU): the rows of a tile are strided over its share
constexpr int kBitsChunk = 256;       // queries per pass
int32_t bits_scan_blocks(int64_t total, int64_t nq, int32_t k, int32_t words);
// partial[(q * nblk + block) * k ..] = the block's k best (distance, row) of query q (queries[q * words ..], qpop[q] its
// popcount) over the live rows whose slot holds exactly `words` words (mask != nullptr:
// whose mask byte is set too); launch_exact_merge folds them
hipError_t launch_bits_scan(const int64_t* slots, const int64_t* pool, const float* rn, const uint8_t* mask, int64_t total,
                            const uint64_t* queries, const int32_t* qpop, int32_t nq, int32_t words, int32_t metric, int32_t k,
                            int32_t nblk, TopEntry* partial, hipStream_t s);

// rn[i] = NaN for the rows of mask, and their int8 row pairs (i < i8_rows; rp8 may be null) as tombstone_rp8_kernel does
hipError_t launch_tombstone_mask(const uint8_t* mask, float* rn, float* rp8, int64_t i8_rows, int l2, int64_t total,
                                 hipStream_t s);

// ---------------------------------------------------------------- per-query filters (kernels_where_each.hip)
constexpr int kWhereEachMaxPrograms = MLVDB_WHERE_EACH_MAX_PROGRAMS;
constexpr int kWhereEachMaxOps = MLVDB_WHERE_EACH_MAX_OPS;
static_assert(sizeof(WhereOp) == 32, "the programs of a call are staged in 32 KiB of LDS");
// one block row of the two gathered kernels below (the walk itself: gather_walk.h): <= QT queries of one program (positions
// sel0.. of the call's sorted query list) and that program's label list labels[lab_begin, lab_begin + lab_count)
struct GatherTile {
    int32_t lab_begin, lab_count, sel0, nsel;
};
// bits[i]: bit p = row i is live and matches program p; seg_cnt[p][seg] = program p's matches in segment seg
// (segment = rows [seg * seg_rows, (seg + 1) * seg_rows), seg_rows a multiple of 64)
// (ops reach it with their column's slot in cols[] in the high bits of op.type: where_each_pack)
hipError_t launch_where_each_eval(const WhereOp* prog, const int32_t* prog_off, int32_t n_progs, int32_t n_ops,
                                  const int64_t* set, const int64_t* const* cols, int32_t ncols, const float* rn, int64_t total,
                                  int64_t seg_rows, int32_t nseg, unsigned long long* bits, uint32_t* seg_cnt, hipStream_t s);
// seg_cnt[p][*] -> exclusive prefix sums in place; totals[p] = program p's matches
hipError_t launch_where_each_scan(uint32_t* seg_cnt, int32_t n_progs, int32_t nseg, int64_t* totals, hipStream_t s);
// ascending label lists of the programs in gmask at labels + base[p]
hipError_t launch_where_each_scatter(const unsigned long long* bits, int64_t total, int64_t seg_rows, int32_t nseg,
                                     int32_t n_progs, const uint32_t* seg_off, unsigned long long gmask, const int64_t* base,
                                     int32_t* labels, hipStream_t s);
// mask[i] = bit p of bits[i]
hipError_t launch_where_each_expand(const unsigned long long* bits, int32_t p, int64_t total, uint8_t* mask, hipStream_t s);
// LDS of a gathered top-k kernel (where_gather_kernel, grouped_gather_kernel) for qt queries per tile: the query tile or the
// block merge's lists, whichever is larger (it must stay <= 64 KiB)
size_t where_gather_lds(int32_t qt, int32_t ld);
// partial[(sel * nchunk + chunk) * k + j] for every query of every tile (qt in 1, 2, 4; k <= 64)
hipError_t launch_where_gather(const float* X, const float* Qpad, const double* qaux, const int32_t* labels,
                               const GatherTile* tiles, int32_t ntiles, int32_t ld, int32_t space, int32_t qt, int32_t k,
                               int32_t nchunk, TopEntry* partial, hipStream_t s);
// The gathered range kernel: the tiles' queries (positions q_base .. q_base + 255 of the sorted query list; qt in 1, 2, 4)
// against their programs' label lists; every hit (fp64 distance <= radius) is counted in rhit_cnt[sel - q_base] (exact, whatever the list
// holds) and the first kCandCap of a query stored in rhits[(sel - q_base) * kCandCap ..] -- the input of launch_range_rank.
hipError_t launch_where_gather_range(const float* X, const float* Qpad, const double* qaux, const int32_t* labels,
                                     const GatherTile* tiles, int32_t ntiles, int32_t ld, int32_t space, int32_t qt,
                                     int32_t nchunk, float radius, int32_t q_base, RangeHit* rhits, uint32_t* rhit_cnt,
                                     hipStream_t s);

// ---------------------------------------------------------------- distinct-by-attribute kNN (kernels_distinct.hip)
constexpr int kDistinctMaxList = 1024;  // longest ranked list the pick walks (the list pass's top_k)
struct DistinctArgs {
    const float* X;
    const float* rn;
    const int64_t* group;  // the int64 attribute column: one group code per row, INT64_MIN = in no group
    int64_t total;
    int32_t ld;
    int32_t space;
    const float* Qpad;     // [nq][ld]
    const double* qaux;    // [nq]
    const int32_t* qsel;   // [nq_sel] query indices to process, or nullptr for 0..nq_sel-1
    int32_t nq_sel;
    const int32_t* nq_sel_dev;  // optional: the actual count lives on the device (<= nq_sel); blocks beyond it exit
    int32_t k;
    DistinctEntry* partial;  // [nq_sel][nblk][k]
};
// One wave per query over its ranked list (lab / d64: [nq][L], cnt[q] valid entries): the first entry of each group until
// k_eff are kept.  Complete queries (k_eff kept, or fewer than L valid entries) get their final outputs; the others are
// appended to qsel[*nflag ...] (*nflag zeroed by the caller).
hipError_t launch_distinct_pick(const int64_t* lab, const double* d64, const int32_t* cnt, int32_t nq, int32_t L,
                                const int64_t* group, int32_t k, int32_t k_eff, int32_t* qsel, int32_t* nflag,
                                int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64, int64_t* out_groups,
                                hipStream_t s);
ExactPlan plan_distinct(int64_t nrows, int32_t ld, int32_t nq_sel, int32_t k);
hipError_t launch_distinct_scan(const DistinctArgs& a, const ExactPlan& p, hipStream_t s);
// merge partial lists -> final outputs at the original query index (at most k_eff <= k groups, the rest padded)
hipError_t launch_distinct_merge(const DistinctEntry* partial, int32_t nq_sel, const int32_t* nq_sel_dev, const int32_t* qsel,
                                 int32_t nblk, int32_t k, int32_t k_eff, int64_t* out_labels, float* out_dist,
                                 int32_t* out_counts, double* out_d64, int64_t* out_groups, hipStream_t s);

// ---------------------------------------------------------------- scored kNN (kernels_score.hip, include/mlvdb_score.h)
constexpr int kScoreMaxOps = MLVDB_SCORE_MAX_OPS;
constexpr int kScoreMaxConds = MLVDB_SCORE_MAX_CONDS;
constexpr int kScoreMaxOperands = MLVDB_SCORE_MAX_OPS / 2;  // n pushes need n - 1 binary ops: at most 16 pushes in 32 ops
// One op of a validated score program as the device reads it
struct ScoreOp {
    int32_t op;
    int32_t slot;  // ATTR: the operand's index in ScoreProgram::operands; MATCH: the cond's index
    int64_t a;     // CONST: the double's bits
};
// One distinct (column, default) pair the ATTR ops of a program push, the column resolved on the host
struct ScoreOperand {
    const int64_t* col;
    int64_t dflt;  // the bits of the double an absent value pushes
    int32_t type;  // MLVDB_ATTR_INT64 or MLVDB_ATTR_FLOAT64
    int32_t pad;
};
// A validated call's programs, one fixed block: uploaded as it stands and staged in LDS once per block of the scan.  The
// cond programs are concatenated (cond c: cond_ops[cond_off[c] .. cond_off[c + 1])), their set ranges rebased onto one
// concatenated set table that stays in HBM (ScoredArgs::set), as the per-query filters pack theirs.
struct ScoreProgram {
    ScoreOp ops[kScoreMaxOps];
    ScoreOperand operands[kScoreMaxOperands];
    int32_t cond_off[kScoreMaxConds + 1];
    int32_t n_ops, n_operands, n_conds;
    WhereOp cond_ops[kWhereMaxOps];
};
static_assert(sizeof(ScoreProgram) % 16 == 0, "staged in LDS behind the query tile, 16-byte words");
struct ScoredArgs {
    const float* X;
    const float* rn;
    int64_t total;
    int32_t ld;
    int32_t space;
    const float* Qpad;   // [nq][ld]
    const double* qaux;  // [nq]
    int32_t nq;
    int32_t k;
    const ScoreProgram* prog;
    const int64_t* set;  // the conds' concatenated set table (may be null without one)
    TopEntry* partial;   // [nq][nblk][k]: (score, row), the input of launch_exact_merge
};
// the exact scan's geometry; the LDS also holds the programs and, per wave, a panel's operand values
ExactPlan plan_scored(int64_t nrows, int32_t ld, int32_t nq, int32_t k);
hipError_t launch_scored_scan(const ScoredArgs& a, const ExactPlan& p, hipStream_t s);

// ---------------------------------------------------------------- grouped kNN (kernels_grouped.hip)
constexpr int kGroupedMaxSize = MLVDB_GROUPED_MAX_SIZE;  // rows returned per group: one WaveTopK
constexpr int kGroupedBlocks = 2048;   // blocks the chunk rule aims at for one gathered launch chain
constexpr int kGroupedMinChunk = 256;  // fewest rows of a list chunk that is not the whole list (a multiple of 64)
// Rows per chunk of a member list (mirrored in tests/grouped_helpers.py): `work` = the rows all tiles of
// the chunk of queries would gather unsplit (sum over tiles of their list's length).  The rows are cut so that about
// kGroupedBlocks blocks share the work evenly, whatever the lists' lengths: a huge group (a bool column) spreads over the
// machine, a group of a hundred rows stays one block.
__host__ __device__ inline int64_t grouped_chunk_rows(int64_t work) {
    const int64_t even = ((work + kGroupedBlocks - 1) / kGroupedBlocks + 63) / 64 * 64;
    return even > kGroupedMinChunk ? even : kGroupedMinChunk;
}
// one (query, rank) pair that picked a group: the query's index in the chunk (its row of Qpad / qaux) and where the pair's
// partial lists lie (nch lists of group_size entries from list part0 on); sorted by group
struct GroupedPair {
    int32_t q, part0, nch, pad;
};
// one block of grouped_gather_kernel: <= QT pairs pair0.. of one group against labels[lab_begin, lab_begin + lab_count), one
// chunk of the group's list; part0: pair0's partial list of this chunk (pair t: part0 + t * nch)
struct GroupedTile {
    int32_t lab_begin, lab_count, pair0, npairs, part0, nch;
};
// counts[slot] += live rows (finite rn) whose value of `col` is the key of `slot`; keys: `slots` (a power of two) codes placed
// by facet_hash with linear probing, INT64_MIN = empty, at most half full
hipError_t launch_grouped_count(const float* rn, const int64_t* col, int64_t total, const long long* keys, uint64_t slots,
                                uint32_t* counts, hipStream_t s);
// labels[cursor[slot]++] = row for the same rows; cursor enters as the exclusive prefix sums of the counts
hipError_t launch_grouped_fill(const float* rn, const int64_t* col, int64_t total, const long long* keys, uint64_t slots,
                               uint32_t* cursor, int32_t* labels, hipStream_t s);
// the tiles (all of npairs <= qt, qt in 1, 2, 4; where_gather_lds(qt, ld) <= 64 KiB) -> partial lists of gsz entries
hipError_t launch_grouped_gather(const float* X, const float* Qpad, const double* qaux, const int32_t* labels,
                                 const GroupedTile* tiles, int32_t ntiles, const GroupedPair* pairs, int32_t ld, int32_t space,
                                 int32_t qt, int32_t gsz, TopEntry* partial, hipStream_t s);
// slot s of [0, nslots): pair pair_of_slot[s]'s partial lists folded into out_*[s * gsz ..] and out_gcnt[s]; -1: padding
hipError_t launch_grouped_merge(const TopEntry* partial, const GroupedPair* pairs, const int32_t* pair_of_slot, int32_t nslots,
                                int32_t gsz, int64_t* out_labels, float* out_dist, double* out_d64, int32_t* out_gcnt,
                                hipStream_t s);

// ---------------------------------------------------------------- diversified kNN (kernels_mmr.hip)
constexpr int kMmrMaxFetch = MLVDB_MMR_MAX_FETCH;  // longest candidate list the selection walks (the plain search's top_k)
// LDS of one block of the select kernel: the picked row as fp64 [ld] + dq / mind / picked flag per candidate (<= 64 KiB)
size_t mmr_select_lds(int32_t ld, int32_t fetch_k);
// One block per query over its ranked list (l_lab / l_dist / l_d64: [nq][fetch_k], l_cnt[q] valid entries): the greedy
// selection of mlvdb_mmr.h, outputs [nq][k] in pick order with padded tails, out_counts[q] = min(k, l_cnt[q]).
hipError_t launch_mmr_select(const float* X, int32_t dim, int32_t ld, int32_t space, const int64_t* l_lab, const float* l_dist,
                             const double* l_d64, const int32_t* l_cnt, int32_t nq, int32_t fetch_k, int32_t k, double lambda,
                             double one_minus_lambda, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                             double* out_d64, int32_t* out_rank, double* out_obj, hipStream_t s);

// ---------------------------------------------------------------- search by stored examples (kernels_like.hip)
constexpr int kLikeMaxFetch = MLVDB_LIKE_MAX_FETCH;        // longest ranked list the strip walks (k + the most examples)
constexpr int kLikeMaxExamples = MLVDB_LIKE_MAX_EXAMPLES;  // examples of one query: one per lane of the strip's wavefront
// One block per query: out[q] ([nq, dim] dense fp32) = (float)(base[q] + sum_j t_j x_j) over the examples
// ex_offsets[q] .. ex_offsets[q + 1] - 1 (<= kLikeMaxExamples, labels inside [0, total): the entry point checked both) in the
// order given, by the rule of mlvdb_like.h; base may be null.
hipError_t launch_like_query(const float* X, int32_t dim, int32_t ld, int32_t space, const int64_t* ex_labels,
                             const double* ex_weights, const int64_t* ex_offsets, const float* base, int32_t nq, float* out,
                             hipStream_t s);
// One wavefront per query over its ranked list (l_lab / l_dist / l_d64: [nq][fetch], l_cnt[q] valid entries): the entries
// whose label is no example of the query (exclude == 0: every entry), order kept, the first k to the outputs [nq][k] with
// padded tails, out_counts[q] their number.
hipError_t launch_like_strip(const int64_t* l_lab, const float* l_dist, const double* l_d64, const int32_t* l_cnt, int32_t nq,
                             int32_t fetch, const int64_t* ex_labels, const int64_t* ex_offsets, int32_t exclude, int32_t k,
                             int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64, hipStream_t s);

// ---------------------------------------------------------------- similarity join (kernels_join.hip, include/mlvdb_join.h)
constexpr int kJoinWave = 256;  // left rows of one wave: one pass of the range chain (kFilterQueries)
// One block per left row: out ([n, dim] dense fp32) = the stored values of rows labels[0 .. n) (inside [0, total): the entry
// point checked it).
hipError_t launch_join_gather_queries(const float* X, const int64_t* labels, int32_t n, int32_t dim, int32_t ld, float* out,
                                      hipStream_t s);
// rn[lo .. hi) = NaN and, with rp8 (the masked row pairs; may be null), their pairs "not a row" (l2: the x slot stays).
hipError_t launch_join_mask_advance(float* rn, float* rp8, int l2, int64_t lo, int64_t hi, hipStream_t s);
// One block per left row over its ranked list (l_lab / l_dist: [n][cap_eff], l_cnt[i] the exact inner count): the entries with
// label == left[i] (OTHERS) or <= left[i] (LATER) dropped, the first `capacity` survivors to out_labels / out_dist
// ([n][capacity]), out_kept[i] their number, out_count[i] the exact number of partners, out_flag[i] = 1 where a truncated
// list cannot give it (the row wants a wave of its own).  self64 (may be null when no list is truncated): the distance of
// each row to itself; rn: the call's masked norms.
hipError_t launch_join_strip(const int64_t* l_lab, const float* l_dist, const int64_t* l_cnt, int64_t cap_eff,
                             const int64_t* left, int32_t n, int32_t mode, const double* self64, float radius, const float* rn,
                             int64_t capacity, int64_t* out_labels, float* out_dist, int64_t* out_count, int32_t* out_kept,
                             int32_t* out_flag, hipStream_t s);
// One block per left row (n <= kJoinWave): its kept entries to p_lab / p_dist at base + the kept counts of the unflagged rows
// before it.
hipError_t launch_join_pack(const int64_t* d_lab, const float* d_dist, const int32_t* kept, const int32_t* flag, int32_t n,
                            int64_t capacity, int64_t base, int64_t* p_lab, float* p_dist, hipStream_t s);

// ---------------------------------------------------------------- recommend / discover (kernels_examples.hip, include/mlvdb_examples.h)
constexpr int64_t kExamplesChunk = 1024;           // queries of one chunk
constexpr int64_t kExamplesChunkExamples = 16384;  // ... and their examples (always at least one query)
// The per-(query, row) state a bag of several tiles carries from one launch to the next: BEST (p, n), DISCOVER (d_target,
// pairs missed so far -- a small integer, exact), CONTEXT (s, unused)
struct __attribute__((aligned(16))) ExamplesState {
    double a, b;
};
struct ExamplesArgs {
    const float* X;
    const float* rn;
    int64_t total;
    int32_t ld;
    int32_t space;
    const float* Qpad;          // [examples of the chunk][ld]
    const double* qaux;         // [examples of the chunk]
    const ExamplesTile* tiles;  // the tiles of THIS launch, one per block row
    int32_t ntiles;
    int32_t k;
    const int32_t* excl;   // the chunk's exclusion table (ExamplesTile::excl_off)
    ExamplesState* state;  // [state slots][total]
    double* held;          // [state slots][total]: tiles of one example only -- the POS distance of the pair a tile boundary splits
    TopEntry* partial;     // [queries of the chunk][partial_stride][k]: (value, row, tier); a query's last tile writes its lists
    int32_t partial_stride;
};
// raw[j] >= 0: row raw[j] of `vectors` ([., dim], uploaded); else the stored row labels[j] -> out[j][0 .. dim)
hipError_t launch_examples_stage(const float* X, int32_t dim, int32_t ld, const int64_t* labels, const int32_t* raw,
                                 const float* vectors, int32_t n, float* out, hipStream_t s);
// plan_exact's geometry for tiles of qt examples, ntiles block rows
ExactPlan plan_examples(int64_t nrows, int32_t ld, int32_t qt, int32_t ntiles);
// the tile width for bags of at most `most` examples: the smallest of 1, 2, 4, 8 that holds them (8 beyond), halved like
// plan_exact's until the fp64 image fits
int32_t examples_tile_width(int32_t ld, int32_t most);
hipError_t launch_examples_scan(const ExamplesArgs& a, const ExactPlan& p, hipStream_t s);
// nblk_of[q]: the blocks that wrote query q's partial lists
hipError_t launch_examples_merge(const TopEntry* partial, int32_t nq, const int32_t* nblk_of, int32_t stride, int32_t k,
                                 int64_t* out_labels, int32_t* out_tier, double* out_value, int32_t* out_counts, hipStream_t s);

// ---------------------------------------------------------------- late-interaction search (kernels_maxsim.hip)
constexpr int kMaxsimMaxTokens = MLVDB_MAXSIM_MAX_TOKENS;
constexpr int kMaxsimMaxGroups = MLVDB_MAXSIM_MAX_GROUPS;
constexpr int kMaxsimChunkTokens = 4096;  // most tokens of one chunk of queries, whatever the workspace budget allows
struct MaxsimArgs {
    const float* X;
    const int32_t* row_doc;    // [total] dense id of the row's document, -1 = not counted
    int64_t total;
    int32_t ld;
    int32_t space;
    const float* Qpad;         // [ntok][ld] the chunk's tokens, prepared as queries
    const double* qaux;        // [ntok]
    int32_t ntok;
    int32_t ndocs;             // G
    unsigned long long* best;  // [ntok][G] order keys of the best distances, preset to all ones
};
// row_doc[i] for i < total: keys / dense = the host-built code table (group_table.h) and the dense id of every slot
hipError_t launch_maxsim_slot(const float* rn, const int64_t* col, int64_t total, const long long* keys, uint64_t slots,
                              const int32_t* dense, int32_t* row_doc, hipStream_t s);
// the exact scan's geometry (p = plan_exact(total, ld, ntok, k)) with the [token, document] minimum as its sink
hipError_t launch_maxsim_scan(const MaxsimArgs& a, const ExactPlan& p, hipStream_t s);
// blocks per query of the rank kernel
int32_t maxsim_rank_blocks(int32_t ndocs);
// query q of nq <= 65535: tokens tok_off[q] .. tok_off[q + 1] of `best`; partial[(q * nblk + block) * k ..] = the block's k
// smallest (score, dense id), the input of launch_exact_merge
hipError_t launch_maxsim_rank(const unsigned long long* best, const int32_t* tok_off, int32_t nq, int32_t ndocs, int32_t k,
                              int32_t nblk, TopEntry* partial, hipStream_t s);

// ---------------------------------------------------------------- facet counts and histograms (kernels_facet.hip)
constexpr int kFacetLdsSlots = 4096;  // per-block table of the value kernel: int64 key + uint32 count = 48 KiB, three blocks per CU
constexpr int kFacetLdsProbes = 8;    // linear probes in the block table; a key that finds no slot goes to the global table
constexpr int kFacetPeelRounds = 8;   // wave peel: at most this many leading values get one add for all their lanes
constexpr int kFacetMaxEdges = MLVDB_FACET_MAX_EDGES;
// The one hash of both tables (mirrored in tests/facet_helpers.py): slot = facet_hash(v) & (slots - 1)
__host__ __device__ inline uint64_t facet_hash(int64_t v) {
    const uint64_t x = (uint64_t)v * 0x9E3779B97F4A7C15ull;
    return x ^ (x >> 32);
}
// words of the counters a facet call zeroes before its launch
enum { kFacetMatched = 0, kFacetAbsent = 1, kFacetDistinct = 2, kFacetOverflow = 3, kFacetCursor = 4, kFacetCounters = 8 };
// The global table of one value-facet call: `mask + 1` slots (a power of two >= 2 max_values), keys INT64_MIN = empty
struct FacetTable {
    unsigned long long* keys;
    unsigned long long* counts;
    uint64_t mask;
    unsigned long long max_values;
    unsigned long long* ctr;  // [kFacetCounters]
};
// One pass over rn, the program's columns and `col` (int64): every live matching row counted under its value in `t`,
// ctr[matched / absent / distinct / overflow] updated.  n_ops == 0: no program, every live row matches.
hipError_t launch_facet_values(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* col,
                               int64_t total, const FacetTable& t, hipStream_t s);
// the non-empty slots of `t` packed through ctr[kFacetCursor] into out_keys / out_counts (max_values entries each), in no order
// ... of a list column: every value of a hit row's list counts once; kFacetAbsent counts the hits with no value at all
hipError_t launch_facet_list_values(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* col,
                                    const int64_t* pool, int64_t total, const FacetTable& t, hipStream_t s);
hipError_t launch_facet_collect(const FacetTable& t, long long* out_keys, unsigned long long* out_counts, hipStream_t s);
// The same pass into bins[n_edges + 1] (zeroed by the caller): bin = number of edges <= value; `edges` on the device, int64 or
// the bits of doubles by `type` (MLVDB_ATTR_*)
hipError_t launch_facet_bins(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* col,
                             int32_t type, int64_t total, const int64_t* edges, int32_t n_edges, unsigned long long* bins,
                             unsigned long long* ctr, hipStream_t s);

// ---------------------------------------------------------------- attribute statistics (kernels_stats.hip)
// per-block table: 48 B per slot of an int64 column (48 KiB, three blocks per CU), 32 B of a float64 one
constexpr int kStatsLdsSlots = 1024;
constexpr int kStatsLdsSlotsOne = 64;  // ... of an ungrouped call: one key
constexpr int kStatsRecord = 8;       // words of a packed group: key, rows, count, min, max, sum hi, sum lo, 0
// Order-preserving uint64 images: integer order of the images = integer order of int64 values / IEEE totalOrder of doubles
// (-0.0 below +0.0).  Image 0 is INT64_MIN / a NaN: never a present value.
__host__ __device__ inline uint64_t stats_image_i64(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
__host__ __device__ inline uint64_t stats_image_f64(uint64_t bits) { return bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull); }
__host__ __device__ inline uint64_t stats_bits_f64(uint64_t image) {  // the image back to the double's bits
    return image ^ ((image >> 63) ? 0x8000000000000000ull : ~0ull);
}
// E = floor(log2 m) of the group's largest finite magnitude m from the bits of its min and max (include/mlvdb_stats.h);
// false when the group's fixed-point sum is 0 by definition: it holds an infinity, or m == 0
__host__ __device__ inline bool stats_exponent(uint64_t min_bits, uint64_t max_bits, int* E) {
    const uint64_t a = min_bits & 0x7FFFFFFFFFFFFFFFull, b = max_bits & 0x7FFFFFFFFFFFFFFFull, m = a > b ? a : b;
    if (m >= 0x7FF0000000000000ull || m == 0) return false;
    int top = 51;  // a subnormal: the place of its leading bit
    while (!(m >> 52) && !((m >> top) & 1)) --top;
    *E = (m >> 52) ? (int)(m >> 52) - 1023 : top - 1074;
    return true;
}
// The global table of one call: `mask + 1` slots (a power of two >= 2 max_groups), keys INT64_MIN = empty, placed by
// facet_hash with linear probing; min / max as images (min starts at ~0, max at 0), sum hi:lo a 128-bit two's complement
struct StatsTable {
    unsigned long long *keys, *mn, *rows, *count, *mx, *hi, *lo;
    uint64_t mask;
    unsigned long long max_groups;
    unsigned long long* ctr;  // [kFacetCounters], the words of a facet call
};
// Pass 1 over rn, the program's columns, `by` (int64; nullptr: one group under key 0) and `col` (int64, or float64 by
// `f64`): every live matching row with a value of `by` counted under it in `t` -- rows, count, min, max and, of an int64
// column, the sum; ctr[matched / absent (no value of by) / distinct / overflow] updated.  n_ops == 0: no program.
hipError_t launch_stats_pass1(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* by,
                              const int64_t* col, bool f64, int64_t total, const StatsTable& t, hipStream_t s);
// Pass 2 of a float64 column over the final table of pass 1: the fixed-point terms of every group's sum added to hi:lo.
// Does nothing when pass 1 overflowed.
hipError_t launch_stats_pass2(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* by,
                              const int64_t* col, int64_t total, const StatsTable& t, hipStream_t s);
// the non-empty slots of `t` packed through ctr[kFacetCursor] into out[max_groups][kStatsRecord], in no order
hipError_t launch_stats_collect(const StatsTable& t, unsigned long long* out, hipStream_t s);

// ---------------------------------------------------------------- ordered metadata queries (kernels_order.hip)
// A row's composite key: its value mapped to an order-preserving uint64 (complemented for a descending call) above its
// 32-bit label -- 96 bits, unique per row.  The N-th smallest composite is found by most-significant-digit histogram passes.
constexpr int kOrderMaxRows = MLVDB_ORDER_MAX_ROWS;
constexpr int kOrderDigitBits = 11;                   // 2048 bins: 8 KiB of LDS per block, 16 KiB per pass in HBM
constexpr int kOrderBins = 1 << kOrderDigitBits;
constexpr int kOrderPasses = 9;                       // 8 digits of 11 bits and one of 8: 96 bits
constexpr int kOrderMaxBlocks = 1024;                 // blocks of a pass over the index (each flushes <= kOrderBins adds)
// low bits of the composite below the digit of pass p (the last digit is the 8 bits left over)
__host__ __device__ inline int order_shift(int pass) { return pass < 8 ? 85 - kOrderDigitBits * pass : 0; }
// What the kernels of one call hand to each other and, at the end, to the host (zeroed by the call before its first launch)
struct OrderState {
    unsigned long long matched, absent;  // first pass
    unsigned long long below;            // candidates whose composite lies below the selected bucket
    unsigned long long want;             // N = min(offset + limit, candidates): the rank that is looked for, 1-based
    unsigned long long key;              // the selected bucket: the digits fixed so far, in place, the bits below `low_bits`
    uint32_t label;                      //   of key:label zero
    uint32_t low_bits;                   // bits of the composite not fixed yet
    uint32_t done;                       // the bucket and everything below it fit one block: no further digit pass runs
    uint32_t n_collect;                  // ... that many rows: what the collect pass must find (0: nothing to return)
    uint32_t cursor;                     // rows the collect pass met (may exceed kOrderMaxRows: the excess is not stored)
    uint32_t overflow;                   // ... and then this is set
    uint32_t passes;                     // digit passes that ran
    uint32_t n_out;                      // rows written to the output buffers
};
// One digit pass: the candidates (live rows -- of `mask` when given, else with a finite norm -- with a present value) inside the
// selected bucket counted by their digit into hist[kOrderBins]; pass 0 also counts matched / absent.  Nothing runs once
// st->done is set.  Then the one-block scan: the digit that holds rank st->want, st updated.
// type == MLVDB_ATTR_GEO (mlvdb_geo_nearest): the key is hav of the row's point from the packed point `centre`, ascending
hipError_t launch_order_hist(const uint8_t* mask, const float* rn, const int64_t* col, int32_t type, int32_t descending,
                             int64_t centre, int64_t total, int32_t pass, unsigned long long* hist, OrderState* st,
                             hipStream_t s);
hipError_t launch_order_scan(const unsigned long long* hist, int32_t pass, int64_t offset, int64_t limit, OrderState* st,
                             hipStream_t s);
// The candidates at or below the selected bucket -> keys / labels[kOrderMaxRows] through st->cursor
hipError_t launch_order_collect(const uint8_t* mask, const float* rn, const int64_t* col, int32_t type, int32_t descending,
                                int64_t centre, int64_t total, OrderState* st, unsigned long long* keys, uint32_t* labels,
                                hipStream_t s);
// One workgroup sorts them and writes ranks [offset, st->want) to out_labels / out_values[kOrderMaxRows] (values: col[label])
// and, of a geo call, their distances in metres to out_dist[kOrderMaxRows] (otherwise not touched)
hipError_t launch_order_sort(const unsigned long long* keys, const uint32_t* labels, const int64_t* col, int32_t type,
                             int64_t centre, int64_t total, int64_t offset, OrderState* st, int64_t* out_labels,
                             int64_t* out_values, double* out_dist, hipStream_t s);

// ---------------------------------------------------------------- clustering (kernels_cluster.hip, include/mlvdb_cluster.h)
constexpr int32_t kClusterNoCandidate = -2;  // assignment of a row that is no candidate (-1: an unassigned candidate)
enum : uint32_t { kClusterFirst = 1, kClusterLast = 2 };
// One launch of the assignment scan: the tile of centroids [first, min(m, first + qt)) of the prepared batch.
struct AssignArgs {
    const float* X;
    const float* rn;
    int64_t total;
    int32_t ld;
    int32_t space;
    const float* Qpad;   // [m][ld]
    const double* qaux;  // [m]
    int32_t m, first;
    uint32_t flags;      // (launch_assign_scan sets them from `first`)
    double* best;        // [total]: the best distance so far / of the assignment
    int32_t* sidx;       // [total]: its centroid, between the tiles
    int32_t* assign;     // [total]: the previous assignment in, this one out (kClusterNoCandidate: not written)
    unsigned long long* moved;  // += the candidates whose centroid changed
};
// plan_exact's geometry for one tile of qt centroids
ExactPlan plan_assign(int64_t nrows, int32_t ld, int32_t qt);
hipError_t launch_assign_scan(const AssignArgs& a, const ExactPlan& p, hipStream_t s);
// w[row] = 1 / (sqrt(nx) + 1e-30) for rows [0, total), nx in accumulate_rows' order
hipError_t launch_cluster_weights(const float* X, int32_t ld, int64_t total, double* w, hipStream_t s);
// The members of every cluster in ascending label order: members[base[c] .. base[c] + counts[c]); hist holds
// cluster_list_blocks(total) x m words; *matched += the candidates (assign != kClusterNoCandidate)
hipError_t launch_cluster_list(const int32_t* assign, int64_t total, int32_t m, int32_t* hist, int64_t* counts, int64_t* base,
                               int32_t* members, unsigned long long* matched, hipStream_t s);
// The blocked sums over the segment table (cluster_segments; partial: [nsegs][ld + 1]): cost[c], and with `means` the new
// centroid rows cent[c][0 .. dim) of the clusters that have members
hipError_t launch_cluster_sums(const float* X, int32_t dim, int32_t ld, bool cosine, const ClusterSegment* segs, int32_t nsegs,
                               const int32_t* seg_first, const int32_t* members, const double* w, const double* best,
                               const int64_t* counts, int32_t m, bool means, double* partial, float* cent, double* cost,
                               hipStream_t s);
// column[row] = assign[row] (INT64_MIN for -1) for every candidate row
hipError_t launch_cluster_write(const int32_t* assign, int64_t total, int64_t* column, hipStream_t s);

}  // namespace mlvdb
