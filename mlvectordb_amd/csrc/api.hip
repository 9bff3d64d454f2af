// C ABI of libmlvdb_hip.so (declared in include/mlvdb_hip.h): index handle, HBM management,
// and the orchestration of the scan kernels.  Nothing here touches the CPU for arithmetic:
// if no HIP device is usable every entry point fails with MLVDB_ERR_NO_DEVICE.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>

#include "device_memory.h"
#include "geo_common.h"
#include "internal.h"

using namespace mlvdb;

namespace {

thread_local std::string g_error;

}  // namespace

// The blocks sized by the row capacity: they are allocated, regrown and compacted together (reserve_rows, mlvdb_index_compact).
struct RowStore {
    DevBuf X, rn, Xb, col[MLVDB_MAX_ATTRS];
};

// Every device or pinned block of an index is a DevBuf / PinBuf member (device_memory.h) and goes with the handle.  The raw
// X / Xb / rn / attr_col[] / list_pool[] / host_flags pointers are views of such members for the kernels' arguments, set
// where the owner is committed; with_row_mask points rn at the masked copy for the length of a call.
struct mlvdb_index {
    int device = 0;
    int32_t dim = 0, ld = 0, space = 0;
    int32_t ld8 = 0;      // width of the int8 shadow: round_up(ld, 256), zero padded; 0 = this index keeps none
    int32_t strategy = MLVDB_STRATEGY_AUTO;
    Tuning tn;            // tuning state: from the environment at creation, mlvdb_index_set_tuning afterwards; never getenv later
    bool profiling = false;
    float* X = nullptr;   // panels, capacity * ld floats
    void* Xb = nullptr;   // bf16 shadow of X for the filter scan (capacity * ld bf16), or nullptr
    bool shadow = false;  // keep the bf16 shadow (decided at creation: dim % 64 == 0 and not disabled)
    bool i8_only = false; // ld8 > 0 (default; SHADOW_BF16 at creation keeps both): no bf16 shadow, the
                          // int8 one serves every pass (1.25x instead of 1.75x the corpus in HBM); only an index whose rows
                          // quantise too badly for int8 bounds (l2 / ip, rmax8 > 0.03) converts the fp32 rows in registers
    float* rn = nullptr;  // row norms, NaN = tombstoned / not a row
    RowStore rows;        // owns X, Xb, rn and attr_col[]
    int64_t capacity = 0, total = 0, deleted = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;  // mlvdb_index_get_rows_at: a hit-enrichment gather must not queue behind the next scan
    DevBuf gather_out, gather_lab;     // its private buffers (a search may be running on `stream` from another host thread)
    std::mutex aux_mutex;              // ... shared by the two entry points that use it (get_rows_at, pair_distances): a consumer
                                       // thread enriching wave i and a caller scoring pairs must not swap the buffers under each other
    // workspaces (grow only)
    DevBuf stage, qpad, qaux, partial, qsel, seed_lab, seed_dist, seed_cnt, seed_d64;
    DevBuf cand_range, rhits, rhit_cnt;  // range passes: larger candidate lists, exact hits, hit counts
    DevBuf row_mask, rn_masked;  // filtered search
    DevBuf qerr, rowerr;         // rounding errors of the bf16 images: per query / maximum over the rows (device scalars: kRowErrWords)
    unsigned int row_stats[kRowErrWords] = {};  // where an append reads rowerr back to
    float norm_max = 0.f, norm_min = __builtin_inff();  // largest / smallest norm of a non-zero row ever appended (magnitudes_in_window)
    // experimental int8 shadow (MLVDB_I8=1, cosine, ld % 256 == 0): built lazily at search time, rebuilt after any mutation
    DevBuf x8, rp8, rowerr8, qimg8, sq8;
    DevBuf l2tag;  // l2: which pass scale the offsets plane behind rp8 ([0..3]) / rp8_masked ([4..7]) was computed for: filter_l2_offsets_kernel
    int64_t i8_rows = 0;      // rows [0, i8_rows) of the int8 shadow are current (0 after compact / reset / regrowth)
    float i8_err = 0.f;       // host copy of rowerr8 (read back whenever rows were converted)
    uint32_t i8_odd_groups = 0;  // ... and of its third word: 8-row scale groups whose largest row error exceeds 0.03
    bool sqmin_fresh = false;  // fmisc was just (re)allocated: FilterArgs::sqmin[] not initialised yet
    bool mask_active = false;  // h->rn is a masked copy (mlvdb_search_batch_filtered)
    bool mask_pairs_ready = false;  // ... and rp8_masked holds the masked copy of the int8 shadow's row pairs
    DevBuf rp8_masked;
    // metadata filters (mlvdb_where.h): typed attribute columns of `capacity` values each (absent-filled beyond the rows), and
    // the validated program of the current call (host copy kept until the call's stream has consumed it) + its match counter
    int32_t attr_type[MLVDB_MAX_ATTRS] = {};  // MLVDB_ATTR_*, 0 = not defined
    int64_t* attr_col[MLVDB_MAX_ATTRS] = {};  // nullptr while capacity == 0
    std::vector<WhereOp> where_ops;
    DevBuf where_prog, where_cnt;
    // list columns (mlvdb_list.h): per attribute an append-only value pool of list_cap int64, list_used of them allocated
    // (garbage of overwritten lists included until mlvdb_index_compact repacks it); the block sums of a scan and the CSR of
    // a read-back
    int64_t* list_pool[MLVDB_MAX_ATTRS] = {};
    DevBuf pool[MLVDB_MAX_ATTRS];  // owns list_pool[]
    int64_t list_cap[MLVDB_MAX_ATTRS] = {};
    int64_t list_used[MLVDB_MAX_ATTRS] = {};
    DevBuf list_sums, list_out;
    // sparse vector columns (mlvdb_sparse.h): a pass's tiles, term unions and weights; its answers
    DevBuf sparse_in, sparse_out;
    // binary vector columns (mlvdb_bits.h): a pass's queries and their popcounts; its answers
    DevBuf bits_in, bits_out;
    // hybrid search (mlvdb_hybrid.h): a chunk's dense and sparse queries, its two ranked lists, the union with the completed
    // components, and its outputs -- sized by the chunk (<= kHybridChunk queries), k and the fetch sizes, never by the corpus
    DevBuf hyb_q, hyb_list, hyb_union, hyb_out;
    // per-query filters (mlvdb_where_each.h): the call's programs, one 64-bit word per row, per-segment counts / offsets,
    // match totals, the gathered route's label lists, tiles, queries and outputs
    DevBuf each_prog, each_bits, each_seg, each_tot, each_lab, each_tiles, each_q, each_qpad, each_qaux, each_out;
    // distinct kNN (mlvdb_distinct.h): a chunk's queries, its ranked lists from the plain search, its outputs, and the
    // flagged queries' list + counter -- all sized by the chunk (<= kDistinctChunk queries), k and L, never by the corpus
    DevBuf dist_q, dist_list, dist_out, dist_sel;
    // grouped kNN (mlvdb_grouped.h): the code table of a chunk's picked groups with its counts / cursors, the tiles, pairs and
    // slot map, the outputs -- sized by the chunk (<= kDistinctChunk queries), k and group_size -- and the member lists: 4 B
    // per listed row, never more than 4 B x live rows
    DevBuf grp_tab, grp_tiles, grp_out, grp_lab;
    // diversified kNN (mlvdb_mmr.h): a chunk's queries, its ranked candidate lists from the plain search and its outputs --
    // sized by the chunk (<= kMmrChunk queries), k and fetch_k, never by the corpus
    DevBuf mmr_q, mmr_list, mmr_out;
    // search by stored examples (mlvdb_like.h): a chunk's synthesised queries (+ its base rows), its examples, the ranked
    // lists of the inner search and the stripped outputs -- sized by the chunk (<= kLikeChunk queries), k and the example
    // counts, never by the corpus
    DevBuf like_q, like_ex, like_list, like_out;
    // late-interaction search (mlvdb_maxsim.h): the code table of the call's documents with their dense ids, the dense id of
    // every row (4 B per row), the [token, document] keys of a chunk of queries (<= MAXSIM_WS_MB MiB, or one query's), the
    // chunk's token offsets and its ranked outputs
    DevBuf ms_tab, ms_rowdoc, ms_best, ms_misc, ms_out;
    // scored kNN (mlvdb_score.h): the call's programs with the conds' set table, a chunk's queries and its outputs -- sized
    // by the chunk (<= kDistinctChunk queries) and k, never by the corpus
    DevBuf score_prog, score_q, score_out;
    // recommend / discover (mlvdb_examples.h): a chunk's examples, tiles and exclusion table, its staged example rows, its
    // outputs -- sized by the chunk (<= kExamplesChunk queries) and k -- and the per-(query, row) state of its bags of more
    // than one tile: 16 B (24 B with one-example tiles) per row and such query, at most EXAMPLES_WS_MB MiB (or one query's)
    DevBuf ex_in, ex_q, ex_out, ex_state;
    // similarity join (mlvdb_join.h): the call's left labels (pack_range_hits reuses labels_in), a wave's labels, self
    // distances, results and dense outputs -- sized by the wave (<= kJoinWave rows) and `capacity` -- and the packed hits of
    // the call so far: 12 B per returned hit, grown as they come, never beyond total_capacity
    DevBuf join_left, join_ws, join_lab, join_dist;
    // clustering (mlvdb_cluster.h): the call's centroid labels and raw rows, the dense centroids, the per-row workspace (20 B per
    // row, 28 B for cosine k-means, and the listing's histograms), the segment table and the segment sums of one iteration
    DevBuf cl_in, cl_cent, cl_ws, cl_segs, cl_part;
    // facets (mlvdb_facet.h): the global value table + its packed copy, sized by the call's max_values; counters, bin edges and
    // bin counts -- never sized by the corpus
    DevBuf facet_tab, facet_misc;
    // attribute statistics (mlvdb_stats.h): the global group table, its packed copy and the counters, sized by the call's
    // max_groups, never by the corpus
    DevBuf stats_tab;
    // ordered queries (mlvdb_order.h): the call's state, one histogram per digit pass, the collected (key, label) pairs and the
    // ranked window -- sized by MLVDB_ORDER_MAX_ROWS and the histograms, never by the corpus
    DevBuf order_ws;
    // attribute updates (mlvdb_mutate.h): a call's assignments and counters, or the labels and values of a scatter
    DevBuf mutate_ws;
    // fp16 row-major shadow for the mid bounds (kernels_refine.hip): built lazily by the first range query / top_k > 64 search
    DevBuf x16, s16, rowerr16, picks, npicks;
    int64_t l2_rows = 0;      // rows [0, l2_rows) of the fp16 shadow are current (0 after compact / reset / regrowth)
    bool l2_failed = false;   // its allocation failed once (HBM full): the callers fall back, nobody retries per call
    DevBuf qimg, fmisc, cand, rescr, wgbuf, wgcnt, io_q, io_lab, io_dist, io_cnt, io_d64, counters, labels_in;
    DevBuf page_lab, page_dist, page_cnt, page_d64, cur_d, cur_l;  // top_k > MLVDB_MAX_TOPK paging
    PinBuf pin_in, pin_out;          // pinned staging of the host-pointer entries (queries in; labels / distances / counts out)
    DevBuf io_out;                   // one device buffer for all outputs of a host-pointer search: one D2H copy
    bool flags_in_out = false;       // search_host: the deferred overflow flags travel behind the outputs (flags_out, device)
    uint32_t* flags_out = nullptr;
    uint32_t* host_flags = nullptr;  // pinned, kFilterQueries words
    PinBuf flags_pin;                // owns host_flags
    bool deferred = false;           // search_host: the pass left its overflow flags in host_flags instead of launching the
    FilterArgs deferred_fa{};        //   exact fallback; its arguments, for the (rare) fallback after the sync
    int64_t host_fallbacks = 0;      // fallback queries decided on the host (added to the device-side count in the stats)
    bool host_overflow[256] = {};    // flags of the last collect_overflow
    std::string err;
    // statistics / profiling
    mlvdb_stats stats{};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> scan_events;
    size_t scan_events_used = 0;
    hipEvent_t total_events[2] = {nullptr, nullptr};
    bool stats_pending = false;
    hipStream_t counters_stream = nullptr;  // stream of the last call that wrote the device counters
    bool counters_pending = false;
    ~mlvdb_index() {  // (mlvdb_index_destroy has set the device and drained it; the memory members free themselves afterwards)
        for (auto& p : scan_events) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        for (auto& ev : total_events)
            if (ev) (void)hipEventDestroy(ev);
        if (stream) (void)hipStreamDestroy(stream);
        if (aux_stream) (void)hipStreamDestroy(aux_stream);
    }
};

namespace {

int fail(mlvdb_index* h, int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess) {
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        (void)hipGetLastError();  // reported here: the next launch's hipGetLastError() must not find it again
    } else
        snprintf(buf, sizeof buf, "%s", what);
    if (h)
        h->err = buf;
    else
        g_error = buf;
    return code;
}

#define HIP_TRY(h, call)                                                                    \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess)                                                              \
            return fail(h, e__ == hipErrorOutOfMemory ? MLVDB_ERR_OUT_OF_MEMORY : MLVDB_ERR_HIP, #call, e__); \
    } while (0)

// One output array of a chunk: n values at dev -> out + at; a null `out` means the caller does not want that array.
struct Down {
    void* host;
    const void* dev;
    size_t bytes;
    template <class T>
    Down(T* out, size_t at, const T* dev, size_t n) : host(out ? out + at : nullptr), dev(dev), bytes(n * sizeof(T)) {}
};

// A chunk's outputs to the host: wait, copy each wanted array down, wait.
int copy_down(mlvdb_index* h, hipStream_t s, std::initializer_list<Down> outs) {
    // The first wait is measured, not caution: a D2H copy enqueued behind the kernels would park at the head of the copy
    // queue until they end, and the copies of the index's other stream wait with it (search_host).  On a drained stream
    // it does no device work.
    HIP_TRY(h, hipStreamSynchronize(s));
    for (const Down& o : outs)
        if (o.host) HIP_TRY(h, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MLVDB_OK;
}

// A workspace of several fields, stated once: `fields` is a list of c.take<T>(n) calls assigning the field pointers.  It runs
// over no block to measure, `buf` grows to exactly that many bytes, and it runs again over the block.  The size and the
// layout cannot disagree, and a field that would not lie aligned is an error before any pointer exists.
template <class Fields>
int carve(mlvdb_index* h, DevBuf& buf, Fields&& fields) {
    Carver measure;
    fields(measure);
    if (measure.misaligned) return fail(h, MLVDB_ERR_INTERNAL, "workspace layout: a field does not lie aligned");
    HIP_TRY(h, buf.ensure(measure.at));
    Carver c{buf.as<char>()};
    fields(c);
    return MLVDB_OK;
}

#define CARVE(h, buf, ...) do { if (int rc__ = carve(h, buf, __VA_ARGS__)) return rc__; } while (0)

// ... the layout most blocks have (ListBlock): n entries and nq counts.
int carve_list(mlvdb_index* h, DevBuf& buf, size_t n, size_t nq, ListBlock& l) {
    return carve(h, buf, [&](Carver& c) { l.take(c, n, nq); });
}

// Bytes from the field `from` up to the field `to` of one carved block: the length of a memset that clears adjacent fields.
size_t span_bytes(const void* from, const void* to) { return (size_t)((const char*)to - (const char*)from); }

// ---- tuning state: name table, the one environment read, KEY=VAL parsing
struct TuningField {
    const char* name;
    int Tuning::*field;
};
const TuningField kTuningFields[] = {
#define X(field, name, dflt) {name, &Tuning::field},
    MLVDB_TUNING_FIELDS(X)
#undef X
};

// mlvdb_index_create only: MLVDB_<NAME> for every field of the table (internal.h); MLVDB_SHADOW=bf16 is the historical
// spelling of MLVDB_SHADOW_BF16=1.  Nothing else in the library reads the environment.
Tuning tuning_from_env() {
    Tuning t;
    char key[80];
    for (const TuningField& f : kTuningFields) {
        snprintf(key, sizeof key, "MLVDB_%s", f.name);
        if (const char* v = getenv(key)) t.*(f.field) = atoi(v);
        if (!strcmp(f.name, "SHADOW_BF16"))
            if (const char* v = getenv("MLVDB_SHADOW")) t.shadow_bf16 = !strcmp(v, "bf16") ? 1 : t.shadow_bf16;
    }
    return t;
}

const TuningField* find_tuning_field(const char* key, size_t len) {
    if (len > 6 && !strncmp(key, "MLVDB_", 6)) {
        key += 6;
        len -= 6;
    }
    for (const TuningField& f : kTuningFields)
        if (strlen(f.name) == len && !strncmp(f.name, key, len)) return &f;
    return nullptr;
}

// ---- attribute columns (mlvdb_where.h): the absent sentinel of a column type, and new column buffers for a capacity change
int64_t attr_absent(int32_t type) { return type == MLVDB_ATTR_FLOAT64 ? (int64_t)0x7ff8000000000000ll : INT64_MIN; }
// "has a slot and a pool": list columns (mlvdb_list.h), sparse vector columns (mlvdb_sparse.h) and binary vector columns
// (mlvdb_bits.h), which share the storage
bool pooled(int32_t type) { return type == MLVDB_ATTR_INT64_LIST || type == MLVDB_ATTR_SPARSE || type == MLVDB_ATTR_BITS; }

// nb.col[a] = a fresh column of `cap` values for every defined attribute: rows [0, keep) copied from the current column
// (old_of_new == nullptr: regrowth) or gathered through old_of_new (compaction), the rest absent.  Enqueued on h->stream;
// the caller commits them with the rows (commit_rows) after the stream has drained.
int attr_alloc(mlvdb_index* h, int64_t cap, int64_t keep, const int32_t* old_of_new, RowStore& nb) {
    for (int a = 0; a < MLVDB_MAX_ATTRS; ++a) {
        if (!h->attr_type[a] || cap == 0) continue;
        hipError_t e = nb.col[a].exact((size_t)cap * sizeof(int64_t));
        int64_t* ncol = nb.col[a].as<int64_t>();
        const bool copy = keep > 0 && h->attr_col[a];
        if (e == hipSuccess) e = launch_attr_fill(ncol, attr_absent(h->attr_type[a]), copy ? keep : 0, cap - (copy ? keep : 0), h->stream);
        if (e == hipSuccess && copy)
            e = old_of_new ? launch_attr_gather(h->attr_col[a], ncol, old_of_new, keep, h->stream)
                           : hipMemcpyAsync(ncol, h->attr_col[a], (size_t)keep * sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess)
            return fail(h, e == hipErrorOutOfMemory ? MLVDB_ERR_OUT_OF_MEMORY : MLVDB_ERR_HIP, "attribute columns", e);
    }
    return MLVDB_OK;
}

// The new blocks of a capacity change become the index's (h->stream has drained): the old ones are freed, the views follow.
void commit_rows(mlvdb_index* h, RowStore& nb, int64_t cap) {
    h->rows = std::move(nb);
    h->X = h->rows.X.as<float>();
    h->rn = h->rows.rn.as<float>();
    h->Xb = h->rows.Xb.p;
    for (int a = 0; a < MLVDB_MAX_ATTRS; ++a) h->attr_col[a] = h->rows.col[a].as<int64_t>();
    h->capacity = cap;
}

// ... and the new value pool of list attribute a (list_pool_reserve, list_repack).
void commit_pool(mlvdb_index* h, int a, DevBuf& np, int64_t cap) {
    h->pool[a] = std::move(np);
    h->list_pool[a] = h->pool[a].as<int64_t>();
    h->list_cap[a] = cap;
}

// ---- list columns (mlvdb_list.h): the value pools
// Room for `extra` more values behind list_used[a]: the pool regrows by doubling, its used part copied.
int list_pool_reserve(mlvdb_index* h, int a, int64_t extra) {
    const int64_t need = h->list_used[a] + extra;
    if (need <= h->list_cap[a]) return MLVDB_OK;
    const int64_t cap = std::max<int64_t>({need, 2 * h->list_cap[a], 1024});
    Staged<DevBuf> np(h->stream);
    HIP_TRY(h, np.exact((size_t)cap * sizeof(int64_t)));
    hipError_t e = hipSuccess;
    if (h->list_used[a] > 0)
        e = hipMemcpyAsync(np.p, h->list_pool[a], (size_t)h->list_used[a] * sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, MLVDB_ERR_HIP, "list pool regrowth", e);
    commit_pool(h, a, np, cap);
    return MLVDB_OK;
}

// The summed list lengths of n slots (rn != nullptr: of the live rows among them) -> *sum; h->list_sums keeps the scanned
// block sums launch_list_move reads.  Waits for the stream.
int list_scan(mlvdb_index* h, const int64_t* slots, const float* rn, int64_t n, int64_t* sum) {
    *sum = 0;
    if (n <= 0) return MLVDB_OK;
    hipStream_t s = h->stream;
    const int64_t nblocks = (n + kListBlock - 1) / kListBlock;
    HIP_TRY(h, h->list_sums.ensure((size_t)(nblocks + 1) * sizeof(int64_t)));
    HIP_TRY(h, launch_list_block_sums(slots, rn, n, h->list_sums.as<int64_t>(), s));
    HIP_TRY(h, launch_list_scan_sums(h->list_sums.as<int64_t>(), nblocks, s));
    HIP_TRY(h, hipMemcpyAsync(sum, h->list_sums.as<int64_t>() + nblocks, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MLVDB_OK;
}

// The pool of list attribute a rebuilt from rows [0, rows) of its column (all of them live: after a compaction), every
// list copied to a range of its own in row order and the slots rewritten: what overwritten lists left behind is gone, and
// rows that shared a range no longer do.
int list_repack(mlvdb_index* h, int a, int64_t rows) {
    hipStream_t s = h->stream;
    int64_t sum = 0;
    if (int rc = list_scan(h, h->attr_col[a], nullptr, rows, &sum)) return rc;
    Staged<DevBuf> np(s);
    if (sum > 0) HIP_TRY(h, np.exact((size_t)sum * sizeof(int64_t)));
    hipError_t e = launch_list_move(h->attr_col[a], rows, h->list_sums.as<int64_t>(), h->list_pool[a], np.as<int64_t>(),
                                    h->attr_col[a], nullptr, nullptr, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(h, MLVDB_ERR_HIP, "list pool repack", e);
    commit_pool(h, a, np, sum);
    h->list_used[a] = sum;
    return MLVDB_OK;
}

int list_repack_all(mlvdb_index* h, int64_t rows) {
    for (int a = 0; a < MLVDB_MAX_ATTRS; ++a)
        if (pooled(h->attr_type[a]) && h->attr_col[a])
            if (int rc = list_repack(h, a, rows)) return rc;
    return MLVDB_OK;
}

// The device scalars row_norms_kernel maintains (internal.h: kRowErrWords) and their host copies, as of an index without rows.
int clear_row_stats(mlvdb_index* h, bool keep_row_error = false) {
    static const unsigned int empty[kRowErrWords] = {0u, 0u, 0x7f800000u, 0u};  // {no error, largest norm 0, smallest +inf, -}
    const int first = keep_row_error ? 1 : 0;  // (compaction: the bf16 error of the rows that left stays, an upper bound)
    HIP_TRY(h, hipMemcpyAsync(h->rowerr.as<unsigned int>() + first, empty + first, (kRowErrWords - first) * sizeof(unsigned int),
                              hipMemcpyHostToDevice, h->stream));
    h->norm_max = 0.f;
    h->norm_min = __builtin_inff();
    return MLVDB_OK;
}

// After rows were appended (their row_norms_kernel is on h->stream): the norm range of the index, for use_filter.  The
// caller synchronises the stream.
int fetch_row_stats(mlvdb_index* h) {
    HIP_TRY(h, hipMemcpyAsync(h->row_stats, h->rowerr.p, sizeof h->row_stats, hipMemcpyDeviceToHost, h->stream));
    return MLVDB_OK;
}
void commit_row_stats(mlvdb_index* h) {
    std::memcpy(&h->norm_max, &h->row_stats[1], sizeof(float));
    std::memcpy(&h->norm_min, &h->row_stats[2], sizeof(float));
}

// Do the norms of the index's non-zero rows lie inside the magnitude window of the filter path (internal.h, DESIGN
// "Magnitudes")?  Tombstones do not narrow the range again; compaction (from the live rows' norms) and mlvdb_index_reset do.
bool magnitudes_in_window(const mlvdb_index* h) {
    return h->norm_max <= norm_window_hi(h->space) && h->norm_min >= norm_window_lo(h->space);  // (no non-zero row: 0 and +inf)
}

int reserve_rows(mlvdb_index* h, int64_t rows) {
    if (!h->rowerr.p) {  // largest relative bf16 rounding error of any row appended so far (0 = no rows), and their norm range
        HIP_TRY(h, h->rowerr.ensure(kRowErrWords * sizeof(unsigned int)));
        if (int rc = clear_row_stats(h)) return rc;
    }
    if (rows <= h->capacity) return MLVDB_OK;
    int64_t want = rows;
    if (h->capacity > 0 && want < h->capacity + h->capacity / 2) want = h->capacity + h->capacity / 2;
    const int64_t cap = round_up_rows(want);
    Staged<RowStore> nb(h->stream);
    HIP_TRY(h, nb.X.exact((size_t)cap * h->ld * sizeof(float)));
    hipError_t e = nb.rn.exact((size_t)cap * sizeof(float));
    if (e == hipSuccess && h->shadow) e = nb.Xb.exact((size_t)cap * h->ld * 2);
    if (e != hipSuccess) return fail(h, MLVDB_ERR_OUT_OF_MEMORY, "allocating the row norms / bf16 shadow", e);
    float* nX = nb.X.as<float>();
    float* nrn = nb.rn.as<float>();
    void* nXb = nb.Xb.p;
    if (int rc = attr_alloc(h, cap, h->total, nullptr, nb)) return rc;  // the attribute columns grow with the rows
    const size_t used_floats = (size_t)((h->total + 15) / 16) * 16 * h->ld;
    HIP_TRY(h, hipMemsetAsync(nX + used_floats, 0, ((size_t)cap * h->ld - used_floats) * sizeof(float), h->stream));
    HIP_TRY(h, hipMemsetAsync(nrn, 0xFF, (size_t)cap * sizeof(float), h->stream));  // 0xFFFFFFFF = NaN
    if (nXb) {
        HIP_TRY(h, hipMemsetAsync(static_cast<char*>(nXb) + used_floats * 2, 0, ((size_t)cap * h->ld - used_floats) * 2,
                                  h->stream));
        if (h->total > 0)
            HIP_TRY(h, hipMemcpyAsync(nXb, h->Xb, used_floats * 2, hipMemcpyDeviceToDevice, h->stream));
    }
    if (h->total > 0) {
        HIP_TRY(h, hipMemcpyAsync(nX, h->X, used_floats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(nrn, h->rn, (size_t)h->total * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    commit_rows(h, nb, cap);
    return MLVDB_OK;
}

// ---- profiling helpers
// Statistics accumulate over calls until mlvdb_index_last_stats reads (and resets) them, so a
// caller can enqueue many query waves without synchronising and still get per-kernel times.
// Timing-only events (profiling): created without the system-scope fence an event record otherwise carries -- the cache
// write-back / invalidate it costs sits between the kernels of the pass being measured (hip_runtime_api.h,
// hipEventDisableSystemFence: "events that are only being used to measure timing").  Nothing synchronises-with these events:
// results are read after a stream synchronisation.
static hipError_t create_timing_event(hipEvent_t* ev) { return hipEventCreateWithFlags(ev, hipEventDisableSystemFence); }

int begin_call(mlvdb_index* h, hipStream_t s) {
    if (h->scan_events_used > 8192) {  // nobody is reading them: start over rather than grow forever
        h->scan_events_used = 0;
        h->stats = mlvdb_stats{};
        h->stats_pending = false;
    }
    if (h->profiling && !h->stats_pending) {
        for (auto& ev : h->total_events)
            if (!ev) HIP_TRY(h, create_timing_event(&ev));
        HIP_TRY(h, hipEventRecord(h->total_events[0], s));
    }
    return MLVDB_OK;
}

int end_call(mlvdb_index* h, hipStream_t s) {
    if (h->profiling) {
        HIP_TRY(h, hipEventRecord(h->total_events[1], s));
        h->stats_pending = true;
    }
    return MLVDB_OK;
}

int scan_event(mlvdb_index* h, hipStream_t s, bool start) {
    if (!h->profiling) return MLVDB_OK;
    if (start) {
        if (h->scan_events_used == h->scan_events.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_TRY(h, create_timing_event(&a));
            HIP_TRY(h, create_timing_event(&b));
            h->scan_events.emplace_back(a, b);
        }
        HIP_TRY(h, hipEventRecord(h->scan_events[h->scan_events_used].first, s));
    } else {
        HIP_TRY(h, hipEventRecord(h->scan_events[h->scan_events_used].second, s));
        ++h->scan_events_used;
    }
    return MLVDB_OK;
}

// One scan launch of a pass over `rows` rows: timed when profiling, counted in the statistics.
template <class Launch>
int scan_step(mlvdb_index* h, hipStream_t s, int64_t rows, Launch&& launch) {
    int rc = scan_event(h, s, true);
    if (rc) return rc;
    HIP_TRY(h, launch());
    rc = scan_event(h, s, false);
    if (rc) return rc;
    h->stats.scan_launches += 1;
    h->stats.rows_scanned += rows;
    return MLVDB_OK;
}

// ---- exact scan of rows [0,row_end) for a set of queries of the prepared batch.
// Qpad/qaux point at query 0 of the set's index space; qsel (device) lists the members or is null.
int run_exact(mlvdb_index* h, hipStream_t s, const float* Qpad, const double* qaux, int32_t nq_sel,
              const int32_t* qsel, int64_t row_end, int32_t k, int64_t* out_labels,
              float* out_dist, int32_t* out_counts, double* out_d64, bool is_main_scan,
              const int32_t* nq_sel_dev = nullptr, const double* cursor_d = nullptr,
              const int32_t* cursor_l = nullptr) {
    if (nq_sel <= 0) return MLVDB_OK;
    ExactPlan plan = plan_exact(row_end, h->ld, nq_sel, k);
    if (nq_sel_dev) {
        // device-decided fallback: usually zero or a few queries are selected, so spread each query
        // tile over many blocks; blocks of unselected tiles exit at once
        const int64_t by_mem = (int64_t)(64u << 20) / ((int64_t)nq_sel * k * (int64_t)sizeof(TopEntry));
        plan.nblk = (int)std::max<int64_t>(8, std::min<int64_t>(256, by_mem));
    }
    HIP_TRY(h, h->partial.ensure((size_t)nq_sel * plan.nblk * k * sizeof(TopEntry)));
    ExactArgs a{};
    a.X = h->X;
    a.rn = h->rn;
    a.row_end = row_end;
    a.ld = h->ld;
    a.space = h->space;
    a.Qpad = Qpad;
    a.qaux = qaux;
    a.qsel = qsel;
    a.nq_sel = nq_sel;
    a.nq_sel_dev = nq_sel_dev;
    a.k = k;
    a.cursor_d = cursor_d;
    a.cursor_l = cursor_l;
    a.partial = h->partial.as<TopEntry>();
    if (is_main_scan) {
        int rc = scan_step(h, s, row_end * plan.nqtiles, [&] { return launch_exact_scan(a, plan, s); });
        if (rc) return rc;
    } else {
        HIP_TRY(h, launch_exact_scan(a, plan, s));
    }
    HIP_TRY(h, launch_exact_merge(a.partial, nq_sel, nq_sel_dev, qsel, plan.nblk, k, out_labels, out_dist, out_counts,
                                  out_d64, s));
    return MLVDB_OK;
}

__global__ void fill_empty_kernel(int64_t* labels, float* dist, int32_t* counts, double* d64, int64_t nq, int32_t k) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        labels[i] = -1;
        dist[i] = __builtin_inff();
        if (d64) d64[i] = __builtin_inf();
    }
    if (i < nq) counts[i] = 0;
}

__global__ void copy_words_kernel(const uint32_t* src, uint32_t* dst) { dst[threadIdx.x] = src[threadIdx.x]; }

// The workspace of one pass over queries q0 .. q0 + nq of the call (their prepared form lives in h->qpad / qaux / qerr at q0).
// range_lists: the pass keeps its own, larger candidate lists -- true hits + the band of the bound, per query anything from
// none to tens of thousands -- and the exact hit arrays of the range kernels (range and big-k passes).
int setup_filter_ws(mlvdb_index* h, FilterArgs& fa, int32_t q0, int32_t nq, bool range_lists) {
    HIP_TRY(h, h->qimg.ensure(filter_qimg_bytes((h->ld + 63) / 64 * 64)));
    {
        const void* before = h->fmisc.p;
        HIP_TRY(h, h->fmisc.ensure(9 * kFilterQueries * sizeof(uint32_t)));
        if (h->fmisc.p != before) h->sqmin_fresh = true;  // the two scalars the fused prep's atomics start from: see begin_pass
    }
    HIP_TRY(h, h->cand.ensure((size_t)kFilterQueries * kCandCap * sizeof(CandEntry)));
    HIP_TRY(h, h->rescr.ensure((size_t)kFilterQueries * kCandCap * sizeof(RangeHit)));  // exact scores of the rescored candidates
    if (h->Xb || h->i8_only) {  // the assembly scan appends through workgroup-private buffers
        HIP_TRY(h, h->wgbuf.ensure((size_t)kScanMaxGrid * kWgCap * sizeof(WgEntry)));
        HIP_TRY(h, h->wgcnt.ensure((size_t)kScanMaxGrid * 8 * sizeof(uint32_t)));
    }
    HIP_TRY(h, h->flags_pin.ensure(kFilterQueries * sizeof(uint32_t)));
    h->host_flags = static_cast<uint32_t*>(h->flags_pin.p);
    fa.tn = &h->tn;
    fa.X = h->X;
    fa.Xb = h->Xb;
    fa.rn = h->rn;
    fa.total = h->total;
    fa.ld = h->ld;
    fa.ld8 = h->ld8;
    fa.space = h->space;
    fa.Qpad = h->qpad.as<float>() + (size_t)q0 * h->ld;
    fa.qaux = h->qaux.as<double>() + q0;
    fa.qerr = h->qerr.as<float>() + q0;
    fa.row_err = h->rowerr.as<float>();
    fa.nq = nq;
    fa.qimg = h->qimg.p;
    fa.qscale = h->fmisc.as<float>();
    fa.thr = h->fmisc.as<float>() + kFilterQueries;
    fa.cnt = h->fmisc.as<uint32_t>() + 2 * kFilterQueries;
    fa.overflow = h->fmisc.as<uint32_t>() + 3 * kFilterQueries;
    fa.ke = h->fmisc.as<float>() + 4 * kFilterQueries;
    // (words 5 x 256 .. 6 x 256 are free)
    fa.ke8 = h->fmisc.as<float>() + 6 * kFilterQueries;  // 257 floats
    fa.sqmin = h->fmisc.as<uint32_t>() + 7 * kFilterQueries + 128;  // [0..1] smallest scale / largest error (cosine); [2..3] l2c QMAX by parity
    fa.l2c_out = h->fmisc.as<float>() + 7 * kFilterQueries + 132;
    fa.rmaxq = h->fmisc.as<float>() + 8 * kFilterQueries;
    fa.rs = h->rescr.as<RangeHit>();
    fa.cand = h->cand.as<CandEntry>();
    fa.cand_cap = kCandCap;
    fa.wgbuf = h->wgbuf.as<WgEntry>();
    fa.wgcnt = h->wgcnt.as<uint32_t>();
    if (range_lists) {
        HIP_TRY(h, h->cand_range.ensure((size_t)kFilterQueries * kRangeCandCap * sizeof(CandEntry)));
        HIP_TRY(h, h->rhits.ensure((size_t)kFilterQueries * kCandCap * sizeof(RangeHit)));
        HIP_TRY(h, h->rhit_cnt.ensure(kFilterQueries * sizeof(uint32_t)));
        fa.cand = h->cand_range.as<CandEntry>();
        fa.cand_cap = kRangeCandCap;
        fa.rhits = h->rhits.as<RangeHit>();
        fa.rhit_cnt = h->rhit_cnt.as<uint32_t>();
    }
    return MLVDB_OK;
}

// Collect the overflowed queries of a pass on the host; returns their count (device list in h->qsel).
int collect_overflow(mlvdb_index* h, hipStream_t s, const FilterArgs& fa, int32_t* n_flagged) {
    HIP_TRY(h, hipStreamSynchronize(s));  // (a D2H copy enqueued behind a long kernel parks in the copy queue: search_host)
    HIP_TRY(h, hipMemcpyAsync(h->host_flags, fa.overflow, kFilterQueries * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    int32_t sel[kFilterQueries];
    int32_t n = 0;
    for (int q = 0; q < kFilterQueries; ++q) h->host_overflow[q] = q < fa.nq && h->host_flags[q] != 0;
    for (int q = 0; q < fa.nq; ++q)
        if (h->host_flags[q]) sel[n++] = q;
    *n_flagged = n;
    if (n) {
        HIP_TRY(h, h->qsel.ensure(kFilterQueries * sizeof(int32_t)));
        HIP_TRY(h, hipMemcpyAsync(h->qsel.p, sel, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s));  // `sel` is on this stack frame
    }
    return MLVDB_OK;
}

// int8 shadow of a cosine index (kernels_filter.hip, "int8 shadow"): kept current lazily -- rows appended since the
// last pass are converted here, tombstones are patched in by mlvdb_index_tombstone, compaction / reset / regrowth
// start it over.  MLVDB_I8=0 keeps the pass on the bf16 shadow.
// (l2: only the |x| slot -- the x-slot of an l2 pair holds its group's scale or error and must survive the row: shadow8_rows_kernel)
__global__ void tombstone_rp8_kernel(const int64_t* labels, int64_t n, float* rp8, int64_t rows, int l2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && labels[i] >= 0 && labels[i] < rows) {
        rp8[2 * labels[i] + 1] = __builtin_nanf("");
        if (!l2) rp8[2 * labels[i]] = __builtin_nanf("");
    }
}

bool i8_bounds_usable(const mlvdb_index* h);

bool i8_eligible(const mlvdb_index* h) {
    return h->tn.i8 != 0 && (h->Xb || h->i8_only) && h->ld8 > 0;  // (tools/scan_ab.py switches I8 inside one process: set_tuning)
}

// The l2 offsets plane of a pair buffer is valid for the pairs it was computed from: whatever rewrites pairs forgets the tag
// (slot 0: rp8, slot 1: rp8_masked); the next pass's filter_l2_offsets_kernel then recomputes the plane.
int forget_l2_offsets(mlvdb_index* h, int slot, hipStream_t s) {
    if (h->space != kSpaceL2) return MLVDB_OK;
    if (!h->l2tag.p) {
        HIP_TRY(h, h->l2tag.ensure(8 * sizeof(uint32_t)));
        HIP_TRY(h, hipMemsetAsync(h->l2tag.p, 0, 8 * sizeof(uint32_t), s));
        return MLVDB_OK;
    }
    HIP_TRY(h, hipMemsetAsync(h->l2tag.as<uint32_t>() + 4 * slot, 0, 4 * sizeof(uint32_t), s));
    return MLVDB_OK;
}

// Bring the int8 shadow up to date (rows appended since the last pass).  Must run with the index's own norms in h->rn
// (a row-mask search swaps them for a masked copy afterwards).
int update_i8_shadow(mlvdb_index* h, hipStream_t s) {
    // (l2: a third float-sized word per row behind the pairs: the integer offsets of the folded admission test, per pass)
    const size_t need_x8 = (size_t)h->capacity * h->ld8, need_rp = (size_t)h->capacity * (h->space == kSpaceL2 ? 3 : 2) * sizeof(float);
    if (h->x8.bytes < need_x8 || h->rp8.bytes < need_rp || !h->rowerr8.p) {
        HIP_TRY(h, h->x8.ensure(need_x8));
        HIP_TRY(h, h->rp8.ensure(need_rp));
        HIP_TRY(h, h->rowerr8.ensure(4 * sizeof(float)));  // {largest relative row error, smallest row norm, odd groups (u32), -}
        h->i8_rows = 0;
    }
    if (h->i8_rows == 0) {
        HIP_TRY(h, hipMemsetAsync(h->x8.p, 0, need_x8, s));
        HIP_TRY(h, hipMemsetAsync(h->rp8.p, 0xff, need_rp, s));  // NaN: not a row
        if (int rc = forget_l2_offsets(h, 0, s)) return rc;
        HIP_TRY(h, hipMemsetAsync(h->rowerr8.p, 0, sizeof(float), s));
        HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->rowerr8.as<float>() + 1), 0x7f800000, 1, s));  // +inf
        HIP_TRY(h, hipMemsetAsync(h->rowerr8.as<float>() + 2, 0, sizeof(uint32_t), s));
    }
    if (h->i8_rows < h->total) {
        if (int rc = forget_l2_offsets(h, 0, s)) return rc;
        HIP_TRY(h, launch_shadow8_rows(h->X, h->rn, h->x8.p, h->rp8.as<float>(), h->rowerr8.as<float>(), h->i8_rows, h->total,
                                       h->ld, h->ld8, h->space, s));
        h->i8_rows = h->total;
        uint32_t words[3] = {0u, 0u, 0u};
        HIP_TRY(h, hipMemcpyAsync(words, h->rowerr8.p, sizeof words, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        std::memcpy(&h->i8_err, &words[0], sizeof(float));
        h->i8_odd_groups = words[2];
    }
    return MLVDB_OK;
}

// Can the int8 shadow serve this call?  The index keeps one, it is current -- brought up to date here; under a row mask the
// masked copy of the row pairs must have been built instead (without it: the bf16 / fp32 bodies) -- and its bounds are usable:
// one scale per row means a row with an outlier component quantises badly.  Cosine bounds carry every row's own error; l2 / ip
// still use the index-wide maximum, which would then admit everything: beyond 0.03 (typical data sits at 0.008-0.015) they
// keep to the bf16 shadow, whose error is relative per component (i8_bounds_usable).
int i8_ready(mlvdb_index* h, hipStream_t s, bool* ready) {
    *ready = false;
    if (!i8_eligible(h)) return MLVDB_OK;
    if (h->mask_active) {
        if (!h->mask_pairs_ready) return MLVDB_OK;
    } else {
        int rc = update_i8_shadow(h, s);
        if (rc) return rc;
    }
    *ready = i8_bounds_usable(h);
    return MLVDB_OK;
}

int attach_i8(mlvdb_index* h, hipStream_t s, FilterArgs& fa) {
    bool ready = false;
    int rc = i8_ready(h, s, &ready);
    if (rc || !ready) return rc;
    HIP_TRY(h, h->qimg8.ensure((size_t)kFilterQueries * h->ld8));
    HIP_TRY(h, h->sq8.ensure(kFilterQueries * sizeof(float)));
    fa.X8 = h->x8.p;
    fa.rp8 = h->mask_active ? h->rp8_masked.as<float>() : h->rp8.as<float>();  // a masked-out row is a NaN pair: "not a row"
    // l2: pairs + offsets through one buffer descriptor (32-bit offsets): 12 bytes per row must stay below 4 GB
    fa.rp8_cap = h->space == kSpaceL2 ? h->capacity : 0;  // (l2_int8_ok held: i8_bounds_usable)
    if (fa.rp8_cap > 0) {
        fa.l2c = 1;
        if (!h->l2tag.p) {
            rc = forget_l2_offsets(h, 0, s);  // (allocates, zeroed)
            if (rc) return rc;
        }
        fa.l2tag = h->tn.l2_offset_cache != 0 ? h->l2tag.as<uint32_t>() + (h->mask_active ? 4 : 0) : nullptr;
    }
    fa.row_err8 = h->rowerr8.as<float>();
    fa.qimg8 = h->qimg8.p;
    fa.sq8 = h->sq8.as<float>();
    return MLVDB_OK;
}

// The prologue of a filter pass over queries q0 .. q0 + nq of the call: workspace, the int8 shadow when it serves the pass,
// then everything the pass needs of its queries in one fused launch (+ the one-block fin for int8 passes of several queries).
// `queries_raw`: the call's queries [.][dim] as the caller gave them (device); their padded copy, norms and image errors go
// to h->qpad / qaux / qerr at q0.
int begin_pass(mlvdb_index* h, hipStream_t s, FilterArgs& fa, const float* queries_raw, int32_t q0, int32_t nq, bool range_lists) {
    int rc = setup_filter_ws(h, fa, q0, nq, range_lists);
    if (rc) return rc;
    rc = attach_i8(h, s, fa);
    if (rc) return rc;
    HIP_TRY(h, filter_set_body(fa));  // the pass's one body choice: the prep, the scans and the stats below read fa.body
    if (h->sqmin_fresh) {  // what the fused prep's atomicMin / atomicMax start from; afterwards every fin kernel restores it
        HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(fa.sqmin), 0x7f7f7f7f, 1, s));
        HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(fa.sqmin + 1), 0, 1, s));
        h->sqmin_fresh = false;
    }
    HIP_TRY(h, launch_filter_prep_fused(fa, queries_raw + (size_t)q0 * h->dim, h->dim, h->qpad.as<float>() + (size_t)q0 * h->ld,
                                        h->qaux.as<double>() + q0, h->qerr.as<float>() + q0, s));
    if (fa.body == kBodyI8 && fa.rp8_cap > 0) {
        // l2: this pass's integer offsets (they depend on its largest query scale and on which rows are live): 29 us for 10M rows
        // (it stays in the pass's stream: DESIGN "tried and dropped")
        const int64_t rows = std::min<int64_t>(h->capacity, (h->total + kFilterTile - 1) / kFilterTile * kFilterTile);
        HIP_TRY(h, launch_filter_l2_offsets(fa, rows, s));
    }
    h->stats.bound_dtype = fa.body == kBodyI8 ? 2 : 1;
    return MLVDB_OK;
}

// The end of a kNN pass: exact fp64 rescoring of the candidate lists (unless the last refine did it: ranked), then the exact
// fallback for overflowed queries.
int finish_filter_pass(mlvdb_index* h, hipStream_t s, FilterArgs& fa, int32_t q0, int32_t nq, int32_t k, int64_t* out_labels,
                       float* out_dist, int32_t* out_counts, double* out_d64, bool defer_fallback, bool ranked) {
    // counters: [0] rescored pairs, [1] fallback queries (accumulated over the passes of a call), [2] flag count
    unsigned long long* stats = h->counters.as<unsigned long long>();
    // (its ranking kernel also compacts the overflowed queries for the device-decided fallback below: qsel, nflag)
    HIP_TRY(h, h->qsel.ensure(kFilterQueries * sizeof(int32_t)));
    int32_t* nflag = reinterpret_cast<int32_t*>(stats + 2);
    if (!ranked)
        HIP_TRY(h, launch_filter_rescore(fa, k, q0, out_labels, out_dist, out_counts, out_d64, stats,
                                         defer_fallback ? nullptr : h->qsel.as<int32_t>(), nflag, s));
    // overflowed queries (adversarial near-ties) are re-run on the exact scan.  The decision stays on
    // the device: the list is compacted there and the scan's blocks exit at once when it is empty,
    // so the call never waits for the host.
    if (defer_fallback) {
        // host-pointer entry, single pass: the caller synchronises anyway to copy the results out, so the overflow
        // flags ride along to pinned memory and the exact fallback is only launched if a query needs it (search_host)
        // -- three launches fewer on every ordinary call, which is 5 % of a batch-1 call
        if (h->flags_in_out) {  // a kernel on the pass's stream, not a copy-engine job
            copy_words_kernel<<<1, kFilterQueries, 0, s>>>(fa.overflow, h->flags_out);
            HIP_TRY(h, hipGetLastError());
        } else
            HIP_TRY(h, hipMemcpyAsync(h->host_flags, fa.overflow, kFilterQueries * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        h->deferred_fa = fa;
        h->deferred = true;
        return MLVDB_OK;
    }
    return run_exact(h, s, fa.Qpad, fa.qaux, nq, h->qsel.as<int32_t>(), h->total, k, out_labels + (size_t)q0 * k,
                     out_dist + (size_t)q0 * k, out_counts + q0, out_d64 ? out_d64 + (size_t)q0 * k : nullptr, false, nflag);
}

// tuning aid (DEBUG_ENTRIES): entries appended by the scan launch over rows [b, e) (synchronises the stream)
int print_scan_entries(mlvdb_index* h, hipStream_t s, const FilterArgs& fa, int64_t b, int64_t e) {
    std::vector<uint32_t> wc((size_t)kScanMaxGrid * 8, 0u);
    HIP_TRY(h, hipMemcpyAsync(wc.data(), fa.wgcnt, wc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    uint64_t sum = 0, mx = 0;
    const int waves = (int)std::min<int64_t>(256, (e - b + 255) / 256) * 8;  // 8-wave workgroups of 256-row tiles
    for (int i = 0; i < waves; ++i) {
        sum += wc[(size_t)i];
        mx = std::max<uint64_t>(mx, wc[(size_t)i]);
    }
    fprintf(stderr, "[mlvdb] scan rows [%lld, %lld): %llu entries appended (%.1f per query), max per wave %llu\n",
            (long long)b, (long long)e, (unsigned long long)sum, (double)sum / fa.nq, (unsigned long long)mx);
    return MLVDB_OK;
}

// One pass of <= 256 queries through the filter path; outputs at query index q0.. of the batch.  `queries_raw`: see begin_pass.
int run_filter_pass(mlvdb_index* h, hipStream_t s, const float* queries_raw, int32_t q0, int32_t nq, int32_t k,
                    int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64, bool defer_fallback = false) {
    FilterArgs fa{};
    int rc = begin_pass(h, s, fa, queries_raw, q0, nq, false);
    if (rc) return rc;
    fa.scan_q4 = k <= 64;
    // Small batches (k <= 64, int8 shadow, no row mask), up to SMALL_NQ queries (at most 8; default 2):
    //  - seed (SMALL_SEED): the exact k-th best of the prefix by a kernel made for it (one 16-row group per wave all over the
    //    chip + a one-block selection of the k-th: 8 + 10 us) instead of the dense int8 pass + exact-threshold refine (7 + 15.5 us
    //    of latency chains at batch 1); the prefix rows then belong to the first scan round.
    //  - finish (SMALL_FINISH): the refine after the LAST round also rescores and ranks (one launch instead of three:
    //    launch_filter_finish_small).  One block per query: at 4-8 queries the rescoring kernel's spread over the whole chip
    //    wins again -- 0.261 vs 0.247 ms at 4; neither step gains there (profiles/r03/small_batch_fused_finish_and_prefix_seed_1m.txt).
    const int small_nq = std::max(0, std::min(8, h->tn.small_nq));
    const bool small = fa.body == kBodyI8 && nq <= small_nq && k <= 64;
    const bool small_finish = small && filter_refine_can_fuse(fa) && h->tn.small_finish != 0;
    // One query on a small corpus (SMALL_BATCH; two queries: 0.214-0.220 vs 0.211-0.219 ms -- no gain) goes ONE round: the exact
    // k-th best of an 11,520-row prefix puts the threshold at quantile k / 11,520; one scan launch over every row then appends
    // ~total (k / 11,520) x band entries per query -- 1M x 768, k = 10: 870 x band (~4 on N(0,1) rows) of the list's 8,192 --
    // and the fused finish prunes, rescores and ranks: five launches instead of seven (no 65k-row first round, no refine
    // after it): 0.197-0.199 vs 0.206-0.212 ms at batch 1 (profiles/r04/small_batch_one_round_vs_rounds_1m.txt).  Taken only
    // while the estimate with band = 6 stays inside the list; a list that overflows all the same sends its query to the exact
    // scan, as everywhere.
    const int64_t m1 = 3 * kSeedRows;
    const bool one_round = h->tn.small_batch != 0 && small_finish && nq <= std::min(1, small_nq) && !h->mask_active &&
                           h->tn.small_seed != 0 && h->total > 4 * m1 && (double)h->total * k * 6.0 <= 6000.0 * (double)m1;
    // seed: a dense pass of the filter kernel over the first rows puts every bound into the lists,
    // the update kernel turns them into thresholds; the remaining rows follow in rounds of growing
    // size so that thresholds tighten early
    // rows of the dense seeding pass: a multiple of kFilterTile (the first scan round starts there), at most kSeedRows
    // (MLVDB_SEED_ROWS, in units of kFilterTile = 768 rows: tuning, read per call)
    const int64_t seed_rows = one_round ? m1 : std::min<int64_t>(kSeedRows, std::max<int64_t>(1, h->tn.seed_rows) * kFilterTile);
    const int64_t n_seed = std::min<int64_t>(h->total, seed_rows);
    int64_t first_row = seed_rows;
    // l2 index with a few badly quantising rows: the dense int8 pass would bound every seed row with the index-wide error,
    // and those inflated bounds then crowd the refines' picks -- the threshold stalls at the seed's quantile.  Such a pass takes
    // its thresholds from the EXACT k-th best score among the seed rows (exact fp64 scan of that prefix + merge + one tiny kernel)
    const bool seed_exact = fa.body == kBodyI8 && h->space == kSpaceL2 && h->i8_err > 0.03f;
    if (one_round || (small && !h->mask_active && !seed_exact && h->tn.small_seed != 0)) {
        HIP_TRY(h, h->seed_d64.ensure(((size_t)kFilterQueries * 64 + (size_t)8 * kSeedRows) * sizeof(double)));
        double* d64 = h->seed_d64.as<double>();
        HIP_TRY(h, launch_prefix_exact(h->X, fa.rn, fa.Qpad, fa.qaux, nq, (int32_t)n_seed, h->ld, h->space, d64, s));
        HIP_TRY(h, launch_filter_prefix_thr(fa, d64, (int32_t)n_seed, k, s));
        first_row = 0;
    } else if (seed_exact) {
        HIP_TRY(h, h->seed_lab.ensure((size_t)kFilterQueries * k * sizeof(int64_t)));
        HIP_TRY(h, h->seed_dist.ensure((size_t)kFilterQueries * k * sizeof(float)));
        HIP_TRY(h, h->seed_cnt.ensure(kFilterQueries * sizeof(int32_t)));
        HIP_TRY(h, h->seed_d64.ensure((size_t)kFilterQueries * k * sizeof(double)));
        rc = run_exact(h, s, fa.Qpad, fa.qaux, nq, nullptr, n_seed, k, h->seed_lab.as<int64_t>(),
                       h->seed_dist.as<float>(), h->seed_cnt.as<int32_t>(), h->seed_d64.as<double>(), false);
        if (rc) return rc;
        HIP_TRY(h, launch_filter_seed_thr(fa, h->seed_d64.as<double>(), k, s));
        first_row = 0;
    } else {
        HIP_TRY(h, launch_filter_seed_scan(fa, n_seed, k, s));  // includes the first threshold update
    }
    // scan rounds: [seed, r1) [r1, r2) [r2, total), each followed by an exact-threshold refine; in units of kFilterTile rows
    // (MLVDB_ROUND1 / MLVDB_ROUND2: tuning, read per call); one_round: [0, total)
    // r1 = 85: 3840 + 240 tiles of 256 rows -- one tile for (nearly) every CU costs what 192 tiles did (64: +1.5 % per 10M-row
    // wave; 170: the same as 85; r2 = 1024 .. 2389: within noise, 4096: +2.5 %; profiles/r02/scan_ab_round_sizes_10m.txt)
    const int64_t r1 = std::max<int64_t>(6, h->tn.round1), r2 = std::max<int64_t>(r1, h->tn.round2);
    const int64_t bounds[] = {first_row, one_round ? h->total : (int64_t)kFilterTile * r1,
                              one_round ? h->total : (int64_t)kFilterTile * r2, h->total};
    bool ranked = false;
    for (int r = 0; r < 3; ++r) {
        const int64_t b = std::min(bounds[r], h->total), e = std::min(bounds[r + 1], h->total);
        if (e <= b) continue;
        rc = scan_step(h, s, e - b, [&] { return launch_filter_scan(fa, b, e, s); });
        if (rc) return rc;
        if (h->tn.debug_entries) {
            rc = print_scan_entries(h, s, fa, b, e);
            if (rc) return rc;
        }
        if (small_finish && e == h->total) {  // the last round of a small batch
            HIP_TRY(h, h->qsel.ensure(kFilterQueries * sizeof(int32_t)));
            unsigned long long* stats = h->counters.as<unsigned long long>();
            HIP_TRY(h, launch_filter_finish_small(fa, k, q0, out_labels, out_dist, out_counts, out_d64, stats,
                                                  defer_fallback ? nullptr : h->qsel.as<int32_t>(),
                                                  reinterpret_cast<int32_t*>(stats + 2), s));
            ranked = true;
            break;
        }
        HIP_TRY(h, launch_filter_refine_update(fa, k, -1, s));
    }
    return finish_filter_pass(h, s, fa, q0, nq, k, out_labels, out_dist, out_counts, out_d64, defer_fallback, ranked);
}

// ---- the fp16 row-major shadow of the mid bounds (kernels_refine.hip): kept current lazily, like the int8 shadow.
// *m gets X16 == nullptr when the index keeps none (Tuning L2_SHADOW=0, or HBM was full when it was first wanted): the
// callers then do without the second level.
int attach_mid(mlvdb_index* h, hipStream_t s, MidArgs* m) {
    *m = MidArgs{};
    if (!h->tn.l2_shadow || h->l2_failed || h->total == 0) return MLVDB_OK;
    const int32_t ld16 = (h->dim + 63) / 64 * 64;
    const size_t need = (size_t)h->capacity * ld16 * sizeof(uint16_t), need_s = (size_t)h->capacity * sizeof(float);
    if (h->x16.bytes < need || h->s16.bytes < need_s || !h->rowerr16.p) {
        hipError_t e = h->x16.ensure(need);
        if (e == hipSuccess) e = h->s16.ensure(need_s);
        if (e == hipSuccess) e = h->rowerr16.ensure(sizeof(float));
        if (e != hipSuccess) {  // not an error of the call: the index works without it
            (void)hipGetLastError();
            h->x16.release();
            h->s16.release();
            h->l2_failed = true;
            return MLVDB_OK;
        }
        h->l2_rows = 0;
    }
    if (h->l2_rows == 0) {
        HIP_TRY(h, hipMemsetAsync(h->x16.p, 0, need, s));  // (the columns dim..ld16 of every row stay zero)
        HIP_TRY(h, hipMemsetAsync(h->rowerr16.p, 0, sizeof(float), s));
    }
    if (h->l2_rows < h->total) {
        HIP_TRY(h, launch_shadow16_rows(h->X, h->x16.p, h->s16.as<float>(), h->rowerr16.as<float>(), h->l2_rows, h->total, h->ld,
                                        ld16, s));
        h->l2_rows = h->total;
    }
    m->X16 = h->x16.as<_Float16>();
    m->s16 = h->s16.as<float>();
    m->row_err16 = h->rowerr16.as<float>();
    m->ld16 = ld16;
    return MLVDB_OK;
}

int run_paged_exact(mlvdb_index* h, hipStream_t s, const float* Qpad, const double* qaux, int64_t nq_space,
                    const int32_t* qsel, int32_t nsel, int32_t k, int64_t* out_labels, float* out_dist,
                    int32_t* out_counts, double* out_d64);

// ---- top_k in (64, 1024]: one pass of <= 256 queries on the filter path (round 4; DESIGN "big-k passes").
// Structure: dense seeding pass over the first <= 65,280 rows (every bound into the query's 65,536-slot list) -> [select
// the best-bounded entries -> mid (fp16) bounds for those not refined yet -> threshold = k-th largest mid LOWER bound, prune]
// -> scan rounds of geometrically growing size, each followed by the same three kernels -> mid bounds for whatever is left
// unrefined -> exact fp64 rescoring of the survivors (~1.02 k rows per query) -> ranking by (distance, label).
// Round sizes: a launch may append ~BIGK_BUDGET entries per 256 queries x k before its waves' append buffers (2,048 entries
// each) run over; with n rows seen the k-th best is at quantile k / n, so the next m rows yield ~nq m (k / n) band entries:
// m = n BUDGET / (nq k).  A query whose list or wave buffer overflows all the same is served by the paged exact scan.
// *handled = false: the index has no mid shadow (the caller takes the paged exact scan).
int run_bigk_pass(mlvdb_index* h, hipStream_t s, const float* queries_raw, int32_t q0, int32_t nq, int32_t k,
                  int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64, bool* handled) {
    *handled = false;
    MidArgs m{};
    int rc = attach_mid(h, s, &m);
    if (rc) return rc;
    if (!m.X16) return MLVDB_OK;
    FilterArgs fa{};
    rc = begin_pass(h, s, fa, queries_raw, q0, nq, true);
    if (rc) return rc;
    HIP_TRY(h, h->picks.ensure((size_t)kFilterQueries * kPicksCap * sizeof(uint32_t)));
    HIP_TRY(h, h->npicks.ensure(kFilterQueries * sizeof(uint32_t)));
    uint32_t* picks = h->picks.as<uint32_t>();
    uint32_t* npicks = h->npicks.as<uint32_t>();
    MidArgs mp = m;  // refine the picks / (m) everything still unrefined
    mp.picks = picks;
    mp.npicks = npicks;
    mp.picks_cap = kPicksCap;
    const int32_t want = k + std::max(32, k / 4);
    auto refine = [&](int32_t forced_cnt) -> int {
        HIP_TRY(h, launch_bigk_select(fa, want, forced_cnt, picks, npicks, kPicksCap, s));
        HIP_TRY(h, launch_mid_score(fa, mp, s));
        HIP_TRY(h, launch_bigk_thr_prune(fa, m, k, forced_cnt, s));
        return MLVDB_OK;
    };
    // seed: dense over the first rows (a multiple of 128; a whole number of 768-row units when rounds follow)
    // How many: the first scan round appends ~32 rows x nq x (k / n_seed) x 8 entries per wave and tile, which must stay
    // well inside a wave's buffer: n_seed >= ~66 k nq / 256 (k = 100: 6,912 rows, k = 1000: the 65,280 a list takes)
    const int64_t want_seed = std::min<int64_t>(kBigSeedRows, std::max<int64_t>(kSeedRows, ((int64_t)66 * k * std::max(nq, 16) / 256 + kFilterTile - 1) / kFilterTile * kFilterTile));
    const int64_t n_seed = h->total > want_seed ? want_seed : (h->total + 127) / 128 * 128;
    HIP_TRY(h, launch_filter_dense_scan(fa, n_seed, s));
    rc = refine((int32_t)n_seed);
    if (rc) return rc;
    // growth of the rows seen per round: bounded by the waves' append buffers (BIGK_BUDGET entries per launch and 256 queries:
    // 256 workgroups x 8 waves x ~1,000 slots, less the band factor ~8) and by the query's own list (half of its 65,536 slots
    // for one round's band: m (k / n) 8 <= 32,768)
    const double growth = std::min(std::min(24.0, 1.0 + 4096.0 / k),
                                   std::max(1.5, 1.0 + (double)std::max(1, h->tn.bigk_budget) / ((double)std::max(nq, 16) * k)));
    int64_t b = std::min<int64_t>(n_seed, h->total);
    while (b < h->total) {
        int64_t e = (int64_t)((double)b * growth) / kFilterTile * kFilterTile;
        if (e <= b) e = b + kFilterTile;
        if (e > h->total || (double)e * 1.25 > (double)h->total) e = h->total;  // (no sliver of a last round)
        rc = scan_step(h, s, e - b, [&] { return launch_filter_scan(fa, b, e, s); });
        if (rc) return rc;
        rc = refine(-1);
        if (rc) return rc;
        b = e;
    }
    // whatever survived without a mid bound (the band of the last rounds) gets one; the threshold then rests on all of them
    HIP_TRY(h, launch_mid_score(fa, m, s));
    HIP_TRY(h, launch_bigk_thr_prune(fa, m, k, -1, s));
    unsigned long long* stats = h->counters.as<unsigned long long>();
    HIP_TRY(h, launch_knn_rescore_rank(fa, k, q0, out_labels, out_dist, out_counts, out_d64, stats, s));
    // overflowed queries (a list or a wave's append buffer ran over, or more than 8,192 rows tie into the top k): the
    // paged exact scan serves them; the decision needs the host here (one synchronisation per pass, top_k > 64 only)
    int32_t n_flagged = 0;
    rc = collect_overflow(h, s, fa, &n_flagged);
    if (rc) return rc;
    if (n_flagged) {
        h->host_fallbacks += n_flagged;
        rc = run_paged_exact(h, s, fa.Qpad, fa.qaux, nq, h->qsel.as<int32_t>(), n_flagged, k, out_labels + (size_t)q0 * k,
                             out_dist + (size_t)q0 * k, out_counts + q0, out_d64 ? out_d64 + (size_t)q0 * k : nullptr);
        if (rc) return rc;
    }
    *handled = true;
    return MLVDB_OK;
}

// ---- top_k above MLVDB_MAX_TOPK: rank-ordered pages of the exact scan.  Page p returns the next
// entries strictly after the cursor (fp64 distance, label) of page p-1, so pages never overlap.
// Query ids: blockIdx / thread index i addresses qsel[i] when a selection is given.
__global__ void page_init_kernel(double* cur_d, int32_t* cur_l, int32_t* out_counts, const int32_t* qsel, int64_t nsel) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nsel) {
        const int64_t q = qsel ? qsel[i] : i;
        cur_d[q] = -__builtin_inf();
        cur_l[q] = -1;
        out_counts[q] = 0;
    }
}

__global__ void page_commit_kernel(const int64_t* page_lab, const float* page_dist, const int32_t* page_cnt,
                                   const double* page_d64, const int32_t* qsel, int32_t kp, int32_t offset, int32_t k,
                                   int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64,
                                   double* cur_d, int32_t* cur_l) {
    const int q = qsel ? qsel[blockIdx.x] : blockIdx.x;
    const int i = threadIdx.x;  // kp <= 64 threads
    const int n = page_cnt[q];
    if (i < kp) {
        const int64_t o = (int64_t)q * k + offset + i;
        const bool ok = i < n;
        out_labels[o] = ok ? page_lab[(int64_t)q * kp + i] : -1;
        out_dist[o] = ok ? page_dist[(int64_t)q * kp + i] : __builtin_inff();
        if (out_d64) out_d64[o] = ok ? page_d64[(int64_t)q * kp + i] : __builtin_inf();
    }
    if (i == 0) {
        out_counts[q] += n;
        if (n > 0) {
            cur_d[q] = page_d64[(int64_t)q * kp + n - 1];
            cur_l[q] = (int32_t)page_lab[(int64_t)q * kp + n - 1];
        }
        if (n < kp) {  // exhausted: later pages must find nothing
            cur_d[q] = __builtin_inf();
            cur_l[q] = 0x7fffffff;
        }
    }
}

// nq_space = size of the query index space of Qpad/qaux and of the outputs; (qsel, nsel) = the queries to serve
int run_paged_exact(mlvdb_index* h, hipStream_t s, const float* Qpad, const double* qaux, int64_t nq_space,
                    const int32_t* qsel, int32_t nsel, int32_t k, int64_t* out_labels, float* out_dist,
                    int32_t* out_counts, double* out_d64) {
    const int32_t page = MLVDB_MAX_TOPK;
    HIP_TRY(h, h->page_lab.ensure((size_t)nq_space * page * sizeof(int64_t)));
    HIP_TRY(h, h->page_dist.ensure((size_t)nq_space * page * sizeof(float)));
    HIP_TRY(h, h->page_cnt.ensure((size_t)nq_space * sizeof(int32_t)));
    HIP_TRY(h, h->page_d64.ensure((size_t)nq_space * page * sizeof(double)));
    HIP_TRY(h, h->cur_d.ensure((size_t)nq_space * sizeof(double)));
    HIP_TRY(h, h->cur_l.ensure((size_t)nq_space * sizeof(int32_t)));
    page_init_kernel<<<(unsigned)((nsel + 255) / 256), 256, 0, s>>>(h->cur_d.as<double>(), h->cur_l.as<int32_t>(),
                                                                    out_counts, qsel, nsel);
    HIP_TRY(h, hipGetLastError());
    for (int32_t offset = 0; offset < k; offset += page) {
        const int32_t kp = std::min(page, k - offset);
        int rc = run_exact(h, s, Qpad, qaux, nsel, qsel, h->total, kp, h->page_lab.as<int64_t>(),
                           h->page_dist.as<float>(), h->page_cnt.as<int32_t>(), h->page_d64.as<double>(), true, nullptr,
                           h->cur_d.as<double>(), h->cur_l.as<int32_t>());
        if (rc) return rc;
        page_commit_kernel<<<(unsigned)nsel, 64, 0, s>>>(h->page_lab.as<int64_t>(), h->page_dist.as<float>(),
                                                         h->page_cnt.as<int32_t>(), h->page_d64.as<double>(), qsel, kp,
                                                         offset, k, out_labels, out_dist, out_counts, out_d64,
                                                         h->cur_d.as<double>(), h->cur_l.as<int32_t>());
        HIP_TRY(h, hipGetLastError());
    }
    return MLVDB_OK;
}

// Range fallback for queries whose candidate list overflowed: copy the nearest hits found by the paged
// exact kNN into the range outputs and publish the exact counts.
__global__ void range_fallback_commit_kernel(const int32_t* qsel, const uint32_t* exact_cnt, const int64_t* knn_lab,
                                             const float* knn_dist, int32_t kmax, int32_t q0, int64_t cap_eff,
                                             int64_t* out_labels, float* out_dist, int64_t* out_counts) {
    const int q = qsel[blockIdx.x];
    const int64_t n = exact_cnt[q];
    const int64_t emit = n < cap_eff ? n : cap_eff;
    for (int64_t i = threadIdx.x; i < emit; i += blockDim.x) {
        out_labels[(int64_t)(q0 + q) * cap_eff + i] = knn_lab[(int64_t)q * kmax + i];
        out_dist[(int64_t)(q0 + q) * cap_eff + i] = knn_dist[(int64_t)q * kmax + i];
    }
    if (threadIdx.x == 0) out_counts[q0 + q] = n;
}

// valid prefixes of the dense per-query result rows -> one packed array (offsets from the host)
__global__ void range_pack_kernel(const int64_t* lab, const float* dist, const int64_t* offsets, int64_t cap_eff, int64_t* plab,
                                  float* pdist) {
    const int64_t q = blockIdx.x;
    const int64_t o = offsets[q], n = offsets[q + 1] - o;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        plab[o + i] = lab[q * cap_eff + i];
        pdist[o + i] = dist[q * cap_eff + i];
    }
}

__global__ void range_reset_kernel(uint32_t* cnt, const int32_t* qsel) { cnt[qsel[threadIdx.x]] = 0; }
// (thr: a resolved list holds exact hits with u = 0, so the mid pruning must keep every entry whatever threshold the scan had --
// an l2 query that filter_l2_offsets_kernel took off the filter carries +inf, which dropped all of its hits)
__global__ void range_resolve_kernel(uint32_t* overflow, float* thr, const uint32_t* cnt, const int32_t* qsel, uint32_t cap) {
    const int q = qsel[threadIdx.x];
    overflow[q] = cnt[q] > cap ? 1u : 0u;
    thr[q] = -3.4e38f;
}

// (l2: the int8 bodies are the l2c ones -- folded test, per-row integer offsets read through the row pairs' descriptor, which needs
// pairs + offsets, 12 bytes per row, below 4 GB; SCAN_L2C=0 takes l2 off the int8 shadow: bf16 / fp32 / exact paths)
bool l2_int8_ok(const mlvdb_index* h) {
    return h->space != kSpaceL2 || (h->tn.scan_l2c && (uint64_t)h->capacity * 12ull < 0xfff00000ull);
}
// One scale per row (l2 / ip: per group of 8 rows): a row with an outlier component quantises badly.  Cosine bounds carry every
// row's own error (any index-wide maximum up to 0.5 will do).  ip bounds use the index-wide maximum: beyond 0.03 (typical data:
// 0.008-0.015) they would admit everything (I8_ERR_IP, thousandths).  l2 bounds carry per-group errors (round 4), so a FEW odd
// rows cost only their own groups: the index stays on the int8 shadow while at most 64 + 0.05 % of its rows sit in groups above
// 0.03 (shadow8_rows_kernel counts them) and the worst stays under I8_ERR_L2 thousandths (1100: any finite row -- a group
// quantised to zeros has error 1 and Cauchy-Schwarz's bound; 30: round 3's index-wide rule); such a pass seeds its thresholds
// exactly (run_filter_pass) because the dense int8 seeding pass does use the index-wide maximum.
// profiles/r04/outlier_row_ab_l2_ip_4m_before.txt: 5 rows with a 40-sigma component among 4M x 768 made every l2 / ip wave
// 3.3 x slower (fp32 rows converted in registers), 54 x on d = 300 (exact scan); outlier_row_ab_l2_4m.txt: l2 now 1.1-1.2 x.
bool i8_bounds_usable(const mlvdb_index* h) {
    if (!l2_int8_ok(h)) return false;
    if (h->space == kSpaceCosine) return h->i8_err <= 0.5f;
    if (h->i8_err <= 0.03f) return true;
    if (h->space == kSpaceIp) return h->i8_err <= 0.001f * (float)h->tn.i8_err_ip;
    return h->i8_err <= 0.001f * (float)h->tn.i8_err_l2 && (int64_t)h->i8_odd_groups * 8 <= 64 + h->total / 2000;
}

// Is a filter body available for this index right now?  ld % 64 == 0: always (bf16 shadow, int8 shadow, or the fp32 rows
// converted in registers).  Any other ld has only the int8 body: the (zero-padded) int8 shadow is brought up to date here
// and its bounds must be usable (i8_ready, the test attach_i8 makes: l2 / ip rows that quantise too badly go to the exact scan).
bool use_filter(const mlvdb_index* h, int64_t nq, bool ready);

int filter_ready(mlvdb_index* h, hipStream_t s, int64_t nq, bool* ready) {
    *ready = false;
    if (h->strategy == MLVDB_STRATEGY_EXACT || h->total == 0) return MLVDB_OK;
    if (!use_filter(h, nq, true)) return MLVDB_OK;  // AUTO would take the exact scan anyway: no shadow is built for this call
    if (filter_supported(h->ld)) {
        *ready = true;
        return MLVDB_OK;
    }
    return i8_ready(h, s, ready);
}

bool use_filter(const mlvdb_index* h, int64_t nq, bool ready) {
    if (h->strategy == MLVDB_STRATEGY_EXACT || !ready) return false;
    // rows beyond the magnitude window: no shadow holds them and the fp32 bounds overflow -- the exact scans (fp64) serve the
    // index whatever strategy is set, a forced MLVDB_STRATEGY_FILTER included
    if (!magnitudes_in_window(h)) return false;
    if (h->strategy == MLVDB_STRATEGY_FILTER) return true;
    const bool shadowed = h->Xb != nullptr || h->i8_only;
    // dim < 64: the padded int8 shadow (256 B per row) is wider than the fp32 rows (4 ld B), and the exact scan of such short
    // rows is bound by its per-row work, not by HBM (4M rows, d = 16 / 32 / 48: 0.16-0.21 ms for one query, 0.30-0.36 for 4,
    // 0.45-0.58 ms per 8-query pass; the int8 chain: 0.28 ms for 5-64 queries, 0.37 ms for 256; 500k rows x 32: 0.12-0.16
    // against 0.17 / 0.20 / 0.35 / 1.67 ms for 5 / 8 / 16 / 256 queries -- profiles/r04/dim_ab_small_dims_{4m,500k}.txt).
    // Up to 4 queries the exact scan wins at any size; beyond, the filter wins once the exact passes (one per 8 queries)
    // cover some 400k rows between them.
    if (h->i8_only && h->ld8 >= 4 * h->ld) return nq > 4 && h->total >= 32768 && (nq + 7) / 8 * h->total >= 400000;
    if (nq >= 12 || (nq >= 8 && shadowed)) return h->total >= 32768;
    // small batches: the narrow filter kernel streams the bf16 shadow, half the bytes of the exact fp32 scan; below
    // ~125k rows of 768 columns the exact scan's two launches win (profiles/r01/small_batch_ab_crossover.txt)
    return shadowed && h->total * (int64_t)h->ld >= (int64_t)96 << 20;
}

int check_handle(mlvdb_index* h) {
    if (!h) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "null index handle");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(h, MLVDB_ERR_HIP, "hipSetDevice", e);
    return MLVDB_OK;
}

// The header promises "never throws, returns an int status": every extern "C" body runs inside this guard, so that a
// host-side allocation failure (std::vector / std::string growth) or any other C++ exception becomes a status code
// instead of unwinding through the caller's C / ctypes frames (std::terminate -> SIGABRT).
template <class F>
int guarded(mlvdb_index* h, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        try { return fail(h, MLVDB_ERR_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)"); } catch (...) { return MLVDB_ERR_OUT_OF_MEMORY; }
    } catch (const std::exception& e) {
        try { return fail(h, MLVDB_ERR_INTERNAL, e.what()); } catch (...) { return MLVDB_ERR_INTERNAL; }
    } catch (...) {
        try { return fail(h, MLVDB_ERR_INTERNAL, "unknown C++ exception"); } catch (...) { return MLVDB_ERR_INTERNAL; }
    }
}

// ... and the entry that works on its handle's device: the guard, then check_handle, then the body.  (The entries that
// only read or set host state of the handle check it themselves and never call hipSetDevice.)
constexpr struct OnDevice {} kOnDevice;
template <class F>
int guarded(mlvdb_index* h, OnDevice, F&& body) noexcept {
    return guarded(h, [&]() -> int {
        if (int rc = check_handle(h)) return rc;
        return body();
    });
}

// ---- the refusals several entries share, each with its one status and text.  Which refusal wins when a call has two
// faults is behaviour: an entry calls these in its own order, between its own checks, and none of them checks two things.
int check_nq(mlvdb_index* h, int64_t nq) {
    return nq < 0 || nq > (1 << 24) ? fail(h, MLVDB_ERR_INVALID_ARG, "nq out of range") : MLVDB_OK;
}
int check_k_min(mlvdb_index* h, int32_t k) { return k < 1 ? fail(h, MLVDB_ERR_INVALID_ARG, "k must be >= 1") : MLVDB_OK; }
// k <= MLVDB_MAX_TOPK / the 2^31 - 1 rows the pooled-column kernels index, refused under the family's prefix ("distinct: ", ...)
int check_k_max(mlvdb_index* h, int32_t k, const char* prefix) {
    return k > MLVDB_MAX_TOPK ? fail(h, MLVDB_ERR_UNSUPPORTED, (std::string(prefix) + "k above MLVDB_MAX_TOPK").c_str()) : MLVDB_OK;
}
int check_row_limit(mlvdb_index* h, const char* prefix) {
    return h->total > INT32_MAX ? fail(h, MLVDB_ERR_UNSUPPORTED, (std::string(prefix) + "more than 2^31 - 1 rows").c_str()) : MLVDB_OK;
}
int check_k_max_paged(mlvdb_index* h, int32_t k) {
    return k > MLVDB_MAX_TOPK_PAGED ? fail(h, MLVDB_ERR_UNSUPPORTED, "k above MLVDB_MAX_TOPK_PAGED") : MLVDB_OK;
}

// rows [first, first + n) lie inside the index, and a non-empty range has its buffer
int check_row_range(mlvdb_index* h, int64_t first, int64_t n, bool have_buffer = true) {
    if (first < 0 || n < 0 || first > h->total || n > h->total - first || (n > 0 && !have_buffer))
        return fail(h, MLVDB_ERR_INVALID_ARG, "row range out of bounds");
    return MLVDB_OK;
}

// n >= 1 labels of a by-label write: inside [0, total), none twice.
int labels_check(mlvdb_index* h, const int64_t* labels, int64_t n) {
    std::vector<int64_t> sorted(labels, labels + n);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= h->total) return fail(h, MLVDB_ERR_INVALID_ARG, "label outside [0, total)");
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        return fail(h, MLVDB_ERR_INVALID_ARG, "a label appears twice");
    return MLVDB_OK;
}

// The head of a by-label write: the arguments (have_buffers: the entry's other arrays of n values), *updated zeroed, nothing
// to do for no label, the labels themselves; then `write`, the entry's remaining checks and its work.
template <class F>
int with_labels(mlvdb_index* h, const int64_t* labels, int64_t n, int64_t* updated, bool have_buffers, const char* what, F&& write) {
    if (!updated || n < 0 || (n > 0 && (!labels || !have_buffers))) return fail(h, MLVDB_ERR_INVALID_ARG, what);
    *updated = 0;
    if (n == 0) return MLVDB_OK;
    if (int rc = labels_check(h, labels, n)) return rc;
    return write();
}

// Null-tolerant padding of one output array, and of the outputs most searches share: n entries (label -1, distances
// sign x inf -- +1 for distances, -1 for scores; dist64 may be null) and nq zeroed counts.
template <class T, class V>
void pad(T* out, int64_t n, V value) {
    if (out) std::fill(out, out + n, (T)value);
}

void pad_outputs(int64_t* labels, float* dist, double* dist64, int64_t n, int32_t* counts, int64_t nq, float sign = 1.0f) {
    pad(labels, n, -1);
    pad(dist, n, sign * __builtin_inff());
    pad(dist64, n, sign * __builtin_inf());
    pad(counts, nq, 0);
}

}  // namespace

// ============================================================================== C ABI
extern "C" {

int mlvdb_abi_version(void) { return MLVDB_ABI_VERSION; }

const char* mlvdb_last_global_error(void) { return g_error.c_str(); }

const char* mlvdb_last_error(const mlvdb_index* h) { return h ? h->err.c_str() : g_error.c_str(); }

int mlvdb_device_count(int* count) {
    return guarded(nullptr, [&]() -> int {
    if (!count) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *count = 0;
        return fail(nullptr, MLVDB_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)", e);
    }
    *count = n;
    return MLVDB_OK;
    });
}

int64_t mlvdb_layout_offset(int64_t row, int32_t col, int32_t ld) { return layout_offset(row, col, ld); }
int32_t mlvdb_layout_ld(int32_t dim) { return layout_ld(dim); }

int mlvdb_index_create(int device, int32_t dim, int32_t space, int64_t capacity_hint, mlvdb_index** out) {
    return guarded(nullptr, [&]() -> int {
    if (!out) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (dim <= 0 || dim > 8192) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "dim must be in 1..8192");
    if (space < 0 || space > 2) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "space must be MLVDB_SPACE_L2/COSINE/IP");
    if (capacity_hint < 0) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "capacity_hint < 0");
    int n = 0;
    int rc = mlvdb_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "device index out of range");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, MLVDB_ERR_HIP, "hipSetDevice", e);
    mlvdb_index* h = new (std::nothrow) mlvdb_index();
    if (!h) return fail(nullptr, MLVDB_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->device = device;
    h->dim = dim;
    h->ld = layout_ld(dim);
    h->space = space;
    h->tn = tuning_from_env();  // the one moment the environment is consulted
    {
        // Which shadow the index keeps (decided here, once).  The int8 shadow has its own width ld8 = round_up(ld, 256), zero
        // padded -- zero columns change neither a dot product nor a norm -- so every dim gets the int8 body (round 4; dim < 64
        // too: there the shadow is wider than the fp32 rows, it is built by the first batch large enough to want it, see
        // use_filter; I8_PAD=0: only dim % 256 == 0, round 3).  It is the only shadow wherever it streams fewer bytes per row than the
        // bf16 one would (ld8 < 2 ld) or no bf16 body exists (ld % 64 != 0): seeding pass, small batches, scans, range and
        // row-mask searches all run on it.  ld = 64 / 128 keep the bf16 shadow (same bytes, tighter bounds).
        // SHADOW_BF16=1 (MLVDB_SHADOW=bf16) keeps the bf16 shadow as well (the bf16 bodies for A/B, I8=0).
        const Tuning& tn = h->tn;
        h->ld8 = 0;
        if (!tn.no_shadow) {
            const int32_t cand = (h->ld + 255) / 256 * 256;
            if (cand == h->ld || (tn.i8_pad && (cand < 2 * h->ld || !filter_supported(h->ld)))) h->ld8 = cand;
        }
        h->i8_only = h->ld8 > 0 && !tn.shadow_bf16;
        h->shadow = filter_supported(h->ld) && !tn.no_shadow && !h->i8_only;
    }
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return fail(nullptr, MLVDB_ERR_HIP, "hipStreamCreate", e);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->counters.ensure(64);
    if (e != hipSuccess) {
        delete h;
        return fail(nullptr, MLVDB_ERR_HIP, "allocating the counters", e);
    }
    if (capacity_hint > 0) {
        rc = reserve_rows(h, capacity_hint);
        if (rc) {
            g_error = h->err;
            delete h;
            return rc;
        }
    }
    *out = h;
    return MLVDB_OK;
    });
}

int mlvdb_index_destroy(mlvdb_index* h) {
    return guarded(h, [&]() -> int {
    if (!h) return MLVDB_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipDeviceSynchronize();
    delete h;
    return MLVDB_OK;
    });
}

int mlvdb_index_append_device(mlvdb_index* h, const float* rows_device, int64_t n, int64_t* first_label) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (n < 0 || (n > 0 && !rows_device)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad rows / n");
    if (h->total + n > 0x7fffff00ll) return fail(h, MLVDB_ERR_UNSUPPORTED, "more than 2^31 rows per index");
    if (first_label) *first_label = h->total;
    if (n == 0) return MLVDB_OK;
    if (int rc = reserve_rows(h, h->total + n)) return rc;
    HIP_TRY(h, launch_scatter_rows(rows_device, h->X, h->total, n, h->dim, h->ld, h->stream));
    HIP_TRY(h, launch_row_norms(h->X, h->rn, h->total, n, h->ld, h->rowerr.as<unsigned int>(), h->stream));
    if (h->Xb) HIP_TRY(h, launch_shadow_rows(h->X, h->Xb, h->total, n, h->ld, h->stream));
    if (int rc2 = fetch_row_stats(h)) return rc2;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    commit_row_stats(h);
    h->total += n;
    return MLVDB_OK;
    });
}

int mlvdb_index_append(mlvdb_index* h, const float* rows, int64_t n, int64_t* first_label) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (n < 0 || (n > 0 && !rows)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad rows / n");
    if (h->total + n > 0x7fffff00ll) return fail(h, MLVDB_ERR_UNSUPPORTED, "more than 2^31 rows per index");
    if (first_label) *first_label = h->total;
    if (n == 0) return MLVDB_OK;
    if (int rc = reserve_rows(h, h->total + n)) return rc;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(256u << 20) / ((int64_t)h->dim * 4));
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        HIP_TRY(h, h->stage.ensure((size_t)m * h->dim * sizeof(float)));
        HIP_TRY(h, hipMemcpyAsync(h->stage.p, rows + (size_t)done * h->dim, (size_t)m * h->dim * sizeof(float),
                                  hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, launch_scatter_rows(h->stage.as<float>(), h->X, h->total + done, m, h->dim, h->ld, h->stream));
        HIP_TRY(h, launch_row_norms(h->X, h->rn, h->total + done, m, h->ld, h->rowerr.as<unsigned int>(), h->stream));
        if (h->Xb) HIP_TRY(h, launch_shadow_rows(h->X, h->Xb, h->total + done, m, h->ld, h->stream));
        if (int rc2 = fetch_row_stats(h)) return rc2;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        commit_row_stats(h);
    }
    h->total += n;
    return MLVDB_OK;
    });
}

int mlvdb_index_tombstone(mlvdb_index* h, const int64_t* labels, int64_t n, int64_t* newly_deleted) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (n < 0 || (n > 0 && !labels)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad labels / n");
    if (newly_deleted) *newly_deleted = 0;
    if (n == 0 || h->total == 0) return MLVDB_OK;
    HIP_TRY(h, h->labels_in.ensure((size_t)n * sizeof(int64_t)));
    HIP_TRY(h, hipMemcpyAsync(h->labels_in.p, labels, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->counters.p, 0, sizeof(unsigned long long), h->stream));
    HIP_TRY(h, launch_tombstone(h->rn, h->labels_in.as<int64_t>(), n, h->total, h->counters.as<unsigned long long>(),
                                h->stream));
    if (h->rp8.p && h->i8_rows > 0) {  // the int8 shadow's row constants carry the tombstones too (before the sync below:
                                       // a search on another stream may follow this call at once)
        tombstone_rp8_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(h->labels_in.as<int64_t>(), n, h->rp8.as<float>(), h->i8_rows, h->space == kSpaceL2 ? 1 : 0);
        HIP_TRY(h, hipGetLastError());
        if (int rc2 = forget_l2_offsets(h, 0, h->stream)) return rc2;  // (a dead row changes its lane group's P0)
    }
    unsigned long long changed = 0;
    HIP_TRY(h, hipMemcpyAsync(&changed, h->counters.p, sizeof changed, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->deleted += (int64_t)changed;
    if (newly_deleted) *newly_deleted = (int64_t)changed;
    return MLVDB_OK;
    });
}

int mlvdb_index_compact(mlvdb_index* h, int64_t* old_labels, int64_t capacity, int64_t* live_out) {
    return guarded(h, kOnDevice, [&]() -> int {
    const int64_t want = h->total - h->deleted;
    if (capacity < want || (want > 0 && !old_labels)) return fail(h, MLVDB_ERR_INVALID_ARG, "old_labels too small");
    if (live_out) *live_out = want;
    if (h->deleted == 0) {  // nothing to drop: identity (the list pools still shed their overwritten lists)
        for (int64_t i = 0; i < want; ++i) old_labels[i] = i;
        return list_repack_all(h, want);
    }
    hipStream_t s = h->stream;
    const int64_t nblocks = (h->total + 1023) / 1024;
    HIP_TRY(h, h->partial.ensure((size_t)nblocks * sizeof(uint32_t) + 64));
    HIP_TRY(h, h->labels_in.ensure((size_t)std::max<int64_t>(want, 1) * sizeof(int32_t)));
    uint32_t* scratch = h->partial.as<uint32_t>();
    int32_t* old_of_new = h->labels_in.as<int32_t>();
    unsigned long long* live_d = h->counters.as<unsigned long long>();
    HIP_TRY(h, launch_compact_map(h->rn, h->total, scratch, live_d, old_of_new, s));
    unsigned long long live = 0;
    HIP_TRY(h, hipMemcpyAsync(&live, live_d, sizeof live, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if ((int64_t)live != want) return fail(h, MLVDB_ERR_INTERNAL, "live-row count disagrees with the tombstone accounting");
    // new buffers sized for the live rows (zero / NaN filled), gather, swap
    const int64_t cap = round_up_rows(std::max<int64_t>(want, 1));
    std::vector<int32_t> host_map((size_t)want);  // (before nb: an abandoned call drains the stream's copy into it first)
    Staged<RowStore> nb(s);
    hipError_t e = nb.X.exact((size_t)cap * h->ld * sizeof(float));
    if (e == hipSuccess) e = nb.rn.exact((size_t)cap * sizeof(float));
    if (e == hipSuccess && h->Xb) e = nb.Xb.exact((size_t)cap * h->ld * 2);
    if (e != hipSuccess) return fail(h, MLVDB_ERR_OUT_OF_MEMORY, "allocating the compaction buffers", e);
    float* nX = nb.X.as<float>();
    float* nrn = nb.rn.as<float>();
    void* nXb = nb.Xb.p;
    HIP_TRY(h, hipMemsetAsync(nX, 0, (size_t)cap * h->ld * sizeof(float), s));
    HIP_TRY(h, hipMemsetAsync(nrn, 0xFF, (size_t)cap * sizeof(float), s));  // NaN = not a row
    if (nXb) HIP_TRY(h, hipMemsetAsync(nXb, 0, (size_t)cap * h->ld * 2, s));
    HIP_TRY(h, launch_compact_rows(h->X, nX, h->Xb, nXb, h->rn, nrn, old_of_new, want, h->ld, s));
    // the norm range starts over from the rows that stay: a tombstoned row outside the magnitude window leaves with them
    // (read back at the synchronisation below, committed with the new buffers)
    const float old_max = h->norm_max, old_min = h->norm_min;
    if (int rc2 = clear_row_stats(h, true)) return rc2;
    h->norm_max = old_max;  // (the index still holds the old rows until the swap)
    h->norm_min = old_min;
    HIP_TRY(h, launch_norm_range(nrn, want, h->rowerr.as<unsigned int>(), s));
    if (int rc2 = fetch_row_stats(h)) return rc2;
    if (int rc2 = attr_alloc(h, cap, want, old_of_new, nb)) return rc2;  // the attribute columns move with their rows
    if (want > 0)
        HIP_TRY(h, hipMemcpyAsync(host_map.data(), old_of_new, (size_t)want * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    commit_row_stats(h);
    for (int64_t i = 0; i < want; ++i) old_labels[i] = host_map[(size_t)i];
    commit_rows(h, nb, cap);
    h->total = want;
    h->deleted = 0;
    h->i8_rows = 0;
    h->l2_rows = 0;
    return list_repack_all(h, want);  // the slots moved with their rows: now the pools are repacked in the new row order
    });
}

int mlvdb_index_counts(const mlvdb_index* h, int64_t* total, int64_t* deleted) {
    return guarded(const_cast<mlvdb_index*>(h), [&]() -> int {
    if (!h) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "null index handle");
    if (total) *total = h->total;
    if (deleted) *deleted = h->deleted;
    return MLVDB_OK;
    });
}

int mlvdb_index_reset(mlvdb_index* h, int32_t space) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (space > 2) return fail(h, MLVDB_ERR_INVALID_ARG, "space must be < 0 (keep) or a MLVDB_SPACE_* value");
    if (h->capacity > 0) {
        HIP_TRY(h, hipMemsetAsync(h->X, 0, (size_t)h->capacity * h->ld * sizeof(float), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->rn, 0xFF, (size_t)h->capacity * sizeof(float), h->stream));
        if (h->Xb) HIP_TRY(h, hipMemsetAsync(h->Xb, 0, (size_t)h->capacity * h->ld * 2, h->stream));
        for (int a = 0; a < MLVDB_MAX_ATTRS; ++a)  // attribute values go, their definitions stay
            if (h->attr_col[a]) HIP_TRY(h, launch_attr_fill(h->attr_col[a], attr_absent(h->attr_type[a]), 0, h->capacity, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (h->rowerr.p)
        if (int rc2 = clear_row_stats(h)) return rc2;
    for (int64_t& used : h->list_used) used = 0;  // the list pools are empty again (their allocations stay)
    h->total = 0;
    h->deleted = 0;
    h->i8_rows = 0;
    h->l2_rows = 0;
    if (space >= 0) h->space = space;
    return MLVDB_OK;
    });
}

int mlvdb_index_get_rows(mlvdb_index* h, int64_t first, int64_t n, float* out_rows) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (first < 0 || n < 0 || first + n > h->total || (n > 0 && !out_rows))
        return fail(h, MLVDB_ERR_INVALID_ARG, "row range out of bounds");
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(256u << 20) / ((int64_t)h->dim * 4));
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        HIP_TRY(h, h->stage.ensure((size_t)m * h->dim * sizeof(float)));
        HIP_TRY(h, launch_gather_rows(h->X, h->stage.as<float>(), first + done, m, h->dim, h->ld, h->stream));
        HIP_TRY(h, hipMemcpyAsync(out_rows + (size_t)done * h->dim, h->stage.p, (size_t)m * h->dim * sizeof(float),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MLVDB_OK;
    });
}

int mlvdb_index_get_rows_at(mlvdb_index* h, const int64_t* labels, int64_t n, float* out_rows) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (n < 0 || (n > 0 && (!labels || !out_rows))) return fail(h, MLVDB_ERR_INVALID_ARG, "bad labels / n / out_rows");
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] < 0 || labels[i] >= h->total) return fail(h, MLVDB_ERR_INVALID_ARG, "label out of range");
    // Own stream and buffers: rows are immutable once appended, so this may overlap a search that another host thread
    // has in flight on h->stream (QueryProcessor.find_similar_stream enriches wave i while wave i+1 is scanned).
    hipStream_t s = h->aux_stream;
    std::lock_guard<std::mutex> aux_lock(h->aux_mutex);
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(64u << 20) / ((int64_t)h->dim * 4));
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        HIP_TRY(h, h->gather_out.ensure((size_t)m * h->dim * sizeof(float)));
        HIP_TRY(h, h->gather_lab.ensure((size_t)m * sizeof(int64_t)));
        HIP_TRY(h, hipMemcpyAsync(h->gather_lab.p, labels + done, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, launch_gather_rows_at(h->X, h->gather_out.as<float>(), h->gather_lab.as<int64_t>(), m, h->dim, h->ld, s));
        HIP_TRY(h, hipMemcpyAsync(out_rows + (size_t)done * h->dim, h->gather_out.p, (size_t)m * h->dim * sizeof(float),
                                  hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return MLVDB_OK;
    });
}

static int search_device_impl(mlvdb_index* h, const float* queries_device, int64_t nq, int32_t k,
                              int64_t* out_labels_device, float* out_dist_device, int32_t* out_counts_device,
                              double* out_dist64_device, void* stream, bool defer_fallback);

int mlvdb_search_batch_device(mlvdb_index* h, const float* queries_device, int64_t nq, int32_t k,
                              int64_t* out_labels_device, float* out_dist_device, int32_t* out_counts_device,
                              double* out_dist64_device, void* stream) {
    return guarded(h, [&]() -> int {
    return search_device_impl(h, queries_device, nq, k, out_labels_device, out_dist_device, out_counts_device,
                              out_dist64_device, stream, false);
    });
}

static int search_device_impl(mlvdb_index* h, const float* queries_device, int64_t nq, int32_t k,
                              int64_t* out_labels_device, float* out_dist_device, int32_t* out_counts_device,
                              double* out_dist64_device, void* stream, bool defer_fallback) {
    int rc = check_handle(h);
    if (rc) return rc;
    h->deferred = false;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max_paged(h, k)) return rc;
    if (nq == 0) return MLVDB_OK;
    if (!queries_device || !out_labels_device || !out_dist_device || !out_counts_device)
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the caller's default (null) stream
    rc = begin_call(h, s);
    if (rc) return rc;
    if (h->total == 0 || h->total == h->deleted) {
        fill_empty_kernel<<<(unsigned)((nq * k + 255) / 256), 256, 0, s>>>(out_labels_device, out_dist_device,
                                                                            out_counts_device, out_dist64_device, nq, k);
        HIP_TRY(h, hipGetLastError());
        return end_call(h, s);
    }
    HIP_TRY(h, h->qpad.ensure((size_t)nq * h->ld * sizeof(float)));
    HIP_TRY(h, h->qaux.ensure((size_t)nq * sizeof(double)));
    if (!h->counters_pending) HIP_TRY(h, hipMemsetAsync(h->counters.p, 0, 32, s));
    h->counters_stream = s;
    HIP_TRY(h, h->qerr.ensure((size_t)nq * sizeof(float)));
    bool ready = false;
    rc = filter_ready(h, s, nq, &ready);
    if (rc) return rc;
    // the route of the call, decided once: top_k <= 64 on the filter path or the exact scan; above, big-k filter passes
    // (top_k 65..1024: passes of 256 queries with 65,536-slot lists, mid bounds, exact rescoring of the survivors) or
    // rank-ordered pages of the exact scan
    enum { kRouteBigK, kRoutePaged, kRouteFilter, kRouteExact } route;
    const bool filt = use_filter(h, nq, ready);
    if (k > MLVDB_MAX_TOPK)
        route = k <= kBigKMax && h->tn.bigk && filt && h->total - h->deleted > (int64_t)k ? kRouteBigK : kRoutePaged;
    else
        route = filt ? kRouteFilter : kRouteExact;
    if (route == kRouteBigK) {
        h->counters_pending = true;
        for (int64_t q0 = 0; q0 < nq; q0 += kFilterQueries) {
            const int32_t n = (int32_t)std::min<int64_t>(kFilterQueries, nq - q0);
            bool handled = false;
            rc = run_bigk_pass(h, s, queries_device, (int32_t)q0, n, k, out_labels_device, out_dist_device, out_counts_device,
                               out_dist64_device, &handled);
            if (rc) return rc;
            // the one decision left to a pass: the first one found no mid shadow (L2_SHADOW=0, or HBM was full when it was
            // wanted) and did nothing, so the paged exact scan serves the whole call
            if (!handled) {
                route = kRoutePaged;
                break;
            }
        }
    }
    if (route == kRoutePaged || route == kRouteExact)  // (the filter passes prepare their own queries: one fused launch each)
        HIP_TRY(h, launch_query_prep(queries_device, (int32_t)nq, h->dim, h->ld, h->space, h->qpad.as<float>(),
                                     h->qaux.as<double>(), h->qerr.as<float>(), s));
    h->stats.strategy_used = route == kRouteBigK || route == kRouteFilter ? MLVDB_STRATEGY_FILTER : MLVDB_STRATEGY_EXACT;
    if (route == kRoutePaged) {
        rc = run_paged_exact(h, s, h->qpad.as<float>(), h->qaux.as<double>(), nq, nullptr, (int32_t)nq, k, out_labels_device,
                             out_dist_device, out_counts_device, out_dist64_device);
        if (rc) return rc;
    } else if (route == kRouteFilter) {
        h->counters_pending = true;
        for (int64_t q0 = 0; q0 < nq; q0 += kFilterQueries) {
            const int32_t n = (int32_t)std::min<int64_t>(kFilterQueries, nq - q0);
            rc = run_filter_pass(h, s, queries_device, (int32_t)q0, n, k, out_labels_device, out_dist_device, out_counts_device,
                                 out_dist64_device, defer_fallback && nq <= kFilterQueries);
            if (rc) return rc;
        }
    } else if (route == kRouteExact) {
        rc = run_exact(h, s, h->qpad.as<float>(), h->qaux.as<double>(), (int32_t)nq, nullptr, h->total, k,
                       out_labels_device, out_dist_device, out_counts_device, out_dist64_device, true);
        if (rc) return rc;
    }
    return end_call(h, s);
}

namespace {
int search_host(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int64_t* out_labels, float* out_dist,
                int32_t* out_counts, double* out_dist64) {
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max_paged(h, k)) return rc;
    if (nq == 0) return MLVDB_OK;
    if (!queries || !out_labels || !out_dist || !out_counts) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    // queries: user memory -> pinned staging -> device (one DMA); outputs: ONE device buffer [d64 | labels | dist | counts]
    // -> one DMA into pinned memory -> user arrays
    const size_t qbytes = (size_t)nq * h->dim * sizeof(float);
    const size_t b64 = out_dist64 ? (size_t)nq * k * sizeof(double) : 0, blab = (size_t)nq * k * sizeof(int64_t);
    const size_t bdist = (size_t)nq * k * sizeof(float), bcnt = (size_t)nq * sizeof(int32_t);
    const size_t obytes = b64 + blab + bdist + bcnt;
    HIP_TRY(h, h->io_q.ensure(qbytes));
    const size_t fbytes = kFilterQueries * sizeof(uint32_t), obytes_all = ((obytes + 15) & ~(size_t)15) + fbytes;
    HIP_TRY(h, h->io_out.ensure(obytes_all));
    char* dout = h->io_out.as<char>();
    double* d_d64 = out_dist64 ? reinterpret_cast<double*>(dout) : nullptr;
    int64_t* d_lab = reinterpret_cast<int64_t*>(dout + b64);
    float* d_dist = reinterpret_cast<float*>(dout + b64 + blab);
    int32_t* d_cnt = reinterpret_cast<int32_t*>(dout + b64 + blab + bdist);
    // Pinned staging.  The pinned D2H copy is enqueued only AFTER the kernels have
    // finished (one more host wait, ~10 us): enqueued behind them it parks at the head of the copy engine's queue for the
    // whole scan and every copy of the index's other stream -- the hit-enrichment gather of find_similar_stream -- waits
    // with it; measured on 4M rows: protocol stream 1.92 ms per wave parked vs 1.20 unparked (engine alone 1.07;
    // profiles/r03/protocol_stream_pinned_io_modes_4m.txt).  A blocking event wait instead of hipStreamSynchronize: no change.
    // (pinned staging only while it stays small: a paged search with nq = 1024, k = 16384 would pin ~400 MB per handle -- per
    // shard under MultiDeviceEngine -- for the handle's lifetime, and every growth goes through hipHostFree / hipHostMalloc,
    // which synchronise the device; above 16 MB pageable copies are used and nothing stays pinned)
    constexpr size_t kPinnedMax = (size_t)16 << 20;
    const bool pinned = qbytes <= kPinnedMax && obytes_all <= kPinnedMax;
    h->flags_in_out = pinned;  // the pass copies its overflow flags device-to-device behind the outputs (no parked D2H either)
    h->flags_out = reinterpret_cast<uint32_t*>(dout + ((obytes + 15) & ~(size_t)15));
    if (pinned) {
        HIP_TRY(h, h->pin_in.ensure(qbytes));
        HIP_TRY(h, h->pin_out.ensure(obytes_all));
        std::memcpy(h->pin_in.p, queries, qbytes);
        HIP_TRY(h, hipMemcpyAsync(h->io_q.p, h->pin_in.p, qbytes, hipMemcpyHostToDevice, h->stream));
    } else {
        HIP_TRY(h, hipMemcpyAsync(h->io_q.p, queries, qbytes, hipMemcpyHostToDevice, h->stream));
    }
    int rc = search_device_impl(h, h->io_q.as<float>(), nq, k, d_lab, d_dist, d_cnt, d_d64, h->stream, true);
    if (rc) return rc;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (pinned) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));  // the copy must not park behind the kernels (see above)
            HIP_TRY(h, hipMemcpyAsync(h->pin_out.p, dout, obytes_all, hipMemcpyDeviceToHost, h->stream));
        } else {  // pageable copies straight into the caller's arrays
            if (out_dist64) HIP_TRY(h, hipMemcpyAsync(out_dist64, d_d64, b64, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(out_labels, d_lab, blab, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(out_dist, d_dist, bdist, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(out_counts, d_cnt, bcnt, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->deferred) {
            // the pass left the overflow decision to us (run_filter_pass, defer_fallback): usually nothing is flagged
            h->deferred = false;
            int32_t sel[kFilterQueries];
            int32_t n = 0;
            const uint32_t* flags = pinned ? reinterpret_cast<const uint32_t*>(static_cast<const char*>(h->pin_out.p) + ((obytes + 15) & ~(size_t)15))
                                           : h->host_flags;
            for (int q = 0; q < (int)nq; ++q)
                if (flags[q]) sel[n++] = q;
            if (n > 0) {
                h->host_fallbacks += n;
                const FilterArgs& fa = h->deferred_fa;
                HIP_TRY(h, hipMemcpyAsync(h->qsel.p, sel, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
                HIP_TRY(h, hipStreamSynchronize(h->stream));  // `sel` is on this stack frame
                rc = run_exact(h, h->stream, fa.Qpad, fa.qaux, n, h->qsel.as<int32_t>(), h->total, k, d_lab, d_dist, d_cnt, d_d64,
                               false);
                if (rc) return rc;
                continue;  // copy the corrected outputs
            }
        }
        if (!pinned) break;
        const char* po = static_cast<const char*>(h->pin_out.p);
        if (out_dist64) std::memcpy(out_dist64, po, b64);
        std::memcpy(out_labels, po + b64, blab);
        std::memcpy(out_dist, po + b64 + blab, bdist);
        std::memcpy(out_counts, po + b64 + blab + bdist, bcnt);
        break;
    }
    return MLVDB_OK;
}
}  // namespace

extern "C++" {
namespace {
// A filtered call: h->row_mask holds its row mask (h->total bytes, on the device).  For the duration of `call` the index's
// norms -- and, when the int8 shadow serves the call, its row pairs -- are swapped for masked copies, so a masked-out row
// looks tombstoned to every kernel the call reaches (seeding, bounds, mid prune, rescoring, exact and paged fallbacks).
template <class F>
int with_row_mask(mlvdb_index* h, int64_t nq, F&& call) {
    HIP_TRY(h, h->rn_masked.ensure((size_t)h->capacity * sizeof(float)));
    HIP_TRY(h, launch_mask_norms(h->rn, h->row_mask.as<uint8_t>(), h->rn_masked.as<float>(), h->total, h->capacity, h->stream));
    // the int8 shadow serves masked searches too: bring it up to date with the index's own norms, then mask a copy of its
    // row pairs (8 bytes per row) exactly like the norms
    h->mask_pairs_ready = false;
    if (i8_eligible(h) && h->strategy != MLVDB_STRATEGY_EXACT && use_filter(h, nq, true)) {  // (not for a call the exact scan takes)
        int rc = update_i8_shadow(h, h->stream);
        if (rc) return rc;
        HIP_TRY(h, h->rp8_masked.ensure((size_t)h->capacity * (h->space == kSpaceL2 ? 3 : 2) * sizeof(float)));
        HIP_TRY(h, launch_mask_pairs(h->rp8.as<float>(), h->row_mask.as<uint8_t>(), h->rp8_masked.as<float>(), h->total,
                                     h->capacity, h->space == kSpaceL2 ? 1 : 0, h->stream));
        rc = forget_l2_offsets(h, 1, h->stream);
        if (rc) return rc;
        h->mask_pairs_ready = true;
    }
    float* const all_rows = h->rn;  // every kernel of the call reads the masked norms instead
    h->rn = h->rn_masked.as<float>();
    h->mask_active = true;
    const int rc = call();
    h->rn = all_rows;
    h->mask_active = false;
    h->mask_pairs_ready = false;
    return rc;
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_ex(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const uint8_t* row_mask,
                          int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (!row_mask || h->total == 0) return search_host(h, queries, nq, k, out_labels, out_dist, out_counts, out_dist64);
    HIP_TRY(h, h->row_mask.ensure((size_t)h->total));
    HIP_TRY(h, hipMemcpyAsync(h->row_mask.p, row_mask, (size_t)h->total, hipMemcpyHostToDevice, h->stream));
    return with_row_mask(h, nq, [&]() { return search_host(h, queries, nq, k, out_labels, out_dist, out_counts, out_dist64); });
    });
}

int mlvdb_search_batch(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int64_t* out_labels,
                       float* out_dist, int32_t* out_counts) {
    return guarded(h, [&]() -> int {
    return mlvdb_search_batch_ex(h, queries, nq, k, nullptr, out_labels, out_dist, out_counts, nullptr);
    });
}

int mlvdb_search_batch_filtered(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const uint8_t* row_mask,
                                int64_t* out_labels, float* out_dist, int32_t* out_counts) {
    return guarded(h, [&]() -> int {
    return mlvdb_search_batch_ex(h, queries, nq, k, row_mask, out_labels, out_dist, out_counts, nullptr);
    });
}

// The valid prefixes of the dense device results (io_lab / io_dist: cap_eff slots per query) packed at `offsets` into one
// device buffer [labels | distances] and brought to the host in one DMA through pinned memory; *labels / *dist point at them
// there.  Pinned staging only while it stays small (search_host): above 16 MB a caller whose own arrays have the packed
// layout (direct_lab / direct_dist; nullptr: none) gets pageable copies straight into those instead.
static int pack_range_hits(mlvdb_index* h, hipStream_t s, int64_t nq, int64_t cap_eff, const std::vector<int64_t>& offsets,
                           int64_t* direct_lab, float* direct_dist, const int64_t** labels, const float** dist) {
    const size_t plab = (size_t)offsets[(size_t)nq] * sizeof(int64_t), pdst = (size_t)offsets[(size_t)nq] * sizeof(float);
    HIP_TRY(h, h->labels_in.ensure(((size_t)nq + 1) * sizeof(int64_t)));
    HIP_TRY(h, h->seed_lab.ensure(plab + pdst));
    const bool pinned = !direct_lab || plab + pdst <= ((size_t)16 << 20);
    if (pinned) HIP_TRY(h, h->pin_out.ensure(plab + pdst));
    int64_t* d_pl = h->seed_lab.as<int64_t>();
    float* d_pd = reinterpret_cast<float*>(h->seed_lab.as<char>() + plab);
    std::memcpy(h->pin_in.p, offsets.data(), ((size_t)nq + 1) * sizeof(int64_t));
    HIP_TRY(h, hipMemcpyAsync(h->labels_in.p, h->pin_in.p, ((size_t)nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    range_pack_kernel<<<(unsigned)nq, 256, 0, s>>>(h->io_lab.as<int64_t>(), h->io_dist.as<float>(), h->labels_in.as<int64_t>(),
                                                   cap_eff, d_pl, d_pd);
    HIP_TRY(h, hipGetLastError());
    if (pinned) {
        HIP_TRY(h, hipMemcpyAsync(h->pin_out.p, d_pl, plab + pdst, hipMemcpyDeviceToHost, s));
        *labels = static_cast<const int64_t*>(h->pin_out.p);
        *dist = reinterpret_cast<const float*>(static_cast<const char*>(h->pin_out.p) + plab);
    } else {
        HIP_TRY(h, hipMemcpyAsync(direct_lab, d_pl, plab, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(direct_dist, d_pd, pdst, hipMemcpyDeviceToHost, s));
        *labels = direct_lab;
        *dist = direct_dist;
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return MLVDB_OK;
}

// The range passes of a call (between its begin_call and end_call; the index holds live rows, nq >= 1): the ranked hits of
// query i -- its nearest min(count, cap_eff) -- are left on the device in rows i of h->io_lab / h->io_dist (cap_eff slots each),
// counts[i] is its exact hit count and offsets ([nq + 1]) the packed layout of the returned hits.
// queries == nullptr: the caller has left them on the device, dense in h->io_q (at least nq * dim floats, written on `s`).
// row_begin: the caller knows that no row below it can be a hit (the join has masked them out): the filter scan starts at
// that row's tile; every other kernel of the chain sees all rows.
static int range_ranked(mlvdb_index* h, hipStream_t s, const float* queries, int64_t nq, float radius, int64_t cap_eff,
                        std::vector<int64_t>& counts, std::vector<int64_t>& offsets, int64_t row_begin = 0) {
    int rc = MLVDB_OK;
    HIP_TRY(h, h->io_q.ensure((size_t)nq * h->dim * sizeof(float)));
    HIP_TRY(h, h->qpad.ensure((size_t)nq * h->ld * sizeof(float)));
    HIP_TRY(h, h->qaux.ensure((size_t)nq * sizeof(double)));
    HIP_TRY(h, h->io_lab.ensure((size_t)nq * cap_eff * sizeof(int64_t)));
    HIP_TRY(h, h->io_dist.ensure((size_t)nq * cap_eff * sizeof(float)));
    HIP_TRY(h, h->io_cnt.ensure((size_t)nq * sizeof(int64_t)));
    HIP_TRY(h, h->pin_in.ensure(std::max((size_t)nq * h->dim * sizeof(float), ((size_t)nq + 1) * sizeof(int64_t))));
    if (queries) {
        std::memcpy(h->pin_in.p, queries, (size_t)nq * h->dim * sizeof(float));  // pinned staging: one DMA (search_host)
        HIP_TRY(h, hipMemcpyAsync(h->io_q.p, h->pin_in.p, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, h->qerr.ensure((size_t)nq * sizeof(float)));
    bool ready = false;
    rc = filter_ready(h, s, nq, &ready);
    if (rc) return rc;
    const bool filt = use_filter(h, nq, ready);
    if (!filt)  // (the filter passes prepare their own queries: one fused launch each)
        HIP_TRY(h, launch_query_prep(h->io_q.as<float>(), (int32_t)nq, h->dim, h->ld, h->space, h->qpad.as<float>(),
                                     h->qaux.as<double>(), h->qerr.as<float>(), s));
    h->stats.strategy_used = filt ? MLVDB_STRATEGY_FILTER : MLVDB_STRATEGY_EXACT;
    for (int64_t q0 = 0; q0 < nq; q0 += kFilterQueries) {
        const int32_t n = (int32_t)std::min<int64_t>(kFilterQueries, nq - q0);
        // int8 bounds wherever the filter serves the pass (half the scan time of the bf16 body): their band admits ~8x more
        // candidates than there are hits, which the mid bounds and the flat rescoring below absorb
        FilterArgs fa{};
        if (filt) {  // (also clears the candidate counters)
            rc = begin_pass(h, s, fa, h->io_q.as<float>(), (int32_t)q0, n, true);
            if (rc) return rc;
        } else {
            rc = setup_filter_ws(h, fa, (int32_t)q0, n, true);
            if (rc) return rc;
            HIP_TRY(h, launch_filter_state(fa, s));  // per-query state only (no image: the exact range scan reads Qpad)
            h->stats.bound_dtype = 0;
        }
        rc = scan_step(h, s, filt ? h->total - row_begin : h->total, [&]() -> hipError_t {
            if (!filt) return launch_exact_range_scan(fa, radius, nullptr, 0, s);
            const hipError_t e = launch_filter_range_thr(fa, radius, s);
            return e != hipSuccess ? e : launch_filter_scan(fa, row_begin, h->total, s);
        });
        if (rc) return rc;
        int32_t n_flagged = 0;
        rc = collect_overflow(h, s, fa, &n_flagged);
        if (rc) return rc;
        if (n_flagged) {
            // more candidates than list slots (or a wave buffer overflowed): the exact range scan restricted to those
            // queries stores exactly their hits; a list that now fits is complete, larger ones stay flagged
            h->stats.fallback_queries += n_flagged;
            const int32_t* qsel = h->qsel.as<int32_t>();
            range_reset_kernel<<<1, n_flagged, 0, s>>>(fa.cnt, qsel);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, launch_exact_range_scan(fa, radius, qsel, n_flagged, s));
            range_resolve_kernel<<<1, n_flagged, 0, s>>>(fa.overflow, fa.thr, fa.cnt, qsel, (uint32_t)fa.cand_cap);
            HIP_TRY(h, hipGetLastError());
        }
        // mid bounds first (round 4): the int8 band admits ~8x the hits; a pass over the candidates' fp16 rows (whole 128-byte
        // lines, half the bytes of the fp32 rows) prunes it to ~1.01x, so the exact gather below touches (nearly) only hits
        if (filt && h->tn.range_l2) {
            MidArgs m{};
            rc = attach_mid(h, s, &m);
            if (rc) return rc;
            if (m.X16) {
                HIP_TRY(h, launch_mid_score(fa, m, s));
                HIP_TRY(h, launch_bigk_thr_prune(fa, m, 0, -1, s));
            }
        }
        // exact fp64 distance of every candidate (blocks over query x candidate chunk), then sort + emit per query
        HIP_TRY(h, launch_range_rescore(fa, radius, (int32_t)q0, cap_eff, h->io_lab.as<int64_t>(),
                                        h->io_dist.as<float>(), h->io_cnt.as<int64_t>(), s));
        // queries with more hits than one block sorts (> kCandCap), or more than a list holds: their nearest
        // min(count, capacity) hits come from the paged exact kNN; cnt[q] holds the exact count in both cases
        int32_t n_still = 0;
        rc = collect_overflow(h, s, fa, &n_still);
        if (rc) return rc;
        if (n_still) {
            const int32_t* qsel = h->qsel.as<int32_t>();
            HIP_TRY(h, hipMemcpyAsync(h->host_flags, fa.cnt, kFilterQueries * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
            int64_t kmax = 1;
            for (int q = 0; q < n; ++q)
                if (h->host_overflow[q]) kmax = std::max<int64_t>(kmax, std::min<int64_t>(h->host_flags[q], cap_eff));
            if (n_flagged == 0) h->stats.fallback_queries += n_still;
            HIP_TRY(h, h->seed_lab.ensure((size_t)kFilterQueries * kmax * sizeof(int64_t)));
            HIP_TRY(h, h->seed_dist.ensure((size_t)kFilterQueries * kmax * sizeof(float)));
            HIP_TRY(h, h->seed_cnt.ensure(kFilterQueries * sizeof(int32_t)));
            rc = run_paged_exact(h, s, fa.Qpad, fa.qaux, kFilterQueries, qsel, n_still, (int32_t)kmax,
                                 h->seed_lab.as<int64_t>(), h->seed_dist.as<float>(), h->seed_cnt.as<int32_t>(), nullptr);
            if (rc) return rc;
            range_fallback_commit_kernel<<<n_still, 256, 0, s>>>(qsel, fa.cnt, h->seed_lab.as<int64_t>(),
                                                                 h->seed_dist.as<float>(), (int32_t)kmax, (int32_t)q0, cap_eff,
                                                                 h->io_lab.as<int64_t>(), h->io_dist.as<float>(),
                                                                 h->io_cnt.as<int64_t>());
            HIP_TRY(h, hipGetLastError());
        }
    }
    // the exact counts, and where each query's returned hits go in a packed array
    HIP_TRY(h, h->pin_out.ensure((size_t)nq * sizeof(int64_t)));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, hipMemcpyAsync(h->pin_out.p, h->io_cnt.p, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    counts.assign(static_cast<const int64_t*>(h->pin_out.p), static_cast<const int64_t*>(h->pin_out.p) + nq);
    offsets.assign((size_t)nq + 1, 0);
    for (int64_t i = 0; i < nq; ++i) offsets[(size_t)i + 1] = offsets[(size_t)i] + std::min<int64_t>(std::max<int64_t>(counts[i], 0), cap_eff);
    return MLVDB_OK;
}

// Both range entries.  out_offsets == nullptr: the dense form (out_labels / out_dist are [nq, capacity]); otherwise the packed
// form: the hits of query i are entries out_offsets[i] .. out_offsets[i + 1] of out_labels / out_dist (total_capacity entries).
static int range_batch_impl(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity, int64_t* out_labels,
                            float* out_dist, int64_t* out_counts, int64_t* out_offsets, int64_t total_capacity, bool packed) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (packed && !out_offsets) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_nq(h, nq)) return rc;
    if (capacity < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "capacity must be >= 1");
    if (out_offsets && total_capacity < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "total_capacity must be >= 0");
    if (nq == 0) {
        if (out_offsets) out_offsets[0] = 0;
        return MLVDB_OK;
    }
    if (!queries || !out_counts || ((!out_labels || !out_dist) && (!out_offsets || total_capacity > 0)))
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    hipStream_t s = h->stream;
    rc = begin_call(h, s);
    if (rc) return rc;
    if (h->total == 0 || h->total == h->deleted) {
        for (int64_t i = 0; i < nq; ++i) out_counts[i] = 0;
        if (out_offsets)
            for (int64_t i = 0; i <= nq; ++i) out_offsets[i] = 0;
        return end_call(h, s);
    }
    const int64_t cap_eff = std::min<int64_t>(capacity, MLVDB_MAX_TOPK_PAGED);  // most hits returned per query
    std::vector<int64_t> counts, offsets;
    rc = range_ranked(h, s, queries, nq, radius, cap_eff, counts, offsets);
    if (rc) return rc;
    // copy back.  Hit counts vary by orders of magnitude between queries, so the dense [nq, cap_eff] device
    // arrays are mostly padding: when the hits are a small part of them, pack the rows' valid prefixes on the
    // device and send only those (25 MB -> 0.4 MB at 256 queries x 8192 slots with 128 hits on average).
    const int64_t total_hits = offsets[(size_t)nq];
    bool over = false, hard = false;
    for (int64_t i = 0; i < nq; ++i) {
        out_counts[i] = counts[i];
        over |= counts[i] > capacity;
        hard |= counts[i] > cap_eff && capacity > cap_eff;
    }
    const size_t plab = (size_t)total_hits * sizeof(int64_t), pdst = (size_t)total_hits * sizeof(float);
    const int64_t* pl = nullptr;
    const float* pd = nullptr;
    bool fits = true;
    if (out_offsets) {
        // packed form: offsets and counts always; the hits when they fit (pageable copies straight into the caller's arrays
        // when they are too many for the pinned staging)
        std::memcpy(out_offsets, offsets.data(), ((size_t)nq + 1) * sizeof(int64_t));
        fits = total_hits <= total_capacity;
        if (fits && total_hits > 0) {
            rc = pack_range_hits(h, s, nq, cap_eff, offsets, out_labels, out_dist, &pl, &pd);
            if (rc) return rc;
            if (pl != out_labels) {
                std::memcpy(out_labels, pl, plab);
                std::memcpy(out_dist, pd, pdst);
            }
        }
    } else if (total_hits * 4 < nq * cap_eff) {
        if (total_hits > 0) {
            rc = pack_range_hits(h, s, nq, cap_eff, offsets, nullptr, nullptr, &pl, &pd);
            if (rc) return rc;
            for (int64_t i = 0; i < nq; ++i) {
                const int64_t n = offsets[(size_t)i + 1] - offsets[(size_t)i];
                std::memcpy(out_labels + (size_t)i * capacity, pl + offsets[(size_t)i], (size_t)n * sizeof(int64_t));
                std::memcpy(out_dist + (size_t)i * capacity, pd + offsets[(size_t)i], (size_t)n * sizeof(float));
            }
        }
    } else {
        HIP_TRY(h, hipMemcpy2DAsync(out_labels, (size_t)capacity * sizeof(int64_t), h->io_lab.p, (size_t)cap_eff * sizeof(int64_t),
                                    (size_t)cap_eff * sizeof(int64_t), (size_t)nq, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpy2DAsync(out_dist, (size_t)capacity * sizeof(float), h->io_dist.p, (size_t)cap_eff * sizeof(float),
                                    (size_t)cap_eff * sizeof(float), (size_t)nq, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    rc = end_call(h, s);
    if (rc) return rc;
    if (!fits)
        return fail(h, MLVDB_ERR_OVERFLOW, "range query: more hits in all than total_capacity; out_counts / out_offsets hold "
                                           "the exact counts and the layout the hits need, out_labels / out_dist nothing");
    if (hard)
        return fail(h, MLVDB_ERR_UNSUPPORTED,
                    "range query: a query has more than MLVDB_MAX_TOPK_PAGED hits; out_counts holds the exact counts, the "
                    "outputs the nearest MLVDB_MAX_TOPK_PAGED");
    if (over) return fail(h, MLVDB_ERR_OVERFLOW, "some query has more hits than `capacity`; out_counts holds the exact counts");
    return MLVDB_OK;
}

int mlvdb_range_batch(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity,
                      int64_t* out_labels, float* out_dist, int64_t* out_counts) {
    return guarded(h, [&]() -> int {
    return range_batch_impl(h, queries, nq, radius, capacity, out_labels, out_dist, out_counts, nullptr, 0, false);
    });
}

int mlvdb_range_batch_packed(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity,
                             int64_t total_capacity, int64_t* out_labels, float* out_dist, int64_t* out_offsets,
                             int64_t* out_counts) {
    return guarded(h, [&]() -> int {
    return range_batch_impl(h, queries, nq, radius, capacity, out_labels, out_dist, out_counts, out_offsets, total_capacity, true);
    });
}

int mlvdb_pair_distances(mlvdb_index* h, const float* queries, int64_t nq, const int64_t* labels, int64_t m,
                         double* out_dist64, float* out_dist) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (nq < 0 || nq > (1 << 24) || m < 0 || m > (1 << 24)) return fail(h, MLVDB_ERR_INVALID_ARG, "nq / m out of range");
    if (nq == 0 || m == 0) return MLVDB_OK;
    if (!queries || !labels || !out_dist64) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    for (int64_t i = 0; i < nq * m; ++i)
        if (labels[i] >= h->total) return fail(h, MLVDB_ERR_INVALID_ARG, "label out of range");
    hipStream_t s = h->aux_stream;  // rows are immutable once appended: may overlap a search in flight on h->stream
    std::lock_guard<std::mutex> aux_lock(h->aux_mutex);
    // private buffers of the auxiliary stream (gather_out / gather_lab) + query staging of its own
    const size_t qbytes = (size_t)nq * h->dim * sizeof(float), pbytes = (size_t)nq * h->ld * sizeof(float);
    const size_t abytes = (size_t)nq * sizeof(double), o64 = (size_t)nq * m * sizeof(double), o32 = (size_t)nq * m * sizeof(float);
    HIP_TRY(h, h->gather_lab.ensure((size_t)nq * m * sizeof(int64_t)));
    HIP_TRY(h, h->gather_out.ensure(qbytes + pbytes + abytes + o64 + o32 + 64));
    char* base = h->gather_out.as<char>();
    double* d_o64 = reinterpret_cast<double*>(base);  // 8-byte aligned pieces first
    double* d_aux = reinterpret_cast<double*>(base + o64);
    float* d_pad = reinterpret_cast<float*>(base + o64 + abytes);
    float* d_q = reinterpret_cast<float*>(base + o64 + abytes + pbytes);
    float* d_o32 = reinterpret_cast<float*>(base + o64 + abytes + pbytes + qbytes);
    HIP_TRY(h, hipMemcpyAsync(d_q, queries, qbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->gather_lab.p, labels, (size_t)nq * m * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_query_prep(d_q, (int32_t)nq, h->dim, h->ld, h->space, d_pad, d_aux, nullptr, s));
    HIP_TRY(h, launch_pair_distances(h->X, d_pad, d_aux, h->gather_lab.as<int64_t>(), (int32_t)nq, (int32_t)m, h->ld, h->space,
                                     d_o64, out_dist ? d_o32 : nullptr, s));
    HIP_TRY(h, hipMemcpyAsync(out_dist64, d_o64, o64, hipMemcpyDeviceToHost, s));
    if (out_dist) HIP_TRY(h, hipMemcpyAsync(out_dist, d_o32, o32, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MLVDB_OK;
    });
}

int mlvdb_index_set_strategy(mlvdb_index* h, int32_t strategy) {
    return guarded(h, [&]() -> int {
    if (!h) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "null index handle");
    if (strategy < 0 || strategy > 2) return fail(h, MLVDB_ERR_INVALID_ARG, "unknown strategy");
    if (strategy == MLVDB_STRATEGY_FILTER && !filter_supported(h->ld) && h->ld8 == 0)
        return fail(h, MLVDB_ERR_UNSUPPORTED, "filter strategy needs an index created with a shadow (NO_SHADOW / I8_PAD=0 took it away)");
    h->strategy = strategy;
    return MLVDB_OK;
    });
}

int mlvdb_index_set_tuning(mlvdb_index* h, const char* assignment) {
    return guarded(h, [&]() -> int {
    if (!h) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "null index handle");
    const char* eq = assignment ? strchr(assignment, '=') : nullptr;
    if (!eq || eq == assignment) return fail(h, MLVDB_ERR_INVALID_ARG, "tuning assignment must be KEY=VALUE");
    const TuningField* f = find_tuning_field(assignment, (size_t)(eq - assignment));
    if (!f) return fail(h, MLVDB_ERR_INVALID_ARG, "unknown tuning key");
    if (!strcmp(f->name, "NO_SHADOW") || !strcmp(f->name, "SHADOW_BF16") || !strcmp(f->name, "I8_PAD"))
        return fail(h, MLVDB_ERR_UNSUPPORTED, "creation-time knob: set MLVDB_<KEY> in the environment before mlvdb_index_create");
    char* end = nullptr;
    const long v = strtol(eq + 1, &end, 10);
    if (end == eq + 1 || *end != '\0') return fail(h, MLVDB_ERR_INVALID_ARG, "tuning value must be an integer");
    h->tn.*(f->field) = (int)v;
    return MLVDB_OK;
    });
}

int mlvdb_index_get_tuning(const mlvdb_index* h, const char* key, int32_t* value) {
    return guarded(const_cast<mlvdb_index*>(h), [&]() -> int {
    if (!h) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "null index handle");
    if (!key || !value) return fail(const_cast<mlvdb_index*>(h), MLVDB_ERR_INVALID_ARG, "null key / value");
    const TuningField* f = find_tuning_field(key, strlen(key));
    if (!f) return fail(const_cast<mlvdb_index*>(h), MLVDB_ERR_INVALID_ARG, "unknown tuning key");
    *value = h->tn.*(f->field);
    return MLVDB_OK;
    });
}

int mlvdb_index_set_profiling(mlvdb_index* h, int32_t enabled) {
    return guarded(h, [&]() -> int {
    if (!h) return fail(nullptr, MLVDB_ERR_INVALID_ARG, "null index handle");
    h->profiling = enabled != 0;
    return MLVDB_OK;
    });
}

int mlvdb_index_last_stats(mlvdb_index* h, mlvdb_stats* out) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (!out) return fail(h, MLVDB_ERR_INVALID_ARG, "out is null");
    if (h->counters_pending) {
        unsigned long long c[2] = {0, 0};
        HIP_TRY(h, hipMemcpyAsync(c, h->counters.p, sizeof c, hipMemcpyDeviceToHost, h->counters_stream));
        HIP_TRY(h, hipStreamSynchronize(h->counters_stream));
        h->stats.candidates_rescored = (int64_t)c[0];
        h->stats.fallback_queries = (int64_t)c[1];
        h->counters_pending = false;
    }
    if (h->stats_pending) {
        HIP_TRY(h, hipEventSynchronize(h->total_events[1]));
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->total_events[0], h->total_events[1]));
        h->stats.total_ms = ms;
        double scan = 0.0;
        for (size_t i = 0; i < h->scan_events_used; ++i) {
            HIP_TRY(h, hipEventElapsedTime(&ms, h->scan_events[i].first, h->scan_events[i].second));
            scan += ms;
        }
        h->stats.scan_ms = scan;
        h->stats_pending = false;
    }
    h->stats.fallback_queries += h->host_fallbacks;  // fallbacks decided on the host (search_host)
    h->host_fallbacks = 0;
    *out = h->stats;
    // reset: the next call starts a new accumulation window
    const int32_t strategy = h->stats.strategy_used;
    h->stats = mlvdb_stats{};
    h->stats.strategy_used = strategy;
    h->scan_events_used = 0;
    return MLVDB_OK;
    });
}

namespace {
// ---- metadata filters (mlvdb_where.h)
int attr_check(mlvdb_index* h, int32_t attr) {
    if (attr < 0 || attr >= MLVDB_MAX_ATTRS) return fail(h, MLVDB_ERR_INVALID_ARG, "attribute index out of range");
    if (!h->attr_type[attr]) return fail(h, MLVDB_ERR_INVALID_ARG, "attribute not defined");
    return MLVDB_OK;
}

// ... for the entries that read or write a column's values as scalars: a list column's slots (mlvdb_list.h) are neither
// integers to rank, bin or group by, nor something a raw write may forge; a sparse column's (mlvdb_sparse.h) are the same.
int scalar_check(mlvdb_index* h, int32_t attr) {
    if (h->attr_type[attr] == MLVDB_ATTR_INT64_LIST)
        return fail(h, MLVDB_ERR_INVALID_ARG, "a list column: this entry needs a scalar column (see mlvdb_list.h)");
    if (h->attr_type[attr] == MLVDB_ATTR_SPARSE)
        return fail(h, MLVDB_ERR_INVALID_ARG, "a sparse column: this entry needs a scalar column (see mlvdb_sparse.h)");
    if (h->attr_type[attr] == MLVDB_ATTR_BITS)
        return fail(h, MLVDB_ERR_INVALID_ARG, "a bits column: this entry needs a scalar column (see mlvdb_bits.h)");
    return MLVDB_OK;
}

// ... for the entries that rank, bin or group by a column's values: a geo column's packed points (mlvdb_geo.h) are stored as
// int64 but are no integers to order or count by.
int value_check(mlvdb_index* h, int32_t attr) {
    if (h->attr_type[attr] == MLVDB_ATTR_GEO)
        return fail(h, MLVDB_ERR_INVALID_ARG, "a geo column: this entry needs an int64 or float64 value column (see mlvdb_geo.h)");
    return MLVDB_OK;
}

// ... and for those that need a defined column of one type (`what` says so in the entry's words): a pooled one, or an int64
// one to group or count by.
int typed_attr_check(mlvdb_index* h, int32_t attr, int32_t type, const char* what) {
    if (int rc = attr_check(h, attr)) return rc;
    return h->attr_type[attr] != type ? fail(h, MLVDB_ERR_INVALID_ARG, what) : MLVDB_OK;
}

int int64_attr_check(mlvdb_index* h, int32_t attr, const char* what) {
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = value_check(h, attr)) return rc;
    return h->attr_type[attr] != MLVDB_ATTR_INT64 ? fail(h, MLVDB_ERR_INVALID_ARG, what) : MLVDB_OK;
}

// Values about to be written to a column: on a geo column every non-absent one must be a point inside the ranges.
int geo_values_check(mlvdb_index* h, int32_t attr, const void* values, int64_t n) {
    if (h->attr_type[attr] != MLVDB_ATTR_GEO) return MLVDB_OK;
    const int64_t* v = static_cast<const int64_t*>(values);
    for (int64_t i = 0; i < n; ++i)
        if (v[i] != INT64_MIN && !geo_valid(v[i]))
            return fail(h, MLVDB_ERR_INVALID_ARG, "a geo value outside lat_e7 in [-9e8, 9e8], lon_e7 in [-18e8, 18e8]");
    return MLVDB_OK;
}

// Host validation of a program (stack depth >= 1 throughout and exactly 1 at the end, defined attributes, ops valid for their
// column's type, set ranges inside the table and sorted) -> h->where_ops, the form the kernel reads.  Nothing is launched for a
// program refused here.
int where_prepare(mlvdb_index* h, const mlvdb_where* w) {
    if (!w) return fail(h, MLVDB_ERR_INVALID_ARG, "where is null");
    if (w->n_ops < 1 || w->n_ops > MLVDB_WHERE_MAX_OPS || !w->ops)
        return fail(h, MLVDB_ERR_INVALID_ARG, "a program holds 1..MLVDB_WHERE_MAX_OPS ops");
    if (w->n_set < 0 || (w->n_set > 0 && !w->set)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad set table");
    h->where_ops.resize((size_t)w->n_ops);
    int depth = 0;
    for (int32_t i = 0; i < w->n_ops; ++i) {
        const mlvdb_where_op& o = w->ops[i];
        WhereOp& d = h->where_ops[(size_t)i];
        d = WhereOp{o.op, 0, o.a, o.b, nullptr};
        switch (o.op) {
            case MLVDB_WHERE_AND:
            case MLVDB_WHERE_OR:
                if (depth < 2) return fail(h, MLVDB_ERR_INVALID_ARG, "AND / OR needs two operands on the stack");
                --depth;
                continue;
            case MLVDB_WHERE_NOT:
                if (depth < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "NOT needs an operand on the stack");
                continue;
            case MLVDB_WHERE_TRUE:
                break;
            case MLVDB_WHERE_EQ: case MLVDB_WHERE_NE: case MLVDB_WHERE_LT: case MLVDB_WHERE_LE:
            case MLVDB_WHERE_GT: case MLVDB_WHERE_GE: case MLVDB_WHERE_IN: case MLVDB_WHERE_EXISTS:
                if (int rc = attr_check(h, o.attr)) return rc;
                d.type = h->attr_type[o.attr];
                d.col = h->attr_col[o.attr];
                if (d.type == MLVDB_ATTR_INT64_LIST && o.op != MLVDB_WHERE_EXISTS)
                    return fail(h, MLVDB_ERR_INVALID_ARG, "a list column takes HAS, HAS_ANY, HAS_ALL, LEN and EXISTS only");
                if (d.type == MLVDB_ATTR_GEO && o.op != MLVDB_WHERE_EXISTS)
                    return fail(h, MLVDB_ERR_INVALID_ARG, "a geo column takes GEO_RADIUS, GEO_BOX and EXISTS only");
                if (d.type == MLVDB_ATTR_SPARSE) {
                    if (o.op != MLVDB_WHERE_EXISTS) return fail(h, MLVDB_ERR_INVALID_ARG, "a sparse column takes EXISTS and LEN only");
                    d.type = MLVDB_ATTR_INT64_LIST;  // the same slot: the evaluators see a list column
                }
                if (d.type == MLVDB_ATTR_BITS) {
                    if (o.op != MLVDB_WHERE_EXISTS) return fail(h, MLVDB_ERR_INVALID_ARG, "a bits column takes EXISTS only");
                    d.type = MLVDB_ATTR_INT64_LIST;  // the same slot: the evaluators see a list column
                }
                if (o.op == MLVDB_WHERE_IN) {
                    if (d.type != MLVDB_ATTR_INT64) return fail(h, MLVDB_ERR_INVALID_ARG, "IN needs an int64 column");
                    if (o.a < 0 || o.b < 0 || o.a > w->n_set || o.b > w->n_set - o.a)
                        return fail(h, MLVDB_ERR_INVALID_ARG, "IN: set range outside the set table");
                    for (int64_t j = o.a + 1; j < o.a + o.b; ++j)
                        if (w->set[j - 1] > w->set[j]) return fail(h, MLVDB_ERR_INVALID_ARG, "IN: set range not sorted ascending");
                }
                break;
            case MLVDB_WHERE_HAS: case MLVDB_WHERE_HAS_ANY: case MLVDB_WHERE_HAS_ALL: case MLVDB_WHERE_LEN: {
                if (int rc = attr_check(h, o.attr)) return rc;
                d.type = h->attr_type[o.attr];
                d.col = h->attr_col[o.attr];
                if (d.type == MLVDB_ATTR_SPARSE) {
                    if (o.op != MLVDB_WHERE_LEN) return fail(h, MLVDB_ERR_INVALID_ARG, "a sparse column takes EXISTS and LEN only");
                    d.type = MLVDB_ATTR_INT64_LIST;  // the same slot: the evaluators see a list column
                }
                if (d.type == MLVDB_ATTR_BITS) return fail(h, MLVDB_ERR_INVALID_ARG, "a bits column takes EXISTS only");
                if (d.type != MLVDB_ATTR_INT64_LIST) return fail(h, MLVDB_ERR_INVALID_ARG, "HAS, HAS_ANY, HAS_ALL and LEN need a list column");
                if (o.op == MLVDB_WHERE_LEN) break;  // (its bounds stay in a, b: it reads the slot alone)
                d.b = (int64_t)reinterpret_cast<intptr_t>(h->list_pool[o.attr]);  // the pool's address rides in b
                if (o.op == MLVDB_WHERE_HAS) break;
                const bool all = o.op == MLVDB_WHERE_HAS_ALL;
                if (o.a < 0 || o.b < 0 || o.a > w->n_set || o.b > w->n_set - o.a)
                    return fail(h, MLVDB_ERR_INVALID_ARG, "HAS_ANY / HAS_ALL: set range outside the set table");
                if (o.a > INT32_MAX || o.b > INT32_MAX)
                    return fail(h, MLVDB_ERR_INVALID_ARG, "HAS_ANY / HAS_ALL: set offset and count must be below 2^31");
                if (all && o.b < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "HAS_ALL: an empty set range");
                for (int64_t j = o.a + 1; j < o.a + o.b; ++j)
                    if (all ? w->set[j - 1] >= w->set[j] : w->set[j - 1] > w->set[j])
                        return fail(h, MLVDB_ERR_INVALID_ARG, all ? "HAS_ALL: set range not strictly ascending"
                                                                  : "HAS_ANY: set range not sorted ascending");
                d.a = (o.a << 32) | o.b;
                break;
            }
            case MLVDB_WHERE_GEO_BOX: case MLVDB_WHERE_GEO_RADIUS: {
                if (int rc = attr_check(h, o.attr)) return rc;
                d.type = h->attr_type[o.attr];
                d.col = h->attr_col[o.attr];
                if (d.type != MLVDB_ATTR_GEO) return fail(h, MLVDB_ERR_INVALID_ARG, "GEO_RADIUS and GEO_BOX need a geo column");
                if (!geo_valid(o.a))
                    return fail(h, MLVDB_ERR_INVALID_ARG, "GEO_RADIUS / GEO_BOX: a is not a point (lat_e7, lon_e7 out of range)");
                if (o.op == MLVDB_WHERE_GEO_BOX) {
                    if (!geo_valid(o.b)) return fail(h, MLVDB_ERR_INVALID_ARG, "GEO_BOX: b is not a point (lat_e7, lon_e7 out of range)");
                    if (geo_lat(o.a) > geo_lat(o.b))
                        return fail(h, MLVDB_ERR_INVALID_ARG, "GEO_BOX: the south-west corner lies north of the north-east one");
                } else {
                    double thr;
                    std::memcpy(&thr, &o.b, sizeof thr);
                    if (!(thr >= 0.0 && thr <= 1.0))  // (NaN fails both)
                        return fail(h, MLVDB_ERR_INVALID_ARG, "GEO_RADIUS: the threshold sin^2(r / 2R) must be in [0, 1]");
                }
                break;
            }
            default:
                return fail(h, MLVDB_ERR_INVALID_ARG, "unknown where op");
        }
        if (++depth > MLVDB_WHERE_MAX_DEPTH) return fail(h, MLVDB_ERR_INVALID_ARG, "program deeper than MLVDB_WHERE_MAX_DEPTH");
    }
    if (depth != 1) return fail(h, MLVDB_ERR_INVALID_ARG, "a program must leave exactly one value on the stack");
    return MLVDB_OK;
}

// The validated program (h->where_ops) and its set table -> h->where_prog on the device, enqueued on h->stream.
int where_upload(mlvdb_index* h, const mlvdb_where* w, const int64_t** set_d) {
    hipStream_t s = h->stream;
    const size_t nops = h->where_ops.size(), nset = (size_t)w->n_set;
    WhereOp* ops_d = nullptr;
    int64_t* sets_d = nullptr;
    CARVE(h, h->where_prog, [&](Carver& c) {
        ops_d = c.take<WhereOp>(nops);
        sets_d = c.take<int64_t>(nset);
        c.take<char>(sizeof(int64_t));  // slack behind the set table
    });
    HIP_TRY(h, hipMemcpyAsync(ops_d, h->where_ops.data(), nops * sizeof(WhereOp), hipMemcpyHostToDevice, s));
    *set_d = sets_d;
    if (nset) HIP_TRY(h, hipMemcpyAsync(sets_d, w->set, nset * sizeof(int64_t), hipMemcpyHostToDevice, s));
    return MLVDB_OK;
}

// Validate, upload and evaluate a program into h->row_mask (live matching rows); matches != nullptr: also wait for their count.
int where_run(mlvdb_index* h, const mlvdb_where* w, int64_t* matches) {
    if (int rc = where_prepare(h, w)) return rc;
    if (matches) *matches = 0;
    if (h->total == 0) return MLVDB_OK;
    hipStream_t s = h->stream;
    const int64_t* set_d = nullptr;
    if (int rc = where_upload(h, w, &set_d)) return rc;
    HIP_TRY(h, h->where_cnt.ensure(sizeof(unsigned long long)));
    HIP_TRY(h, h->row_mask.ensure((size_t)h->total));
    HIP_TRY(h, hipMemsetAsync(h->where_cnt.p, 0, sizeof(unsigned long long), s));
    HIP_TRY(h, launch_where_eval(h->where_prog.as<WhereOp>(), w->n_ops, set_d, h->rn, h->total, h->row_mask.as<uint8_t>(),
                                 h->where_cnt.as<unsigned long long>(), s));
    if (matches) {
        unsigned long long n = 0;
        HIP_TRY(h, hipMemcpyAsync(&n, h->where_cnt.p, sizeof n, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        *matches = (int64_t)n;
    }
    return MLVDB_OK;
}

// The `matches` rows of h->row_mask as labels in ascending order -> h->labels_in (enqueued): the compaction map of the masked
// norms (NaN = tombstoned or no match).
int mask_labels(mlvdb_index* h, int64_t matches) {
    hipStream_t s = h->stream;
    const int64_t nblocks = (h->total + 1023) / 1024;
    HIP_TRY(h, h->rn_masked.ensure((size_t)h->capacity * sizeof(float)));
    HIP_TRY(h, h->partial.ensure((size_t)nblocks * sizeof(uint32_t) + 64));
    HIP_TRY(h, h->labels_in.ensure((size_t)matches * sizeof(int32_t)));
    HIP_TRY(h, launch_mask_norms(h->rn, h->row_mask.as<uint8_t>(), h->rn_masked.as<float>(), h->total, h->capacity, s));
    HIP_TRY(h, launch_compact_map(h->rn_masked.as<float>(), h->total, h->partial.as<uint32_t>(),
                                  h->where_cnt.as<unsigned long long>(), h->labels_in.as<int32_t>(), s));
    return MLVDB_OK;
}

// An optional program evaluated into h->row_mask for the kernels that read it at one byte per row (no wait, no copy):
// *mask is that mask, or nullptr without a program.  Requires h->total > 0.
int where_mask(mlvdb_index* h, const mlvdb_where* where, const uint8_t** mask) {
    *mask = nullptr;
    if (!where) return MLVDB_OK;
    if (int rc = where_run(h, where, nullptr)) return rc;
    *mask = h->row_mask.as<uint8_t>();
    return MLVDB_OK;
}
}  // namespace

int mlvdb_attr_define(mlvdb_index* h, int32_t attr, int32_t type) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (attr < 0 || attr >= MLVDB_MAX_ATTRS) return fail(h, MLVDB_ERR_INVALID_ARG, "attribute index out of range");
    if (type != MLVDB_ATTR_INT64 && type != MLVDB_ATTR_FLOAT64 && type != MLVDB_ATTR_GEO && !pooled(type))
        return fail(h, MLVDB_ERR_INVALID_ARG, "unknown attribute type");
    if (h->attr_type[attr]) {
        if (h->attr_type[attr] != type) return fail(h, MLVDB_ERR_INVALID_ARG, "attribute already defined with another type");
        return MLVDB_OK;
    }
    if (h->capacity > 0) {
        Staged<DevBuf> col(h->stream);
        HIP_TRY(h, col.exact((size_t)h->capacity * sizeof(int64_t)));
        hipError_t e = launch_attr_fill(col.as<int64_t>(), attr_absent(type), 0, h->capacity, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, MLVDB_ERR_HIP, "attribute column fill", e);
        h->rows.col[attr] = std::move(col);
        h->attr_col[attr] = h->rows.col[attr].as<int64_t>();
    }
    h->attr_type[attr] = type;
    return MLVDB_OK;
    });
}

int mlvdb_attr_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const void* values) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = scalar_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n, values != nullptr)) return rc;
    if (n == 0) return MLVDB_OK;
    if (int rc = geo_values_check(h, attr, values, n)) return rc;
    // (the sentinels are values like any other here: INT64_MIN / NaN written to a row make it absent)
    HIP_TRY(h, hipMemcpyAsync(h->attr_col[attr] + first, values, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MLVDB_OK;
    });
}

int mlvdb_attr_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, void* out_values) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = scalar_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n, out_values != nullptr)) return rc;
    if (n == 0) return MLVDB_OK;
    HIP_TRY(h, hipMemcpyAsync(out_values, h->attr_col[attr] + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MLVDB_OK;
    });
}

int mlvdb_where_count(mlvdb_index* h, const mlvdb_where* where, int64_t* matches) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (!matches) return fail(h, MLVDB_ERR_INVALID_ARG, "matches is null");
    return where_run(h, where, matches);
    });
}

int mlvdb_where_labels(mlvdb_index* h, const mlvdb_where* where, int64_t* out_labels, int64_t capacity, int64_t* matches) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (!matches || capacity < 0 || (capacity > 0 && !out_labels)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad output buffers");
    const int rc = where_run(h, where, matches);
    if (rc || *matches == 0 || capacity == 0) return rc;
    hipStream_t s = h->stream;
    if (int rc2 = mask_labels(h, *matches)) return rc2;
    const int64_t n = std::min(capacity, *matches);
    std::vector<int32_t> host((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(host.data(), h->labels_in.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int64_t i = 0; i < n; ++i) out_labels[i] = host[(size_t)i];
    return MLVDB_OK;
    });
}

int mlvdb_search_batch_where(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const mlvdb_where* where,
                             int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = where_run(h, where, nullptr)) return rc;  // the mask stays on the device: no wait, no copy
    if (h->total == 0) return search_host(h, queries, nq, k, out_labels, out_dist, out_counts, out_dist64);
    return with_row_mask(h, nq, [&]() { return search_host(h, queries, nq, k, out_labels, out_dist, out_counts, out_dist64); });
    });
}

int mlvdb_range_batch_packed_where(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity,
                                   int64_t total_capacity, const mlvdb_where* where, int64_t* out_labels, float* out_dist,
                                   int64_t* out_offsets, int64_t* out_counts) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = where_run(h, where, nullptr)) return rc;
    auto call = [&]() {
        return range_batch_impl(h, queries, nq, radius, capacity, out_labels, out_dist, out_counts, out_offsets, total_capacity, true);
    };
    if (h->total == 0) return call();
    return with_row_mask(h, nq, call);
    });
}

extern "C++" {
namespace {
// The tail of an entry that takes an optional program, everything else checked: no program -> the call; else the program
// into h->row_mask (where_run validates it before its first launch; the mask stays on the device: no wait, no copy) and
// the call under that mask.
template <class F>
int with_where(mlvdb_index* h, const mlvdb_where* where, int64_t nq, F&& call) {
    if (!where) return nq == 0 ? MLVDB_OK : call();
    const int rc = where_run(h, where, nullptr);
    if (rc || nq == 0) return rc;
    if (h->total == 0) return call();
    return with_row_mask(h, nq, call);
}

// ---- per-query filters (mlvdb_where_each.h)
constexpr int32_t kGatherQT = 4;  // queries per tile of the gathered kernels

// ... fewer only when the tile would not fit in LDS; where even one query does not (where_gather_lds(1, ld) > 64 KiB),
// nothing is gathered: the callers check.
int32_t gather_qt(const mlvdb_index* h) {
    int32_t qt = kGatherQT;
    while (qt > 1 && where_gather_lds(qt, h->ld) > 64 * 1024) qt >>= 1;
    return qt;
}

// The programs of a call validated (where_prepare, each against its own set table) and packed for the device: ops
// concatenated (off[p] .. off[p + 1]), the IN ranges rebased onto one concatenated set table.
// Every column op also carries its column's slot in `cols` (the referenced columns, each read once per row by the
// evaluation) in the high bits of its type.
struct EachPrograms {
    std::vector<WhereOp> ops;
    std::vector<int32_t> off;
    std::vector<int64_t> set;
    std::vector<const int64_t*> cols;
};

int where_each_pack(mlvdb_index* h, const mlvdb_where* programs, int32_t n, EachPrograms& out) {
    if (n < 0 || n > MLVDB_WHERE_EACH_MAX_PROGRAMS)
        return fail(h, MLVDB_ERR_INVALID_ARG, "n_programs outside 0..MLVDB_WHERE_EACH_MAX_PROGRAMS");
    if (n > 0 && !programs) return fail(h, MLVDB_ERR_INVALID_ARG, "programs is null");
    int64_t n_ops = 0;
    for (int32_t p = 0; p < n; ++p) n_ops += programs[p].n_ops > 0 ? programs[p].n_ops : 0;
    if (n_ops > MLVDB_WHERE_EACH_MAX_OPS) return fail(h, MLVDB_ERR_INVALID_ARG, "more than MLVDB_WHERE_EACH_MAX_OPS ops over all programs");
    out.ops.clear();
    out.set.clear();
    out.cols.clear();
    out.off.assign(1, 0);
    for (int32_t p = 0; p < n; ++p) {
        if (int rc = where_prepare(h, &programs[p])) return rc;
        const int64_t rebase = (int64_t)out.set.size();
        for (WhereOp o : h->where_ops) {
            if (o.op == MLVDB_WHERE_IN) o.a += rebase;
            if (o.op == MLVDB_WHERE_HAS_ANY || o.op == MLVDB_WHERE_HAS_ALL) {  // (offset << 32 | count: where_prepare)
                if ((o.a >> 32) + rebase > INT32_MAX)
                    return fail(h, MLVDB_ERR_INVALID_ARG, "HAS_ANY / HAS_ALL: the call's set tables exceed 2^31 values");
                o.a += rebase << 32;
            }
            if (o.col) {
                const auto* col = static_cast<const int64_t*>(o.col);
                auto it = std::find(out.cols.begin(), out.cols.end(), col);
                if (it == out.cols.end()) it = out.cols.insert(out.cols.end(), col);
                o.type |= (int32_t)(it - out.cols.begin()) << 8;
            }
            out.ops.push_back(o);
        }
        out.set.insert(out.set.end(), programs[p].set, programs[p].set + programs[p].n_set);
        out.off.push_back((int32_t)out.ops.size());
    }
    return MLVDB_OK;
}

// Segments of the evaluation / scatter (kernels_where_each.hip): one wave per run of seg_rows rows.
struct EachSegs {
    int64_t seg_rows = 64;
    int32_t nseg = 0;
};

EachSegs each_segments(int64_t total) {
    EachSegs sg;
    if (total <= 0) return sg;
    const int64_t want = std::min<int64_t>(4096, (total + 63) / 64);
    sg.seg_rows = ((total + want - 1) / want + 63) / 64 * 64;
    sg.nseg = (int32_t)((total + sg.seg_rows - 1) / sg.seg_rows);
    return sg;
}

// h->each_tot: the programs' match totals and the bases of their label lists (the gather stage's), one of each per program
struct EachTotals {
    int64_t *total = nullptr, *base = nullptr;
    void take(Carver& c) {
        total = c.take<int64_t>(kWhereEachMaxPrograms);
        base = c.take<int64_t>(kWhereEachMaxPrograms);
    }
};

// Every program on every row in one pass: h->each_bits, the per-segment counts (exclusive offsets afterwards) and
// matches[p] on the host (the call's one synchronisation).  Requires h->total > 0 and at least one program.
int where_each_eval(mlvdb_index* h, const EachPrograms& pk, const EachSegs& sg, int64_t* matches) {
    hipStream_t s = h->stream;
    const int32_t n = (int32_t)pk.off.size() - 1;
    WhereOp* ops_d = nullptr;
    int32_t* off_d = nullptr;
    int64_t* set_d = nullptr;
    const int64_t** cols_d = nullptr;
    CARVE(h, h->each_prog, [&](Carver& c) {
        ops_d = c.take<WhereOp>(pk.ops.size());
        off_d = c.take<int32_t>(pk.off.size());
        c.pad_to(16);
        set_d = c.take<int64_t>(pk.set.size());
        cols_d = c.take<const int64_t*>(pk.cols.size());
        c.take<char>(16);  // slack
    });
    HIP_TRY(h, h->each_bits.ensure((size_t)h->total * sizeof(unsigned long long)));
    HIP_TRY(h, h->each_seg.ensure((size_t)n * sg.nseg * sizeof(uint32_t)));
    EachTotals tot;
    if (int rc = carve(h, h->each_tot, [&](Carver& c) { tot.take(c); })) return rc;
    HIP_TRY(h, hipMemcpyAsync(ops_d, pk.ops.data(), pk.ops.size() * sizeof(WhereOp), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(off_d, pk.off.data(), pk.off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (!pk.set.empty()) HIP_TRY(h, hipMemcpyAsync(set_d, pk.set.data(), pk.set.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (!pk.cols.empty()) HIP_TRY(h, hipMemcpyAsync(cols_d, pk.cols.data(), pk.cols.size() * sizeof(void*), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_where_each_eval(ops_d, off_d, n, (int32_t)pk.ops.size(), set_d, cols_d, (int32_t)pk.cols.size(), h->rn, h->total,
                                      sg.seg_rows, sg.nseg, h->each_bits.as<unsigned long long>(), h->each_seg.as<uint32_t>(), s));
    HIP_TRY(h, launch_where_each_scan(h->each_seg.as<uint32_t>(), n, sg.nseg, tot.total, s));
    HIP_TRY(h, hipMemcpyAsync(matches, tot.total, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // (the host vectors above are consumed by now)
    return MLVDB_OK;
}

// The queries `sel` of a host batch as one contiguous host batch.
std::vector<float> pick_queries(const float* queries, int32_t dim, const std::vector<int32_t>& sel) {
    std::vector<float> out(sel.size() * (size_t)dim);
    for (size_t i = 0; i < sel.size(); ++i)
        std::memcpy(out.data() + i * dim, queries + (size_t)sel[i] * dim, (size_t)dim * sizeof(float));
    return out;
}

// Outputs of a sub-batch (rows 0..sel.size()-1 of lab / dist / cnt / d64) into the caller's rows sel[i].
void put_rows(const std::vector<int32_t>& sel, int32_t k, const int64_t* lab, const float* dist, const int32_t* cnt,
              const double* d64, int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64) {
    for (size_t i = 0; i < sel.size(); ++i) {
        const size_t q = (size_t)sel[i];
        std::memcpy(out_labels + q * k, lab + i * k, (size_t)k * sizeof(int64_t));
        std::memcpy(out_dist + q * k, dist + i * k, (size_t)k * sizeof(float));
        if (out_dist64) std::memcpy(out_dist64 + q * k, d64 + i * k, (size_t)k * sizeof(double));
        out_counts[q] = cnt[i];
    }
}

// search_host of the sub-batch `sel` (masked by h->row_mask when `masked`), scattered into the caller's rows.
int search_rows(mlvdb_index* h, const float* queries, const std::vector<int32_t>& sel, int32_t k, bool masked,
                int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64) {
    const int64_t m = (int64_t)sel.size();
    const std::vector<float> q = pick_queries(queries, h->dim, sel);
    std::vector<int64_t> lab((size_t)m * k);
    std::vector<float> dist((size_t)m * k);
    std::vector<int32_t> cnt((size_t)m);
    std::vector<double> d64(out_dist64 ? (size_t)m * k : 0);
    double* p64 = out_dist64 ? d64.data() : nullptr;
    auto call = [&]() { return search_host(h, q.data(), m, k, lab.data(), dist.data(), cnt.data(), p64); };
    const int rc = masked ? with_row_mask(h, m, call) : call();
    if (rc) return rc;
    put_rows(sel, k, lab.data(), dist.data(), cnt.data(), p64, out_labels, out_dist, out_counts, out_dist64);
    return MLVDB_OK;
}

// The queries of a call by program: qof[p] = program p's, ascending; plain = the unfiltered ones (entry -1); any: some
// program has a query.  Part of an entry's checks: nothing is launched before it.
struct EachSplit {
    std::vector<std::vector<int32_t>> qof;
    std::vector<int32_t> plain;
    bool any = false;
};

int where_each_split(mlvdb_index* h, const int32_t* program_of_query, int64_t nq, int32_t n_programs, EachSplit& out) {
    out.qof.assign((size_t)n_programs, {});
    for (int64_t i = 0; i < nq; ++i) {
        const int32_t p = program_of_query[i];
        if (p < -1 || p >= n_programs) return fail(h, MLVDB_ERR_INVALID_ARG, "program_of_query entry outside [-1, n_programs)");
        (p < 0 ? out.plain : out.qof[(size_t)p]).push_back((int32_t)i);
        out.any = out.any || p >= 0;
    }
    return MLVDB_OK;
}

// The route of every program (NONE: no query or no match) and the programs of the two others, ascending.  GATHER while the
// gathered rows stay a small share of what the masked scan would read (matches x tiles x 1000 <= live x WHERE_GATHER), the
// label lists of all gathered programs together stay below 2^31 entries, a tile fits in LDS and the caller allows it.
struct EachRoutes {
    std::vector<int32_t> routes, gp, sp;
};

EachRoutes where_each_routes(const mlvdb_index* h, const std::vector<std::vector<int32_t>>& qof,
                             const std::vector<int64_t>& matches, int32_t qt, bool gather_allowed) {
    EachRoutes r;
    r.routes.assign(qof.size(), MLVDB_WHERE_ROUTE_NONE);
    const bool gather_fits = gather_allowed && where_gather_lds(qt, h->ld) <= 64 * 1024;
    const __int128 live = h->total - h->deleted;
    int64_t nlab = 0;
    for (size_t p = 0; p < qof.size(); ++p) {
        const size_t nqp = qof[p].size();
        if (nqp == 0 || matches[p] == 0) continue;
        const __int128 tiles = (__int128)((nqp + qt - 1) / qt);
        const bool gather = gather_fits && (__int128)matches[p] * tiles * 1000 <= live * h->tn.where_gather &&
                            nlab + matches[p] <= INT32_MAX;
        if (gather) nlab += matches[p];
        r.routes[p] = gather ? MLVDB_WHERE_ROUTE_GATHER : MLVDB_WHERE_ROUTE_SCAN;
        (gather ? r.gp : r.sp).push_back((int32_t)p);
    }
    return r;
}

// The SCAN route's row mask: program p's bit of h->each_bits, expanded into h->row_mask.
int each_row_mask(mlvdb_index* h, int32_t p) {
    HIP_TRY(h, h->row_mask.ensure((size_t)h->total));
    HIP_TRY(h, launch_where_each_expand(h->each_bits.as<unsigned long long>(), p, h->total, h->row_mask.as<uint8_t>(), h->stream));
    return MLVDB_OK;
}

// What the gather stage leaves its caller: the gathered queries sorted by program (sel: their positions in the call,
// prog_of_sel: their programs; the prepared batch h->each_qpad / each_qaux holds them in this order), the tiles (on the
// device in h->each_tiles), the longest label list and the number of queries.  q and base are the host sides of copies the
// stage enqueued: they live until the caller has synchronised.
struct GatherStage {
    std::vector<int32_t> sel, prog_of_sel;
    std::vector<GatherTile> tiles;
    int64_t max_m = 0;
    int32_t ng = 0;
    std::vector<float> q;
    std::vector<int64_t> base;
};

// The head of the GATHER route for the programs `gp` (their queries in qof[p], matches[p] rows each), all enqueued: the
// label lists (h->each_lab, one scatter pass over the bit words), the tiles of <= qt queries of one program -- none straddling
// a multiple of `group` positions when group > 0 -- and the gathered queries, prepared as every exact path prepares them.
int gather_stage(mlvdb_index* h, const float* queries, int32_t qt, size_t group, const EachSegs& sg, int32_t n_programs,
                 const std::vector<int32_t>& gp, const std::vector<std::vector<int32_t>>& qof, const int64_t* matches,
                 GatherStage& st) {
    hipStream_t s = h->stream;
    st.base.assign(kWhereEachMaxPrograms, 0);
    unsigned long long gmask = 0;
    int64_t nlab = 0;
    for (int32_t p : gp) {
        gmask |= 1ull << p;
        st.base[p] = nlab;
        const std::vector<int32_t>& qs = qof[p];
        for (size_t t0 = 0; t0 < qs.size();) {
            const size_t pos = st.sel.size() + t0;
            GatherTile t;
            t.lab_begin = (int32_t)nlab;
            t.lab_count = (int32_t)matches[p];
            t.sel0 = (int32_t)pos;
            t.nsel = (int32_t)std::min<size_t>({(size_t)qt, qs.size() - t0, group ? group - pos % group : (size_t)qt});
            st.tiles.push_back(t);
            t0 += (size_t)t.nsel;
        }
        st.sel.insert(st.sel.end(), qs.begin(), qs.end());
        st.prog_of_sel.insert(st.prog_of_sel.end(), qs.size(), p);
        nlab += matches[p];
        st.max_m = std::max(st.max_m, matches[p]);
    }
    st.ng = (int32_t)st.sel.size();
    HIP_TRY(h, h->each_lab.ensure((size_t)nlab * sizeof(int32_t)));
    EachTotals tot;  // (where_each_eval sized the block: this only finds the bases in it)
    Carver in_tot{h->each_tot.as<char>()};
    tot.take(in_tot);
    int64_t* base_d = tot.base;
    HIP_TRY(h, hipMemcpyAsync(base_d, st.base.data(), st.base.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_where_each_scatter(h->each_bits.as<unsigned long long>(), h->total, sg.seg_rows, sg.nseg, n_programs,
                                         h->each_seg.as<uint32_t>(), gmask, base_d, h->each_lab.as<int32_t>(), s));
    st.q = pick_queries(queries, h->dim, st.sel);
    HIP_TRY(h, h->each_q.ensure(st.q.size() * sizeof(float)));
    HIP_TRY(h, h->each_qpad.ensure((size_t)st.ng * h->ld * sizeof(float)));
    HIP_TRY(h, h->each_qaux.ensure((size_t)st.ng * sizeof(double)));
    HIP_TRY(h, h->each_tiles.ensure(st.tiles.size() * sizeof(GatherTile)));
    HIP_TRY(h, hipMemcpyAsync(h->each_q.p, st.q.data(), st.q.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->each_tiles.p, st.tiles.data(), st.tiles.size() * sizeof(GatherTile), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_query_prep(h->each_q.as<float>(), st.ng, h->dim, h->ld, h->space, h->each_qpad.as<float>(),
                                 h->each_qaux.as<double>(), nullptr, s));
    return MLVDB_OK;
}

// The GATHER route of a kNN call: the gather stage, the gathered kernel, exact_merge_kernel, outputs into the caller's rows.
int gather_programs(mlvdb_index* h, const float* queries, int32_t k, int32_t qt, const EachSegs& sg, int32_t n_programs,
                    const std::vector<int32_t>& gp, const std::vector<std::vector<int32_t>>& qof, const int64_t* matches,
                    int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64) {
    hipStream_t s = h->stream;
    GatherStage st;
    if (int rc = gather_stage(h, queries, qt, 0, sg, n_programs, gp, qof, matches, st)) return rc;
    const int32_t ng = st.ng, ntiles = (int32_t)st.tiles.size();
    // chunks per tile: enough blocks to fill the chip (~2048), none shorter than 64 rows, at most 64 partial lists per query
    const int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>({64, (2048 + ntiles - 1) / ntiles, (st.max_m + 63) / 64}));
    HIP_TRY(h, h->partial.ensure((size_t)ng * nchunk * k * sizeof(TopEntry)));
    HIP_TRY(h, launch_where_gather(h->X, h->each_qpad.as<float>(), h->each_qaux.as<double>(), h->each_lab.as<int32_t>(),
                                   h->each_tiles.as<GatherTile>(), ntiles, h->ld, h->space, qt, k, (int32_t)nchunk,
                                   h->partial.as<TopEntry>(), s));
    // outputs [d64 | labels | dist | counts] in the sorted order, one copy back
    const size_t nk = (size_t)ng * k;
    ListBlock o, ho;
    if (int rc = carve_list(h, h->each_out, nk, (size_t)ng, o)) return rc;
    std::vector<char> host(span_bytes(o.d64, o.cnt + ng));
    Carver hc{host.data()};
    ho.take(hc, nk, (size_t)ng);
    HIP_TRY(h, launch_exact_merge(h->partial.as<TopEntry>(), ng, nullptr, nullptr, (int32_t)nchunk, k, o.lab, o.dist, o.cnt,
                                  o.d64, s));
    HIP_TRY(h, hipMemcpyAsync(host.data(), h->each_out.p, host.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    put_rows(st.sel, k, ho.lab, ho.dist, ho.cnt, ho.d64, out_labels, out_dist, out_counts, out_dist64);
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_where_count_each(mlvdb_index* h, const mlvdb_where* programs, int32_t n_programs, int64_t* out_matches) {
    return guarded(h, kOnDevice, [&]() -> int {
    EachPrograms pk;
    if (int rc = where_each_pack(h, programs, n_programs, pk)) return rc;
    if (n_programs > 0 && !out_matches) return fail(h, MLVDB_ERR_INVALID_ARG, "out_matches is null");
    for (int32_t p = 0; p < n_programs; ++p) out_matches[p] = 0;
    if (n_programs == 0 || h->total == 0) return MLVDB_OK;
    return where_each_eval(h, pk, each_segments(h->total), out_matches);
    });
}

int mlvdb_search_batch_where_each(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const mlvdb_where* programs,
                                  int32_t n_programs, const int32_t* program_of_query, int64_t* out_labels, float* out_dist,
                                  int32_t* out_counts, double* out_dist64, int32_t* out_routes) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max_paged(h, k)) return rc;
    EachPrograms pk;
    if (int rc = where_each_pack(h, programs, n_programs, pk)) return rc;
    if (nq > 0 && (!queries || !program_of_query || !out_labels || !out_dist || !out_counts))
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    EachSplit split;
    if (int rc = where_each_split(h, program_of_query, nq, n_programs, split)) return rc;
    std::vector<int64_t> matches((size_t)n_programs, 0);
    const EachSegs sg = each_segments(h->total);
    if (split.any && h->total > 0) {
        if (int rc = where_each_eval(h, pk, sg, matches.data())) return rc;
    }
    const int32_t qt = gather_qt(h);
    const EachRoutes rt = where_each_routes(h, split.qof, matches, qt, k <= MLVDB_MAX_TOPK);
    if (out_routes) std::copy(rt.routes.begin(), rt.routes.end(), out_routes);
    // NONE: padding, as a call whose program matches nothing returns it
    for (int32_t p = 0; p < n_programs; ++p) {
        if (rt.routes[(size_t)p] != MLVDB_WHERE_ROUTE_NONE) continue;
        for (int32_t q : split.qof[(size_t)p])
            pad_outputs(out_labels + (size_t)q * k, out_dist + (size_t)q * k, out_dist64 ? out_dist64 + (size_t)q * k : nullptr, k,
                        out_counts + q, 1);
    }
    if (!rt.gp.empty()) {
        if (int rc = gather_programs(h, queries, k, qt, sg, n_programs, rt.gp, split.qof, matches.data(), out_labels, out_dist,
                                     out_counts, out_dist64))
            return rc;
    }
    // SCAN: the program's row mask out of its bit, then exactly the masked call of mlvdb_search_batch_where
    for (int32_t p : rt.sp) {
        if (int rc = each_row_mask(h, p)) return rc;
        if (int rc = search_rows(h, queries, split.qof[(size_t)p], k, true, out_labels, out_dist, out_counts, out_dist64))
            return rc;
    }
    if (!split.plain.empty()) return search_rows(h, queries, split.plain, k, false, out_labels, out_dist, out_counts, out_dist64);
    return MLVDB_OK;
    });
}

extern "C++" {
namespace {
// ---- per-query filters in a range call (mlvdb_where_each_range.h)
static_assert(MLVDB_WHERE_EACH_RANGE_LIST == kCandCap, "the GATHER route lists what the ranking kernel ranks");

// What the sub-batches of a call found, by query of the call: its exact hit count and where its returned hits lie in lab / dist.
struct RangeParts {
    std::vector<int64_t> count, begin, len;  // [nq]
    std::vector<int64_t> lab;
    std::vector<float> dist;
};

// A sub-batch's answer (counts / offsets by its own queries 0.., packed hits pl / pd) as the answer of the call's queries sel[i].
void take_hits(RangeParts& parts, const std::vector<int32_t>& sel, const std::vector<int64_t>& counts,
               const std::vector<int64_t>& offsets, const int64_t* pl, const float* pd) {
    const size_t at = parts.lab.size(), n = (size_t)offsets[sel.size()];
    if (n) {
        parts.lab.insert(parts.lab.end(), pl, pl + n);
        parts.dist.insert(parts.dist.end(), pd, pd + n);
    }
    for (size_t i = 0; i < sel.size(); ++i) {
        const size_t q = (size_t)sel[i];
        parts.count[q] = counts[i];
        parts.begin[q] = (int64_t)at + offsets[i];
        parts.len[q] = offsets[i + 1] - offsets[i];
    }
}

// The range passes of the sub-batch `sel` (masked by h->row_mask when `masked`): exactly what range_batch_impl runs for a call
// of those queries, its ranked hits packed on the device and taken into `parts`.
int range_rows(mlvdb_index* h, const float* queries, const std::vector<int32_t>& sel, float radius, int64_t cap_eff, bool masked,
               RangeParts& parts) {
    const int64_t m = (int64_t)sel.size();
    const std::vector<float> q = pick_queries(queries, h->dim, sel);
    auto call = [&]() -> int {
        hipStream_t s = h->stream;
        int rc = begin_call(h, s);
        if (rc) return rc;
        std::vector<int64_t> counts, offsets;
        if (int rc = range_ranked(h, s, q.data(), m, radius, cap_eff, counts, offsets)) return rc;
        const int64_t* pl = nullptr;
        const float* pd = nullptr;
        if (offsets[(size_t)m] > 0) {
            if (int rc = pack_range_hits(h, s, m, cap_eff, offsets, nullptr, nullptr, &pl, &pd)) return rc;
        }
        take_hits(parts, sel, counts, offsets, pl, pd);
        return end_call(h, s);
    };
    return masked ? with_row_mask(h, m, call) : call();
}

// The GATHER route of a range call: the gather stage, then per group of 256 gathered queries (the ranking kernel's workspace
// holds 256 hit lists; no tile straddles two groups) the gathered range kernel and range_rank_kernel; one synchronisation
// reads the exact counts back.  A query with more hits than its list holds (> kCandCap) gets nothing here: it is appended to
// redo[its program] for the SCAN route.
int gather_range_programs(mlvdb_index* h, const float* queries, float radius, int64_t cap_eff, int32_t qt, const EachSegs& sg,
                          int32_t n_programs, const std::vector<int32_t>& gp, const std::vector<std::vector<int32_t>>& qof,
                          const int64_t* matches, RangeParts& parts, std::vector<std::vector<int32_t>>& redo) {
    hipStream_t s = h->stream;
    GatherStage st;
    if (int rc = gather_stage(h, queries, qt, kFilterQueries, sg, n_programs, gp, qof, matches, st)) return rc;
    const std::vector<int32_t>& sel = st.sel;
    const std::vector<GatherTile>& tiles = st.tiles;
    const int64_t ng = st.ng;
    const int64_t per_group = std::min<int64_t>((int64_t)tiles.size(), kFilterQueries);  // (at most: tiles of a full group)
    // chunks per tile as the gathered kNN cuts them: enough blocks to fill the chip (~2048), none shorter than 64 rows
    const int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>({64, (2048 + per_group - 1) / per_group, (st.max_m + 63) / 64}));
    // the ranking kernel's workspace (what setup_filter_ws gives a range pass, without the candidate lists) and outputs
    {
        const void* before = h->fmisc.p;
        HIP_TRY(h, h->fmisc.ensure(9 * kFilterQueries * sizeof(uint32_t)));
        if (h->fmisc.p != before) h->sqmin_fresh = true;
    }
    HIP_TRY(h, h->rhits.ensure((size_t)kFilterQueries * kCandCap * sizeof(RangeHit)));
    HIP_TRY(h, h->rhit_cnt.ensure(kFilterQueries * sizeof(uint32_t)));
    HIP_TRY(h, h->io_lab.ensure((size_t)ng * cap_eff * sizeof(int64_t)));
    HIP_TRY(h, h->io_dist.ensure((size_t)ng * cap_eff * sizeof(float)));
    HIP_TRY(h, h->io_cnt.ensure((size_t)ng * sizeof(int64_t)));
    HIP_TRY(h, h->pin_in.ensure(((size_t)ng + 1) * sizeof(int64_t)));  // (pack_range_hits stages the offsets there)
    HIP_TRY(h, h->pin_out.ensure((size_t)ng * sizeof(int64_t)));
    FilterArgs fa{};
    fa.cnt = h->fmisc.as<uint32_t>() + 2 * kFilterQueries;
    fa.overflow = h->fmisc.as<uint32_t>() + 3 * kFilterQueries;
    fa.rhits = h->rhits.as<RangeHit>();
    fa.rhit_cnt = h->rhit_cnt.as<uint32_t>();
    size_t t_lo = 0;
    for (int64_t g0 = 0; g0 < ng; g0 += kFilterQueries) {
        fa.nq = (int32_t)std::min<int64_t>(kFilterQueries, ng - g0);
        size_t t_hi = t_lo;
        while (t_hi < tiles.size() && tiles[t_hi].sel0 < g0 + kFilterQueries) ++t_hi;
        HIP_TRY(h, hipMemsetAsync(fa.rhit_cnt, 0, kFilterQueries * sizeof(uint32_t), s));
        HIP_TRY(h, hipMemsetAsync(fa.overflow, 0, kFilterQueries * sizeof(uint32_t), s));
        HIP_TRY(h, launch_where_gather_range(h->X, h->each_qpad.as<float>(), h->each_qaux.as<double>(), h->each_lab.as<int32_t>(),
                                             h->each_tiles.as<GatherTile>() + t_lo, (int32_t)(t_hi - t_lo), h->ld, h->space, qt,
                                             (int32_t)nchunk, radius, (int32_t)g0, fa.rhits, fa.rhit_cnt, s));
        HIP_TRY(h, launch_range_rank(fa, (int32_t)g0, cap_eff, h->io_lab.as<int64_t>(), h->io_dist.as<float>(),
                                     h->io_cnt.as<int64_t>(), s));
        t_lo = t_hi;
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, hipMemcpyAsync(h->pin_out.p, h->io_cnt.p, (size_t)ng * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    const std::vector<int64_t> counts(static_cast<const int64_t*>(h->pin_out.p), static_cast<const int64_t*>(h->pin_out.p) + ng);
    std::vector<int64_t> offsets((size_t)ng + 1, 0);
    int64_t n_redo = 0;
    for (int64_t i = 0; i < ng; ++i) {
        const bool flagged = counts[(size_t)i] > kCandCap;  // (the ranking kernel wrote none of its hits)
        if (flagged) {
            redo[(size_t)st.prog_of_sel[(size_t)i]].push_back(sel[(size_t)i]);
            ++n_redo;
        }
        offsets[(size_t)i + 1] = offsets[(size_t)i] + (flagged ? 0 : std::min<int64_t>(counts[(size_t)i], cap_eff));
    }
    h->stats.fallback_queries += n_redo;
    const int64_t* pl = nullptr;
    const float* pd = nullptr;
    if (offsets[(size_t)ng] > 0) {
        int rc = pack_range_hits(h, s, ng, cap_eff, offsets, nullptr, nullptr, &pl, &pd);
        if (rc) return rc;
    }
    take_hits(parts, sel, counts, offsets, pl, pd);
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_range_batch_packed_where_each(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity,
                                        int64_t total_capacity, const mlvdb_where* programs, int32_t n_programs,
                                        const int32_t* program_of_query, int64_t* out_labels, float* out_dist,
                                        int64_t* out_offsets, int64_t* out_counts, int32_t* out_routes) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched: the range arguments as range_batch_impl checks them
    if (!out_offsets) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_nq(h, nq)) return rc;
    if (capacity < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "capacity must be >= 1");
    if (total_capacity < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "total_capacity must be >= 0");
    EachPrograms pk;
    if (int rc = where_each_pack(h, programs, n_programs, pk)) return rc;
    if (nq > 0 && (!queries || !program_of_query || !out_counts || ((!out_labels || !out_dist) && total_capacity > 0)))
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    EachSplit split;
    if (int rc = where_each_split(h, program_of_query, nq, n_programs, split)) return rc;
    EachRoutes rt;
    rt.routes.assign((size_t)n_programs, MLVDB_WHERE_ROUTE_NONE);
    RangeParts parts;
    parts.count.assign((size_t)nq, 0);
    parts.begin.assign((size_t)nq, 0);
    parts.len.assign((size_t)nq, 0);
    const int64_t cap_eff = std::min<int64_t>(capacity, MLVDB_MAX_TOPK_PAGED);  // most hits returned per query
    if (nq > 0 && h->total > h->deleted) {
        std::vector<int64_t> matches((size_t)n_programs, 0);
        const EachSegs sg = each_segments(h->total);
        if (split.any) {
            if (int rc = where_each_eval(h, pk, sg, matches.data())) return rc;
        }
        const int32_t qt = gather_qt(h);
        rt = where_each_routes(h, split.qof, matches, qt, true);  // (a range call has no k to bound)
        // GATHER; the queries whose hits its lists could not hold join the SCAN route of their program
        std::vector<std::vector<int32_t>> redo((size_t)n_programs);
        if (!rt.gp.empty()) {
            if (int rc = gather_range_programs(h, queries, radius, cap_eff, qt, sg, n_programs, rt.gp, split.qof, matches.data(), parts,
                                               redo))
                return rc;
        }
        // SCAN: the program's row mask out of its bit, then exactly the masked passes of mlvdb_range_batch_packed_where
        for (int32_t p = 0; p < n_programs; ++p) {
            const std::vector<int32_t>& qs = rt.routes[(size_t)p] == MLVDB_WHERE_ROUTE_SCAN ? split.qof[(size_t)p] : redo[(size_t)p];
            if (qs.empty()) continue;
            if (int rc = each_row_mask(h, p)) return rc;
            if (int rc = range_rows(h, queries, qs, radius, cap_eff, true, parts)) return rc;
        }
        if (!split.plain.empty()) {
            if (int rc = range_rows(h, queries, split.plain, radius, cap_eff, false, parts)) return rc;
        }
    }
    if (out_routes) std::copy(rt.routes.begin(), rt.routes.end(), out_routes);
    // the packed output, once for the whole call, under the rules of range_batch_impl
    out_offsets[0] = 0;
    bool over = false, hard = false;
    for (int64_t i = 0; i < nq; ++i) {
        out_offsets[i + 1] = out_offsets[i] + parts.len[(size_t)i];
        out_counts[i] = parts.count[(size_t)i];
        over |= parts.count[(size_t)i] > capacity;
        hard |= parts.count[(size_t)i] > cap_eff && capacity > cap_eff;
    }
    if (out_offsets[nq] > total_capacity)
        return fail(h, MLVDB_ERR_OVERFLOW, "range query: more hits in all than total_capacity; out_counts / out_offsets hold "
                                           "the exact counts and the layout the hits need, out_labels / out_dist nothing");
    for (int64_t i = 0; i < nq; ++i) {
        const size_t n = (size_t)parts.len[(size_t)i];
        if (n == 0) continue;
        std::memcpy(out_labels + out_offsets[i], parts.lab.data() + parts.begin[(size_t)i], n * sizeof(int64_t));
        std::memcpy(out_dist + out_offsets[i], parts.dist.data() + parts.begin[(size_t)i], n * sizeof(float));
    }
    if (hard)
        return fail(h, MLVDB_ERR_UNSUPPORTED,
                    "range query: a query has more than MLVDB_MAX_TOPK_PAGED hits; out_counts holds the exact counts, the "
                    "outputs the nearest MLVDB_MAX_TOPK_PAGED");
    if (over) return fail(h, MLVDB_ERR_OVERFLOW, "some query has more hits than `capacity`; out_counts holds the exact counts");
    return MLVDB_OK;
    });
}

extern "C++" {
namespace {
// ---- distinct-by-attribute kNN (mlvdb_distinct.h)
constexpr int64_t kDistinctChunk = 1024;  // queries per round of list pass + pick + grouped scan (bounds the workspaces)

// Where a chunk's outputs lie in h->dist_out: n queries of k entries each
struct DistinctOut {
    double* d64 = nullptr;
    int64_t* grp = nullptr;
    int64_t* lab = nullptr;
    float* dist = nullptr;
    int32_t* cnt = nullptr;
    void take(Carver& c, size_t nk, size_t n) {
        d64 = c.take<double>(nk);
        grp = c.take<int64_t>(nk);
        lab = c.take<int64_t>(nk);
        dist = c.take<float>(nk);
        cnt = c.take<int32_t>(n);
    }
};

// L of the list pass: k <= 64 costs the filter path what k = 64 does, hence the floor; 0: no list pass
int32_t distinct_list_len(const mlvdb_index* h, int32_t k) {
    const int32_t os = h->tn.distinct_oversample;
    return os > 0 ? (int32_t)std::min<int64_t>(kDistinctMaxList, std::max<int64_t>(64, (int64_t)os * k)) : 0;
}

// One chunk of n <= kDistinctChunk queries (host pointer), outputs left on the device (`o`, enqueued on h->stream, not waited
// for): the plain device search for L neighbours -> the pick (final outputs of the complete queries, the others flagged) ->
// one synchronisation for the flagged count -> the grouped exact scan + merge of the flagged queries.
int distinct_chunk(mlvdb_index* h, const float* queries, int32_t n, int32_t k, int32_t k_eff, const int64_t* group, int32_t L,
                   DistinctOut& o) {
    hipStream_t s = h->stream;
    const size_t nk = (size_t)n * k;
    HIP_TRY(h, h->dist_q.ensure((size_t)n * h->dim * sizeof(float)));
    if (int rc = carve(h, h->dist_out, [&](Carver& c) { o.take(c, nk, (size_t)n); })) return rc;
    int32_t *nflag_d = nullptr, *qsel_d = nullptr;  // the flagged queries and their counter
    CARVE(h, h->dist_sel, [&](Carver& c) {
        nflag_d = c.take<int32_t>(1);
        qsel_d = c.take<int32_t>((size_t)n);
    });
    float* dq = h->dist_q.as<float>();
    HIP_TRY(h, hipMemcpyAsync(dq, queries, (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice, s));
    int32_t nsel = n;               // queries of the chunk the grouped scan serves
    const int32_t* qsel = nullptr;  // ... all of them without a list pass
    if (L > 0) {
        const size_t nl = (size_t)n * L;
        ListBlock l;
        if (int rc = carve_list(h, h->dist_list, nl, (size_t)n, l)) return rc;
        if (int rc = search_device_impl(h, dq, n, L, l.lab, l.dist, l.cnt, l.d64, s, false)) return rc;
        HIP_TRY(h, hipMemsetAsync(nflag_d, 0, sizeof(int32_t), s));
        HIP_TRY(h, launch_distinct_pick(l.lab, l.d64, l.cnt, n, L, group, k, k_eff, qsel_d, nflag_d, o.lab, o.dist, o.cnt,
                                        o.d64, o.grp, s));
        if (int rc = copy_down(h, s, {{&nsel, 0, nflag_d, 1}})) return rc;
        qsel = qsel_d;
        h->host_fallbacks += nsel;
    }
    if (nsel > 0) {
        HIP_TRY(h, h->qpad.ensure((size_t)n * h->ld * sizeof(float)));
        HIP_TRY(h, h->qaux.ensure((size_t)n * sizeof(double)));
        HIP_TRY(h, launch_query_prep(dq, n, h->dim, h->ld, h->space, h->qpad.as<float>(), h->qaux.as<double>(), nullptr, s));
        const ExactPlan plan = plan_distinct(h->total, h->ld, nsel, k);
        HIP_TRY(h, h->partial.ensure((size_t)nsel * plan.nblk * k * sizeof(DistinctEntry)));
        DistinctArgs a{};
        a.X = h->X;
        a.rn = h->rn;
        a.group = group;
        a.total = h->total;
        a.ld = h->ld;
        a.space = h->space;
        a.Qpad = h->qpad.as<float>();
        a.qaux = h->qaux.as<double>();
        a.qsel = qsel;
        a.nq_sel = nsel;
        a.nq_sel_dev = nullptr;
        a.k = k;
        a.partial = h->partial.as<DistinctEntry>();
        if (int rc = scan_step(h, s, h->total * plan.nqtiles, [&] { return launch_distinct_scan(a, plan, s); })) return rc;
        HIP_TRY(h, launch_distinct_merge(a.partial, nsel, nullptr, qsel, plan.nblk, k, k_eff, o.lab, o.dist, o.cnt, o.d64,
                                         o.grp, s));
        h->stats.strategy_used = MLVDB_STRATEGY_EXACT;
    }
    return MLVDB_OK;
}

// The validated call (h->rn is the masked copy when a program restricts the rows): distinct_chunk per chunk of queries, then
// its outputs to the host.
int distinct_impl(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t attr, int64_t max_groups,
                  int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64, int64_t* out_groups) {
    hipStream_t s = h->stream;
    const int32_t k_eff = max_groups > 0 ? (int32_t)std::min<int64_t>(k, max_groups) : k;
    if (h->total == 0 || h->total == h->deleted) {
        pad_outputs(out_labels, out_dist, out_dist64, nq * k, out_counts, nq);
        pad(out_groups, nq * k, INT64_MIN);
        return MLVDB_OK;
    }
    const int64_t* group = h->attr_col[attr];
    const int32_t L = distinct_list_len(h, k);
    for (int64_t q0 = 0; q0 < nq; q0 += kDistinctChunk) {
        const int32_t n = (int32_t)std::min<int64_t>(kDistinctChunk, nq - q0);
        const size_t nk = (size_t)n * k;
        DistinctOut o{};
        if (int rc = distinct_chunk(h, queries + (size_t)q0 * h->dim, n, k, k_eff, group, L, o)) return rc;
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{out_dist64, at, o.d64, nk}, {out_groups, at, o.grp, nk}, {out_labels, at, o.lab, nk},
                                      {out_dist, at, o.dist, nk}, {out_counts, (size_t)q0, o.cnt, (size_t)n}}))
            return rc;
    }
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_distinct(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t attr, int64_t max_groups,
                                const mlvdb_where* where, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                                double* out_dist64, int64_t* out_groups) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched (the program: with_where)
    if (int rc = int64_attr_check(h, attr, "distinct needs an int64 column")) return rc;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max(h, k, "distinct: ")) return rc;
    if (max_groups < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "max_groups < 0");
    if (nq > 0 && (!queries || !out_labels || !out_dist || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    auto call = [&]() {
        return distinct_impl(h, queries, nq, k, attr, max_groups, out_labels, out_dist, out_counts, out_dist64, out_groups);
    };
    return with_where(h, where, nq, call);
    });
}

// ---- grouped kNN (mlvdb_grouped.h)
extern "C++" {
namespace {
// padding of the nq queries of a grouped call, on the host
void grouped_pad(int64_t nq, int32_t k, int32_t gsz, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                 int32_t* out_gcnt, double* out_dist64, int64_t* out_groups) {
    pad_outputs(out_labels, out_dist, out_dist64, nq * k * gsz, out_counts, nq);
    pad(out_gcnt, nq * k, 0);
    pad(out_groups, nq * k, INT64_MIN);
}

// The member stage of one chunk of n queries: grp / cnt are the distinct stage's group codes [n, k] and counts [n] on the host,
// h->dist_q holds the chunk's raw queries.  Member lists of the picked codes (count, prefix sum, fill), tiles, the gathered
// kernel, the merge -- outputs left in h->grp_out (`o`: n * k * gsz entries, n * k group counts), complete on return.
int grouped_members(mlvdb_index* h, int32_t n, int32_t k, int32_t gsz, int32_t qt_max, const int64_t* col, const int64_t* grp,
                    const int32_t* cnt, ListBlock& o) {
    hipStream_t s = h->stream;
    const int32_t nslots = n * k;
    // the (code, slot) pairs sorted by code, then by query: queries sharing a document share its rows' loads
    std::vector<std::pair<int64_t, int32_t>> picked;
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < cnt[i]; ++j) picked.emplace_back(grp[(size_t)i * k + j], i * k + j);
    std::sort(picked.begin(), picked.end());
    const int32_t npairs = (int32_t)picked.size();
    std::vector<int32_t> first;  // first pair of every distinct code, and npairs
    for (int32_t p = 0; p < npairs; ++p)
        if (p == 0 || picked[p].first != picked[p - 1].first) first.push_back(p);
    const size_t ncodes = first.size();
    first.push_back(npairs);
    // the open-addressing table: the smallest power of two >= 2 x the number of codes
    uint64_t slots = 1;
    while (slots < 2 * (uint64_t)std::max<size_t>(ncodes, 1)) slots *= 2;
    std::vector<int64_t> keys(slots, INT64_MIN);
    std::vector<uint32_t> slot_of(ncodes);
    for (size_t u = 0; u < ncodes; ++u) {
        uint64_t at = facet_hash(picked[first[u]].first) & (slots - 1);
        while (keys[at] != INT64_MIN) at = (at + 1) & (slots - 1);
        keys[at] = picked[first[u]].first;
        slot_of[u] = (uint32_t)at;
    }
    long long* keys_d = nullptr;
    uint32_t* counts_d = nullptr;  // counts, then the fill's cursors
    CARVE(h, h->grp_tab, [&](Carver& c) {
        keys_d = c.take<long long>(slots);
        counts_d = c.take<uint32_t>(slots);
    });
    std::vector<uint32_t> counts(slots, 0);
    if (npairs > 0) {
        HIP_TRY(h, hipMemcpyAsync(keys_d, keys.data(), slots * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemsetAsync(counts_d, 0, slots * sizeof(uint32_t), s));
        HIP_TRY(h, launch_grouped_count(h->rn, col, h->total, keys_d, slots, counts_d, s));
        if (int rc = copy_down(h, s, {{counts.data(), 0, counts_d, slots}})) return rc;
    }
    // prefix sum over the slots: list begins (the fill's cursors)
    std::vector<uint32_t> begin(slots, 0);
    int64_t members = 0;
    for (uint64_t t = 0; t < slots; ++t) {
        begin[t] = (uint32_t)members;
        members += counts[t];
    }
    if (members > h->total - h->deleted || members > INT32_MAX) return fail(h, MLVDB_ERR_INTERNAL, "grouped: more members than live rows");
    if (members > 0) {
        HIP_TRY(h, h->grp_lab.ensure((size_t)members * sizeof(int32_t)));
        HIP_TRY(h, hipMemcpyAsync(counts_d, begin.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, launch_grouped_fill(h->rn, col, h->total, keys_d, slots, counts_d, h->grp_lab.as<int32_t>(), s));
    }
    // tiles: <= qt_max pairs of one group against one chunk of its list; the rows per chunk from the work of the whole chunk of
    // queries (grouped_chunk_rows); tiles of 1 / 2 / 3-4 pairs take the QT = 1 / 2 / 4 instance
    int64_t work = 0;
    for (size_t u = 0; u < ncodes; ++u)
        work += (int64_t)((first[u + 1] - first[u] + qt_max - 1) / qt_max) * counts[slot_of[u]];
    const int64_t chunk_rows = grouped_chunk_rows(work);
    std::vector<GroupedTile> tiles[3];  // by instance: QT 1, 2, 4
    std::vector<GroupedPair> pairs((size_t)npairs);
    std::vector<int32_t> pair_of_slot((size_t)nslots, -1);
    int64_t nparts = 0;
    for (size_t u = 0; u < ncodes; ++u) {
        const int64_t c = counts[slot_of[u]], b = begin[slot_of[u]];
        const int32_t nch = (int32_t)std::max<int64_t>(1, (c + chunk_rows - 1) / chunk_rows);
        for (int32_t p0 = first[u]; p0 < first[u + 1];) {
            const int32_t take = std::min(qt_max, first[u + 1] - p0);
            const int cls = take == 1 ? 0 : take == 2 ? 1 : 2;
            for (int32_t t = 0; t < take; ++t) {
                pairs[(size_t)p0 + t] = GroupedPair{picked[(size_t)p0 + t].second / k, (int32_t)(nparts + (int64_t)t * nch), nch, 0};
                pair_of_slot[(size_t)picked[(size_t)p0 + t].second] = p0 + t;
            }
            for (int32_t ch = 0; ch < nch; ++ch) {
                const int64_t lo = std::min<int64_t>(c, ch * chunk_rows), hi = std::min<int64_t>(c, lo + chunk_rows);
                tiles[cls].push_back(GroupedTile{(int32_t)(b + lo), (int32_t)(hi - lo), p0, take, (int32_t)(nparts + ch), nch});
            }
            nparts += (int64_t)take * nch;
            p0 += take;
        }
    }
    if (nparts * gsz > INT32_MAX) return fail(h, MLVDB_ERR_INTERNAL, "grouped: partial lists beyond 2^31 entries");
    GroupedTile* tiles_d[3] = {};
    GroupedPair* pairs_d = nullptr;
    int32_t* pos_d = nullptr;
    CARVE(h, h->grp_tiles, [&](Carver& c) {
        for (int cls = 0; cls < 3; ++cls) tiles_d[cls] = c.take<GroupedTile>(tiles[cls].size());
        c.pad_to(16);
        pairs_d = c.take<GroupedPair>(pairs.size());
        pos_d = c.take<int32_t>(pair_of_slot.size());
        c.take<char>(16);  // slack
    });
    for (int cls = 0; cls < 3; ++cls)
        if (!tiles[cls].empty())
            HIP_TRY(h, hipMemcpyAsync(tiles_d[cls], tiles[cls].data(), tiles[cls].size() * sizeof(GroupedTile), hipMemcpyHostToDevice, s));
    if (npairs > 0) HIP_TRY(h, hipMemcpyAsync(pairs_d, pairs.data(), pairs.size() * sizeof(GroupedPair), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(pos_d, pair_of_slot.data(), pair_of_slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // the chunk's queries, prepared as every exact path prepares them, staged by query index
    HIP_TRY(h, h->qpad.ensure((size_t)n * h->ld * sizeof(float)));
    HIP_TRY(h, h->qaux.ensure((size_t)n * sizeof(double)));
    HIP_TRY(h, launch_query_prep(h->dist_q.as<float>(), n, h->dim, h->ld, h->space, h->qpad.as<float>(), h->qaux.as<double>(),
                                 nullptr, s));
    HIP_TRY(h, h->partial.ensure((size_t)std::max<int64_t>(nparts, 1) * gsz * sizeof(TopEntry)));
    static const int32_t kQt[3] = {1, 2, 4};
    for (int cls = 0; cls < 3; ++cls)
        HIP_TRY(h, launch_grouped_gather(h->X, h->qpad.as<float>(), h->qaux.as<double>(), h->grp_lab.as<int32_t>(), tiles_d[cls],
                                         (int32_t)tiles[cls].size(), pairs_d, h->ld, h->space, kQt[cls], gsz,
                                         h->partial.as<TopEntry>(), s));
    if (int rc = carve_list(h, h->grp_out, (size_t)nslots * gsz, (size_t)nslots, o)) return rc;  // (its counts: the group counts)
    HIP_TRY(h, launch_grouped_merge(h->partial.as<TopEntry>(), pairs_d, pos_d, nslots, gsz, o.lab, o.dist, o.d64, o.cnt, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // (the host vectors above are consumed by now)
    return MLVDB_OK;
}

// The validated call (h->rn is the masked copy when a program restricts the rows).  Per chunk of queries: the distinct stage
// with its outputs left on the device -> group codes and counts to the host -> the member stage -> outputs to the host.
int grouped_impl(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t gsz, int32_t qt_max, int32_t attr,
                 int64_t max_groups, int64_t* out_labels, float* out_dist, int32_t* out_counts, int32_t* out_gcnt,
                 double* out_dist64, int64_t* out_groups) {
    hipStream_t s = h->stream;
    if (h->total == 0 || h->total == h->deleted) {
        grouped_pad(nq, k, gsz, out_labels, out_dist, out_counts, out_gcnt, out_dist64, out_groups);
        return MLVDB_OK;
    }
    const int32_t k_eff = max_groups > 0 ? (int32_t)std::min<int64_t>(k, max_groups) : k;
    const int64_t* col = h->attr_col[attr];
    const int32_t L = distinct_list_len(h, k);
    std::vector<int64_t> grp;
    std::vector<int32_t> cnt;
    for (int64_t q0 = 0; q0 < nq; q0 += kDistinctChunk) {
        const int32_t n = (int32_t)std::min<int64_t>(kDistinctChunk, nq - q0);
        const size_t nk = (size_t)n * k, ng = nk * gsz;
        DistinctOut o{};
        if (int rc = distinct_chunk(h, queries + (size_t)q0 * h->dim, n, k, k_eff, col, L, o)) return rc;
        grp.resize(nk);
        cnt.resize((size_t)n);
        if (int rc = copy_down(h, s, {{grp.data(), 0, o.grp, nk}, {cnt.data(), 0, o.cnt, (size_t)n}})) return rc;
        ListBlock m;
        if (int rc = grouped_members(h, n, k, gsz, qt_max, col, grp.data(), cnt.data(), m)) return rc;
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{out_dist64, at * gsz, m.d64, ng}, {out_labels, at * gsz, m.lab, ng},
                                      {out_dist, at * gsz, m.dist, ng}, {out_gcnt, at, m.cnt, nk}}))
            return rc;
        if (out_groups) std::memcpy(out_groups + at, grp.data(), nk * sizeof(int64_t));
        std::memcpy(out_counts + q0, cnt.data(), (size_t)n * sizeof(int32_t));
    }
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_grouped(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t group_size, int32_t attr,
                               int64_t max_groups, const mlvdb_where* where, int64_t* out_labels, float* out_dist,
                               int32_t* out_counts, int32_t* out_group_counts, double* out_dist64, int64_t* out_groups) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched (the program: with_where)
    if (int rc = int64_attr_check(h, attr, "grouped needs an int64 column")) return rc;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (group_size < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "group_size must be >= 1");
    if (int rc = check_k_max(h, k, "grouped: ")) return rc;
    if (group_size > kGroupedMaxSize) return fail(h, MLVDB_ERR_UNSUPPORTED, "grouped: group_size above MLVDB_GROUPED_MAX_SIZE");
    if (max_groups < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "max_groups < 0");
    if (nq > 0 && (!queries || !out_labels || !out_dist || !out_counts || !out_group_counts))
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    const int32_t qt = gather_qt(h);  // pairs per tile of the gathered kernel
    if (where_gather_lds(qt, h->ld) > 64 * 1024)
        return fail(h, MLVDB_ERR_UNSUPPORTED, "grouped: one query of this dimension needs more than 64 KiB of LDS");
    auto call = [&]() {
        return grouped_impl(h, queries, nq, k, group_size, qt, attr, max_groups, out_labels, out_dist, out_counts,
                            out_group_counts, out_dist64, out_groups);
    };
    return with_where(h, where, nq, call);
    });
}

// ---- diversified kNN (mlvdb_mmr.h)
extern "C++" {
namespace {
constexpr int64_t kMmrChunk = 1024;  // queries per round of plain search + selection (bounds the workspaces)

// The validated call (h->rn is the masked copy when a program restricts the rows).  Per chunk of queries: the plain device
// search for fetch_k neighbours (fp64 distances wanted) -> one launch of the select kernel -> outputs to the host.
int mmr_impl(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t fetch_k, double lambda, int64_t* out_labels,
             float* out_dist, int32_t* out_counts, double* out_dist64, int32_t* out_rank, double* out_objective) {
    hipStream_t s = h->stream;
    if (h->total == 0 || h->total == h->deleted) {
        pad_outputs(out_labels, out_dist, out_dist64, nq * k, out_counts, nq);
        pad(out_rank, nq * k, -1);
        pad(out_objective, nq * k, __builtin_inf());
        return MLVDB_OK;
    }
    const double one_minus_lambda = 1.0 - lambda;  // formed once, here
    for (int64_t q0 = 0; q0 < nq; q0 += kMmrChunk) {
        const int32_t n = (int32_t)std::min<int64_t>(kMmrChunk, nq - q0);
        const size_t nk = (size_t)n * k, nl = (size_t)n * fetch_k;
        HIP_TRY(h, h->mmr_q.ensure((size_t)n * h->dim * sizeof(float)));
        ListBlock l;
        if (int rc = carve_list(h, h->mmr_list, nl, (size_t)n, l)) return rc;
        double *o_d64 = nullptr, *o_obj = nullptr;
        int64_t* o_lab = nullptr;
        float* o_dist = nullptr;
        int32_t *o_rank = nullptr, *o_cnt = nullptr;
        CARVE(h, h->mmr_out, [&](Carver& c) {
            o_d64 = c.take<double>(nk);
            o_obj = c.take<double>(nk);
            o_lab = c.take<int64_t>(nk);
            o_dist = c.take<float>(nk);
            o_rank = c.take<int32_t>(nk);
            o_cnt = c.take<int32_t>((size_t)n);
        });
        float* dq = h->mmr_q.as<float>();
        HIP_TRY(h, hipMemcpyAsync(dq, queries + (size_t)q0 * h->dim, (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice, s));
        if (int rc = search_device_impl(h, dq, n, fetch_k, l.lab, l.dist, l.cnt, l.d64, s, false)) return rc;
        HIP_TRY(h, launch_mmr_select(h->X, h->dim, h->ld, h->space, l.lab, l.dist, l.d64, l.cnt, n, fetch_k, k, lambda,
                                     one_minus_lambda, o_lab, o_dist, o_cnt, o_d64, o_rank, o_obj, s));
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{out_dist64, at, o_d64, nk}, {out_objective, at, o_obj, nk}, {out_rank, at, o_rank, nk},
                                      {out_labels, at, o_lab, nk}, {out_dist, at, o_dist, nk},
                                      {out_counts, (size_t)q0, o_cnt, (size_t)n}}))
            return rc;
    }
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_mmr(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t fetch_k, double lambda,
                           const mlvdb_where* where, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                           double* out_dist64, int32_t* out_rank, double* out_objective) {
    return guarded(h, [&]() -> int {
    int rc = check_handle(h);
    if (rc) return rc;
    // everything is checked before anything is launched (the program: with_where)
    if (nq < 0 || nq > (1 << 24)) return fail(h, MLVDB_ERR_INVALID_ARG, "nq out of range");
    if (k < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "k must be >= 1");
    if (k > MLVDB_MAX_TOPK) return fail(h, MLVDB_ERR_UNSUPPORTED, "mmr: k above MLVDB_MAX_TOPK");
    if (fetch_k < k) return fail(h, MLVDB_ERR_INVALID_ARG, "mmr: fetch_k below k");
    if (fetch_k > kMmrMaxFetch) return fail(h, MLVDB_ERR_UNSUPPORTED, "mmr: fetch_k above MLVDB_MMR_MAX_FETCH");
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(h, MLVDB_ERR_INVALID_ARG, "mmr: lambda outside [0, 1]");
    if (mmr_select_lds(h->ld, fetch_k) > 64 * 1024)
        return fail(h, MLVDB_ERR_UNSUPPORTED, "mmr: the picked row and fetch_k candidates need more than 64 KiB of LDS");
    if (nq > 0 && (!queries || !out_labels || !out_dist || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    auto call = [&]() {
        return mmr_impl(h, queries, nq, k, fetch_k, lambda, out_labels, out_dist, out_counts, out_dist64, out_rank,
                        out_objective);
    };
    // the first launches: where_run(h, where, ...) for the program, then mmr_impl under with_row_mask(h, nq, ...)
    return with_where(h, where, nq, call);
    });
}

// ---- search by stored examples (mlvdb_like.h)
extern "C++" {
namespace {
constexpr int64_t kLikeChunk = 1024;  // queries per round of synthesis + plain search + strip (bounds the workspaces)

// The validated call (h->rn is the masked copy when a program restricts the rows; the examples' values are read from h->X,
// which no mask touches).  Per chunk of queries: examples (+ base rows) to the device -> one launch of the query kernel ->
// the plain device search for `fetch` neighbours (fp64 distances wanted) -> one launch of the strip kernel -> outputs to
// the host.
int like_impl(mlvdb_index* h, const int64_t* ex_labels, const double* ex_weights, const int64_t* ex_offsets, const float* base,
              int64_t nq, int32_t k, int32_t fetch, int32_t exclude, int64_t* out_labels, float* out_dist, int32_t* out_counts,
              double* out_dist64, float* out_queries) {
    hipStream_t s = h->stream;
    if (h->total == 0) {  // no row, so no example: every query is its base row
        pad_outputs(out_labels, out_dist, out_dist64, nq * k, out_counts, nq);
        if (out_queries && base) std::memcpy(out_queries, base, (size_t)nq * h->dim * sizeof(float));
        return MLVDB_OK;
    }
    std::vector<int64_t> off((size_t)kLikeChunk + 1);  // a chunk's own offsets
    for (int64_t q0 = 0; q0 < nq; q0 += kLikeChunk) {
        const int32_t n = (int32_t)std::min<int64_t>(kLikeChunk, nq - q0);
        const size_t nk = (size_t)n * k, nl = (size_t)n * fetch, nd = (size_t)n * h->dim;
        const int64_t e0 = ex_offsets[q0];
        const size_t ne = (size_t)(ex_offsets[q0 + n] - e0);
        for (int32_t i = 0; i <= n; ++i) off[(size_t)i] = ex_offsets[q0 + i] - e0;  // (the last chunk's copy has completed)
        float *dq = nullptr, *dbase = nullptr;
        CARVE(h, h->like_q, [&](Carver& c) {
            dq = c.take<float>(nd);
            if (base) dbase = c.take<float>(nd);
        });
        double* e_w = nullptr;
        int64_t *e_lab = nullptr, *e_off = nullptr;
        CARVE(h, h->like_ex, [&](Carver& c) {
            e_w = c.take<double>(ne);
            e_lab = c.take<int64_t>(ne);
            e_off = c.take<int64_t>((size_t)n + 1);
        });
        ListBlock l, o;
        if (int rc = carve_list(h, h->like_list, nl, (size_t)n, l)) return rc;
        if (int rc = carve_list(h, h->like_out, nk, (size_t)n, o)) return rc;
        if (ne > 0) {
            HIP_TRY(h, hipMemcpyAsync(e_w, ex_weights + e0, ne * sizeof(double), hipMemcpyHostToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(e_lab, ex_labels + e0, ne * sizeof(int64_t), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(h, hipMemcpyAsync(e_off, off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (base) HIP_TRY(h, hipMemcpyAsync(dbase, base + (size_t)q0 * h->dim, nd * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(h, launch_like_query(h->X, h->dim, h->ld, h->space, e_lab, e_w, e_off, dbase, n, dq, s));
        if (int rc = search_device_impl(h, dq, n, fetch, l.lab, l.dist, l.cnt, l.d64, s, false)) return rc;
        HIP_TRY(h, launch_like_strip(l.lab, l.dist, l.d64, l.cnt, n, fetch, e_lab, e_off, exclude, k, o.lab, o.dist, o.cnt, o.d64, s));
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{out_dist64, at, o.d64, nk}, {out_queries, (size_t)q0 * h->dim, dq, nd},
                                      {out_labels, at, o.lab, nk}, {out_dist, at, o.dist, nk},
                                      {out_counts, (size_t)q0, o.cnt, (size_t)n}}))
            return rc;
    }
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_like(mlvdb_index* h, const int64_t* example_labels, const double* example_weights,
                            const int64_t* example_offsets, const float* base_queries, int64_t nq, int32_t k,
                            int32_t exclude_examples, const mlvdb_where* where, int64_t* out_labels, float* out_dist,
                            int32_t* out_counts, double* out_dist64, float* out_queries) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched (the program: with_where)
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (k > kLikeMaxFetch) return fail(h, MLVDB_ERR_UNSUPPORTED, "like: k above MLVDB_LIKE_MAX_FETCH");
    if (nq > 0 && (!example_offsets || !out_labels || !out_dist || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    int32_t most = 0;  // M: the most distinct example labels of one query
    if (nq > 0) {
        if (example_offsets[0] != 0) return fail(h, MLVDB_ERR_INVALID_ARG, "like: example_offsets must start at 0");
        for (int64_t i = 0; i < nq; ++i)
            if (example_offsets[i + 1] < example_offsets[i])
                return fail(h, MLVDB_ERR_INVALID_ARG, "like: example_offsets must ascend");
        if (example_offsets[nq] > 0 && (!example_labels || !example_weights)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
        int64_t seen[kLikeMaxExamples];
        for (int64_t i = 0; i < nq; ++i) {
            const int64_t e0 = example_offsets[i], m = example_offsets[i + 1] - e0;
            if (m > kLikeMaxExamples) return fail(h, MLVDB_ERR_UNSUPPORTED, "like: more than MLVDB_LIKE_MAX_EXAMPLES examples in a query");
            if (m == 0 && !base_queries) return fail(h, MLVDB_ERR_INVALID_ARG, "like: a query with no example and no base row");
            for (int64_t j = 0; j < m; ++j) {
                const int64_t label = example_labels[e0 + j];
                if (label < 0 || label >= h->total) return fail(h, MLVDB_ERR_INVALID_ARG, "like: example label out of range");
                if (!std::isfinite(example_weights[e0 + j])) return fail(h, MLVDB_ERR_INVALID_ARG, "like: example weight not finite");
                seen[j] = label;
            }
            std::sort(seen, seen + m);
            most = std::max(most, (int32_t)(std::unique(seen, seen + m) - seen));
        }
    }
    if (k + most > kLikeMaxFetch) return fail(h, MLVDB_ERR_UNSUPPORTED, "like: k + examples above MLVDB_LIKE_MAX_FETCH");
    const int32_t fetch = exclude_examples ? k + most : k;
    auto call = [&]() {
        return like_impl(h, example_labels, example_weights, example_offsets, base_queries, nq, k, fetch, exclude_examples,
                         out_labels, out_dist, out_counts, out_dist64, out_queries);
    };
    // the first launches: where_run(h, where, ...) for the program, then like_impl under with_row_mask(h, nq, ...)
    return with_where(h, where, nq, call);
    });
}

// ---- similarity join (mlvdb_join.h)
extern "C++" {
namespace {
// Room for `need` packed hits behind the `used` the call already holds (join_lab / join_dist grow by doubling, bounded by the
// caller's total_capacity; what they hold moves along).
int join_reserve(mlvdb_index* h, hipStream_t s, int64_t used, int64_t need, int64_t total_capacity) {
    const int64_t have = (int64_t)(h->join_lab.bytes / sizeof(int64_t));
    if (need <= have && (size_t)need * sizeof(float) <= h->join_dist.bytes) return MLVDB_OK;
    const int64_t cap = std::min<int64_t>(total_capacity, std::max<int64_t>({need, 2 * have, 65536}));
    Staged<DevBuf> nl(s), nd(s);
    HIP_TRY(h, nl.exact((size_t)cap * sizeof(int64_t)));
    HIP_TRY(h, nd.exact((size_t)cap * sizeof(float)));
    if (used > 0) {
        HIP_TRY(h, hipMemcpyAsync(nl.p, h->join_lab.p, (size_t)used * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(nd.p, h->join_dist.p, (size_t)used * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    h->join_lab = std::move(nl);
    h->join_dist = std::move(nd);
    return MLVDB_OK;
}

// The validated call, under with_row_mask: h->rn is the masked copy of the norms (`where`, or every live row), and
// h->rp8_masked that of the row pairs when the int8 shadow serves the call.  Per wave of <= kJoinWave left rows: their values
// gathered into h->io_q -> LATER: the rows below the wave's first label leave the masked copies -> the range passes at
// capacity + kJoinWave, the filter scan starting at that label's tile -> strip -> counts to the host -> pack.  A row whose
// truncated list cannot give its count (LATER, not the head of its wave) heads the next wave: a wave always resolves its
// first row, so the call ends.
int join_impl(mlvdb_index* h, const int64_t* left, int64_t n_left, int32_t mode, float radius, int64_t capacity,
              int64_t total_capacity, int64_t* out_labels, float* out_dist, int64_t* out_offsets, int64_t* out_counts) {
    hipStream_t s = h->stream;
    int rc = begin_call(h, s);
    if (rc) return rc;
    const int64_t cap_eff = capacity + kJoinWave;  // the wave's own rows may stand in the way of the nearest `capacity`
    const bool later = mode == MLVDB_JOIN_LATER;
    const bool want_hits = total_capacity > 0;
    HIP_TRY(h, h->join_left.ensure((size_t)n_left * sizeof(int64_t)));
    HIP_TRY(h, hipMemcpyAsync(h->join_left.p, left, (size_t)n_left * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, h->io_q.ensure((size_t)kJoinWave * h->dim * sizeof(float)));  // (range_ranked asks for no more: no regrowth there)
    int64_t *w_lab = nullptr, *w_count = nullptr, *d_lab = nullptr;
    double* w_self = nullptr;
    int32_t *w_kept = nullptr, *w_flag = nullptr;
    float* d_dist = nullptr;
    CARVE(h, h->join_ws, [&](Carver& c) {
        w_lab = c.take<int64_t>(kJoinWave);
        w_count = c.take<int64_t>(kJoinWave);
        w_self = c.take<double>(kJoinWave);
        d_lab = c.take<int64_t>((size_t)kJoinWave * capacity);
        d_dist = c.take<float>((size_t)kJoinWave * capacity);
        w_kept = c.take<int32_t>(kJoinWave);
        w_flag = c.take<int32_t>(kJoinWave);
    });
    std::vector<int64_t> kept_of((size_t)n_left, 0), start_of((size_t)n_left, 0);
    std::vector<int64_t> redo, wave, wave_labels, counts, offsets;
    int64_t h_count[kJoinWave];
    int32_t h_kept[kJoinWave], h_flag[kJoinWave];
    int64_t next = 0, hidden = 0, used = 0;  // left rows taken; LATER: labels [0, hidden) are masked out; packed hits so far
    bool in_order = true, fits = true, over = false;
    while (next < n_left || !redo.empty()) {
        const int64_t* labels_d = nullptr;
        wave.clear();
        if (!redo.empty()) {  // rows of the last wave again, the first flagged one at the head
            wave.swap(redo);
            wave_labels.resize(wave.size());
            for (size_t j = 0; j < wave.size(); ++j) wave_labels[j] = left[wave[j]];
            HIP_TRY(h, hipMemcpyAsync(w_lab, wave_labels.data(), wave.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
            labels_d = w_lab;
            in_order = false;
        } else {
            const int64_t n = std::min<int64_t>(kJoinWave, n_left - next);
            for (int64_t j = 0; j < n; ++j) wave.push_back(next + j);
            labels_d = h->join_left.as<int64_t>() + next;
            next += n;
        }
        const int32_t n = (int32_t)wave.size();
        const int64_t a_lo = left[wave[0]];
        HIP_TRY(h, launch_join_gather_queries(h->X, labels_d, n, h->dim, h->ld, h->io_q.as<float>(), s));
        if (later && a_lo > hidden) {
            HIP_TRY(h, launch_join_mask_advance(h->rn, h->mask_pairs_ready ? h->rp8_masked.as<float>() : nullptr,
                                                h->space == kSpaceL2 ? 1 : 0, hidden, a_lo, s));
            // (the l2 offsets plane behind the masked pairs was computed from the pairs of the last wave)
            if (h->mask_pairs_ready)
                if (int rc2 = forget_l2_offsets(h, 1, s)) return rc2;
            hidden = a_lo;
        }
        rc = range_ranked(h, s, nullptr, n, radius, cap_eff, counts, offsets, later ? a_lo : 0);
        if (rc) return rc;
        bool truncated = false;
        for (int32_t j = 0; j < n; ++j) truncated |= counts[(size_t)j] > cap_eff;
        if (truncated)  // the distance of each row to itself, with the bits the range passes gave it (their Qpad / qaux)
            HIP_TRY(h, launch_pair_distances(h->X, h->qpad.as<float>(), h->qaux.as<double>(), labels_d, n, 1, h->ld, h->space,
                                             w_self, nullptr, s));
        HIP_TRY(h, launch_join_strip(h->io_lab.as<int64_t>(), h->io_dist.as<float>(), h->io_cnt.as<int64_t>(), cap_eff, labels_d,
                                     n, mode, truncated ? w_self : nullptr, radius, h->rn, capacity, d_lab, d_dist, w_count,
                                     w_kept, w_flag, s));
        rc = copy_down(h, s, {{h_count, 0, w_count, (size_t)n}, {h_kept, 0, w_kept, (size_t)n}, {h_flag, 0, w_flag, (size_t)n}});
        if (rc) return rc;
        const int64_t base = used;
        for (int32_t j = 0; j < n; ++j) {
            const size_t i = (size_t)wave[(size_t)j];
            if (h_flag[j]) {
                redo.push_back(wave[(size_t)j]);
                continue;
            }
            out_counts[i] = h_count[j];
            over |= h_count[j] > capacity;
            kept_of[i] = h_kept[j];
            start_of[i] = used;
            used += h_kept[j];
        }
        fits = fits && used <= total_capacity;
        if (want_hits && fits && used > base) {
            rc = join_reserve(h, s, base, used, total_capacity);
            if (rc) return rc;
            HIP_TRY(h, launch_join_pack(d_lab, d_dist, w_kept, w_flag, n, capacity, base, h->join_lab.as<int64_t>(),
                                        h->join_dist.as<float>(), s));
        }
    }
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n_left; ++i) out_offsets[i + 1] = out_offsets[i] + kept_of[(size_t)i];
    if (fits && used > 0) {
        if (in_order) {  // the packed array is the answer
            rc = copy_down(h, s, {{out_labels, 0, h->join_lab.as<int64_t>(), (size_t)used},
                                  {out_dist, 0, h->join_dist.as<float>(), (size_t)used}});
            if (rc) return rc;
        } else {  // some rows were resolved after later ones: their hits move to their places on the host
            std::vector<int64_t> p_lab((size_t)used);
            std::vector<float> p_dist((size_t)used);
            rc = copy_down(h, s, {{p_lab.data(), 0, h->join_lab.as<int64_t>(), (size_t)used},
                                  {p_dist.data(), 0, h->join_dist.as<float>(), (size_t)used}});
            if (rc) return rc;
            for (int64_t i = 0; i < n_left; ++i) {
                const size_t m = (size_t)kept_of[(size_t)i];
                if (!m) continue;
                std::memcpy(out_labels + out_offsets[i], p_lab.data() + start_of[(size_t)i], m * sizeof(int64_t));
                std::memcpy(out_dist + out_offsets[i], p_dist.data() + start_of[(size_t)i], m * sizeof(float));
            }
        }
    }
    rc = end_call(h, s);
    if (rc) return rc;
    if (!fits)
        return fail(h, MLVDB_ERR_OVERFLOW, "join: more hits in all than total_capacity; out_counts / out_offsets hold the exact "
                                           "counts and the layout the hits need, out_labels / out_dist nothing");
    if (over) return fail(h, MLVDB_ERR_OVERFLOW, "join: some row has more partners than `capacity`; out_counts holds the exact counts");
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_join_within(mlvdb_index* h, const int64_t* left_labels, int64_t n_left, int32_t mode, float radius,
                      int64_t capacity, int64_t total_capacity, const mlvdb_where* where, int64_t* out_labels,
                      float* out_dist, int64_t* out_offsets, int64_t* out_counts) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched (the program: where_run validates it first)
    if (int rc = check_nq(h, n_left)) return rc;
    if (mode != MLVDB_JOIN_OTHERS && mode != MLVDB_JOIN_LATER) return fail(h, MLVDB_ERR_INVALID_ARG, "join: unknown mode");
    if (capacity < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "capacity must be >= 1");
    if (total_capacity < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "total_capacity must be >= 0");
    if (capacity > MLVDB_JOIN_MAX_CAPACITY) return fail(h, MLVDB_ERR_UNSUPPORTED, "join: capacity above MLVDB_JOIN_MAX_CAPACITY");
    if (!out_offsets || (n_left > 0 && (!left_labels || !out_counts)) || (total_capacity > 0 && (!out_labels || !out_dist)))
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    for (int64_t i = 0; i < n_left; ++i) {
        if (left_labels[i] < 0 || left_labels[i] >= h->total) return fail(h, MLVDB_ERR_INVALID_ARG, "join: left label out of range");
        if (i > 0 && left_labels[i] <= left_labels[i - 1])
            return fail(h, MLVDB_ERR_INVALID_ARG, "join: left labels must ascend strictly");
    }
    if (where)
        if (int rc = where_prepare(h, where)) return rc;
    if (n_left == 0 || h->total == h->deleted) {  // no left row, or no live row to be a partner
        for (int64_t i = 0; i < n_left; ++i) out_counts[i] = 0;
        for (int64_t i = 0; i <= n_left; ++i) out_offsets[i] = 0;
        return MLVDB_OK;
    }
    if (where) {
        if (int rc = where_run(h, where, nullptr)) return rc;
    } else {  // the call always runs under a row mask: all ones
        HIP_TRY(h, h->row_mask.ensure((size_t)h->total));
        HIP_TRY(h, hipMemsetAsync(h->row_mask.p, 1, (size_t)h->total, h->stream));
    }
    return with_row_mask(h, std::min<int64_t>(n_left, kJoinWave), [&]() {
        return join_impl(h, left_labels, n_left, mode, radius, capacity, total_capacity, out_labels, out_dist, out_offsets,
                         out_counts);
    });
    });
}

// ---- facet counts and histograms (mlvdb_facet.h)
extern "C++" {
namespace {
// The program of a facet call on the device (where == nullptr: no program, n_ops 0); validated by the caller.
struct DevProgram {
    const WhereOp* ops = nullptr;
    int32_t n_ops = 0;
    const int64_t* set = nullptr;
};

int facet_program(mlvdb_index* h, const mlvdb_where* where, DevProgram& pg) {
    if (!where) return MLVDB_OK;
    if (int rc = where_upload(h, where, &pg.set)) return rc;
    pg.ops = h->where_prog.as<WhereOp>();
    pg.n_ops = where->n_ops;
    return MLVDB_OK;
}

// (list: the column is a list column and every value of a row's list counts -- mlvdb_facet_list_values)
int facet_values_run(mlvdb_index* h, int32_t attr, const mlvdb_where* where, int64_t max_values, int64_t* out_values,
                     int64_t* out_counts, int64_t* n_values, int64_t* matched, int64_t* absent, bool list) {
    hipStream_t s = h->stream;
    DevProgram pg;
    if (int rc = facet_program(h, where, pg)) return rc;
    uint64_t slots = 64;  // a power of two >= 2 max_values: the table is at most half full when the call succeeds
    while (slots < 2 * (uint64_t)max_values) slots *= 2;
    FacetTable t{};
    long long* packed_keys = nullptr;
    unsigned long long* packed_counts = nullptr;
    CARVE(h, h->facet_tab, [&](Carver& c) {
        t.keys = c.take<unsigned long long>(slots);
        t.counts = c.take<unsigned long long>(slots);
        packed_keys = c.take<long long>((size_t)max_values);
        packed_counts = c.take<unsigned long long>((size_t)max_values);
    });
    HIP_TRY(h, h->facet_misc.ensure(kFacetCounters * sizeof(unsigned long long)));
    t.mask = slots - 1;
    t.max_values = (unsigned long long)max_values;
    t.ctr = h->facet_misc.as<unsigned long long>();
    HIP_TRY(h, launch_attr_fill(reinterpret_cast<int64_t*>(t.keys), INT64_MIN, 0, (int64_t)slots, s));
    HIP_TRY(h, hipMemsetAsync(t.counts, 0, slots * sizeof(unsigned long long), s));
    HIP_TRY(h, hipMemsetAsync(t.ctr, 0, kFacetCounters * sizeof(unsigned long long), s));
    if (list)
        HIP_TRY(h, launch_facet_list_values(pg.ops, pg.n_ops, pg.set, h->rn, h->attr_col[attr], h->list_pool[attr], h->total, t, s));
    else
        HIP_TRY(h, launch_facet_values(pg.ops, pg.n_ops, pg.set, h->rn, h->attr_col[attr], h->total, t, s));
    HIP_TRY(h, launch_facet_collect(t, packed_keys, packed_counts, s));
    unsigned long long ctr[kFacetCounters] = {};
    HIP_TRY(h, hipMemcpyAsync(ctr, t.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *matched = (int64_t)ctr[kFacetMatched];
    *absent = (int64_t)ctr[kFacetAbsent];
    *n_values = (int64_t)ctr[kFacetDistinct];
    if (ctr[kFacetOverflow] || ctr[kFacetDistinct] > (unsigned long long)max_values) {
        *n_values = std::max<int64_t>(*n_values, max_values + 1);
        return fail(h, MLVDB_ERR_OVERFLOW, "facet: more than max_values distinct values");
    }
    const size_t n = (size_t)ctr[kFacetDistinct];
    if (ctr[kFacetCursor] != ctr[kFacetDistinct]) return fail(h, MLVDB_ERR_INTERNAL, "facet: table and counter disagree");
    if (n == 0) return MLVDB_OK;
    std::vector<std::pair<int64_t, int64_t>> pairs(n);
    std::vector<int64_t> keys(n), counts(n);
    HIP_TRY(h, hipMemcpyAsync(keys.data(), packed_keys, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(counts.data(), packed_counts, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) pairs[i] = {keys[i], counts[i]};
    std::sort(pairs.begin(), pairs.end());  // (the values are distinct: the order is total)
    for (size_t i = 0; i < n; ++i) {
        out_values[i] = pairs[i].first;
        out_counts[i] = pairs[i].second;
    }
    return MLVDB_OK;
}

int facet_bins_impl(mlvdb_index* h, int32_t attr, const mlvdb_where* where, const void* edges, int32_t n_edges,
                    int64_t* out_counts, int64_t* matched, int64_t* absent) {
    hipStream_t s = h->stream;
    DevProgram pg;
    if (int rc = facet_program(h, where, pg)) return rc;
    const size_t nbins = (size_t)n_edges + 1;
    unsigned long long *ctr_d = nullptr, *bins_d = nullptr;  // adjacent: cleared, and read back, as one run
    int64_t* edges_d = nullptr;
    CARVE(h, h->facet_misc, [&](Carver& c) {
        ctr_d = c.take<unsigned long long>(kFacetCounters);
        bins_d = c.take<unsigned long long>(nbins);
        edges_d = c.take<int64_t>((size_t)n_edges);
    });
    HIP_TRY(h, hipMemsetAsync(ctr_d, 0, span_bytes(ctr_d, edges_d), s));
    HIP_TRY(h, hipMemcpyAsync(edges_d, edges, (size_t)n_edges * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_facet_bins(pg.ops, pg.n_ops, pg.set, h->rn, h->attr_col[attr], h->attr_type[attr], h->total, edges_d, n_edges,
                                 bins_d, ctr_d, s));
    std::vector<int64_t> host(kFacetCounters + nbins);
    HIP_TRY(h, hipMemcpyAsync(host.data(), ctr_d, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *matched = host[kFacetMatched];
    *absent = host[kFacetAbsent];
    std::copy(host.begin() + kFacetCounters, host.end(), out_counts);
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_facet_values(mlvdb_index* h, int32_t attr, const mlvdb_where* where, int64_t max_values, int64_t* out_values,
                       int64_t* out_counts, int64_t* n_values, int64_t* matched, int64_t* absent) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = int64_attr_check(h, attr, "value facets need an int64 column")) return rc;
    if (max_values < 1 || max_values > MLVDB_FACET_MAX_VALUES)
        return fail(h, MLVDB_ERR_INVALID_ARG, "max_values must be in 1..MLVDB_FACET_MAX_VALUES");
    if (!out_values || !out_counts || !n_values || !matched || !absent) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    *n_values = *matched = *absent = 0;
    if (h->total == 0) return MLVDB_OK;
    return facet_values_run(h, attr, where, max_values, out_values, out_counts, n_values, matched, absent, false);
    });
}

int mlvdb_facet_bins(mlvdb_index* h, int32_t attr, const mlvdb_where* where, const void* edges, int32_t n_edges,
                     int64_t* out_counts, int64_t* matched, int64_t* absent) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = scalar_check(h, attr)) return rc;
    if (int rc = value_check(h, attr)) return rc;
    if (n_edges < 1 || n_edges > MLVDB_FACET_MAX_EDGES)
        return fail(h, MLVDB_ERR_INVALID_ARG, "n_edges must be in 1..MLVDB_FACET_MAX_EDGES");
    if (!edges || !out_counts || !matched || !absent) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (h->attr_type[attr] == MLVDB_ATTR_INT64) {
        const int64_t* e = static_cast<const int64_t*>(edges);
        if (e[0] == INT64_MIN) return fail(h, MLVDB_ERR_INVALID_ARG, "an int64 edge must not be INT64_MIN (the absent marker)");
        for (int32_t i = 1; i < n_edges; ++i)
            if (!(e[i - 1] < e[i])) return fail(h, MLVDB_ERR_INVALID_ARG, "edges must be strictly ascending");
    } else {
        const double* e = static_cast<const double*>(edges);
        if (e[0] != e[0]) return fail(h, MLVDB_ERR_INVALID_ARG, "a float64 edge must not be NaN");
        for (int32_t i = 1; i < n_edges; ++i)  // (a NaN edge fails the comparison too)
            if (!(e[i - 1] < e[i])) return fail(h, MLVDB_ERR_INVALID_ARG, "edges must be strictly ascending and not NaN");
    }
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    *matched = *absent = 0;
    for (int32_t i = 0; i <= n_edges; ++i) out_counts[i] = 0;
    if (h->total == 0) return MLVDB_OK;
    return facet_bins_impl(h, attr, where, edges, n_edges, out_counts, matched, absent);
    });
}

// ---- attribute statistics (mlvdb_stats.h)
extern "C++" {
namespace {
int attr_stats_impl(mlvdb_index* h, int32_t attr, int32_t by, const mlvdb_where* where, int64_t max_groups, int64_t* out_keys,
                    int64_t* out_rows, int64_t* out_count, void* out_min, void* out_max, int64_t* out_sum_hi,
                    uint64_t* out_sum_lo, int64_t* n_groups, int64_t* matched, int64_t* by_absent) {
    hipStream_t s = h->stream;
    DevProgram pg;
    if (int rc = facet_program(h, where, pg)) return rc;
    const bool f64 = h->attr_type[attr] == MLVDB_ATTR_FLOAT64;
    uint64_t slots = 64;  // a power of two >= 2 max_groups: the table is at most half full when the call succeeds
    while (slots < 2 * (uint64_t)max_groups) slots *= 2;
    StatsTable t{};
    unsigned long long* packed = nullptr;  // the packed groups, kStatsRecord words each
    CARVE(h, h->stats_tab, [&](Carver& c) {
        using u64 = unsigned long long;
        t.keys = c.take<u64>(slots);
        t.mn = c.take<u64>(slots);
        t.rows = c.take<u64>(slots);  // rows .. counters are adjacent: cleared as one run
        t.count = c.take<u64>(slots);
        t.mx = c.take<u64>(slots);
        t.hi = c.take<u64>(slots);
        t.lo = c.take<u64>(slots);
        t.ctr = c.take<u64>(kFacetCounters);
        packed = c.take<u64>((size_t)max_groups * kStatsRecord);
    });
    t.mask = slots - 1;
    t.max_groups = (unsigned long long)max_groups;
    HIP_TRY(h, launch_attr_fill(reinterpret_cast<int64_t*>(t.keys), INT64_MIN, 0, (int64_t)slots, s));
    HIP_TRY(h, hipMemsetAsync(t.mn, 0xFF, span_bytes(t.mn, t.rows), s));
    HIP_TRY(h, hipMemsetAsync(t.rows, 0, span_bytes(t.rows, packed), s));
    const int64_t* by_col = by < 0 ? nullptr : h->attr_col[by];
    HIP_TRY(h, launch_stats_pass1(pg.ops, pg.n_ops, pg.set, h->rn, by_col, h->attr_col[attr], f64, h->total, t, s));
    if (f64) HIP_TRY(h, launch_stats_pass2(pg.ops, pg.n_ops, pg.set, h->rn, by_col, h->attr_col[attr], h->total, t, s));
    HIP_TRY(h, launch_stats_collect(t, packed, s));
    unsigned long long ctr[kFacetCounters] = {};
    HIP_TRY(h, hipMemcpyAsync(ctr, t.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *matched = (int64_t)ctr[kFacetMatched];
    *by_absent = (int64_t)ctr[kFacetAbsent];
    *n_groups = (int64_t)ctr[kFacetDistinct];
    if (ctr[kFacetOverflow] || ctr[kFacetDistinct] > (unsigned long long)max_groups) {
        *n_groups = std::max<int64_t>(*n_groups, max_groups + 1);
        return fail(h, MLVDB_ERR_OVERFLOW, "attr_stats: more than max_groups distinct values of by");
    }
    const size_t n = (size_t)ctr[kFacetDistinct];
    if (ctr[kFacetCursor] != ctr[kFacetDistinct]) return fail(h, MLVDB_ERR_INTERNAL, "attr_stats: table and counter disagree");
    if (n == 0) {  // nothing matched: no group, or the one empty group of an ungrouped call (written by the caller)
        if (by < 0) *n_groups = 1;
        return MLVDB_OK;
    }
    // one copy-down for all outputs: n records of kStatsRecord words
    std::vector<std::array<unsigned long long, kStatsRecord>> recs(n);
    HIP_TRY(h, hipMemcpyAsync(recs.data(), packed, n * sizeof recs[0], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    std::sort(recs.begin(), recs.end(),  // (the keys are distinct: the order is total)
              [](const auto& a, const auto& b) { return (int64_t)a[0] < (int64_t)b[0]; });
    for (size_t i = 0; i < n; ++i) {
        const auto& r = recs[i];
        out_keys[i] = (int64_t)r[0];
        out_rows[i] = (int64_t)r[1];
        out_count[i] = (int64_t)r[2];
        // the images back to the column's own type (count == 0: unspecified)
        static_cast<uint64_t*>(out_min)[i] = f64 ? stats_bits_f64(r[3]) : stats_image_i64((int64_t)r[3]);
        static_cast<uint64_t*>(out_max)[i] = f64 ? stats_bits_f64(r[4]) : stats_image_i64((int64_t)r[4]);
        out_sum_hi[i] = (int64_t)r[5];
        out_sum_lo[i] = r[6];
    }
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_attr_stats(mlvdb_index* h, int32_t attr, int32_t by, const mlvdb_where* where, int64_t max_groups, int64_t* out_keys,
                     int64_t* out_rows, int64_t* out_count, void* out_min, void* out_max, int64_t* out_sum_hi,
                     uint64_t* out_sum_lo, int64_t* n_groups, int64_t* matched, int64_t* by_absent) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = scalar_check(h, attr)) return rc;
    if (int rc = value_check(h, attr)) return rc;
    if (by != -1) {
        if (int rc = int64_attr_check(h, by, "attr_stats: by needs an int64 column")) return rc;
    }
    if (max_groups < 1 || max_groups > MLVDB_FACET_MAX_VALUES)
        return fail(h, MLVDB_ERR_INVALID_ARG, "max_groups must be in 1..MLVDB_FACET_MAX_VALUES");
    if (!out_keys || !out_rows || !out_count || !out_min || !out_max || !out_sum_hi || !out_sum_lo || !n_groups || !matched ||
        !by_absent)
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    *n_groups = by < 0 ? 1 : 0;
    *matched = *by_absent = 0;
    out_keys[0] = out_rows[0] = out_count[0] = out_sum_hi[0] = 0;  // the one group of an ungrouped call when nothing matches
    out_sum_lo[0] = 0;
    static_cast<int64_t*>(out_min)[0] = static_cast<int64_t*>(out_max)[0] = 0;
    if (h->total == 0) return MLVDB_OK;
    return attr_stats_impl(h, attr, by, where, max_groups, out_keys, out_rows, out_count, out_min, out_max, out_sum_hi,
                           out_sum_lo, n_groups, matched, by_absent);
    });
}

// ---- late-interaction search (mlvdb_maxsim.h)
extern "C++" {
namespace {
// padding of the nq queries of a late-interaction call and of their ntok tokens' match rows, on the host
void maxsim_pad(int64_t nq, int64_t ntok, int32_t k, int64_t* out_groups, float* out_score, int32_t* out_counts,
                double* out_score64, int64_t* out_match_labels, double* out_match_dist64) {
    pad(out_groups, nq * k, INT64_MIN);
    pad(out_score, nq * k, __builtin_inff());
    pad(out_score64, nq * k, __builtin_inf());
    pad(out_counts, nq, 0);
    pad(out_match_labels, ntok * k, -1);
    pad(out_match_dist64, ntok * k, __builtin_inf());
}

// The validated call (h->rn is the masked copy when a program restricts the rows): the documents and their table, the dense
// id of every row, then per chunk of queries the [token, document] scan, the ranking and -- when asked for -- the matches by
// the member stage of the grouped search, its queries being the chunk's tokens and its groups each token's query's documents.
int maxsim_impl(mlvdb_index* h, const float* tokens, const int64_t* off, int64_t nq, int32_t k, int32_t attr, int32_t qt_max,
                int64_t* out_groups, float* out_score, int32_t* out_counts, double* out_score64, int64_t* out_match_labels,
                double* out_match_dist64) {
    hipStream_t s = h->stream;
    auto pad_all = [&] {  // (off[0] == 0: off[nq] tokens in all)
        maxsim_pad(nq, off[nq], k, out_groups, out_score, out_counts, out_score64, out_match_labels, out_match_dist64);
    };
    if (h->total == 0 || h->total == h->deleted) {
        pad_all();
        return MLVDB_OK;
    }
    if (int rc = begin_call(h, s)) return rc;
    // 1. the documents: the present codes among the counted rows, ascending -- a document's dense id is its rank in that
    // order, so a tie on the dense id is a tie on the group code
    const int64_t* col = h->attr_col[attr];
    std::unique_ptr<int64_t[]> codes(new int64_t[kMaxsimMaxGroups]), rows_of(new int64_t[kMaxsimMaxGroups]);
    int64_t G = 0, matched = 0, absent = 0;
    if (int rc = facet_values_run(h, attr, nullptr, kMaxsimMaxGroups, codes.get(), rows_of.get(), &G, &matched, &absent, false))
        return rc == MLVDB_ERR_OVERFLOW ? fail(h, rc, "maxsim: more than MLVDB_MAXSIM_MAX_GROUPS documents") : rc;
    rows_of.reset();
    if (G == 0) {  // every counted row's value is absent
        pad_all();
        return end_call(h, s);
    }
    // the open-addressing table, as grouped_members builds it, and the dense id of every slot
    uint64_t slots = 1;
    while (slots < 2 * (uint64_t)G) slots *= 2;
    {
        std::vector<int64_t> keys(slots, INT64_MIN);
        std::vector<int32_t> dense(slots, -1);
        for (int64_t u = 0; u < G; ++u) {
            uint64_t at = facet_hash(codes[u]) & (slots - 1);
            while (keys[at] != INT64_MIN) at = (at + 1) & (slots - 1);
            keys[at] = codes[u];
            dense[at] = (int32_t)u;
        }
        long long* keys_d = nullptr;
        int32_t* dense_d = nullptr;
        CARVE(h, h->ms_tab, [&](Carver& c) {
            keys_d = c.take<long long>(slots);
            dense_d = c.take<int32_t>(slots);
        });
        HIP_TRY(h, h->ms_rowdoc.ensure((size_t)h->total * sizeof(int32_t)));
        HIP_TRY(h, hipMemcpyAsync(keys_d, keys.data(), slots * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(dense_d, dense.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice, s));
        // 2. the dense id of every row: every later pass reads this instead of norm + code + probe
        HIP_TRY(h, launch_maxsim_slot(h->rn, col, h->total, keys_d, slots, dense_d, h->ms_rowdoc.as<int32_t>(), s));
        HIP_TRY(h, hipStreamSynchronize(s));  // (the host vectors above are consumed by now)
    }
    const int64_t budget = (int64_t)std::max(1, h->tn.maxsim_ws_mb) << 20;
    const bool want_matches = out_match_labels || out_match_dist64;
    std::vector<int32_t> tok_off;
    std::vector<int64_t> dense_out, grp;
    std::vector<int32_t> cnt, tcnt;
    for (int64_t q0 = 0; q0 < nq;) {
        // the chunk: queries while their cells fit the budget and their tokens the chunk, always at least one
        int64_t q1 = q0 + 1;
        while (q1 < nq && (off[q1 + 1] - off[q0]) * G * (int64_t)sizeof(unsigned long long) <= budget &&
               off[q1 + 1] - off[q0] <= kMaxsimChunkTokens)
            ++q1;
        const int32_t n = (int32_t)(q1 - q0), ntok = (int32_t)(off[q1] - off[q0]);
        const size_t nk = (size_t)n * k;
        const float* chunk_tokens = tokens + (size_t)off[q0] * h->dim;
        tok_off.resize((size_t)n + 1);
        for (int32_t i = 0; i <= n; ++i) tok_off[(size_t)i] = (int32_t)(off[q0 + i] - off[q0]);
        HIP_TRY(h, h->dist_q.ensure((size_t)ntok * h->dim * sizeof(float)));
        HIP_TRY(h, h->qpad.ensure((size_t)ntok * h->ld * sizeof(float)));
        HIP_TRY(h, h->qaux.ensure((size_t)ntok * sizeof(double)));
        HIP_TRY(h, h->ms_best.ensure((size_t)ntok * G * sizeof(unsigned long long)));
        HIP_TRY(h, h->ms_misc.ensure(((size_t)n + 1) * sizeof(int32_t)));
        ListBlock o;  // (its labels: dense ids)
        if (int rc = carve_list(h, h->ms_out, nk, (size_t)n, o)) return rc;
        unsigned long long* best = h->ms_best.as<unsigned long long>();
        HIP_TRY(h, hipMemcpyAsync(h->dist_q.p, chunk_tokens, (size_t)ntok * h->dim * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->ms_misc.p, tok_off.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemsetAsync(best, 0xff, (size_t)ntok * G * sizeof(unsigned long long), s));
        HIP_TRY(h, launch_query_prep(h->dist_q.as<float>(), ntok, h->dim, h->ld, h->space, h->qpad.as<float>(),
                                     h->qaux.as<double>(), nullptr, s));
        // 3. the scan
        const ExactPlan plan = plan_exact(h->total, h->ld, ntok, k);
        MaxsimArgs a{};
        a.X = h->X;
        a.row_doc = h->ms_rowdoc.as<int32_t>();
        a.total = h->total;
        a.ld = h->ld;
        a.space = h->space;
        a.Qpad = h->qpad.as<float>();
        a.qaux = h->qaux.as<double>();
        a.ntok = ntok;
        a.ndocs = (int32_t)G;
        a.best = best;
        if (int rc = scan_step(h, s, h->total * plan.nqtiles, [&] { return launch_maxsim_scan(a, plan, s); })) return rc;
        h->stats.strategy_used = MLVDB_STRATEGY_EXACT;
        // 4. the ranking: dense ids, fp32 / fp64 scores and counts
        const int32_t rblk = maxsim_rank_blocks((int32_t)G);
        HIP_TRY(h, h->partial.ensure(nk * rblk * sizeof(TopEntry)));
        HIP_TRY(h, launch_maxsim_rank(best, h->ms_misc.as<int32_t>(), n, (int32_t)G, k, rblk, h->partial.as<TopEntry>(), s));
        HIP_TRY(h, launch_exact_merge(h->partial.as<TopEntry>(), n, nullptr, nullptr, rblk, k, o.lab, o.dist, o.cnt, o.d64, s));
        dense_out.resize(nk);
        cnt.resize((size_t)n);
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{dense_out.data(), 0, o.lab, nk}, {cnt.data(), 0, o.cnt, (size_t)n},
                                      {out_score, at, o.dist, nk}, {out_score64, at, o.d64, nk}}))
            return rc;
        for (size_t i = 0; i < nk; ++i) out_groups[at + i] = dense_out[i] >= 0 ? codes[(size_t)dense_out[i]] : INT64_MIN;
        std::memcpy(out_counts + q0, cnt.data(), (size_t)n * sizeof(int32_t));
        // 5. the matches: the member stage (grouped_members) over at most 1024 tokens per call, group_size 1
        for (int32_t t0 = 0; want_matches && t0 < ntok; t0 += (int32_t)kDistinctChunk) {
            const int32_t nt = std::min<int32_t>((int32_t)kDistinctChunk, ntok - t0);
            const size_t ntk = (size_t)nt * k;
            grp.assign(ntk, INT64_MIN);
            tcnt.assign((size_t)nt, 0);
            int32_t qi = (int32_t)(std::upper_bound(tok_off.begin(), tok_off.end(), t0) - tok_off.begin()) - 1;
            for (int32_t t = 0; t < nt; ++t) {
                while (tok_off[(size_t)qi + 1] <= t0 + t) ++qi;  // the query of token t0 + t
                tcnt[(size_t)t] = cnt[(size_t)qi];
                std::copy(out_groups + at + (size_t)qi * k, out_groups + at + ((size_t)qi + 1) * k, grp.begin() + (size_t)t * k);
            }
            // (h->dist_q holds the member stage's queries from row 0 on)
            if (t0 > 0 || nt < ntok)
                HIP_TRY(h, hipMemcpyAsync(h->dist_q.p, chunk_tokens + (size_t)t0 * h->dim, (size_t)nt * h->dim * sizeof(float),
                                          hipMemcpyHostToDevice, s));
            ListBlock m;
            if (int rc = grouped_members(h, nt, k, 1, qt_max, col, grp.data(), tcnt.data(), m)) return rc;
            const size_t mat = ((size_t)off[q0] + (size_t)t0) * k;
            if (int rc = copy_down(h, s, {{out_match_labels, mat, m.lab, ntk}, {out_match_dist64, mat, m.d64, ntk}})) return rc;
        }
        q0 = q1;
    }
    return end_call(h, s);
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_maxsim(mlvdb_index* h, const float* tokens, const int64_t* token_offsets, int64_t nq, int32_t k,
                              int32_t attr, const mlvdb_where* where, int64_t* out_groups, float* out_score,
                              int32_t* out_counts, double* out_score64, int64_t* out_match_labels, double* out_match_dist64) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched (the program: with_where)
    if (int rc = int64_attr_check(h, attr, "maxsim needs an int64 column")) return rc;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max(h, k, "maxsim: ")) return rc;
    if (nq > 0 && (!tokens || !token_offsets || !out_groups || !out_score || !out_counts))
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (nq > 0 && token_offsets[0] != 0) return fail(h, MLVDB_ERR_INVALID_ARG, "maxsim: token_offsets must start at 0");
    for (int64_t i = 0; i < nq; ++i) {
        if (token_offsets[i + 1] <= token_offsets[i])
            return fail(h, MLVDB_ERR_INVALID_ARG, "maxsim: token_offsets must be strictly increasing (a query without tokens)");
        if (token_offsets[i + 1] - token_offsets[i] > kMaxsimMaxTokens)
            return fail(h, MLVDB_ERR_INVALID_ARG, "maxsim: more than MLVDB_MAXSIM_MAX_TOKENS tokens in a query");
    }
    const int32_t qt = gather_qt(h);  // pairs per tile of the member stage's gathered kernel
    if ((out_match_labels || out_match_dist64) && where_gather_lds(qt, h->ld) > 64 * 1024)
        return fail(h, MLVDB_ERR_UNSUPPORTED, "maxsim: the matches of one token of this dimension need more than 64 KiB of LDS");
    auto call = [&]() {
        return maxsim_impl(h, tokens, token_offsets, nq, k, attr, qt, out_groups, out_score, out_counts, out_score64,
                           out_match_labels, out_match_dist64);
    };
    return with_where(h, where, nq, call);
    });
}

// ---- ordered metadata queries (mlvdb_order.h)
extern "C++" {
namespace {
// The whole chain is enqueued at once: the kernels hand their state to each other on the device (OrderState), and the digit
// passes behind a finished selection return at once.  A program is evaluated once into the row mask (where_run), which every
// pass then reads at one byte per row instead of the norms and the program's columns.
// A geo column (mlvdb_geo_nearest): the key is hav from `centre`, and the rows' distances come back in out_dist.
int where_ordered_impl(mlvdb_index* h, int32_t attr, int32_t descending, int64_t centre, const mlvdb_where* where,
                       int64_t offset, int64_t limit, int64_t* out_labels, void* out_values, double* out_dist, int64_t* n_out,
                       int64_t* matched, int64_t* absent) {
    hipStream_t s = h->stream;
    const uint8_t* mask = nullptr;
    if (int rc = where_mask(h, where, &mask)) return rc;
    OrderState* st = nullptr;
    unsigned long long *hist = nullptr, *keys = nullptr;  // one histogram per digit pass; the collected keys
    int64_t *labels_d = nullptr, *values_d = nullptr;     // the ranked window
    double* dist_d = nullptr;
    uint32_t* clabels = nullptr;                           // the collected keys' labels
    CARVE(h, h->order_ws, [&](Carver& c) {
        st = c.take<OrderState>(1);  // the state and the histograms are adjacent: cleared as one run
        c.pad_to(64);
        hist = c.take<unsigned long long>((size_t)kOrderPasses * kOrderBins);
        keys = c.take<unsigned long long>(kOrderMaxRows);
        labels_d = c.take<int64_t>(kOrderMaxRows);
        values_d = c.take<int64_t>(kOrderMaxRows);
        dist_d = c.take<double>(kOrderMaxRows);
        clabels = c.take<uint32_t>(kOrderMaxRows);
    });
    const int64_t* col = h->attr_col[attr];
    const int32_t type = h->attr_type[attr];
    HIP_TRY(h, hipMemsetAsync(st, 0, span_bytes(st, keys), s));
    for (int32_t pass = 0; pass < kOrderPasses; ++pass) {
        unsigned long long* hp = hist + (size_t)pass * kOrderBins;
        HIP_TRY(h, launch_order_hist(mask, h->rn, col, type, descending, centre, h->total, pass, hp, st, s));
        HIP_TRY(h, launch_order_scan(hp, pass, offset, limit, st, s));
    }
    HIP_TRY(h, launch_order_collect(mask, h->rn, col, type, descending, centre, h->total, st, keys, clabels, s));
    HIP_TRY(h, launch_order_sort(keys, clabels, col, type, centre, h->total, offset, st, labels_d, values_d, dist_d, s));
    OrderState host{};
    HIP_TRY(h, hipMemcpyAsync(&host, st, sizeof host, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *matched = (int64_t)host.matched;
    *absent = (int64_t)host.absent;
    const int64_t candidates = *matched - *absent;
    const int64_t n = std::max<int64_t>(0, std::min(candidates - offset, limit));
    if (!host.done || host.overflow || host.cursor != host.n_collect || (int64_t)host.n_out != n ||
        (n > 0 && (int64_t)host.want != offset + n))
        return fail(h, MLVDB_ERR_INTERNAL, "where_ordered: the selection and the collected rows disagree");
    *n_out = n;
    if (n == 0) return MLVDB_OK;
    HIP_TRY(h, hipMemcpyAsync(out_labels, labels_d, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_values, values_d, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (out_dist) HIP_TRY(h, hipMemcpyAsync(out_dist, dist_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_where_ordered(mlvdb_index* h, int32_t attr, int32_t descending, const mlvdb_where* where, int64_t offset,
                        int64_t limit, int64_t* out_labels, void* out_values, int64_t* n_out, int64_t* matched,
                        int64_t* absent) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = scalar_check(h, attr)) return rc;
    if (int rc = value_check(h, attr)) return rc;
    if (offset < 0 || limit < 1 || limit > MLVDB_ORDER_MAX_ROWS || offset > MLVDB_ORDER_MAX_ROWS - limit)
        return fail(h, MLVDB_ERR_INVALID_ARG, "offset >= 0, limit >= 1 and offset + limit <= MLVDB_ORDER_MAX_ROWS");
    if (!out_labels || !out_values || !n_out || !matched || !absent) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    *n_out = *matched = *absent = 0;
    if (h->total == 0) return MLVDB_OK;
    return where_ordered_impl(h, attr, descending != 0, 0, where, offset, limit, out_labels, out_values, nullptr, n_out, matched,
                              absent);
    });
}

// ---- nearest by distance on a geo column (mlvdb_geo.h): the ordered chain with hav from the centre as the key
int mlvdb_geo_nearest(mlvdb_index* h, int32_t attr, int64_t center, const mlvdb_where* where, int64_t offset, int64_t limit,
                      int64_t* out_labels, int64_t* out_points, double* out_dist_m, int64_t* n_out, int64_t* matched,
                      int64_t* absent) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = attr_check(h, attr)) return rc;
    if (h->attr_type[attr] != MLVDB_ATTR_GEO) return fail(h, MLVDB_ERR_INVALID_ARG, "geo_nearest needs a geo column");
    if (!geo_valid(center)) return fail(h, MLVDB_ERR_INVALID_ARG, "geo_nearest: center is not a point (lat_e7, lon_e7 out of range)");
    if (offset < 0 || limit < 1 || limit > MLVDB_ORDER_MAX_ROWS || offset > MLVDB_ORDER_MAX_ROWS - limit)
        return fail(h, MLVDB_ERR_INVALID_ARG, "offset >= 0, limit >= 1 and offset + limit <= MLVDB_ORDER_MAX_ROWS");
    if (!out_labels || !out_points || !out_dist_m || !n_out || !matched || !absent)
        return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    *n_out = *matched = *absent = 0;
    if (h->total == 0) return MLVDB_OK;
    return where_ordered_impl(h, attr, 0, center, where, offset, limit, out_labels, out_points, out_dist_m, n_out, matched, absent);
    });
}

// ---- attribute updates and filtered deletes (mlvdb_mutate.h)
extern "C++" {
namespace {
int attr_set_at_impl(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const void* values, int64_t* updated) {
    hipStream_t s = h->stream;
    const size_t lbytes = (size_t)n * sizeof(int64_t);
    unsigned long long* cnt = nullptr;
    int64_t *labels_d = nullptr, *values_d = nullptr;
    CARVE(h, h->mutate_ws, [&](Carver& c) {
        cnt = c.take<unsigned long long>(1);
        c.pad_to(64);
        labels_d = c.take<int64_t>((size_t)n);
        values_d = c.take<int64_t>((size_t)n);
    });
    HIP_TRY(h, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
    HIP_TRY(h, hipMemcpyAsync(labels_d, labels, lbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(values_d, values, lbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_attr_scatter(h->attr_col[attr], labels_d, values_d, n, h->rn, cnt, s));
    unsigned long long wrote = 0;
    HIP_TRY(h, hipMemcpyAsync(&wrote, cnt, sizeof wrote, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *updated = (int64_t)wrote;
    return MLVDB_OK;
}

// The assignments of a call, checked (1..MLVDB_MAX_ATTRS of them, defined attributes, each at most once, known ops, no NaN
// added) and resolved to their columns; *any_add: a counting pass must come first.
int update_sets_prepare(mlvdb_index* h, const mlvdb_assign* sets, int32_t n_sets, MutateSet (&out)[MLVDB_MAX_ATTRS], bool* any_add) {
    if (n_sets < 1 || n_sets > MLVDB_MAX_ATTRS || !sets) return fail(h, MLVDB_ERR_INVALID_ARG, "a call holds 1..MLVDB_MAX_ATTRS assignments");
    bool seen[MLVDB_MAX_ATTRS] = {};
    *any_add = false;
    for (int32_t j = 0; j < n_sets; ++j) {
        const mlvdb_assign& a = sets[j];
        if (int rc = attr_check(h, a.attr)) return rc;
        if (int rc = scalar_check(h, a.attr)) return rc;  // (ASSIGN and ADD alike)
        if (seen[a.attr]) return fail(h, MLVDB_ERR_INVALID_ARG, "an attribute is assigned twice");
        seen[a.attr] = true;
        if (a.op != MLVDB_SET_ASSIGN && a.op != MLVDB_SET_ADD) return fail(h, MLVDB_ERR_INVALID_ARG, "unknown assignment op");
        if (h->attr_type[a.attr] == MLVDB_ATTR_GEO) {
            if (a.op == MLVDB_SET_ADD) return fail(h, MLVDB_ERR_INVALID_ARG, "ADD on a geo column (ASSIGN a point, or INT64_MIN to clear)");
            if (int rc = geo_values_check(h, a.attr, &a.a, 1)) return rc;
        }
        if (a.op == MLVDB_SET_ADD) {
            *any_add = true;
            if (h->attr_type[a.attr] == MLVDB_ATTR_FLOAT64) {
                double d;
                std::memcpy(&d, &a.a, sizeof d);
                if (d != d) return fail(h, MLVDB_ERR_INVALID_ARG, "ADD of NaN");
            }
        }
        out[j] = MutateSet{h->attr_col[a.attr], a.a, h->attr_type[a.attr], a.op};
    }
    return MLVDB_OK;
}

int attr_update_where_impl(mlvdb_index* h, const mlvdb_where* where, const MutateSet* sets, int32_t n_sets, bool any_add,
                           int64_t* matched, int64_t* refused) {
    hipStream_t s = h->stream;
    const int64_t* set_d = nullptr;
    if (int rc = where_upload(h, where, &set_d)) return rc;
    unsigned long long* cnt = nullptr;  // matched, refused of the counting pass; the same of the storing pass
    MutateSet* sets_d = nullptr;
    CARVE(h, h->mutate_ws, [&](Carver& c) {
        cnt = c.take<unsigned long long>(4);
        c.pad_to(64);
        sets_d = c.take<MutateSet>(MLVDB_MAX_ATTRS);
    });
    HIP_TRY(h, hipMemsetAsync(cnt, 0, span_bytes(cnt, sets_d), s));
    HIP_TRY(h, hipMemcpyAsync(sets_d, sets, sizeof(MutateSet) * (size_t)n_sets, hipMemcpyHostToDevice, s));
    const WhereOp* prog = h->where_prog.as<WhereOp>();
    unsigned long long host[2] = {0, 0};
    if (any_add) {  // all or nothing: count the rows whose sums cannot be stored before anything is
        HIP_TRY(h, launch_attr_update(prog, where->n_ops, set_d, sets_d, n_sets, h->rn, h->total, false, cnt, s));
        HIP_TRY(h, hipMemcpyAsync(host, cnt, sizeof host, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        *matched = (int64_t)host[0];
        *refused = (int64_t)host[1];
        if (host[1] != 0 || host[0] == 0) return MLVDB_OK;
    }
    HIP_TRY(h, launch_attr_update(prog, where->n_ops, set_d, sets_d, n_sets, h->rn, h->total, true, cnt + 2, s));
    HIP_TRY(h, hipMemcpyAsync(host, cnt + 2, sizeof host, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (any_add && ((int64_t)host[0] != *matched || host[1] != 0))
        return fail(h, MLVDB_ERR_INTERNAL, "attr_update_where: the counting pass and the storing pass disagree");
    *matched = (int64_t)host[0];
    return MLVDB_OK;
}

int tombstone_where_impl(mlvdb_index* h, const mlvdb_where* where, int64_t* out_labels, int64_t capacity, int64_t* matches) {
    if (int rc = where_run(h, where, matches)) return rc;  // the mask, and its count
    const bool want_labels = capacity >= 0;
    if (*matches == 0 || (want_labels && capacity < *matches)) return MLVDB_OK;
    hipStream_t s = h->stream;
    std::vector<int32_t> host;
    if (want_labels) {  // before the norms change: the compaction map of the masked norms, as mlvdb_where_labels lists them
        if (int rc = mask_labels(h, *matches)) return rc;
        host.resize((size_t)*matches);
        HIP_TRY(h, hipMemcpyAsync(host.data(), h->labels_in.p, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    const bool shadow = h->rp8.p && h->i8_rows > 0;  // the int8 shadow's row constants carry the tombstones too
    HIP_TRY(h, launch_tombstone_mask(h->row_mask.as<uint8_t>(), h->rn, shadow ? h->rp8.as<float>() : nullptr, h->i8_rows,
                                     h->space == kSpaceL2 ? 1 : 0, h->total, s));
    if (shadow)
        if (int rc = forget_l2_offsets(h, 0, s)) return rc;  // (a dead row changes its lane group's P0)
    HIP_TRY(h, hipStreamSynchronize(s));
    h->deleted += *matches;
    for (size_t i = 0; i < host.size(); ++i) out_labels[i] = host[i];
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_attr_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const void* values, int64_t* updated) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = attr_check(h, attr)) return rc;
    if (int rc = scalar_check(h, attr)) return rc;
    return with_labels(h, labels, n, updated, values != nullptr, "bad labels / values / n", [&]() -> int {
        if (int rc = geo_values_check(h, attr, values, n)) return rc;
        return attr_set_at_impl(h, attr, labels, n, values, updated);
    });
    });
}

int mlvdb_attr_update_where(mlvdb_index* h, const mlvdb_where* where, const mlvdb_assign* sets, int32_t n_sets,
                            int64_t* matched, int64_t* refused) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (!matched || !refused) return fail(h, MLVDB_ERR_INVALID_ARG, "null counter");
    MutateSet resolved[MLVDB_MAX_ATTRS];
    bool any_add = false;
    if (int rc = update_sets_prepare(h, sets, n_sets, resolved, &any_add)) return rc;
    if (int rc = where_prepare(h, where)) return rc;
    *matched = *refused = 0;
    if (h->total == 0) return MLVDB_OK;
    return attr_update_where_impl(h, where, resolved, n_sets, any_add, matched, refused);
    });
}

int mlvdb_tombstone_where(mlvdb_index* h, const mlvdb_where* where, int64_t* out_labels, int64_t capacity, int64_t* matches) {
    return guarded(h, kOnDevice, [&]() -> int {
    // labels into out_labels[capacity], or no labels at all (NULL with a negative capacity)
    if (!matches || (out_labels ? capacity < 0 : capacity > 0)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad output buffers");
    return tombstone_where_impl(h, where, out_labels, capacity, matches);
    });
}

// ---- list columns (mlvdb_list.h)
extern "C++" {
namespace {
int list_attr_check(mlvdb_index* h, int32_t attr) { return typed_attr_check(h, attr, MLVDB_ATTR_INT64_LIST, "not a list column"); }

// One list as the columns hold them: at most MLVDB_LIST_MAX_LEN values, strictly ascending, none INT64_MIN.
int list_check(mlvdb_index* h, const int64_t* v, int64_t len) {
    if (len < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "list offsets must not decrease");
    if (len > MLVDB_LIST_MAX_LEN) return fail(h, MLVDB_ERR_INVALID_ARG, "a list holds at most MLVDB_LIST_MAX_LEN values");
    if (len > 0 && !v) return fail(h, MLVDB_ERR_INVALID_ARG, "values is null");
    for (int64_t j = 0; j < len; ++j) {
        if (v[j] == INT64_MIN) return fail(h, MLVDB_ERR_INVALID_ARG, "INT64_MIN is not a list element");
        if (j > 0 && v[j - 1] >= v[j]) return fail(h, MLVDB_ERR_INVALID_ARG, "a list must be strictly ascending");
    }
    return MLVDB_OK;
}

// The n lists of a CSR checked; nothing is written or launched.
int list_csr_check(mlvdb_index* h, int64_t n, const int64_t* offsets, const int64_t* values, const uint8_t* present) {
    if (!offsets || offsets[0] < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "bad list offsets");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (int rc = list_check(h, values ? values + offsets[i] : nullptr, len)) return rc;
        if (present && !present[i] && len != 0) return fail(h, MLVDB_ERR_INVALID_ARG, "an absent row with values");
    }
    return MLVDB_OK;
}

// The checked CSR appended to the pool of `attr` (enqueued, the pool regrown first if need be) -> the rows' slots.
int list_append(mlvdb_index* h, int32_t attr, int64_t n, const int64_t* offsets, const int64_t* values,
                const uint8_t* present, std::vector<int64_t>& slots) {
    const int64_t count = offsets[n] - offsets[0];
    if (int rc = list_pool_reserve(h, attr, count)) return rc;
    const int64_t base = h->list_used[attr];
    if (count > 0)
        HIP_TRY(h, hipMemcpyAsync(h->list_pool[attr] + base, values + offsets[0], (size_t)count * sizeof(int64_t),
                                  hipMemcpyHostToDevice, h->stream));
    h->list_used[attr] = base + count;
    slots.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        slots[(size_t)i] = (present && !present[i]) ? INT64_MIN
                                                    : (((base + offsets[i] - offsets[0]) << 8) | (offsets[i + 1] - offsets[i]));
    return MLVDB_OK;
}

int list_get_impl(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int64_t* out_offsets, int64_t* out_values,
                  uint8_t* out_present, int64_t capacity, int64_t* needed) {
    hipStream_t s = h->stream;
    const int64_t* slots = h->attr_col[attr] + first;
    if (int rc = list_scan(h, slots, nullptr, n, needed)) return rc;
    if (capacity < *needed) return MLVDB_OK;
    const size_t vbytes = (size_t)*needed * sizeof(int64_t), obytes = (size_t)(n + 1) * sizeof(int64_t);
    int64_t *values_d = nullptr, *offsets_d = nullptr;
    uint8_t* present_d = nullptr;
    CARVE(h, h->list_out, [&](Carver& c) {
        values_d = c.take<int64_t>((size_t)*needed);
        offsets_d = c.take<int64_t>((size_t)n + 1);
        present_d = c.take<uint8_t>((size_t)n);
    });
    HIP_TRY(h, launch_list_move(slots, n, h->list_sums.as<int64_t>(), h->list_pool[attr], values_d, nullptr, offsets_d,
                                present_d, s));
    if (vbytes) HIP_TRY(h, hipMemcpyAsync(out_values, values_d, vbytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_offsets, offsets_d, obytes, hipMemcpyDeviceToHost, s));
    if (out_present) HIP_TRY(h, hipMemcpyAsync(out_present, present_d, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MLVDB_OK;
}

// The checked CSR written to rows [first, first + n) of a pooled column.
int list_set_impl(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const int64_t* offsets, const int64_t* values,
                  const uint8_t* present) {
    std::vector<int64_t> slots;
    if (int rc = list_append(h, attr, n, offsets, values, present, slots)) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->attr_col[attr] + first, slots.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MLVDB_OK;
}

// The checked CSR written to the rows of the checked labels.
int list_set_at_impl(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const int64_t* offsets,
                     const int64_t* values, const uint8_t* present, int64_t* updated) {
    std::vector<int64_t> slots;
    if (int rc = list_append(h, attr, n, offsets, values, present, slots)) return rc;
    return attr_set_at_impl(h, attr, labels, n, slots.data(), updated);  // the slots are scattered like any int64 values
}

}  // namespace
}  // extern "C++"

int mlvdb_attr_list_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const int64_t* offsets,
                        const int64_t* values, const uint8_t* present) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = list_attr_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n)) return rc;
    if (n == 0) return MLVDB_OK;
    if (int rc = list_csr_check(h, n, offsets, values, present)) return rc;
    return list_set_impl(h, attr, first, n, offsets, values, present);
    });
}

int mlvdb_attr_list_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const int64_t* offsets,
                           const int64_t* values, const uint8_t* present, int64_t* updated) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = list_attr_check(h, attr)) return rc;
    return with_labels(h, labels, n, updated, true, "bad labels / n", [&]() -> int {
        if (int rc = list_csr_check(h, n, offsets, values, present)) return rc;
        return list_set_at_impl(h, attr, labels, n, offsets, values, present, updated);
    });
    });
}

int mlvdb_attr_list_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int64_t* out_offsets, int64_t* out_values,
                        uint8_t* out_present, int64_t capacity, int64_t* needed) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = list_attr_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n)) return rc;
    if (!needed || !out_offsets || capacity < 0 || (capacity > 0 && !out_values)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad output buffers");
    *needed = 0;
    if (n == 0) {
        out_offsets[0] = 0;
        return MLVDB_OK;
    }
    return list_get_impl(h, attr, first, n, out_offsets, out_values, out_present, capacity, needed);
    });
}

int mlvdb_attr_list_update_where(mlvdb_index* h, const mlvdb_where* where, int32_t attr, const int64_t* values,
                                 int32_t n_values, int32_t clear, int64_t* matched) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (!matched) return fail(h, MLVDB_ERR_INVALID_ARG, "null counter");
    if (int rc = list_attr_check(h, attr)) return rc;
    if (int rc = clear ? MLVDB_OK : list_check(h, values, n_values)) return rc;
    if (int rc = where_prepare(h, where)) return rc;
    *matched = 0;
    if (h->total == 0) return MLVDB_OK;
    int64_t slot = INT64_MIN;
    if (!clear) {  // the list goes into the pool once; every matching row shares its slot
        const int64_t offsets[2] = {0, n_values};
        std::vector<int64_t> slots;
        if (int rc = list_append(h, attr, 1, offsets, values, nullptr, slots)) return rc;
        slot = slots[0];
        if (int rc = where_prepare(h, where)) return rc;  // (the append may have moved a pool the program reads)
    }
    const MutateSet set{h->attr_col[attr], slot, MLVDB_ATTR_INT64, MLVDB_SET_ASSIGN};
    int64_t refused = 0;
    return attr_update_where_impl(h, where, &set, 1, false, matched, &refused);
    });
}

int mlvdb_attr_list_stats(mlvdb_index* h, int32_t attr, int64_t* pool_used, int64_t* pool_live) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = attr_check(h, attr)) return rc;
    if (!pooled(h->attr_type[attr])) return fail(h, MLVDB_ERR_INVALID_ARG, "not a list, sparse or bits column");
    if (!pool_used || !pool_live) return fail(h, MLVDB_ERR_INVALID_ARG, "null counter");
    *pool_used = h->list_used[attr];
    return list_scan(h, h->attr_col[attr], h->rn, h->total, pool_live);
    });
}

int mlvdb_facet_list_values(mlvdb_index* h, int32_t attr, const mlvdb_where* where, int64_t max_values, int64_t* out_values,
                            int64_t* out_counts, int64_t* n_values, int64_t* matched, int64_t* absent) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = list_attr_check(h, attr)) return rc;
    if (max_values < 1 || max_values > MLVDB_FACET_MAX_VALUES)
        return fail(h, MLVDB_ERR_INVALID_ARG, "max_values must be in 1..MLVDB_FACET_MAX_VALUES");
    if (!out_values || !out_counts || !n_values || !matched || !absent) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    *n_values = *matched = *absent = 0;
    if (h->total == 0) return MLVDB_OK;
    return facet_values_run(h, attr, where, max_values, out_values, out_counts, n_values, matched, absent, true);
    });
}

// ---- sparse vector columns (mlvdb_sparse.h)
extern "C++" {
namespace {
int sparse_attr_check(mlvdb_index* h, int32_t attr) { return typed_attr_check(h, attr, MLVDB_ATTR_SPARSE, "not a sparse column"); }

// One sparse vector: at most max_len entries, terms in [0, 2^31) strictly ascending, weights finite.
int sparse_vector_check(mlvdb_index* h, const int32_t* terms, const float* weights, int64_t len, int64_t max_len) {
    if (len < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "sparse offsets must not decrease");
    if (len > max_len) return fail(h, MLVDB_ERR_INVALID_ARG, "a sparse vector with too many entries");
    if (len > 0 && (!terms || !weights)) return fail(h, MLVDB_ERR_INVALID_ARG, "terms / weights is null");
    for (int64_t j = 0; j < len; ++j) {
        if (terms[j] < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "a sparse term must be in [0, 2^31)");
        if (j > 0 && terms[j - 1] >= terms[j]) return fail(h, MLVDB_ERR_INVALID_ARG, "sparse terms must be strictly ascending");
        if (!std::isfinite(weights[j])) return fail(h, MLVDB_ERR_INVALID_ARG, "a sparse weight must be finite");
    }
    return MLVDB_OK;
}

// The n row vectors of a CSR checked and packed into pool elements ((int64)term << 32 | bits(weight)) -> packed, indexed
// like terms from offsets[0] on; nothing is written or launched.
int sparse_csr_pack(mlvdb_index* h, int64_t n, const int64_t* offsets, const int32_t* terms, const float* weights,
                    const uint8_t* present, std::vector<int64_t>& packed, std::vector<int64_t>& rebased) {
    if (!offsets || offsets[0] < 0) return fail(h, MLVDB_ERR_INVALID_ARG, "bad sparse offsets");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        const bool have = len > 0 && terms && weights;
        if (int rc = sparse_vector_check(h, have ? terms + offsets[i] : nullptr, have ? weights + offsets[i] : nullptr, len,
                                         MLVDB_SPARSE_MAX_NNZ))
            return rc;
        if (present && !present[i] && len != 0) return fail(h, MLVDB_ERR_INVALID_ARG, "an absent row with entries");
    }
    const int64_t base = offsets[0], count = offsets[n] - base;
    packed.resize((size_t)count);
    for (int64_t j = 0; j < count; ++j) {
        uint32_t bits;
        std::memcpy(&bits, &weights[base + j], sizeof bits);
        packed[(size_t)j] = ((int64_t)terms[base + j] << 32) | (int64_t)bits;
    }
    rebased.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) rebased[(size_t)i] = offsets[i] - base;
    return MLVDB_OK;
}

// The CSR of a call's sparse queries (q_offsets[0] == 0 checked by the caller): every query a sparse vector of at most
// MLVDB_SPARSE_MAX_QUERY_TERMS entries.
int sparse_queries_check(mlvdb_index* h, int64_t nq, const int64_t* q_offsets, const int32_t* q_terms, const float* q_weights) {
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t len = q_offsets[i + 1] - q_offsets[i];
        const bool have = len > 0 && q_terms && q_weights;
        if (int rc = sparse_vector_check(h, have ? q_terms + q_offsets[i] : nullptr, have ? q_weights + q_offsets[i] : nullptr, len,
                                         MLVDB_SPARSE_MAX_QUERY_TERMS))
            return rc;
    }
    return MLVDB_OK;
}

// The device part of one pass of at most kSparseChunk queries [q0, q1): tiles, unions and weights up, scan, merge; the ranked
// answers stay on the device in `o` ((q1 - q0) * k entries, q1 - q0 counts).  Returns with the stream drained.
int sparse_pass_device(mlvdb_index* h, int32_t attr, const int64_t* off, const int32_t* terms, const float* weights, int64_t q0,
                       int64_t q1, int32_t k, const uint8_t* mask, const ListBlock& o) {
    hipStream_t s = h->stream;
    const int32_t n = (int32_t)(q1 - q0);
    // greedy tiles: consecutive queries while they are <= kSparseQT and their term union holds <= kSparseMaxUnion terms
    std::vector<SparseTile> tiles;
    std::vector<int32_t> U, cur, merged;
    std::vector<float> W;
    auto close_tile = [&](int32_t tq0, int32_t tq1) {
        const int32_t u0 = (int32_t)U.size();
        tiles.push_back(SparseTile{tq0, tq1 - tq0, u0, (int32_t)cur.size()});
        U.insert(U.end(), cur.begin(), cur.end());
        W.resize((size_t)U.size() * kSparseQT, 0.0f);
        for (int32_t q = tq0; q < tq1; ++q)
            for (int64_t j = off[q0 + q]; j < off[q0 + q + 1]; ++j) {
                const size_t u = (size_t)(std::lower_bound(cur.begin(), cur.end(), terms[j]) - cur.begin());
                W[((size_t)u0 + u) * kSparseQT + (size_t)(q - tq0)] = weights[j];
            }
    };
    int32_t tq0 = 0;
    for (int32_t q = 0; q < n; ++q) {
        const int32_t* qt = terms + off[q0 + q];
        const size_t qn = (size_t)(off[q0 + q + 1] - off[q0 + q]);
        merged.resize(cur.size() + qn);
        merged.resize((size_t)(std::set_union(cur.begin(), cur.end(), qt, qt + qn, merged.begin()) - merged.begin()));
        if (q > tq0 && (q - tq0 == kSparseQT || merged.size() > (size_t)kSparseMaxUnion)) {
            close_tile(tq0, q);
            tq0 = q;
            merged.assign(qt, qt + qn);
        }
        cur.swap(merged);
    }
    close_tile(tq0, n);
    const int32_t ntiles = (int32_t)tiles.size();
    const size_t nk = (size_t)n * k;
    const int32_t nblk = sparse_scan_blocks(h->total, n, k);
    SparseTile* tiles_d = nullptr;
    int32_t* U_d = nullptr;
    float* W_d = nullptr;
    CARVE(h, h->sparse_in, [&](Carver& c) {
        tiles_d = c.take<SparseTile>(tiles.size());
        U_d = c.take<int32_t>(U.size());
        W_d = c.take<float>(W.size());
        c.take<char>(16);  // slack
    });
    HIP_TRY(h, h->partial.ensure(nk * (size_t)nblk * sizeof(TopEntry)));
    HIP_TRY(h, hipMemcpyAsync(tiles_d, tiles.data(), tiles.size() * sizeof(SparseTile), hipMemcpyHostToDevice, s));
    if (!U.empty()) HIP_TRY(h, hipMemcpyAsync(U_d, U.data(), U.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (!W.empty()) HIP_TRY(h, hipMemcpyAsync(W_d, W.data(), W.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_sparse_scan(h->attr_col[attr], h->list_pool[attr], h->rn, mask, h->total, tiles_d, ntiles, U_d, W_d, k, nblk,
                                  h->partial.as<TopEntry>(), s));
    HIP_TRY(h, launch_sparse_merge(h->partial.as<TopEntry>(), n, nblk, k, o.lab, o.dist, o.cnt, o.d64, s));
    HIP_TRY(h, hipStreamSynchronize(s));  // (the host vectors above are consumed by now)
    return MLVDB_OK;
}

// One pass: its device part into h->sparse_out, answers down.
int sparse_pass(mlvdb_index* h, int32_t attr, const int64_t* off, const int32_t* terms, const float* weights, int64_t q0,
                int64_t q1, int32_t k, const uint8_t* mask, int64_t* out_labels, float* out_score, int32_t* out_counts,
                double* out_score64) {
    hipStream_t s = h->stream;
    const int32_t n = (int32_t)(q1 - q0);
    const size_t nk = (size_t)n * k;
    ListBlock o;
    if (int rc = carve_list(h, h->sparse_out, nk, (size_t)n, o)) return rc;
    if (int rc = sparse_pass_device(h, attr, off, terms, weights, q0, q1, k, mask, o)) return rc;
    const size_t at = (size_t)q0 * k;
    return copy_down(h, s, {{out_labels, at, o.lab, nk}, {out_score, at, o.dist, nk}, {out_counts, (size_t)q0, o.cnt, (size_t)n},
                            {out_score64, at, o.d64, nk}});
}
}  // namespace
}  // extern "C++"

int mlvdb_sparse_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const int64_t* offsets, const int32_t* terms,
                     const float* weights, const uint8_t* present) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = sparse_attr_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n)) return rc;
    if (n == 0) return MLVDB_OK;
    std::vector<int64_t> packed, rebased;
    if (int rc = sparse_csr_pack(h, n, offsets, terms, weights, present, packed, rebased)) return rc;
    return list_set_impl(h, attr, first, n, rebased.data(), packed.data(), present);
    });
}

int mlvdb_sparse_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const int64_t* offsets,
                        const int32_t* terms, const float* weights, const uint8_t* present, int64_t* updated) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = sparse_attr_check(h, attr)) return rc;
    return with_labels(h, labels, n, updated, true, "bad labels / n", [&]() -> int {
        std::vector<int64_t> packed, rebased;
        if (int rc = sparse_csr_pack(h, n, offsets, terms, weights, present, packed, rebased)) return rc;
        return list_set_at_impl(h, attr, labels, n, rebased.data(), packed.data(), present, updated);
    });
    });
}

int mlvdb_sparse_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int64_t* out_offsets, int32_t* out_terms,
                     float* out_weights, uint8_t* out_present, int64_t capacity, int64_t* needed) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = sparse_attr_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n)) return rc;
    if (!needed || !out_offsets || capacity < 0 || (capacity > 0 && (!out_terms || !out_weights)))
        return fail(h, MLVDB_ERR_INVALID_ARG, "bad output buffers");
    *needed = 0;
    if (n == 0) {
        out_offsets[0] = 0;
        return MLVDB_OK;
    }
    // the list read-back into a buffer of exactly the size its first launches report, then unpacked
    if (int rc = list_scan(h, h->attr_col[attr] + first, nullptr, n, needed)) return rc;
    if (capacity < *needed) return MLVDB_OK;
    std::vector<int64_t> packed((size_t)*needed);
    if (int rc = list_get_impl(h, attr, first, n, out_offsets, packed.data(), out_present, *needed, needed)) return rc;
    for (size_t j = 0; j < packed.size(); ++j) {
        out_terms[j] = (int32_t)(packed[j] >> 32);
        const uint32_t bits = (uint32_t)(packed[j] & 0xffffffffll);
        std::memcpy(&out_weights[j], &bits, sizeof bits);
    }
    return MLVDB_OK;
    });
}

int mlvdb_search_batch_sparse(mlvdb_index* h, int32_t attr, const int64_t* q_offsets, const int32_t* q_terms,
                              const float* q_weights, int64_t nq, int32_t k, const mlvdb_where* where, int64_t* out_labels,
                              float* out_score, int32_t* out_counts, double* out_score64) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched
    if (int rc = sparse_attr_check(h, attr)) return rc;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max(h, k, "sparse search: ")) return rc;
    if (nq > 0 && (!q_offsets || !out_labels || !out_score || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (nq > 0 && q_offsets[0] != 0) return fail(h, MLVDB_ERR_INVALID_ARG, "sparse search: q_offsets must start at 0");
    if (int rc = sparse_queries_check(h, nq, q_offsets, q_terms, q_weights)) return rc;
    if (int rc = check_row_limit(h, "sparse search: ")) return rc;
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    if (nq == 0) return MLVDB_OK;
    if (h->total == 0) {
        pad_outputs(out_labels, out_score, out_score64, nq * k, out_counts, nq, -1.0f);  // scores: -inf
        return MLVDB_OK;
    }
    const uint8_t* mask = nullptr;  // the program's live matching rows, which every pass reads at one byte per row
    if (int rc = where_mask(h, where, &mask)) return rc;
    for (int64_t q0 = 0; q0 < nq; q0 += kSparseChunk) {
        const int64_t q1 = std::min<int64_t>(nq, q0 + kSparseChunk);
        if (int rc = sparse_pass(h, attr, q_offsets, q_terms, q_weights, q0, q1, k, mask, out_labels, out_score, out_counts,
                              out_score64))
            return rc;
    }
    return MLVDB_OK;
    });
}

// ---- binary vector columns (mlvdb_bits.h)
extern "C++" {
namespace {
int bits_attr_check(mlvdb_index* h, int32_t attr) { return typed_attr_check(h, attr, MLVDB_ATTR_BITS, "not a bits column"); }

int bits_words_check(mlvdb_index* h, int32_t words) {
    if (words < 1 || words > MLVDB_BITS_MAX_WORDS) return fail(h, MLVDB_ERR_INVALID_ARG, "words must be in 1..MLVDB_BITS_MAX_WORDS");
    return MLVDB_OK;
}

// n codes of `words` words as the CSR the pool's entries take: row i owns [offsets[i], offsets[i + 1]), an absent row an
// empty range, the present rows' words back to back in `packed`; nothing is written or launched.
void bits_csr_pack(int64_t n, int32_t words, const uint64_t* codes, const uint8_t* present, std::vector<int64_t>& packed,
                   std::vector<int64_t>& offsets) {
    offsets.resize((size_t)n + 1);
    offsets[0] = 0;
    for (int64_t i = 0; i < n; ++i) offsets[(size_t)i + 1] = offsets[(size_t)i] + ((present && !present[i]) ? 0 : words);
    packed.resize((size_t)offsets[(size_t)n]);
    for (int64_t i = 0; i < n; ++i)
        if (offsets[(size_t)i + 1] > offsets[(size_t)i])
            std::memcpy(packed.data() + offsets[(size_t)i], codes + i * words, (size_t)words * sizeof(uint64_t));
}

// One pass of at most kBitsChunk queries [q0, q1): queries and popcounts up, scan, merge, answers down.
int bits_pass(mlvdb_index* h, int32_t attr, const uint64_t* queries, int64_t q0, int64_t q1, int32_t words, int32_t metric,
              int32_t k, const uint8_t* mask, int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64) {
    hipStream_t s = h->stream;
    const int32_t n = (int32_t)(q1 - q0);
    const size_t nk = (size_t)n * k;
    const uint64_t* q = queries + q0 * words;
    std::vector<int32_t> qpop((size_t)n, 0);
    for (int32_t i = 0; i < n; ++i)
        for (int32_t w = 0; w < words; ++w) qpop[(size_t)i] += __builtin_popcountll(q[(size_t)i * words + w]);
    const int32_t nblk = bits_scan_blocks(h->total, n, k, words);
    uint64_t* q_d = nullptr;
    int32_t* qpop_d = nullptr;
    CARVE(h, h->bits_in, [&](Carver& c) {
        q_d = c.take<uint64_t>((size_t)n * words);
        qpop_d = c.take<int32_t>((size_t)n);
    });
    HIP_TRY(h, h->partial.ensure(nk * (size_t)nblk * sizeof(TopEntry)));
    ListBlock o;
    if (int rc = carve_list(h, h->bits_out, nk, (size_t)n, o)) return rc;
    HIP_TRY(h, hipMemcpyAsync(q_d, q, (size_t)n * words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(qpop_d, qpop.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_bits_scan(h->attr_col[attr], h->list_pool[attr], h->rn, mask, h->total, q_d, qpop_d, n, words, metric, k, nblk,
                                h->partial.as<TopEntry>(), s));
    HIP_TRY(h, launch_exact_merge(h->partial.as<TopEntry>(), n, nullptr, nullptr, nblk, k, o.lab, o.dist, o.cnt, o.d64, s));
    const size_t at = (size_t)q0 * k;
    // (copy_down drains the stream: qpop is consumed by then)
    return copy_down(h, s, {{out_labels, at, o.lab, nk}, {out_dist, at, o.dist, nk}, {out_counts, (size_t)q0, o.cnt, (size_t)n},
                            {out_dist64, at, o.d64, nk}});
}
}  // namespace
}  // extern "C++"

int mlvdb_bits_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int32_t words, const uint64_t* codes,
                   const uint8_t* present) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = bits_attr_check(h, attr)) return rc;
    if (int rc = bits_words_check(h, words)) return rc;
    if (int rc = check_row_range(h, first, n)) return rc;
    if (n == 0) return MLVDB_OK;
    if (!codes) return fail(h, MLVDB_ERR_INVALID_ARG, "codes is null");
    std::vector<int64_t> packed, offsets;
    bits_csr_pack(n, words, codes, present, packed, offsets);
    return list_set_impl(h, attr, first, n, offsets.data(), packed.data(), present);
    });
}

int mlvdb_bits_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, int32_t words, const uint64_t* codes,
                      const uint8_t* present, int64_t* updated) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked before anything is launched
    if (int rc = bits_attr_check(h, attr)) return rc;
    if (int rc = bits_words_check(h, words)) return rc;
    if (!updated || n < 0 || (n > 0 && !labels)) return fail(h, MLVDB_ERR_INVALID_ARG, "bad labels / n");
    *updated = 0;
    if (n == 0) return MLVDB_OK;
    if (!codes) return fail(h, MLVDB_ERR_INVALID_ARG, "codes is null");
    if (int rc = labels_check(h, labels, n)) return rc;
    std::vector<int64_t> packed, offsets;
    bits_csr_pack(n, words, codes, present, packed, offsets);
    return list_set_at_impl(h, attr, labels, n, offsets.data(), packed.data(), present, updated);
    });
}

int mlvdb_bits_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int32_t* out_words, uint64_t* out_codes,
                   int64_t capacity, int64_t* needed) {
    return guarded(h, kOnDevice, [&]() -> int {
    if (int rc = bits_attr_check(h, attr)) return rc;
    if (int rc = check_row_range(h, first, n)) return rc;
    if (!needed || capacity < 0 || (n > 0 && !out_words) || (capacity > 0 && !out_codes))
        return fail(h, MLVDB_ERR_INVALID_ARG, "bad output buffers");
    *needed = 0;
    if (n == 0) return MLVDB_OK;
    // the list read-back: a row's width is the length of its range, 0 for an absent row (a present code has >= 1 word)
    if (int rc = list_scan(h, h->attr_col[attr] + first, nullptr, n, needed)) return rc;
    if (capacity < *needed) return MLVDB_OK;
    std::vector<int64_t> offsets((size_t)n + 1);
    static_assert(sizeof(uint64_t) == sizeof(int64_t), "the codes are read back as the pool's elements");
    if (int rc = list_get_impl(h, attr, first, n, offsets.data(), reinterpret_cast<int64_t*>(out_codes), nullptr, *needed, needed))
        return rc;
    for (int64_t i = 0; i < n; ++i) out_words[i] = (int32_t)(offsets[(size_t)i + 1] - offsets[(size_t)i]);
    return MLVDB_OK;
    });
}

int mlvdb_search_batch_bits(mlvdb_index* h, int32_t attr, const uint64_t* queries, int64_t nq, int32_t words, int32_t metric,
                            int32_t k, const mlvdb_where* where, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                            double* out_dist64) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched
    if (int rc = bits_attr_check(h, attr)) return rc;
    if (int rc = bits_words_check(h, words)) return rc;
    if (metric != MLVDB_BITS_HAMMING && metric != MLVDB_BITS_JACCARD) return fail(h, MLVDB_ERR_INVALID_ARG, "unknown bits metric");
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max(h, k, "bits search: ")) return rc;
    if (nq > 0 && (!queries || !out_labels || !out_dist || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_row_limit(h, "bits search: ")) return rc;
    if (int rc = where ? where_prepare(h, where) : MLVDB_OK) return rc;
    if (nq == 0) return MLVDB_OK;
    if (h->total == 0) {
        pad_outputs(out_labels, out_dist, out_dist64, nq * k, out_counts, nq);
        return MLVDB_OK;
    }
    const uint8_t* mask = nullptr;  // the program's live matching rows, which every pass reads at one byte per row
    if (int rc = where_mask(h, where, &mask)) return rc;
    for (int64_t q0 = 0; q0 < nq; q0 += kBitsChunk) {
        const int64_t q1 = std::min<int64_t>(nq, q0 + kBitsChunk);
        if (int rc = bits_pass(h, attr, queries, q0, q1, words, metric, k, mask, out_labels, out_dist, out_counts, out_dist64))
            return rc;
    }
    return MLVDB_OK;
    });
}

// ---- hybrid search (mlvdb_hybrid.h)
extern "C++" {
namespace {
constexpr int64_t kHybridChunk = kSparseChunk;  // queries per round: one sparse pass, one plain search, three or five launches

// The validated call (h->rn is the masked copy and `mask` h->row_mask when a program restricts the rows).  Per chunk of
// queries: dense and sparse queries up -> the plain device search for fetch_dense neighbours and the sparse pass for
// fetch_sparse, both lists left on the device -> union -> the completion (launch_pair_distances on the members without a
// distance, the gathered scorer on those without a score; skipped when `complete` is false) -> fuse and select -> outputs down.
int hybrid_impl(mlvdb_index* h, const float* queries, int32_t attr, const int64_t* off, const int32_t* terms,
                const float* weights, int64_t nq, int32_t k, int32_t fd, int32_t fs, int32_t method, double w_dense,
                double w_sparse, double rrf_c, const uint8_t* mask, int64_t* out_labels, double* out_fused, int32_t* out_counts,
                double* out_dist64, double* out_sparse64, int32_t* out_rank_dense, int32_t* out_rank_sparse) {
    hipStream_t s = h->stream;
    if (h->total == 0 || h->total == h->deleted) {
        pad(out_labels, nq * k, -1);
        pad(out_fused, nq * k, -__builtin_inf());
        pad(out_counts, nq, 0);
        pad(out_dist64, nq * k, __builtin_inf());
        pad(out_sparse64, nq * k, -__builtin_inf());
        pad(out_rank_dense, nq * k, -1);
        pad(out_rank_sparse, nq * k, -1);
        return MLVDB_OK;
    }
    const bool complete = method != MLVDB_FUSE_RRF || out_dist64 || out_sparse64;
    const int32_t m = fd + fs;
    std::vector<int64_t> roff;
    for (int64_t q0 = 0; q0 < nq; q0 += kHybridChunk) {
        const int32_t n = (int32_t)std::min<int64_t>(kHybridChunk, nq - q0);
        const size_t nk = (size_t)n * k, nm = (size_t)n * m, nt = (size_t)(off[q0 + n] - off[q0]);
        int64_t* d_off = nullptr;  // the chunk's sparse queries (offsets, terms, weights) and its dense ones, raw and prepared
        double* d_aux = nullptr;
        float *dq = nullptr, *d_pad = nullptr, *d_weights = nullptr;
        int32_t* d_terms = nullptr;
        CARVE(h, h->hyb_q, [&](Carver& c) {
            d_off = c.take<int64_t>((size_t)n + 1);
            d_aux = c.take<double>((size_t)n);
            dq = c.take<float>((size_t)n * h->dim);
            d_pad = c.take<float>((size_t)n * h->ld);
            d_terms = c.take<int32_t>(nt);
            d_weights = c.take<float>(nt);
            c.take<char>(16);  // slack
        });
        ListBlock ld, ls;  // the two legs' ranked lists
        CARVE(h, h->hyb_list, [&](Carver& c) {
            ld.take(c, (size_t)n * fd, (size_t)n);
            c.pad_to(8);
            ls.take(c, (size_t)n * fs, (size_t)n);
        });
        double *comp_d = nullptr, *comp_s = nullptr;  // the union: completed components, labels, members to complete, ranks
        int64_t *u_lab = nullptr, *need_d = nullptr, *need_s = nullptr;
        int32_t *u_rd = nullptr, *u_rs = nullptr, *u_cnt = nullptr;
        CARVE(h, h->hyb_union, [&](Carver& c) {
            comp_d = c.take<double>(nm);
            comp_s = c.take<double>(nm);
            u_lab = c.take<int64_t>(nm);
            need_d = c.take<int64_t>(nm);
            need_s = c.take<int64_t>(nm);
            u_rd = c.take<int32_t>(nm);
            u_rs = c.take<int32_t>(nm);
            u_cnt = c.take<int32_t>((size_t)n);
        });
        double *o_fused = nullptr, *o_d64 = nullptr, *o_s64 = nullptr;
        int64_t* o_lab = nullptr;
        int32_t *o_rd = nullptr, *o_rs = nullptr, *o_cnt = nullptr;
        CARVE(h, h->hyb_out, [&](Carver& c) {
            o_fused = c.take<double>(nk);
            o_d64 = c.take<double>(nk);
            o_s64 = c.take<double>(nk);
            o_lab = c.take<int64_t>(nk);
            o_rd = c.take<int32_t>(nk);
            o_rs = c.take<int32_t>(nk);
            o_cnt = c.take<int32_t>((size_t)n);
        });
        roff.resize((size_t)n + 1);
        for (int32_t i = 0; i <= n; ++i) roff[(size_t)i] = off[q0 + i] - off[q0];
        // (the host arrays of these copies are consumed when sparse_pass_device returns: it drains the stream)
        HIP_TRY(h, hipMemcpyAsync(dq, queries + (size_t)q0 * h->dim, (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(d_off, roff.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (nt) {
            HIP_TRY(h, hipMemcpyAsync(d_terms, terms + off[q0], nt * sizeof(int32_t), hipMemcpyHostToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(d_weights, weights + off[q0], nt * sizeof(float), hipMemcpyHostToDevice, s));
        }
        if (int rc = search_device_impl(h, dq, n, fd, ld.lab, ld.dist, ld.cnt, ld.d64, s, false)) return rc;
        if (int rc = sparse_pass_device(h, attr, off, terms, weights, q0, q0 + n, fs, mask, ls)) return rc;
        HIP_TRY(h, launch_hybrid_union(ld.lab, ld.cnt, fd, ls.lab, ls.cnt, fs, n, u_lab, u_rd, u_rs, need_d, need_s, u_cnt, s));
        if (complete) {
            HIP_TRY(h, launch_query_prep(dq, n, h->dim, h->ld, h->space, d_pad, d_aux, nullptr, s));
            HIP_TRY(h, launch_pair_distances(h->X, d_pad, d_aux, need_d, n, m, h->ld, h->space, comp_d, nullptr, s));
            HIP_TRY(h, launch_sparse_pair_score(h->attr_col[attr], h->list_pool[attr], h->total, d_off, d_terms, d_weights, need_s,
                                                u_cnt, n, m, comp_s, s));
        }
        HIP_TRY(h, launch_hybrid_fuse(u_lab, u_rd, u_rs, u_cnt, n, m, ld.d64, fd, ls.d64, fs, complete ? comp_d : nullptr,
                                      complete ? comp_s : nullptr, method, w_dense, w_sparse, rrf_c, k, o_lab, o_fused, o_cnt,
                                      out_dist64 ? o_d64 : nullptr, out_sparse64 ? o_s64 : nullptr,
                                      out_rank_dense ? o_rd : nullptr, out_rank_sparse ? o_rs : nullptr, s));
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{out_labels, at, o_lab, nk}, {out_fused, at, o_fused, nk},
                                      {out_counts, (size_t)q0, o_cnt, (size_t)n}, {out_dist64, at, o_d64, nk},
                                      {out_sparse64, at, o_s64, nk}, {out_rank_dense, at, o_rd, nk},
                                      {out_rank_sparse, at, o_rs, nk}}))
            return rc;
    }
    return MLVDB_OK;
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_hybrid(mlvdb_index* h, const float* queries, int32_t attr, const int64_t* q_offsets,
                              const int32_t* q_terms, const float* q_weights, int64_t nq, int32_t k, int32_t fetch_dense,
                              int32_t fetch_sparse, int32_t method, double w_dense, double w_sparse, double rrf_c,
                              const mlvdb_where* where, int64_t* out_labels, double* out_fused, int32_t* out_counts,
                              double* out_dist64, double* out_sparse64, int32_t* out_rank_dense, int32_t* out_rank_sparse) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched (the program: with_where)
    if (int rc = sparse_attr_check(h, attr)) return rc;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max(h, k, "hybrid: ")) return rc;
    if (fetch_dense < 1 || fetch_sparse < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: fetch_dense / fetch_sparse must be >= 1");
    if (fetch_dense > kHybridMaxFetchDense) return fail(h, MLVDB_ERR_UNSUPPORTED, "hybrid: fetch_dense above MLVDB_HYBRID_MAX_FETCH_DENSE");
    if (fetch_sparse > MLVDB_MAX_TOPK) return fail(h, MLVDB_ERR_UNSUPPORTED, "hybrid: fetch_sparse above MLVDB_MAX_TOPK");
    if (k > fetch_dense + fetch_sparse) return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: k above fetch_dense + fetch_sparse");
    if (method != MLVDB_FUSE_RRF && method != MLVDB_FUSE_LINEAR && method != MLVDB_FUSE_RELATIVE)
        return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: unknown fusion method");
    if (!(std::isfinite(w_dense) && w_dense >= 0.0 && std::isfinite(w_sparse) && w_sparse >= 0.0))
        return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: a weight must be finite and >= 0");
    if (!(std::isfinite(rrf_c) && rrf_c >= 0.0)) return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: the RRF constant must be finite and >= 0");
    if (nq > 0 && (!queries || !q_offsets || !out_labels || !out_fused || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (nq > 0 && q_offsets[0] != 0) return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: q_offsets must start at 0");
    if (int rc = sparse_queries_check(h, nq, q_offsets, q_terms, q_weights)) return rc;
    for (int64_t i = 0; i < nq * h->dim; ++i)
        if (queries[i] != queries[i]) return fail(h, MLVDB_ERR_INVALID_ARG, "hybrid: a NaN in the dense queries");
    if (int rc = check_row_limit(h, "hybrid: ")) return rc;
    auto call = [&]() {
        // (under a program h->row_mask holds the one evaluation both legs read: the dense leg through the masked norms)
        const uint8_t* mask = where && h->total > 0 ? h->row_mask.as<uint8_t>() : nullptr;
        return hybrid_impl(h, queries, attr, q_offsets, q_terms, q_weights, nq, k, fetch_dense, fetch_sparse, method, w_dense,
                           w_sparse, rrf_c, mask, out_labels, out_fused, out_counts, out_dist64, out_sparse64, out_rank_dense,
                           out_rank_sparse);
    };
    // the first launches: where_run(h, where, ...) for the program, then hybrid_impl under with_row_mask(h, nq, ...)
    return with_where(h, where, nq, call);
    });
}

// ---- scored kNN (mlvdb_score.h)
extern "C++" {
namespace {
// Host validation of a score program and its conds (the stack's depth throughout and at the end, the columns ATTR reads, the
// MATCH indices; each cond by where_prepare) -> `out`, the block the scan stages, and the conds' concatenated set table.
// Nothing is launched for a program refused here.
int score_prepare(mlvdb_index* h, const mlvdb_score* sc, ScoreProgram& out, std::vector<int64_t>& set) {
    if (!sc) return fail(h, MLVDB_ERR_INVALID_ARG, "score is null");
    if (sc->n_ops < 1 || sc->n_ops > MLVDB_SCORE_MAX_OPS || !sc->ops)
        return fail(h, MLVDB_ERR_INVALID_ARG, "a score program holds 1..MLVDB_SCORE_MAX_OPS ops");
    if (sc->n_conds < 0 || sc->n_conds > MLVDB_SCORE_MAX_CONDS || (sc->n_conds > 0 && !sc->conds))
        return fail(h, MLVDB_ERR_INVALID_ARG, "score: n_conds outside 0..MLVDB_SCORE_MAX_CONDS");
    int64_t cond_ops = 0;
    for (int32_t c = 0; c < sc->n_conds; ++c) cond_ops += sc->conds[c].n_ops > 0 ? sc->conds[c].n_ops : 0;
    if (cond_ops > MLVDB_WHERE_MAX_OPS) return fail(h, MLVDB_ERR_INVALID_ARG, "score: more than MLVDB_WHERE_MAX_OPS ops over all conds");
    std::memset(&out, 0, sizeof out);
    int depth = 0;
    for (int32_t i = 0; i < sc->n_ops; ++i) {
        const mlvdb_score_op& o = sc->ops[i];
        ScoreOp& d = out.ops[i];
        d = ScoreOp{o.op, 0, o.a};
        switch (o.op) {
            case MLVDB_SCORE_ADD: case MLVDB_SCORE_SUB: case MLVDB_SCORE_MUL: case MLVDB_SCORE_DIV:
            case MLVDB_SCORE_MIN: case MLVDB_SCORE_MAX:
                if (depth < 2) return fail(h, MLVDB_ERR_INVALID_ARG, "score: a binary op needs two operands on the stack");
                --depth;
                continue;
            case MLVDB_SCORE_NEG: case MLVDB_SCORE_ABS:
                if (depth < 1) return fail(h, MLVDB_ERR_INVALID_ARG, "score: NEG / ABS needs an operand on the stack");
                continue;
            case MLVDB_SCORE_CONST: case MLVDB_SCORE_DIST:
                break;
            case MLVDB_SCORE_ATTR: {
                if (int rc = attr_check(h, o.attr)) return rc;
                const int32_t type = h->attr_type[o.attr];
                if (type != MLVDB_ATTR_INT64 && type != MLVDB_ATTR_FLOAT64)
                    return fail(h, MLVDB_ERR_INVALID_ARG, "score: ATTR needs an int64 or float64 column (list, sparse, geo and bits columns hold no number)");
                int32_t j = 0;  // the (column, default) pair's operand
                while (j < out.n_operands && !(out.operands[j].col == h->attr_col[o.attr] && out.operands[j].dflt == o.a)) ++j;
                if (j == out.n_operands) out.operands[out.n_operands++] = ScoreOperand{h->attr_col[o.attr], o.a, type, 0};
                d.slot = j;
                break;
            }
            case MLVDB_SCORE_MATCH:
                if (o.a < 0 || o.a >= sc->n_conds) return fail(h, MLVDB_ERR_INVALID_ARG, "score: MATCH index outside conds");
                d.slot = (int32_t)o.a;
                break;
            default:
                return fail(h, MLVDB_ERR_INVALID_ARG, "unknown score op");
        }
        if (++depth > MLVDB_SCORE_MAX_DEPTH) return fail(h, MLVDB_ERR_INVALID_ARG, "score program deeper than MLVDB_SCORE_MAX_DEPTH");
    }
    if (depth != 1) return fail(h, MLVDB_ERR_INVALID_ARG, "a score program must leave exactly one value on the stack");
    out.n_ops = sc->n_ops;
    out.n_conds = sc->n_conds;
    EachPrograms ep;
    if (int rc = where_each_pack(h, sc->conds, sc->n_conds, ep)) return rc;
    std::copy(ep.ops.begin(), ep.ops.end(), out.cond_ops);
    std::copy(ep.off.begin(), ep.off.end(), out.cond_off);
    set = std::move(ep.set);
    return MLVDB_OK;
}

// Where a chunk's outputs lie in h->score_out: n queries of k entries each (dist: the merge's fp32 image of the scores, unused)
struct ScoredOut {
    double* score = nullptr;
    double* d64 = nullptr;
    int64_t* lab = nullptr;
    float* dist = nullptr;
    int32_t* cnt = nullptr;
    void take(Carver& c, size_t nk, size_t n) {
        score = c.take<double>(nk);
        d64 = c.take<double>(nk);
        lab = c.take<int64_t>(nk);
        dist = c.take<float>(nk);
        cnt = c.take<int32_t>(n);
    }
};

// The validated call (h->rn is the masked copy when a program restricts the rows): the programs to the device, then per chunk
// of queries the scored scan, the merge, the distances of the returned pairs and the outputs to the host.
int scored_impl(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const ScoreProgram& prog,
                const std::vector<int64_t>& set, int64_t* out_labels, double* out_score, int32_t* out_counts,
                double* out_dist64) {
    hipStream_t s = h->stream;
    if (h->total == 0 || h->total == h->deleted) {
        pad(out_labels, nq * k, -1);
        pad(out_score, nq * k, __builtin_inf());
        pad(out_dist64, nq * k, __builtin_inf());
        pad(out_counts, nq, 0);
        return MLVDB_OK;
    }
    if (int rc = begin_call(h, s)) return rc;
    ScoreProgram* prog_d = nullptr;
    int64_t* set_d = nullptr;
    CARVE(h, h->score_prog, [&](Carver& c) {
        prog_d = c.take<ScoreProgram>(1);
        set_d = c.take<int64_t>(set.size());
        c.take<char>(sizeof(int64_t));  // slack behind the set table
    });
    HIP_TRY(h, hipMemcpyAsync(prog_d, &prog, sizeof prog, hipMemcpyHostToDevice, s));
    if (!set.empty()) HIP_TRY(h, hipMemcpyAsync(set_d, set.data(), set.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    for (int64_t q0 = 0; q0 < nq; q0 += kDistinctChunk) {
        const int32_t n = (int32_t)std::min<int64_t>(kDistinctChunk, nq - q0);
        const size_t nk = (size_t)n * k;
        HIP_TRY(h, h->score_q.ensure((size_t)n * h->dim * sizeof(float)));
        HIP_TRY(h, h->qpad.ensure((size_t)n * h->ld * sizeof(float)));
        HIP_TRY(h, h->qaux.ensure((size_t)n * sizeof(double)));
        ScoredOut o{};
        if (int rc = carve(h, h->score_out, [&](Carver& c) { o.take(c, nk, (size_t)n); })) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->score_q.p, queries + (size_t)q0 * h->dim, (size_t)n * h->dim * sizeof(float),
                                  hipMemcpyHostToDevice, s));
        HIP_TRY(h, launch_query_prep(h->score_q.as<float>(), n, h->dim, h->ld, h->space, h->qpad.as<float>(),
                                     h->qaux.as<double>(), nullptr, s));
        const ExactPlan plan = plan_scored(h->total, h->ld, n, k);
        HIP_TRY(h, h->partial.ensure(nk * plan.nblk * sizeof(TopEntry)));
        ScoredArgs a{};
        a.X = h->X;
        a.rn = h->rn;
        a.total = h->total;
        a.ld = h->ld;
        a.space = h->space;
        a.Qpad = h->qpad.as<float>();
        a.qaux = h->qaux.as<double>();
        a.nq = n;
        a.k = k;
        a.prog = prog_d;
        a.set = set_d;
        a.partial = h->partial.as<TopEntry>();
        if (int rc = scan_step(h, s, h->total * plan.nqtiles, [&] { return launch_scored_scan(a, plan, s); })) return rc;
        h->stats.strategy_used = MLVDB_STRATEGY_EXACT;
        HIP_TRY(h, launch_exact_merge(a.partial, n, nullptr, nullptr, plan.nblk, k, o.lab, o.dist, o.cnt, o.score, s));
        // the bits DIST had for every hit: the same accumulate_rows on the returned pairs (a padded label gives +inf)
        if (out_dist64)
            HIP_TRY(h, launch_pair_distances(h->X, a.Qpad, a.qaux, o.lab, n, k, h->ld, h->space, o.d64, nullptr, s));
        const size_t at = (size_t)q0 * k;
        if (int rc = copy_down(h, s, {{out_score, at, o.score, nk}, {out_dist64, at, o.d64, nk}, {out_labels, at, o.lab, nk},
                                      {out_counts, (size_t)q0, o.cnt, (size_t)n}}))
            return rc;
    }
    return end_call(h, s);
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_scored(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const mlvdb_score* score,
                              const mlvdb_where* where, int64_t* out_labels, double* out_score, int32_t* out_counts,
                              double* out_dist64) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched (the outer program: with_where)
    ScoreProgram prog;
    std::vector<int64_t> set;
    if (int rc = score_prepare(h, score, prog, set)) return rc;
    if (int rc = check_nq(h, nq)) return rc;
    if (int rc = check_k_min(h, k)) return rc;
    if (int rc = check_k_max(h, k, "scored: ")) return rc;
    if (nq > 0 && (!queries || !out_labels || !out_score || !out_counts)) return fail(h, MLVDB_ERR_INVALID_ARG, "null buffer");
    if (int rc = check_row_limit(h, "scored: ")) return rc;
    auto call = [&]() { return scored_impl(h, queries, nq, k, prog, set, out_labels, out_score, out_counts, out_dist64); };
    return with_where(h, where, nq, call);
    });
}


// ---- recommend / discover (mlvdb_examples.h)
extern "C++" {
namespace {
// The validated call (h->rn is the masked copy when a program restricts the rows; the examples' values are read from h->X,
// which no mask touches).  Per chunk of queries: the bags cut into tiles (examples_cut), examples, tiles and exclusion labels
// to the device -> the staging kernel and the query prep -> launch t of the scan walks tile t of every query that has one,
// the state workspace carrying a bag from one launch to the next -> the merge -> outputs to the host.
int examples_impl(mlvdb_index* h, int32_t mode, const int64_t* labels, const float* vectors, const int32_t* roles,
                  const int64_t* off, int64_t nq, int32_t k, int32_t exclude, int64_t* out_labels, int32_t* out_tier,
                  double* out_value, int32_t* out_counts) {
    hipStream_t s = h->stream;
    if (h->total == 0 || h->total == h->deleted) {
        pad(out_labels, nq * k, -1);
        pad(out_tier, nq * k, INT32_MAX);
        pad(out_value, nq * k, __builtin_inf());
        pad(out_counts, nq, 0);
        return MLVDB_OK;
    }
    if (int rc = begin_call(h, s)) return rc;
    int32_t most = 0;
    for (int64_t i = 0; i < nq; ++i) most = std::max(most, (int32_t)(off[i + 1] - off[i]));
    const int32_t qt = examples_tile_width(h->ld, most);  // one width for the call: the answer does not depend on it
    const int64_t budget = (int64_t)std::max(1, h->tn.examples_ws_mb) << 20;
    // (tiles of one example carry a pair's POS distance beside the state)
    const int64_t per_query = h->total * (int64_t)(sizeof(ExamplesState) + (qt == 1 ? sizeof(double) : 0));
    std::vector<ExamplesTile> cut, tiles;  // the chunk's tiles query by query / launch by launch
    std::vector<int32_t> first_tile, launch_at, excl, raw, nblk_of;
    std::vector<float> raw_rows;
    std::vector<ExactPlan> plans;
    for (int64_t q0 = 0; q0 < nq;) {
        // the chunk: queries while they and their examples fit the chunk and the state of their bags the budget, always at
        // least one
        cut.clear();
        excl.clear();
        first_tile.assign(1, 0);
        int32_t slots = 0;
        int64_t q1 = q0;
        for (; q1 < nq; ++q1) {
            if (q1 > q0 && (q1 - q0 >= kExamplesChunk || off[q1 + 1] - off[q0] > kExamplesChunkExamples)) break;
            const size_t cut_before = cut.size(), excl_before = excl.size();
            for (int64_t j = off[q1]; exclude && j < off[q1 + 1]; ++j)  // the query's distinct stored labels
                if (labels[j] >= 0 && std::find(excl.begin() + excl_before, excl.end(), (int32_t)labels[j]) == excl.end())
                    excl.push_back((int32_t)labels[j]);
            const int nt = examples_cut(mode, roles + off[q1], (int32_t)(off[q1 + 1] - off[q1]), qt, (int32_t)(off[q1] - off[q0]),
                                        (int32_t)(q1 - q0), (int32_t)excl_before, (int32_t)(excl.size() - excl_before), cut);
            if (nt > 1) {
                if (q1 > q0 && (slots + 1) * per_query > budget) {
                    cut.resize(cut_before);
                    excl.resize(excl_before);
                    break;
                }
                for (size_t i = cut_before; i < cut.size(); ++i) cut[i].state = slots;
                ++slots;
            }
            first_tile.push_back((int32_t)cut.size());
        }
        const int32_t n = (int32_t)(q1 - q0);
        const int64_t e0 = off[q0];
        const size_t ne = (size_t)(off[q1] - e0), nk = (size_t)n * k;
        // launch t: tile t of every query that has one
        int32_t launches = 0;
        for (int32_t i = 0; i < n; ++i) launches = std::max(launches, first_tile[(size_t)i + 1] - first_tile[(size_t)i]);
        tiles.clear();
        launch_at.assign(1, 0);
        for (int32_t t = 0; t < launches; ++t) {
            for (int32_t i = 0; i < n; ++i)
                if (first_tile[(size_t)i] + t < first_tile[(size_t)i + 1]) tiles.push_back(cut[(size_t)(first_tile[(size_t)i] + t)]);
            launch_at.push_back((int32_t)tiles.size());
        }
        plans.clear();
        int32_t stride = 1;
        for (int32_t t = 0; t < launches; ++t) {
            plans.push_back(plan_examples(h->total, h->ld, qt, launch_at[(size_t)t + 1] - launch_at[(size_t)t]));
            stride = std::max(stride, plans.back().nblk);
        }
        nblk_of.resize((size_t)n);
        for (int32_t i = 0; i < n; ++i) nblk_of[(size_t)i] = plans[(size_t)(first_tile[(size_t)i + 1] - first_tile[(size_t)i] - 1)].nblk;
        // the raw examples' rows, packed
        raw.assign(ne, -1);
        raw_rows.clear();
        for (size_t j = 0; j < ne; ++j)
            if (labels[e0 + (int64_t)j] < 0) {
                raw[j] = (int32_t)(raw_rows.size() / (size_t)h->dim);
                raw_rows.insert(raw_rows.end(), vectors + (size_t)(e0 + (int64_t)j) * h->dim, vectors + (size_t)(e0 + (int64_t)j + 1) * h->dim);
            }
        int64_t* lab_d = nullptr;
        ExamplesTile* tiles_d = nullptr;
        float* rows_d = nullptr;
        int32_t *raw_d = nullptr, *excl_d = nullptr, *nblk_d = nullptr;
        CARVE(h, h->ex_in, [&](Carver& c) {
            lab_d = c.take<int64_t>(ne);
            tiles_d = c.take<ExamplesTile>(tiles.size());
            rows_d = c.take<float>(raw_rows.size());
            raw_d = c.take<int32_t>(ne);
            excl_d = c.take<int32_t>(excl.size() + 1);
            nblk_d = c.take<int32_t>((size_t)n);
        });
        double* o_val = nullptr;
        int64_t* o_lab = nullptr;
        int32_t *o_tier = nullptr, *o_cnt = nullptr;
        CARVE(h, h->ex_out, [&](Carver& c) {
            o_val = c.take<double>(nk);
            o_lab = c.take<int64_t>(nk);
            o_tier = c.take<int32_t>(nk);
            o_cnt = c.take<int32_t>((size_t)n);
        });
        HIP_TRY(h, h->ex_q.ensure(ne * h->dim * sizeof(float)));
        HIP_TRY(h, h->qpad.ensure(ne * h->ld * sizeof(float)));
        HIP_TRY(h, h->qaux.ensure(ne * sizeof(double)));
        HIP_TRY(h, h->ex_state.ensure((size_t)slots * (size_t)per_query));
        HIP_TRY(h, h->partial.ensure(nk * (size_t)stride * sizeof(TopEntry)));
        HIP_TRY(h, hipMemcpyAsync(lab_d, labels + e0, ne * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(tiles_d, tiles.data(), tiles.size() * sizeof(ExamplesTile), hipMemcpyHostToDevice, s));
        if (!raw_rows.empty())
            HIP_TRY(h, hipMemcpyAsync(rows_d, raw_rows.data(), raw_rows.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(raw_d, raw.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!excl.empty()) HIP_TRY(h, hipMemcpyAsync(excl_d, excl.data(), excl.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(nblk_d, nblk_of.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, launch_examples_stage(h->X, h->dim, h->ld, lab_d, raw_d, rows_d, (int32_t)ne, h->ex_q.as<float>(), s));
        HIP_TRY(h, launch_query_prep(h->ex_q.as<float>(), (int32_t)ne, h->dim, h->ld, h->space, h->qpad.as<float>(),
                                     h->qaux.as<double>(), nullptr, s));
        ExamplesArgs a{};
        a.X = h->X;
        a.rn = h->rn;
        a.total = h->total;
        a.ld = h->ld;
        a.space = h->space;
        a.Qpad = h->qpad.as<float>();
        a.qaux = h->qaux.as<double>();
        a.k = k;
        a.excl = excl_d;
        a.state = h->ex_state.as<ExamplesState>();
        a.held = reinterpret_cast<double*>(a.state + (size_t)slots * (size_t)h->total);
        a.partial = h->partial.as<TopEntry>();
        a.partial_stride = stride;
        for (int32_t t = 0; t < launches; ++t) {
            a.tiles = tiles_d + launch_at[(size_t)t];
            a.ntiles = launch_at[(size_t)t + 1] - launch_at[(size_t)t];
            const ExactPlan& plan = plans[(size_t)t];
            if (int rc = scan_step(h, s, h->total * a.ntiles, [&] { return launch_examples_scan(a, plan, s); })) return rc;
        }
        h->stats.strategy_used = MLVDB_STRATEGY_EXACT;
        HIP_TRY(h, launch_examples_merge(a.partial, n, nblk_d, stride, k, o_lab, o_tier, o_val, o_cnt, s));
        const size_t at = (size_t)q0 * k;
        // (the wait inside also ends the reads of this chunk's host vectors)
        if (int rc = copy_down(h, s, {{out_value, at, o_val, nk}, {out_labels, at, o_lab, nk}, {out_tier, at, o_tier, nk},
                                      {out_counts, (size_t)q0, o_cnt, (size_t)n}}))
            return rc;
        q0 = q1;
    }
    return end_call(h, s);
}
}  // namespace
}  // extern "C++"

int mlvdb_search_batch_examples(mlvdb_index* h, int32_t mode, const int64_t* example_labels, const float* example_vectors,
                                const int32_t* example_roles, const int64_t* example_offsets, int64_t nq, int32_t k,
                                int32_t exclude_examples, const mlvdb_where* where, int64_t* out_labels, int32_t* out_tier,
                                double* out_value, int32_t* out_counts) {
    return guarded(h, kOnDevice, [&]() -> int {
    // everything is checked on the host before anything is launched (the program: with_where)
    const ExamplesRefusal r = examples_check(mode, example_labels, example_vectors, example_roles, example_offsets, nq, k,
                                             MLVDB_MAX_TOPK, h->total, h->dim, out_labels,
                                             out_tier, out_value, out_counts);
    if (r.code != MLVDB_OK) return fail(h, r.code, r.what);
    if (int rc = check_row_limit(h, "examples: ")) return rc;
    auto call = [&]() {
        return examples_impl(h, mode, example_labels, example_vectors, example_roles, example_offsets, nq, k, exclude_examples,
                             out_labels, out_tier, out_value, out_counts);
    };
    return with_where(h, where, nq, call);
    });
}


// ---- clustering (mlvdb_cluster.h)
extern "C++" {
namespace {
// The validated call (rn: the index's norms, or their masked copy when a program restricts the rows -- evaluated once, before
// anything is written; the centroids' stored rows are read from h->X, which no mask touches).  The centroids staged dense (examples_stage_kernel)
// -> per iteration: the query prep, one scan launch per tile in ascending order, the ordered member lists, ONE wait for the
// moved counter, the candidates and the member counts, the segment table up, the blocked sums and the finish -> the column,
// the outputs.  kmeans == false: one assignment, its counts and costs, no mean.
int cluster_impl(mlvdb_index* h, const float* rn, const int64_t* labels, const float* vectors, int32_t m, bool kmeans, int32_t max_iterations,
                 int32_t assign_attr, float* out_centroids, int64_t* out_rows, double* out_cost, int32_t* iterations,
                 int32_t* converged, int64_t* matched) {
    hipStream_t s = h->stream;
    const size_t md = (size_t)m * h->dim;
    // (an assignment that meets no candidate repeats itself: the second iteration is the first that can say "converged")
    const int32_t idle_iterations = std::min(2, max_iterations);
    if (h->total == 0) {  // (no stored label is valid here: every centroid is raw)
        if (out_centroids) std::copy(vectors, vectors + md, out_centroids);
        pad(out_rows, m, 0);
        pad(out_cost, m, 0.0);
        *matched = 0;
        if (iterations) *iterations = idle_iterations;
        if (converged) *converged = max_iterations >= 2;
        return MLVDB_OK;
    }
    if (int rc = begin_call(h, s)) return rc;
    const int32_t qt = cluster_tile_width(h->ld, m);
    const ExactPlan plan = plan_assign(h->total, h->ld, qt);
    if (plan.qt != qt) return fail(h, MLVDB_ERR_INTERNAL, "cluster: the scan's tile is not the width the centroids were cut by");
    const bool weights = kmeans && h->space == kSpaceCosine;
    const int64_t nblocks = cluster_list_blocks(h->total);
    const size_t total = (size_t)h->total;
    // the raw centroids' rows, packed
    std::vector<int32_t> raw((size_t)m, -1);
    std::vector<int64_t> lab((size_t)m, -1);
    std::vector<float> raw_rows;
    for (int32_t j = 0; j < m; ++j) {
        if (labels) lab[(size_t)j] = labels[j];
        if (lab[(size_t)j] >= 0) continue;
        raw[(size_t)j] = (int32_t)(raw_rows.size() / (size_t)h->dim);
        raw_rows.insert(raw_rows.end(), vectors + (size_t)j * h->dim, vectors + (size_t)(j + 1) * h->dim);
    }
    int64_t* lab_d = nullptr;
    float* rows_d = nullptr;
    int32_t* raw_d = nullptr;
    CARVE(h, h->cl_in, [&](Carver& c) {
        lab_d = c.take<int64_t>((size_t)m);
        rows_d = c.take<float>(raw_rows.size());
        raw_d = c.take<int32_t>((size_t)m);
    });
    double *best_d = nullptr, *w_d = nullptr, *cost_d = nullptr;
    unsigned long long* ctr_d = nullptr;  // [moved, candidates], the member counts right behind them: one copy down
    int64_t *counts_d = nullptr, *base_d = nullptr;
    int32_t *sidx_d = nullptr, *assign_d = nullptr, *members_d = nullptr, *hist_d = nullptr, *first_d = nullptr;
    CARVE(h, h->cl_ws, [&](Carver& c) {
        best_d = c.take<double>(total);
        w_d = c.take<double>(weights ? total : 0);
        cost_d = c.take<double>((size_t)m);
        ctr_d = c.take<unsigned long long>(2);
        counts_d = c.take<int64_t>((size_t)m);
        base_d = c.take<int64_t>((size_t)m);
        sidx_d = c.take<int32_t>(total);
        assign_d = c.take<int32_t>(total);
        members_d = c.take<int32_t>(total);
        hist_d = c.take<int32_t>((size_t)nblocks * (size_t)m);
        first_d = c.take<int32_t>((size_t)m + 1);
    });
    HIP_TRY(h, h->cl_cent.ensure(md * sizeof(float)));
    HIP_TRY(h, h->qpad.ensure((size_t)m * h->ld * sizeof(float)));
    HIP_TRY(h, h->qaux.ensure((size_t)m * sizeof(double)));
    float* const cent_d = h->cl_cent.as<float>();
    HIP_TRY(h, hipMemcpyAsync(lab_d, lab.data(), (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(raw_d, raw.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (!raw_rows.empty())
        HIP_TRY(h, hipMemcpyAsync(rows_d, raw_rows.data(), raw_rows.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_examples_stage(h->X, h->dim, h->ld, lab_d, raw_d, rows_d, m, cent_d, s));
    HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(assign_d), kClusterNoCandidate, total, s));
    if (weights) HIP_TRY(h, launch_cluster_weights(h->X, h->ld, h->total, w_d, s));

    AssignArgs a{};
    a.X = h->X;
    a.rn = rn;
    a.total = h->total;
    a.ld = h->ld;
    a.space = h->space;
    a.Qpad = h->qpad.as<float>();
    a.qaux = h->qaux.as<double>();
    a.m = m;
    a.best = best_d;
    a.sidx = sidx_d;
    a.assign = assign_d;
    a.moved = ctr_d;
    std::vector<int64_t> head((size_t)m + 2);  // moved, candidates, counts[m]
    std::vector<ClusterSegment> segs;
    std::vector<int32_t> seg_first;
    const int32_t last_iteration = kmeans ? max_iterations : 1;
    int32_t t = 1;
    bool done = false;
    for (;; ++t) {
        HIP_TRY(h, launch_query_prep(cent_d, m, h->dim, h->ld, h->space, h->qpad.as<float>(), h->qaux.as<double>(), nullptr, s));
        HIP_TRY(h, hipMemsetAsync(ctr_d, 0, 2 * sizeof(unsigned long long), s));
        for (a.first = 0; a.first < m; a.first += plan.qt)
            if (int rc = scan_step(h, s, h->total, [&] { return launch_assign_scan(a, plan, s); })) return rc;
        HIP_TRY(h, launch_cluster_list(assign_d, h->total, m, hist_d, counts_d, base_d, members_d, ctr_d + 1, s));
        // the iteration's one wait (it also ends the reads of the host vectors uploaded so far)
        HIP_TRY(h, hipMemcpyAsync(head.data(), ctr_d, head.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        done = kmeans && t >= 2 && head[0] == 0;
        cluster_segments(head.data() + 2, m, segs, seg_first);
        HIP_TRY(h, h->cl_segs.ensure(segs.size() * sizeof(ClusterSegment)));
        HIP_TRY(h, h->cl_part.ensure(segs.size() * ((size_t)h->ld + 1) * sizeof(double)));
        if (!segs.empty())
            HIP_TRY(h, hipMemcpyAsync(h->cl_segs.p, segs.data(), segs.size() * sizeof(ClusterSegment), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(first_d, seg_first.data(), seg_first.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, launch_cluster_sums(h->X, h->dim, h->ld, h->space == kSpaceCosine, h->cl_segs.as<ClusterSegment>(),
                                       (int32_t)segs.size(), first_d, members_d, w_d, best_d, counts_d, m, kmeans,
                                       h->cl_part.as<double>(), cent_d, cost_d, s));
        if (done || t == last_iteration) break;
    }
    h->stats.strategy_used = MLVDB_STRATEGY_EXACT;
    if (assign_attr >= 0) HIP_TRY(h, launch_cluster_write(assign_d, h->total, h->attr_col[assign_attr], s));
    // (the wait inside also ends the reads of the last segment table)
    if (int rc = copy_down(h, s, {{out_centroids, 0, cent_d, md}, {out_cost, 0, cost_d, (size_t)m}})) return rc;
    std::copy(head.begin() + 2, head.end(), out_rows);
    *matched = head[1];
    if (iterations) *iterations = t;
    if (converged) *converged = done ? 1 : 0;
    return end_call(h, s);
}

int cluster_entry(mlvdb_index* h, const int64_t* labels, const float* vectors, int32_t m, bool kmeans, int32_t max_iterations,
                  const mlvdb_where* where, int32_t assign_attr, float* out_centroids, int64_t* out_rows, double* out_cost,
                  int32_t* iterations, int32_t* converged, int64_t* matched) {
    // everything is checked on the host before anything is launched (the program: with_where)
    const int32_t attr_type = assign_attr >= 0 && assign_attr < MLVDB_MAX_ATTRS ? h->attr_type[assign_attr] : 0;
    const ClusterRefusal r = cluster_check(labels, vectors, m, h->total, h->dim, h->space, assign_attr, attr_type, out_rows,
                                           out_cost, matched, kmeans, max_iterations, out_centroids && iterations && converged);
    if (r.code != MLVDB_OK) return fail(h, r.code, r.what);
    if (int rc = check_row_limit(h, "cluster: ")) return rc;
    // The candidates: the index's norms, or a masked copy of them (NaN = no candidate) made once, before anything is written.
    // The copy is handed to the scan as an argument: the handle's own pointers stay as they are (nothing to restore on any
    // way out), and the int8 shadow, which this family never reads, is neither refreshed nor masked.
    const float* rn = h->rn;
    if (where) {
        if (int rc = where_run(h, where, nullptr)) return rc;
        if (h->total > 0) {
            HIP_TRY(h, h->rn_masked.ensure((size_t)h->capacity * sizeof(float)));
            HIP_TRY(h, launch_mask_norms(h->rn, h->row_mask.as<uint8_t>(), h->rn_masked.as<float>(), h->total, h->capacity, h->stream));
            rn = h->rn_masked.as<float>();
        }
    }
    return cluster_impl(h, rn, labels, vectors, m, kmeans, max_iterations, assign_attr, out_centroids, out_rows, out_cost,
                        iterations, converged, matched);
}
}  // namespace
}  // extern "C++"

int mlvdb_assign_nearest(mlvdb_index* h, const int64_t* centroid_labels, const float* centroid_vectors, int32_t m,
                         const mlvdb_where* where, int32_t assign_attr, int64_t* out_rows, double* out_cost, int64_t* matched) {
    return guarded(h, kOnDevice, [&]() -> int {
    return cluster_entry(h, centroid_labels, centroid_vectors, m, false, 1, where, assign_attr, nullptr, out_rows, out_cost,
                         nullptr, nullptr, matched);
    });
}

int mlvdb_kmeans(mlvdb_index* h, const int64_t* centroid_labels, const float* centroid_vectors, int32_t m,
                 int32_t max_iterations, const mlvdb_where* where, int32_t assign_attr, float* out_centroids,
                 int64_t* out_rows, double* out_cost, int32_t* iterations, int32_t* converged, int64_t* matched) {
    return guarded(h, kOnDevice, [&]() -> int {
    return cluster_entry(h, centroid_labels, centroid_vectors, m, true, max_iterations, where, assign_attr, out_centroids,
                         out_rows, out_cost, iterations, converged, matched);
    });
}

}  // extern "C"
