// Per-query metadata filters (include/mlvdb_where_each.h): every program of a call evaluated in one pass over the attribute
// columns into one 64-bit word per row, the ascending label lists of the programs routed to the gathered kernel, and that
// kernel -- exact fp64 distances of just the matching rows, by the gathered walk (gather_walk.h) -- and its range sibling (include/mlvdb_where_each_range.h), which keeps every hit
// within the radius instead of the k nearest.  The programs reach these kernels validated (api.hip: where_prepare).
//
// Segments: the rows are cut into `nseg` contiguous runs of `seg_rows` rows (a multiple of 64), one wave each, in the same
// way by the evaluation and the scatter: counts per (program, segment), an exclusive scan per program, and the scatter writes
// each segment's matches in row order -- the label lists come out ascending without any sort.
#include <algorithm>

#include "gather_walk.h"
#include "internal.h"
#include "where_common.h"

namespace mlvdb {

constexpr int kEachWaves = 4;  // waves (segments) per block of the evaluation and the scatter

// byte offset of the column values in the evaluation's LDS: behind the ops and the program offsets
__host__ __device__ static inline size_t each_eval_vals_offset(int32_t n_ops) {
    return ((size_t)n_ops * sizeof(WhereOp) + (kWhereEachMaxPrograms + 1) * sizeof(int32_t) + 15) / 16 * 16;
}

// bits[i] = bit p set <=> row i is live and matches program p; seg_cnt[p * nseg + seg] = matches of program p in segment seg.
// LDS (dynamic): all programs (<= 1024 ops, 32 KiB; prog_off[p] .. prog_off[p + 1] are program p's ops), then one value per
// thread of each of the `ncols` referenced columns.  A row's column values are loaded once, all at the same time, into the
// thread's own LDS slots, and every op of every program reads its column's slot (the high bits of op.type): the columns are
// read once per row, not once per op, and no op waits on a memory load.
__global__ __launch_bounds__(256) void where_each_eval_kernel(const WhereOp* __restrict__ prog,
                                                              const int32_t* __restrict__ prog_off, int32_t n_progs,
                                                              int32_t n_ops, const int64_t* __restrict__ set,
                                                              const int64_t* const* __restrict__ cols, int32_t ncols,
                                                              const float* __restrict__ rn, int64_t total, int64_t seg_rows,
                                                              int32_t nseg, unsigned long long* __restrict__ bits,
                                                              uint32_t* __restrict__ seg_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WhereOp* sp = reinterpret_cast<WhereOp*>(smem);                                   // [n_ops]
    int32_t* soff = reinterpret_cast<int32_t*>(smem + (size_t)n_ops * sizeof(WhereOp));  // [kWhereEachMaxPrograms + 1]
    int64_t* vals = reinterpret_cast<int64_t*>(smem + each_eval_vals_offset(n_ops));      // [ncols][256]
    for (int i = threadIdx.x; i < n_ops; i += blockDim.x) sp[i] = prog[i];
    if ((int)threadIdx.x <= n_progs) soff[threadIdx.x] = prog_off[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * kEachWaves + (threadIdx.x >> 6);
    if (seg >= nseg) return;  // wave-uniform; no block barrier follows
    const int64_t begin = (int64_t)seg * seg_rows;
    const int64_t end = std::min<int64_t>(total, begin + seg_rows);
    int64_t* mine = vals + threadIdx.x;  // this thread's slots, 256 values apart (only this thread touches them)
    uint32_t cnt = 0;                    // lane p: matches of program p in this segment
    for (int64_t i0 = begin; i0 < end; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool in = i < end;
        const bool live = in && rn[i] == rn[i];  // tombstoned rows (NaN norm) match nothing
        for (int c = 0; c < ncols; ++c) mine[c * 256] = in ? cols[c][i] : INT64_MIN;
        auto load = [&](const WhereOp& o) { return mine[(o.type >> 8) * 256]; };
        unsigned long long word = 0;
        for (int p = 0; p < n_progs; ++p) {
            const bool m = where_eval_with(sp + soff[p], soff[p + 1] - soff[p], set, load);
            if (live && m) word |= 1ull << p;
        }
        if (in) bits[i] = word;
        for (int p = 0; p < n_progs; ++p) {
            const uint32_t c = (uint32_t)__popcll(__ballot((word >> p) & 1ull));
            if (lane == p) cnt += c;
        }
    }
    if (lane < n_progs) seg_cnt[(int64_t)lane * nseg + seg] = cnt;
}

hipError_t launch_where_each_eval(const WhereOp* prog, const int32_t* prog_off, int32_t n_progs, int32_t n_ops,
                                  const int64_t* set, const int64_t* const* cols, int32_t ncols, const float* rn, int64_t total,
                                  int64_t seg_rows, int32_t nseg, unsigned long long* bits, uint32_t* seg_cnt, hipStream_t s) {
    if (total <= 0 || nseg <= 0) return hipSuccess;
    if (n_ops > kWhereEachMaxOps || n_progs > kWhereEachMaxPrograms || ncols > MLVDB_MAX_ATTRS) return hipErrorInvalidValue;
    const size_t lds = each_eval_vals_offset(n_ops) + (size_t)ncols * 256 * sizeof(int64_t);
    // configured once, for the largest call (kWhereEachMaxOps ops over MLVDB_MAX_ATTRS columns: 65,808 B): the attribute
    // holds for the rest of the process, so it must cover every size a later call may launch with
    static std::atomic<uint64_t> lds_set{0};
    const size_t lds_max = each_eval_vals_offset(kWhereEachMaxOps) + (size_t)MLVDB_MAX_ATTRS * 256 * sizeof(int64_t);
    if (lds > 48 * 1024) {
        hipError_t e = ensure_dynamic_lds(lds_set, reinterpret_cast<const void*>(where_each_eval_kernel), (int)lds_max);
        if (e != hipSuccess) return e;
    }
    where_each_eval_kernel<<<(unsigned)((nseg + kEachWaves - 1) / kEachWaves), kEachWaves * 64, lds, s>>>(
        prog, prog_off, n_progs, n_ops, set, cols, ncols, rn, total, seg_rows, nseg, bits, seg_cnt);
    return hipGetLastError();
}

// One block per program: seg_cnt[p][*] -> its exclusive prefix sums (in place), totals[p] = the program's matches.
__global__ __launch_bounds__(256) void where_each_scan_kernel(uint32_t* __restrict__ seg_cnt, int32_t nseg,
                                                              int64_t* __restrict__ totals) {
    __shared__ uint32_t part[256];
    uint32_t* c = seg_cnt + (int64_t)blockIdx.x * nseg;
    const int per = (nseg + 255) / 256;
    const int b = threadIdx.x * per, e = std::min(nseg, b + per);
    uint32_t sum = 0;
    for (int i = b; i < e; ++i) sum += c[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {  // 256 partial sums, serially
        uint32_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const uint32_t v = part[t];
            part[t] = run;
            run += v;
        }
        totals[blockIdx.x] = (int64_t)run;
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (int i = b; i < e; ++i) {
        const uint32_t v = c[i];
        c[i] = run;
        run += v;
    }
}

hipError_t launch_where_each_scan(uint32_t* seg_cnt, int32_t n_progs, int32_t nseg, int64_t* totals, hipStream_t s) {
    if (n_progs <= 0 || nseg <= 0) return hipSuccess;
    where_each_scan_kernel<<<(unsigned)n_progs, 256, 0, s>>>(seg_cnt, nseg, totals);
    return hipGetLastError();
}

// Label lists of the programs in `gmask`: labels[base[p] + rank of row i among program p's matches] = i, ascending.
// seg_off: the exclusive prefix sums of where_each_scan_kernel.  Every segment walks its rows again in the same order.
__global__ __launch_bounds__(256) void where_each_scatter_kernel(const unsigned long long* __restrict__ bits, int64_t total,
                                                                 int64_t seg_rows, int32_t nseg, int32_t n_progs,
                                                                 const uint32_t* __restrict__ seg_off,
                                                                 unsigned long long gmask, const int64_t* __restrict__ base,
                                                                 int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * kEachWaves + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const int64_t begin = (int64_t)seg * seg_rows;
    const int64_t end = std::min<int64_t>(total, begin + seg_rows);
    const bool mine = lane < n_progs && ((gmask >> lane) & 1ull);
    // lane p: where this segment's next match of program p goes (labels are < 2^31: the panels address rows as int32)
    int32_t next = mine ? (int32_t)(base[lane] + seg_off[(int64_t)lane * nseg + seg]) : 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t i0 = begin; i0 < end; i0 += 64) {
        const int64_t i = i0 + lane;
        const unsigned long long word = i < end ? bits[i] & gmask : 0ull;
        unsigned long long any = word;  // the programs some row of this step matches (wave-wide OR)
        for (int off = 32; off > 0; off >>= 1) any |= __shfl_xor(any, off);
        while (any) {
            const int p = __builtin_ctzll(any);
            any &= any - 1;
            const bool hit = (word >> p) & 1ull;
            const unsigned long long b = __ballot(hit);
            const int32_t at = __shfl(next, p);
            if (hit) labels[at + __popcll(b & below)] = (int32_t)i;
            if (lane == p) next += __popcll(b);
        }
    }
}

hipError_t launch_where_each_scatter(const unsigned long long* bits, int64_t total, int64_t seg_rows, int32_t nseg,
                                     int32_t n_progs, const uint32_t* seg_off, unsigned long long gmask, const int64_t* base,
                                     int32_t* labels, hipStream_t s) {
    if (total <= 0 || nseg <= 0 || gmask == 0) return hipSuccess;
    where_each_scatter_kernel<<<(unsigned)((nseg + kEachWaves - 1) / kEachWaves), kEachWaves * 64, 0, s>>>(
        bits, total, seg_rows, nseg, n_progs, seg_off, gmask, base, labels);
    return hipGetLastError();
}

// mask[i] = bit p of bits[i]: one program's row mask for the masked scan
__global__ __launch_bounds__(256) void where_each_expand_kernel(const unsigned long long* __restrict__ bits, int32_t p,
                                                                int64_t total, uint8_t* __restrict__ mask) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = (uint8_t)((bits[i] >> p) & 1ull);
}

hipError_t launch_where_each_expand(const unsigned long long* bits, int32_t p, int64_t total, uint8_t* mask, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    where_each_expand_kernel<<<(unsigned)blocks, 256, 0, s>>>(bits, p, total, mask);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the gathered exact top-k
// Block (tile, chunk): the tile's <= QT queries (one program, positions sel0.. of the call's sorted query list, prepared
// in Qpad / qaux at those positions) against chunk `blockIdx.y` of the program's label list, by the gathered walk
// (gather_walk.h).  The sink keeps one WaveTopK per query; the block's lists are merged through LDS into
// partial[(sel * nchunk + chunk) * k ..] (TopEntry), the input of exact_merge_kernel.  Every label is a live row of
// [0, total) (the scatter above wrote only those).
template <int SPACE, int QT>
__global__ __launch_bounds__(256) void where_gather_kernel(const float* __restrict__ X, const float* __restrict__ Qpad,
                                                           const double* __restrict__ qaux, const int32_t* __restrict__ labels,
                                                           const GatherTile* __restrict__ tiles, int32_t ld, int32_t k,
                                                           int32_t nchunk, TopEntry* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    const GatherTile tile = tiles[blockIdx.x];
    int qid[QT];
    double qinv[QT];
    WaveTopK top[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        qid[t] = t < tile.nsel ? tile.sel0 + t : -1;
        top[t].init();
    }
    gather_stage_queries<QT>(qs, Qpad, qaux, qid, ld, qinv);
    const int64_t per = ((int64_t)tile.lab_count + nchunk - 1) / nchunk;
    const int64_t begin = tile.lab_begin + per * blockIdx.y;
    const int64_t end = std::min<int64_t>((int64_t)tile.lab_begin + tile.lab_count, begin + per);
    gather_walk<SPACE, QT>(X, labels, begin, end, qs, ld, qinv, [&](int t, bool have, double dist, int32_t row) {
        top[t].offer(have && qid[t] >= 0, dist, row, k, lane);
    });
    gather_block_merge<QT>(smem, top, qid, k, [&](int t) { return partial + ((int64_t)qid[t] * nchunk + blockIdx.y) * k; });
}

size_t where_gather_lds(int32_t qt, int32_t ld) {
    const size_t q_bytes = (size_t)qt * ld * sizeof(double);
    const size_t m_bytes = (size_t)4 * qt * 64 * (sizeof(double) + sizeof(int32_t));
    return std::max(q_bytes, m_bytes);
}

// (the instances are configured for the largest tile any ld may ask for, 64 KiB: the limit checked here)
hipError_t launch_where_gather(const float* X, const float* Qpad, const double* qaux, const int32_t* labels,
                               const GatherTile* tiles, int32_t ntiles, int32_t ld, int32_t space, int32_t qt, int32_t k,
                               int32_t nchunk, TopEntry* partial, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (k < 1 || k > kWave || nchunk < 1 || where_gather_lds(qt, ld) > 64 * 1024) return hipErrorInvalidValue;
    return with_space_qt(space, qt, [&](auto sp, auto q) {
        constexpr int SPACE = decltype(sp)::value, QT = decltype(q)::value;
        const size_t lds = where_gather_lds(QT, ld);
        if (hipError_t e = ensure_instance_lds<where_gather_kernel<SPACE, QT>>(lds, 64 * 1024)) return e;
        where_gather_kernel<SPACE, QT><<<dim3((unsigned)ntiles, (unsigned)nchunk), 256, lds, s>>>(X, Qpad, qaux, labels, tiles, ld,
                                                                                                 k, nchunk, partial);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------ the gathered exact range
// The same walk; what differs is what a block keeps.  A range query has no k: every (query, matching row) pair is scored
// and every hit (fp64 distance <= radius; the labels are live matching rows already) is counted, so rhit_cnt[query] ends as
// the exact hit count whatever becomes of the list.  A step's hits of one query claim their slots together -- one atomicAdd
// by lane 0 for the ballot's popcount, a hit's own slot from the hits in the lanes below it -- and the first kCandCap of a
// query are stored {fp64 distance, label} in its hit array, the input of range_rank_kernel (kernels_filter.hip), exactly as
// range_score_flat_kernel leaves them.  A query with more hits than that is flagged by the ranking kernel and served by the
// masked range pass (api.hip).  Hits are a small share of the scored pairs, so most steps issue no atomic at all.
// Queries: positions tile.sel0.. of the call's sorted query list; their hit arrays are indexed from q_base (the 256-query
// group of the launch: the ranking kernel's workspace holds 256 lists).
template <int SPACE, int QT>
__global__ __launch_bounds__(256) void where_gather_range_kernel(const float* __restrict__ X, const float* __restrict__ Qpad,
                                                                 const double* __restrict__ qaux,
                                                                 const int32_t* __restrict__ labels,
                                                                 const GatherTile* __restrict__ tiles, int32_t ld,
                                                                 int32_t nchunk, double rad, int32_t q_base,
                                                                 RangeHit* __restrict__ rhits, uint32_t* __restrict__ rhit_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    const GatherTile tile = tiles[blockIdx.x];
    int qid[QT], qloc[QT];  // qloc: the query's list of this launch's workspace, or -1
    double qinv[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        qid[t] = t < tile.nsel ? tile.sel0 + t : -1;
        qloc[t] = qid[t] >= 0 ? qid[t] - q_base : -1;
    }
    gather_stage_queries<QT>(qs, Qpad, qaux, qid, ld, qinv);
    const int64_t per = ((int64_t)tile.lab_count + nchunk - 1) / nchunk;
    const int64_t begin = tile.lab_begin + per * blockIdx.y;
    const int64_t end = std::min<int64_t>((int64_t)tile.lab_begin + tile.lab_count, begin + per);
    const unsigned long long below = (1ull << lane) - 1ull;
    gather_walk<SPACE, QT>(X, labels, begin, end, qs, ld, qinv, [&](int t, bool have, double dist, int32_t row) {
        const bool hit = have && qloc[t] >= 0 && dist <= rad;
        const unsigned long long bal = __ballot(hit);
        if (bal) {  // wave-uniform
            uint32_t first = 0;
            if (lane == 0) first = atomicAdd(&rhit_cnt[qloc[t]], (uint32_t)__popcll(bal));
            first = __shfl(first, 0);
            const uint32_t slot = first + (uint32_t)__popcll(bal & below);
            if (hit && slot < (uint32_t)kCandCap) {  // beyond: counted only
                RangeHit h;
                h.d = dist;
                h.l = row;
                h.pad = 0;
                rhits[(int64_t)qloc[t] * kCandCap + slot] = h;
            }
        }
    });
}

hipError_t launch_where_gather_range(const float* X, const float* Qpad, const double* qaux, const int32_t* labels,
                                     const GatherTile* tiles, int32_t ntiles, int32_t ld, int32_t space, int32_t qt,
                                     int32_t nchunk, float radius, int32_t q_base, RangeHit* rhits, uint32_t* rhit_cnt,
                                     hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (nchunk < 1 || (qt != 1 && qt != 2 && qt != 4) || where_gather_lds(qt, ld) > 64 * 1024) return hipErrorInvalidValue;
    return with_space_qt(space, qt, [&](auto sp, auto q) {
        constexpr int SPACE = decltype(sp)::value, QT = decltype(q)::value;
        const size_t lds = (size_t)QT * ld * sizeof(double);  // (no block merge: the query tile alone)
        if (hipError_t e = ensure_instance_lds<where_gather_range_kernel<SPACE, QT>>(lds, 64 * 1024)) return e;
        where_gather_range_kernel<SPACE, QT><<<dim3((unsigned)ntiles, (unsigned)nchunk), 256, lds, s>>>(
            X, Qpad, qaux, labels, tiles, ld, nchunk, (double)radius, q_base, rhits, rhit_cnt);
        return hipGetLastError();
    });
}

}  // namespace mlvdb
