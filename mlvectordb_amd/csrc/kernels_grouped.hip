// Grouped kNN (include/mlvdb_grouped.h): the member stage behind the distinct stage.  For the group codes a chunk of queries
// picked, two passes over the attribute column list the live rows of every picked group (counts per code, then int32 labels
// into one CSR array), and the gathered kernel scores each list against exactly the (query, rank) pairs that picked its
// group, by the gathered walk (gather_walk.h).
//
// The codes sit in an open-addressing table the host built (facet_hash, linear probing, at most half full, INT64_MIN =
// empty): a row's slot is found by probing, never inserted.  The order of the rows inside a list depends on the order in
// which waves claim positions; nothing downstream depends on it, since every list entry is offered to a selection list whose
// order (fp64 distance, label) is total.
#include <algorithm>

#include "gather_walk.h"
#include "group_table.h"
#include "internal.h"
#include "wave_peel.h"

namespace mlvdb {

// counts[slot] += live rows of the slot's group.  Launch shape of where_eval_kernel: 256 threads, grid-stride, whole waves.
// Consecutive rows of one document share a code: the wave peel turns a wave of one document into one atomic.
__global__ __launch_bounds__(256) void grouped_count_kernel(const float* __restrict__ rn, const int64_t* __restrict__ col,
                                                            int64_t total, const long long* __restrict__ keys, uint64_t mask,
                                                            uint32_t* __restrict__ counts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // i0 is uniform over the block: every lane of a wave runs the same iterations (the peel's ballots need all of them)
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        const int32_t slot = grouped_row_slot(rn, col, i0 + threadIdx.x, total, keys, mask);
        wave_peel_add(slot >= 0, (int64_t)slot, [&](int64_t key, uint32_t n) { atomicAdd(&counts[key], n); });
    }
}

hipError_t launch_grouped_count(const float* rn, const int64_t* col, int64_t total, const long long* keys, uint64_t slots,
                                uint32_t* counts, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    grouped_count_kernel<<<(unsigned)blocks, 256, 0, s>>>(rn, col, total, keys, slots - 1, counts);
    return hipGetLastError();
}

// The same walk again: labels[position claimed from cursor[slot]] = row.  cursor[slot] enters as the slot's list begin (the
// exclusive prefix sum of the counts) and ends as its list end; the same rows are met as in the count (nothing mutates the
// index between the two), so every position claimed lies inside the slot's own list.  The peel claims the positions of all
// lanes of one code with one atomic; a lane's position is the claim plus the number of such lanes below it.
__global__ __launch_bounds__(256) void grouped_fill_kernel(const float* __restrict__ rn, const int64_t* __restrict__ col,
                                                           int64_t total, const long long* __restrict__ keys, uint64_t mask,
                                                           uint32_t* __restrict__ cursor, int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        const int32_t slot = grouped_row_slot(rn, col, i, total, keys, mask);
        bool has = slot >= 0;
        for (int r = 0; r < kFacetPeelRounds; ++r) {
            const unsigned long long active = __ballot(has);
            if (!active) break;
            const int leader = __ffsll((long long)active) - 1;
            const int32_t lead = __shfl(slot, leader);
            const bool same = has && slot == lead;
            const unsigned long long b = __ballot(same);
            const uint32_t n = (uint32_t)__popcll(b);
            uint32_t first = 0;
            if (lane == leader) first = atomicAdd(&cursor[lead], n);
            first = __shfl(first, leader);
            if (same) labels[first + (uint32_t)__popcll(b & below)] = (int32_t)i;
            has = has && !same;
            if (n == 1) break;
        }
        if (has) labels[atomicAdd(&cursor[slot], 1u)] = (int32_t)i;  // a column of many values: the lanes left claim one each
    }
}

hipError_t launch_grouped_fill(const float* rn, const int64_t* col, int64_t total, const long long* keys, uint64_t slots,
                               uint32_t* cursor, int32_t* labels, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    grouped_fill_kernel<<<(unsigned)blocks, 256, 0, s>>>(rn, col, total, keys, slots - 1, cursor, labels);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the gathered scoring of the member lists
// One block per tile: <= QT of the (query, rank) pairs that picked one group against one chunk of that group's label list,
// by the gathered walk (gather_walk.h).  The queries are staged from Qpad / qaux by the pairs' query index -- pairs of one
// query in different groups read the same prepared query, there is no per-pair copy.  The sink keeps one WaveTopK per pair
// with k = group_size; the block's lists are merged through LDS into the pair's partial list of this chunk,
// partial[(tile.part0 + t * tile.nch) * gsz ..].  Every label is a live row of [0, total) (the fill wrote only those).
template <int SPACE, int QT>
__global__ __launch_bounds__(256) void grouped_gather_kernel(const float* __restrict__ X, const float* __restrict__ Qpad,
                                                             const double* __restrict__ qaux,
                                                             const int32_t* __restrict__ labels,
                                                             const GroupedTile* __restrict__ tiles,
                                                             const GroupedPair* __restrict__ pairs, int32_t ld, int32_t gsz,
                                                             TopEntry* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    const GroupedTile tile = tiles[blockIdx.x];
    int qid[QT];
    double qinv[QT];
    WaveTopK top[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        qid[t] = t < tile.npairs ? pairs[tile.pair0 + t].q : -1;
        top[t].init();
    }
    gather_stage_queries<QT>(qs, Qpad, qaux, qid, ld, qinv);
    const int64_t begin = tile.lab_begin;
    gather_walk<SPACE, QT>(X, labels, begin, begin + tile.lab_count, qs, ld, qinv, [&](int t, bool have, double dist, int32_t row) {
        top[t].offer(have && qid[t] >= 0, dist, row, gsz, lane);
    });
    gather_block_merge<QT>(smem, top, qid, gsz, [&](int t) { return partial + ((int64_t)tile.part0 + (int64_t)t * tile.nch) * gsz; });
}

// (the instances are configured for the largest tile any ld may ask for, 64 KiB: the limit checked here)
hipError_t launch_grouped_gather(const float* X, const float* Qpad, const double* qaux, const int32_t* labels,
                                 const GroupedTile* tiles, int32_t ntiles, const GroupedPair* pairs, int32_t ld, int32_t space,
                                 int32_t qt, int32_t gsz, TopEntry* partial, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (gsz < 1 || gsz > kWave || (qt != 1 && qt != 2 && qt != 4) || where_gather_lds(qt, ld) > 64 * 1024)
        return hipErrorInvalidValue;
    return with_space_qt(space, qt, [&](auto sp, auto q) {
        constexpr int SPACE = decltype(sp)::value, QT = decltype(q)::value;
        const size_t lds = where_gather_lds(QT, ld);
        if (hipError_t e = ensure_instance_lds<grouped_gather_kernel<SPACE, QT>>(lds, 64 * 1024)) return e;
        grouped_gather_kernel<SPACE, QT><<<(unsigned)ntiles, 256, lds, s>>>(X, Qpad, qaux, labels, tiles, pairs, ld, gsz, partial);
        return hipGetLastError();
    });
}

// The twin of exact_merge_kernel that writes to [slot, 0 .. gsz): one wave per (query, rank) slot of the chunk, four per
// block.  A slot no pair fills (beyond the query's group count) is padded; the others fold their pair's nch partial lists
// (contiguous: nch * gsz entries) and write the group's members, its padded tail and its member count.
__global__ __launch_bounds__(256) void grouped_merge_kernel(const TopEntry* __restrict__ partial,
                                                            const GroupedPair* __restrict__ pairs,
                                                            const int32_t* __restrict__ pair_of_slot, int32_t nslots,
                                                            int32_t gsz, int64_t* __restrict__ out_labels,
                                                            float* __restrict__ out_dist, double* __restrict__ out_d64,
                                                            int32_t* __restrict__ out_gcnt) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= nslots) return;  // (wave-uniform; no block barrier follows)
    const int32_t p = pair_of_slot[slot];
    WaveTopK m;
    m.init();
    if (p >= 0) {
        const GroupedPair pr = pairs[p];
        const TopEntry* src = partial + (int64_t)pr.part0 * gsz;
        const int64_t n = (int64_t)pr.nch * gsz;
        for (int64_t i0 = 0; i0 < n; i0 += 64) {
            const int64_t i = i0 + lane;
            TopEntry e;
            e.d = __builtin_inf();
            e.l = kNoLabel;
            if (i < n) e = src[i];
            m.offer(e.l != kNoLabel, e.d, e.l, gsz, lane);
        }
    }
    const bool valid = lane < gsz && m.l != kNoLabel;
    if (lane < gsz) {
        const int64_t at = (int64_t)slot * gsz + lane;
        out_labels[at] = valid ? (int64_t)m.l : -1;
        out_dist[at] = valid ? (float)m.d : __builtin_inff();
        out_d64[at] = valid ? m.d : __builtin_inf();
    }
    const int cnt = __popcll(__ballot(valid));
    if (lane == 0) out_gcnt[slot] = cnt;
}

hipError_t launch_grouped_merge(const TopEntry* partial, const GroupedPair* pairs, const int32_t* pair_of_slot, int32_t nslots,
                                int32_t gsz, int64_t* out_labels, float* out_dist, double* out_d64, int32_t* out_gcnt,
                                hipStream_t s) {
    if (nslots <= 0) return hipSuccess;
    if (gsz < 1 || gsz > kWave) return hipErrorInvalidValue;
    grouped_merge_kernel<<<(unsigned)((nslots + 3) / 4), 256, 0, s>>>(partial, pairs, pair_of_slot, nslots, gsz, out_labels,
                                                                      out_dist, out_d64, out_gcnt);
    return hipGetLastError();
}

}  // namespace mlvdb
