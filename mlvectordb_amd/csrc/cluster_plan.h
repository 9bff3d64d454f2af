// Clustering (include/mlvdb_cluster.h), the host side that needs no device: the argument check of the two entries, the cut
// of the m centroids into the tiles the assignment scan walks, the segment table of the blocked sums from the per-cluster
// member counts, and the sizes of the workspace.  Plain C++ -- api.hip includes it, and so does the stand-alone program that
// runs it under the sanitizers (tests/cpp/cluster_plan_main.cpp).
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/mlvdb_cluster.h"
#include "../../include/mlvdb_hip.h"

namespace mlvdb {

constexpr int kClusterMax = MLVDB_CLUSTER_MAX;
constexpr int kClusterSegment = MLVDB_CLUSTER_SEGMENT;
constexpr int kClusterMaxTile = 8;         // the widest tile of the exact scan's geometry
constexpr int64_t kClusterListRows = 4096;  // rows of one listing block: one histogram of m counters each

struct ClusterRefusal {
    int code;  // MLVDB_OK or the status
    const char* what;
};

// Everything the two entries refuse that depends on their arguments alone (the program is where_run's).  attr_type: the
// type of column assign_attr as the handle knows it, 0 for an undefined one (unused with assign_attr == -1).
// kmeans: mlvdb_kmeans' extra arguments are checked too (out_centroids, iterations, converged as `kmeans_out`).
inline ClusterRefusal cluster_check(const int64_t* labels, const float* vectors, int32_t m, int64_t total, int32_t dim,
                                    int32_t space, int32_t assign_attr, int32_t attr_type, const void* out_rows,
                                    const void* out_cost, const void* matched, bool kmeans, int32_t max_iterations,
                                    bool kmeans_out) {
    if (m < 1 || m > kClusterMax) return {MLVDB_ERR_INVALID_ARG, "cluster: m outside 1..MLVDB_CLUSTER_MAX"};
    if (!out_rows || !out_cost || !matched || (kmeans && !kmeans_out)) return {MLVDB_ERR_INVALID_ARG, "null buffer"};
    if (kmeans) {
        if (max_iterations < 1) return {MLVDB_ERR_INVALID_ARG, "cluster: max_iterations must be >= 1"};
        if (max_iterations > MLVDB_CLUSTER_MAX_ITERATIONS)
            return {MLVDB_ERR_UNSUPPORTED, "cluster: max_iterations above MLVDB_CLUSTER_MAX_ITERATIONS"};
        if (space == MLVDB_SPACE_IP) return {MLVDB_ERR_UNSUPPORTED, "cluster: k-means needs l2 or cosine (no mean minimises ip)"};
    }
    if (assign_attr != -1) {
        if (assign_attr < 0 || assign_attr >= MLVDB_MAX_ATTRS) return {MLVDB_ERR_INVALID_ARG, "attribute index out of range"};
        if (attr_type == 0) return {MLVDB_ERR_INVALID_ARG, "attribute not defined"};
        if (attr_type != MLVDB_ATTR_INT64) return {MLVDB_ERR_INVALID_ARG, "cluster: assign_attr must be an int64 column"};
    }
    if (!labels && !vectors) return {MLVDB_ERR_INVALID_ARG, "cluster: neither centroid_labels nor centroid_vectors"};
    for (int32_t j = 0; labels && j < m; ++j) {
        if (labels[j] < -1 || labels[j] >= total) return {MLVDB_ERR_INVALID_ARG, "cluster: centroid label outside [-1, total)"};
        if (labels[j] == -1 && !vectors) return {MLVDB_ERR_INVALID_ARG, "cluster: a raw centroid without centroid_vectors"};
    }
    for (int32_t j = 0; j < m; ++j) {
        if (labels && labels[j] != -1) continue;
        const float* v = vectors + (size_t)j * dim;
        for (int32_t c = 0; c < dim; ++c)
            if (!std::isfinite(v[c])) return {MLVDB_ERR_INVALID_ARG, "cluster: a raw centroid holds a non-finite value"};
    }
    return {MLVDB_OK, ""};
}

// The tile width for m centroids of ld columns: the smallest of 1, 2, 4, 8 that holds them (8 beyond) -- examples_tile_width's
// rule, not plan_exact's, which takes the largest width not above its batch -- halved like plan_exact's until the fp64 image
// of a tile fits 64 KiB.  plan_assign then asks plan_exact for a batch of exactly that many queries, for which the two rules
// agree; the entry checks that they did.  The assignment does not depend on the width.
inline int32_t cluster_tile_width(int32_t ld, int32_t m) {
    int32_t qt = m > 4 ? 8 : m > 2 ? 4 : m > 1 ? 2 : 1;
    while (qt > 1 && (size_t)qt * ld * sizeof(double) > 64 * 1024) qt >>= 1;
    return qt;
}
// ... and the tiles of one assignment: tile i holds centroids [i qt, min(m, (i + 1) qt)), one scan launch each, ascending.
inline int32_t cluster_tile_count(int32_t m, int32_t qt) { return (m + qt - 1) / qt; }

// One segment of the blocked sum: `count` (1 .. kClusterSegment) members of `cluster` from `begin` of the member list.
struct ClusterSegment {
    int64_t begin;
    int32_t count;
    int32_t cluster;
};
static_assert(sizeof(ClusterSegment) == 16, "read as one 16-byte word");

// The segment table from the member counts: the list holds the members cluster by cluster (cluster j from base[j] =
// counts[0] + .. + counts[j - 1]), every cluster is cut into segments of kClusterSegment members, the last may be shorter;
// first[j] .. first[j + 1] - 1 are the segments of cluster j (none for an empty one).  Returns the members listed.
inline int64_t cluster_segments(const int64_t* counts, int32_t m, std::vector<ClusterSegment>& segs, std::vector<int32_t>& first) {
    segs.clear();
    first.assign(1, 0);
    int64_t base = 0;
    for (int32_t j = 0; j < m; ++j) {
        for (int64_t at = 0; at < counts[j]; at += kClusterSegment) {
            const int64_t left = counts[j] - at;
            segs.push_back({base + at, (int32_t)(left < kClusterSegment ? left : kClusterSegment), j});
        }
        base += counts[j];
        first.push_back((int32_t)segs.size());
    }
    return base;
}

// The most segments a call over `candidates` rows may need: sizes the segment sums before the counts are known.
inline int64_t cluster_max_segments(int64_t candidates, int32_t m) { return candidates / kClusterSegment + m; }

// Listing blocks over `total` rows, and the bytes of their [blocks][m] histogram.
inline int64_t cluster_list_blocks(int64_t total) { return (total + kClusterListRows - 1) / kClusterListRows; }

// The bytes one call takes on the device beside the index (the formula of include/mlvdb_cluster.h).
inline size_t cluster_workspace_bytes(int64_t total, int64_t candidates, int32_t m, int32_t dim, int32_t ld, bool weights) {
    size_t b = (size_t)total * (sizeof(double) + 3 * sizeof(int32_t));  // best, tile state, assignment, member list
    if (weights) b += (size_t)total * sizeof(double);
    b += (size_t)cluster_list_blocks(total) * m * sizeof(int32_t);
    b += (size_t)cluster_max_segments(candidates, m) * ((size_t)ld + 1) * sizeof(double);
    b += (size_t)m * ((size_t)dim + ld) * sizeof(float);
    return b;
}

}  // namespace mlvdb
