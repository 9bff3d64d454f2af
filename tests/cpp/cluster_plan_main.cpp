// csrc/cluster_plan.h on the host, meant to run under AddressSanitizer and UBSan: every refusal of cluster_check on
// exactly-sized heap arrays (a read past an array is a report), the tile cut for every m and row width, and the segment
// table for count vectors around the segment size -- every member in exactly one segment, in order, no segment longer
// than MLVDB_CLUSTER_SEGMENT, none empty, only a cluster's last one shorter.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "cluster_plan.h"

using namespace mlvdb;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

namespace {
struct Call {
    std::vector<int64_t> labels = {1, -1, 2};
    std::vector<float> vectors = std::vector<float>(9, 1.0f);
    bool no_labels = false, no_vectors = false;
    int32_t m = 3;
    int64_t total = 10;
    int32_t dim = 3;
    int32_t space = MLVDB_SPACE_L2;
    int32_t attr = 0, attr_type = MLVDB_ATTR_INT64;
    bool kmeans = false, kmeans_out = true;
    int32_t max_iterations = 5;
    int null_out = -1;

    int run() const {
        // exactly-sized copies on the heap: the sanitizer sees any read past them
        std::unique_ptr<int64_t[]> l(new int64_t[labels.size()]);
        std::unique_ptr<float[]> v(new float[vectors.size()]);
        std::copy(labels.begin(), labels.end(), l.get());
        std::copy(vectors.begin(), vectors.end(), v.get());
        int dummy = 0;
        const void* outs[3] = {&dummy, &dummy, &dummy};
        if (null_out >= 0) outs[null_out] = nullptr;
        return cluster_check(no_labels ? nullptr : l.get(), no_vectors ? nullptr : v.get(), m, total, dim, space, attr, attr_type,
                             outs[0], outs[1], outs[2], kmeans, max_iterations, kmeans_out)
            .code;
    }
};

void check_refusals() {
    const int OK = MLVDB_OK, INVALID = MLVDB_ERR_INVALID_ARG, UNSUPPORTED = MLVDB_ERR_UNSUPPORTED;
    Call c;
    CHECK(c.run() == OK);
    c.kmeans = true;
    CHECK(c.run() == OK);
    {  // all raw, no labels at all; all stored, no vectors at all
        Call a;
        a.no_labels = true;
        CHECK(a.run() == OK);
        Call b;
        b.labels = {0, 9, 9};
        b.no_vectors = true;
        b.vectors.clear();
        CHECK(b.run() == OK);
        Call n;
        n.no_labels = n.no_vectors = true;
        CHECK(n.run() == INVALID);
    }
    for (int32_t m : {0, -1, kClusterMax + 1}) {
        Call a;
        a.m = m;
        CHECK(a.run() == INVALID);
    }
    {
        Call a;
        a.m = kClusterMax;
        a.labels.assign(kClusterMax, 3);
        a.no_vectors = true;
        CHECK(a.run() == OK);
    }
    for (int64_t bad : {(int64_t)-2, (int64_t)10, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
        Call a;
        a.labels[2] = bad;
        CHECK(a.run() == INVALID);
    }
    {
        Call a;
        a.no_vectors = true;  // label 1 is raw
        CHECK(a.run() == INVALID);
        Call e;
        e.total = 0;  // an empty index: no stored label is valid
        CHECK(e.run() == INVALID);
        e.labels = {-1, -1, -1};
        CHECK(e.run() == OK);
    }
    for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                      std::numeric_limits<float>::quiet_NaN()}) {
        Call a;
        a.vectors[3 + 2] = bad;  // the raw centroid's row
        CHECK(a.run() == INVALID);
        Call b;
        b.vectors[0] = bad;  // the row of a stored centroid is never read
        CHECK(b.run() == OK);
        b.no_labels = true;
        CHECK(b.run() == INVALID);
    }
    {
        Call a;
        a.attr = -1;
        a.attr_type = 0;
        CHECK(a.run() == OK);
        for (int32_t attr : {-2, MLVDB_MAX_ATTRS, 1 << 30}) {
            a.attr = attr;
            CHECK(a.run() == INVALID);
        }
        Call u;
        u.attr_type = 0;  // not defined
        CHECK(u.run() == INVALID);
        for (int32_t type : {MLVDB_ATTR_FLOAT64, 3, 4, 5, 6}) {
            u.attr_type = type;
            CHECK(u.run() == INVALID);
        }
    }
    for (int i = 0; i < 3; ++i) {
        Call a;
        a.null_out = i;
        CHECK(a.run() == INVALID);
    }
    {
        Call a;
        a.kmeans = true;
        a.kmeans_out = false;
        CHECK(a.run() == INVALID);
        a.kmeans = false;  // the assignment has no such outputs
        CHECK(a.run() == OK);
        Call b;
        b.kmeans = true;
        for (int32_t it : {0, -1}) {
            b.max_iterations = it;
            CHECK(b.run() == INVALID);
        }
        b.max_iterations = MLVDB_CLUSTER_MAX_ITERATIONS;
        CHECK(b.run() == OK);
        b.max_iterations = MLVDB_CLUSTER_MAX_ITERATIONS + 1;
        CHECK(b.run() == UNSUPPORTED);
        Call ip;
        ip.space = MLVDB_SPACE_IP;
        CHECK(ip.run() == OK);
        ip.kmeans = true;
        CHECK(ip.run() == UNSUPPORTED);
        ip.space = MLVDB_SPACE_COSINE;
        CHECK(ip.run() == OK);
    }
}

void check_tiles() {
    for (int32_t ld : {16, 768, 1024, 1040, 2048, 2064, 4096, 4112, 8192})
        for (int32_t m = 1; m <= kClusterMax; ++m) {
            const int32_t qt = cluster_tile_width(ld, m);
            CHECK(qt == 1 || qt == 2 || qt == 4 || qt == 8);
            CHECK(qt <= kClusterMaxTile && (size_t)qt * ld * sizeof(double) <= 64 * 1024);
            CHECK(qt == 1 || qt / 2 < m);  // no wider than m needs
            CHECK(qt == 8 || m <= qt || (size_t)(2 * qt) * ld * sizeof(double) > 64 * 1024);  // no narrower than LDS allows
            const int32_t nt = cluster_tile_count(m, qt);
            CHECK((int64_t)(nt - 1) * qt < m && (int64_t)nt * qt >= m);
        }
}

void check_segments() {
    std::vector<ClusterSegment> segs;
    std::vector<int32_t> first;
    const int64_t S = kClusterSegment;
    const std::vector<std::vector<int64_t>> cases = {
        {0}, {1}, {S - 1}, {S}, {S + 1}, {2 * S}, {2 * S + 1}, {0, 0, 0}, {0, S, 0, 1, 3 * S + 7, 0}, {5, 0, S, S + 1, 0, 2 * S - 1},
        std::vector<int64_t>(kClusterMax, 1), std::vector<int64_t>(kClusterMax, 0), {100000, 3, 0, 70001}};
    for (const auto& counts : cases) {
        std::unique_ptr<int64_t[]> c(new int64_t[counts.size()]);
        std::copy(counts.begin(), counts.end(), c.get());
        const int32_t m = (int32_t)counts.size();
        const int64_t listed = cluster_segments(c.get(), m, segs, first);
        int64_t sum = 0;
        for (int64_t v : counts) sum += v;
        CHECK(listed == sum);
        CHECK((int32_t)first.size() == m + 1 && first[0] == 0 && first[(size_t)m] == (int32_t)segs.size());
        CHECK((int64_t)segs.size() <= cluster_max_segments(sum, m));
        int64_t at = 0;
        for (int32_t j = 0; j < m; ++j) {
            CHECK(first[(size_t)j + 1] - first[(size_t)j] == (counts[(size_t)j] + S - 1) / S);
            int64_t left = counts[(size_t)j];
            for (int32_t g = first[(size_t)j]; g < first[(size_t)j + 1]; ++g) {
                const ClusterSegment& s = segs[(size_t)g];
                CHECK(s.cluster == j && s.begin == at && s.count >= 1 && s.count <= S);
                CHECK(s.count == S || g == first[(size_t)j + 1] - 1);
                at += s.count;
                left -= s.count;
            }
            CHECK(left == 0);
        }
        CHECK(at == sum);
    }
    CHECK(cluster_list_blocks(0) == 0 && cluster_list_blocks(1) == 1 && cluster_list_blocks(kClusterListRows) == 1 &&
          cluster_list_blocks(kClusterListRows + 1) == 2);
    // the header's formula: 20 bytes per row (28 with the cosine weights) and the terms that do not grow with the rows' width
    const size_t n = 1 << 20;
    CHECK(cluster_workspace_bytes(n, 0, 1, 16, 16, false) >= 20 * n && cluster_workspace_bytes(n, 0, 1, 16, 16, false) < 21 * n);
    CHECK(cluster_workspace_bytes(n, 0, 1, 16, 16, true) - cluster_workspace_bytes(n, 0, 1, 16, 16, false) == 8 * n);
}
}  // namespace

int main() {
    check_refusals();
    check_tiles();
    check_segments();
    std::printf("cluster_plan ok\n");
    return 0;
}
