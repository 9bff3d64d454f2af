// Recommend / discover (include/mlvdb_examples.h), the host side that needs no device: the argument check of the entry and
// the cut of a query's bag of examples into the tiles the scan walks.  Plain C++ -- api.hip includes it, and so does the
// stand-alone program that runs it under the sanitizers (tests/cpp/examples_plan_main.cpp).
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/mlvdb_examples.h"
#include "../../include/mlvdb_hip.h"

namespace mlvdb {

constexpr int kExamplesMax = MLVDB_EXAMPLES_MAX;
constexpr int kExamplesMaxTile = 8;  // the widest tile of the exact scan's geometry

// What a slot of a tile does with its distance (4 bits per slot in ExamplesTile::roles)
enum : uint32_t {
    kExEmpty = 0,
    kExPosMin = 1,    // BEST, POS:  a = min(a, d)
    kExNegMin = 2,    // BEST, NEG:  b = min(b, d)
    kExTarget = 3,    // DISCOVER:   a = d
    kExPairPos = 4,   // the POS of a pair: held for the slot behind it
    kExNegCount = 5,  // DISCOVER, the NEG of a pair: b = b + (held < d ? 0 : 1)
    kExNegSum = 6,    // CONTEXT, the NEG of a pair:  a = a + (held > d ? held - d : 0.0)
};
// ExamplesTile::flags
enum : uint32_t { kExFirst = 1, kExLast = 2, kExModeShift = 2, kExHasPos = 16, kExHasNeg = 32 };

// One tile of one query: what a block row (blockIdx.y) of one scan launch works on.
struct ExamplesTile {
    int32_t query;  // the query inside the chunk
    int32_t state;  // its slot in the chunk's state workspace, -1: the bag is this one tile
    uint32_t roles;
    uint32_t flags;
    int32_t ex[kExamplesMaxTile];  // the staged example of every slot, -1: none
    int32_t excl_off, n_excl;      // the query's stored example labels in the chunk's exclusion table (n_excl = 0: keep all)
    int32_t pad[2];
};
static_assert(sizeof(ExamplesTile) == 64, "read as four 16-byte words");

struct ExamplesRefusal {
    int code;  // MLVDB_OK or the status
    const char* what;
};

// Everything the entry refuses that depends on its arguments alone (the program is where_run's).
inline ExamplesRefusal examples_check(int32_t mode, const int64_t* labels, const float* vectors, const int32_t* roles,
                                      const int64_t* offsets, int64_t nq, int32_t k, int32_t max_k, int64_t total, int32_t dim,
                                      const void* out_labels, const void* out_tier, const void* out_value,
                                      const void* out_counts) {
    if (nq < 0 || nq > (1 << 24)) return {MLVDB_ERR_INVALID_ARG, "nq out of range"};
    if (k < 1) return {MLVDB_ERR_INVALID_ARG, "k must be >= 1"};
    if (k > max_k) return {MLVDB_ERR_UNSUPPORTED, "examples: k above MLVDB_MAX_TOPK"};
    if (mode != MLVDB_EXAMPLES_BEST && mode != MLVDB_EXAMPLES_DISCOVER && mode != MLVDB_EXAMPLES_CONTEXT)
        return {MLVDB_ERR_INVALID_ARG, "examples: unknown mode"};
    if (nq == 0) return {MLVDB_OK, ""};
    if (!offsets || !labels || !roles || !out_labels || !out_tier || !out_value || !out_counts)
        return {MLVDB_ERR_INVALID_ARG, "null buffer"};
    if (offsets[0] != 0) return {MLVDB_ERR_INVALID_ARG, "examples: example_offsets must start at 0"};
    for (int64_t i = 0; i < nq; ++i) {
        if (offsets[i + 1] < offsets[i]) return {MLVDB_ERR_INVALID_ARG, "examples: example_offsets must ascend"};
        if (offsets[i + 1] == offsets[i]) return {MLVDB_ERR_INVALID_ARG, "examples: a query without examples"};
        if (offsets[i + 1] - offsets[i] > kExamplesMax)
            return {MLVDB_ERR_UNSUPPORTED, "examples: more than MLVDB_EXAMPLES_MAX examples in a query"};
    }
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t e0 = offsets[i], m = offsets[i + 1] - e0;
        for (int64_t j = e0; j < e0 + m; ++j) {
            if (labels[j] < -1 || labels[j] >= total) return {MLVDB_ERR_INVALID_ARG, "examples: example label outside [-1, total)"};
            if (labels[j] == -1 && !vectors) return {MLVDB_ERR_INVALID_ARG, "examples: a raw example without example_vectors"};
        }
        const int32_t* r = roles + e0;
        bool ok = true;
        if (mode == MLVDB_EXAMPLES_BEST) {
            for (int64_t j = 0; j < m; ++j) ok = ok && (r[j] == MLVDB_EXAMPLE_POS || r[j] == MLVDB_EXAMPLE_NEG);
        } else {
            const int64_t head = mode == MLVDB_EXAMPLES_DISCOVER ? 1 : 0;
            ok = (m - head) % 2 == 0 && (head == 0 ? m >= 2 : r[0] == MLVDB_EXAMPLE_TARGET);
            for (int64_t j = head; ok && j < m; ++j)
                ok = r[j] == ((j - head) % 2 == 0 ? MLVDB_EXAMPLE_POS : MLVDB_EXAMPLE_NEG);
        }
        if (!ok) return {MLVDB_ERR_INVALID_ARG, "examples: the roles of a query do not fit the mode"};
    }
    for (int64_t j = 0; j < offsets[nq]; ++j) {
        if (labels[j] != -1) continue;
        const float* v = vectors + (size_t)j * dim;
        for (int32_t c = 0; c < dim; ++c)
            if (!std::isfinite(v[c])) return {MLVDB_ERR_INVALID_ARG, "examples: a raw example holds a non-finite value"};
    }
    return {MLVDB_OK, ""};
}

// The tiles of one validated query, appended to `out` in walk order: its m examples (roles r[0 .. m), staged at first ..
// first + m - 1) packed in the order given into tiles of qt slots, a pair never split between two -- except with qt = 1,
// where the scan carries the held POS distance beside the state.  `query`, `state`, the exclusion range and the first /
// last flags are filled in; returns the number of tiles.
inline int examples_cut(int32_t mode, const int32_t* r, int32_t m, int32_t qt, int32_t first, int32_t query, int32_t excl_off,
                        int32_t n_excl, std::vector<ExamplesTile>& out) {
    const size_t begin = out.size();
    uint32_t common = (uint32_t)mode << kExModeShift;
    for (int32_t j = 0; j < m; ++j)
        if (mode == MLVDB_EXAMPLES_BEST) common |= r[j] == MLVDB_EXAMPLE_POS ? kExHasPos : kExHasNeg;
    int used = qt;  // slots used in the open tile (none open yet)
    for (int32_t j = 0; j < m;) {
        const bool pair = mode != MLVDB_EXAMPLES_BEST && r[j] != MLVDB_EXAMPLE_TARGET;
        const int unit = pair && qt >= 2 ? 2 : 1;
        if (used + unit > qt) {
            ExamplesTile t{};
            t.query = query;
            t.state = -1;
            t.flags = common;
            for (int& e : t.ex) e = -1;
            t.excl_off = excl_off;
            t.n_excl = n_excl;
            out.push_back(t);
            used = 0;
        }
        ExamplesTile& t = out.back();
        for (int u = 0; u < unit; ++u, ++j, ++used) {
            uint32_t role;
            if (mode == MLVDB_EXAMPLES_BEST) role = r[j] == MLVDB_EXAMPLE_POS ? kExPosMin : kExNegMin;
            else if (!pair) role = kExTarget;
            else if (r[j] == MLVDB_EXAMPLE_POS) role = kExPairPos;
            else role = mode == MLVDB_EXAMPLES_DISCOVER ? kExNegCount : kExNegSum;
            t.ex[used] = first + j;
            t.roles |= role << (4 * used);
        }
    }
    out[begin].flags |= kExFirst;
    out.back().flags |= kExLast;
    return (int)(out.size() - begin);
}

}  // namespace mlvdb
