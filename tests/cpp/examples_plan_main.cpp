// csrc/examples_plan.h on the host, meant to run under AddressSanitizer and UBSan: every refusal of examples_check on
// exactly-sized heap arrays (a read past an array is a report), and examples_cut's tiles for every mode, bag size 1 .. 64
// and tile width -- every example in exactly one slot, in order, a pair split only by tiles of one slot, first / last flags
// on the ends.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "examples_plan.h"

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
    int32_t mode = MLVDB_EXAMPLES_BEST;
    std::vector<int64_t> labels, offsets;
    std::vector<int32_t> roles;
    std::vector<float> vectors;
    bool no_vectors = false;
    int64_t nq = 0;
    int32_t k = 5;
    int64_t total = 10;
    int32_t dim = 3;
    bool null_out = false;

    int run() const {
        // exactly-sized copies on the heap: the sanitizer sees any read past them
        std::unique_ptr<int64_t[]> l(new int64_t[labels.size()]), o(new int64_t[offsets.size()]);
        std::unique_ptr<int32_t[]> r(new int32_t[roles.size()]);
        std::unique_ptr<float[]> v(new float[vectors.size()]);
        std::copy(labels.begin(), labels.end(), l.get());
        std::copy(offsets.begin(), offsets.end(), o.get());
        std::copy(roles.begin(), roles.end(), r.get());
        std::copy(vectors.begin(), vectors.end(), v.get());
        int dummy = 0;
        const void* out = null_out ? nullptr : &dummy;
        return examples_check(mode, l.get(), no_vectors ? nullptr : v.get(), r.get(), o.get(), nq, k, 64, total, dim, out,
                              &dummy, &dummy, &dummy)
            .code;
    }
};

Call best(std::vector<int64_t> labels, std::vector<int32_t> roles) {
    Call c;
    c.labels = labels;
    c.roles = roles;
    c.offsets = {0, (int64_t)labels.size()};
    c.nq = 1;
    c.vectors.assign(labels.size() * 3, 1.0f);
    return c;
}

void refusals() {
    const int P = MLVDB_EXAMPLE_POS, N = MLVDB_EXAMPLE_NEG, T = MLVDB_EXAMPLE_TARGET;
    CHECK(best({1, -1, 2}, {P, N, P}).run() == MLVDB_OK);
    {
        Call c = best({1}, {P});
        c.k = 0;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.k = 65;
        CHECK(c.run() == MLVDB_ERR_UNSUPPORTED);
        c.k = 5;
        c.nq = -1;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.nq = 1;
        c.mode = 3;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.mode = MLVDB_EXAMPLES_BEST;
        c.null_out = true;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
    }
    {
        Call c = best({1, 2}, {P, P});
        c.offsets = {1, 2};
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);  // does not start at 0
        c.offsets = {0, 2, 1};
        c.nq = 2;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);  // descends
        c.offsets = {0, 0, 2};
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);  // an empty bag
    }
    {
        Call c = best(std::vector<int64_t>(65, 1), std::vector<int32_t>(65, P));
        CHECK(c.run() == MLVDB_ERR_UNSUPPORTED);
    }
    CHECK(best({10}, {P}).run() == MLVDB_ERR_INVALID_ARG);
    CHECK(best({-2}, {P}).run() == MLVDB_ERR_INVALID_ARG);
    CHECK(best({1}, {T}).run() == MLVDB_ERR_INVALID_ARG);
    CHECK(best({1}, {7}).run() == MLVDB_ERR_INVALID_ARG);
    {
        Call c = best({-1}, {P});
        c.no_vectors = true;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.no_vectors = false;
        c.vectors[2] = std::numeric_limits<float>::infinity();
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.vectors[2] = std::numeric_limits<float>::quiet_NaN();
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.labels[0] = 4;  // a stored example: its row of example_vectors is not read
        CHECK(c.run() == MLVDB_OK);
    }
    {
        Call c = best({1, 2, 3}, {T, P, N});
        c.mode = MLVDB_EXAMPLES_DISCOVER;
        CHECK(c.run() == MLVDB_OK);
        c.roles = {T, N, P};
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c.roles = {P, P, N};
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c = best({1, 2}, {T, P});
        c.mode = MLVDB_EXAMPLES_DISCOVER;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);  // half a pair
        c = best({1}, {T});
        c.mode = MLVDB_EXAMPLES_DISCOVER;
        CHECK(c.run() == MLVDB_OK);  // no pair: the plain search
    }
    {
        Call c = best({1, 2}, {P, N});
        c.mode = MLVDB_EXAMPLES_CONTEXT;
        CHECK(c.run() == MLVDB_OK);
        c.roles = {N, P};
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
        c = best({1, 2, 3}, {T, P, N});
        c.mode = MLVDB_EXAMPLES_CONTEXT;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);  // a target
        c = best({1}, {P});
        c.mode = MLVDB_EXAMPLES_CONTEXT;
        CHECK(c.run() == MLVDB_ERR_INVALID_ARG);
    }
    {
        Call c;  // nq = 0: nothing is read
        c.offsets = {0};
        CHECK(c.run() == MLVDB_OK);
    }
}

void cuts() {
    for (int mode = 0; mode < 3; ++mode)
        for (int m = 1; m <= kExamplesMax; ++m) {
            if (mode == MLVDB_EXAMPLES_DISCOVER && m % 2 == 0) continue;
            if (mode == MLVDB_EXAMPLES_CONTEXT && m % 2 == 1) continue;
            std::vector<int32_t> roles((size_t)m);
            for (int j = 0; j < m; ++j) {
                if (mode == MLVDB_EXAMPLES_BEST) roles[(size_t)j] = j % 3 == 1 ? MLVDB_EXAMPLE_NEG : MLVDB_EXAMPLE_POS;
                else if (mode == MLVDB_EXAMPLES_DISCOVER) roles[(size_t)j] = j == 0 ? MLVDB_EXAMPLE_TARGET : j % 2 ? MLVDB_EXAMPLE_POS : MLVDB_EXAMPLE_NEG;
                else roles[(size_t)j] = j % 2 ? MLVDB_EXAMPLE_NEG : MLVDB_EXAMPLE_POS;
            }
            for (int qt = 1; qt <= kExamplesMaxTile; qt *= 2) {
                std::vector<ExamplesTile> out(3);  // (something before: the cut appends)
                const int nt = examples_cut(mode, roles.data(), m, qt, 100, 7, 11, 2, out);
                CHECK((int)out.size() == 3 + nt && nt >= (m + qt - 1) / qt);
                int next = 100;
                bool open_pair = false;  // (with qt = 1 a pair spans two tiles: the scan carries its POS distance)
                for (int t = 0; t < nt; ++t) {
                    const ExamplesTile& tile = out[(size_t)(3 + t)];
                    CHECK(tile.query == 7 && tile.state == -1 && tile.excl_off == 11 && tile.n_excl == 2);
                    CHECK(((tile.flags & kExFirst) != 0) == (t == 0) && ((tile.flags & kExLast) != 0) == (t == nt - 1));
                    CHECK(((tile.flags >> kExModeShift) & 3u) == (uint32_t)mode);
                    bool ended = false;
                    for (int s = 0; s < kExamplesMaxTile; ++s) {
                        const uint32_t role = (tile.roles >> (4 * s)) & 15u;
                        if (s >= qt || tile.ex[s] < 0) {
                            CHECK(tile.ex[s] == -1 && role == kExEmpty);
                            ended = true;
                            continue;
                        }
                        CHECK(!ended && tile.ex[s] == next);
                        const int32_t r = roles[(size_t)(next - 100)];
                        ++next;
                        if (mode == MLVDB_EXAMPLES_BEST) CHECK(role == (r == MLVDB_EXAMPLE_POS ? kExPosMin : kExNegMin));
                        else if (r == MLVDB_EXAMPLE_TARGET) CHECK(role == kExTarget && t == 0 && s == 0);
                        else if (r == MLVDB_EXAMPLE_POS) {
                            CHECK(role == kExPairPos && !open_pair);
                            open_pair = true;
                        } else {
                            CHECK(role == (mode == MLVDB_EXAMPLES_DISCOVER ? kExNegCount : kExNegSum) && open_pair);
                            open_pair = false;
                        }
                    }
                    CHECK(!open_pair || qt == 1);  // no pair leaves its tile open
                }
                CHECK(next == 100 + m);
            }
        }
}
}  // namespace

int main() {
    refusals();
    cuts();
    std::printf("examples_plan ok\n");
    return 0;
}
