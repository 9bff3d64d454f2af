// The score program of a scored kNN call evaluated for one (query, row) pair (include/mlvdb_score.h): used by
// scored_scan_kernel (kernels_score.hip).  The program reaches the device validated (api.hip: score_prepare), so nothing
// here checks it again.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

#pragma clang fp contract(off)  // every op below is one rounded binary64 operation (the library's flag, restated)

namespace mlvdb {

// `prog` (usually staged in LDS) on one pair: `dist` is the pair's distance, bit c of `cond` says whether the row matches
// cond c, attr(slot) returns the row's value of ATTR operand `slot` (its default already applied).  The value stack is a
// shift register of MLVDB_SCORE_MAX_DEPTH doubles, s0 the top: a push moves every level down, a binary op combines the top
// two and moves the rest up.  Every op is uniform over the wave, so the branches never diverge, and no level is indexed
// dynamically, so the stack stays in registers.
template <class Attr>
__device__ __forceinline__ double score_eval(const ScoreOp* prog, int32_t n_ops, double dist, uint32_t cond, Attr&& attr) {
    static_assert(MLVDB_SCORE_MAX_DEPTH == 8, "the shift register below has eight levels");
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    for (int p = 0; p < n_ops; ++p) {
        const ScoreOp o = prog[p];
        if (o.op <= MLVDB_SCORE_MATCH) {  // the four pushes
            double v;
            switch (o.op) {
                case MLVDB_SCORE_CONST: v = __longlong_as_double(o.a); break;
                case MLVDB_SCORE_DIST: v = dist; break;
                case MLVDB_SCORE_ATTR: v = attr(o.slot); break;
                default: v = ((cond >> o.slot) & 1u) ? 1.0 : 0.0;  // MLVDB_SCORE_MATCH
            }
            s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0;
            s0 = v;
        } else if (o.op <= MLVDB_SCORE_MAX) {  // the six binary ops: x below y
            const double x = s1, y = s0;
            double v;
            switch (o.op) {
                case MLVDB_SCORE_ADD: v = x + y; break;
                case MLVDB_SCORE_SUB: v = x - y; break;
                case MLVDB_SCORE_MUL: v = x * y; break;
                case MLVDB_SCORE_DIV: v = x / y; break;
                case MLVDB_SCORE_MIN: v = x <= y ? x : (y < x ? y : __builtin_nan("")); break;
                default: v = x >= y ? x : (y > x ? y : __builtin_nan(""));  // MLVDB_SCORE_MAX
            }
            s0 = v;
            s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
        } else {  // NEG / ABS: the sign bit alone
            const long long bits = __double_as_longlong(s0);
            s0 = __longlong_as_double(o.op == MLVDB_SCORE_NEG ? (bits ^ (long long)0x8000000000000000ull)
                                                              : (bits & 0x7fffffffffffffffll));
        }
    }
    return s0;
}

// The value ATTR operand `od` pushes for a row whose stored value is `raw`: (double)v of an int64 column (rounded to nearest
// even), the double itself of a float64 one, the operand's default for an absent value (INT64_MIN / NaN).
__device__ __forceinline__ double score_operand_value(const ScoreOperand& od, int64_t raw) {
    if (od.type == MLVDB_ATTR_INT64) return raw != INT64_MIN ? (double)raw : __longlong_as_double(od.dflt);
    const double v = __longlong_as_double(raw);
    return v == v ? v : __longlong_as_double(od.dflt);
}

}  // namespace mlvdb
