// Greedy k-means++ seeding (include/mlvdb_seed.h): m picks, one stream-ordered chain of steps, no host wait between them.
//   seed_scan_kernel        assign_scan_kernel's shape, geometry and arithmetic -- plan_exact's tiles, gather_stage_queries,
//                           panel_walk; accumulate_rows / finish_distance give every d the scans' bits.  One launch scores
//                           ONE tile of up to QT trial rows; its sink clamps the distance, folds it with best(x) -- read
//                           once per row into a register -- and writes p_t(x) into plane t of [trials][stride] doubles: one
//                           lane per row, 128 B per 16-row panel and plane, +0.0 for a row that is no candidate.  The
//                           trials are independent, so the tiles of a step (ld > 1024: more than one) share no state.
//   seed_block_sums_kernel  one wave per block of 256 labels of one plane: four consecutive doubles per lane (2 KiB
//                           contiguous per wave, every sector byte used), (v0 + v1) + (v2 + v3), then six xor-butterfly
//                           levels over the 64 lanes.  fp64 addition is commutative, so both lanes of a pair hold the
//                           bits of the tree's node.  The block's sum is level 8; levels 1 .. 7 are never stored.
//   seed_upper_tree_kernel  levels 9 .. log2 P: a workgroup lifts kSeedFan nodes through LDS, one level per barrier, and
//                           stores every level it forms; log2(kSeedFan) levels per launch, one launch up to 65,536 rows.
//   seed_pick_kernel        one workgroup: the argmin of the trial roots (strict <, ascending t), the step's outputs, and
//                           the next step's draws -- one wave per draw descends the stored levels (every lane the same
//                           few loads), loads the one block of 256 leaves it ends in, rebuilds that block's eight levels
//                           as a heap in LDS and finishes the descent there.  The labels go straight into the words the
//                           next step's staging reads.
//   seed_commit_kernel      best = the winning plane: 16 B per row against the scan's 4 ld.
// T1, the tree of 1.0 over the candidates, has no plane: its leaves are read off the norms (NaN = no candidate).
// Everything that sums is fp64, one rounded operation per step in the order the header states (the library is built with
// -ffp-contract=off, restated below for this file).  No atomics, no scratch.
#include <algorithm>

#include "internal.h"
#include "panel_walk.h"

#pragma clang fp contract(off)

namespace mlvdb {

static_assert(kSeedBlock == 256, "seed_block_sums_kernel: 64 lanes x 4 leaves");
static_assert(kSeedFan == 256, "seed_upper_tree_kernel: one thread per node it loads");

template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void seed_scan_kernel(const SeedScanArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) qid[t] = a.first + t < a.nslots ? a.first + t : -1;
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);  // (ends with the barrier)
    if (SPACE == kSpaceCosine) {  // (per lane, as in assign_scan_kernel)
#pragma unroll
        for (int t = 0; t < QT; ++t) qinv[t] = lane_read(qinv[t], lane);
    }
    const int nvalid = a.nslots - a.first;  // slots t < nvalid hold a trial; an empty slot writes nothing
    double* const plane0 = a.planes + (int64_t)a.first * a.stride;
    const double* const best_in = a.best;
    const float* const rn = a.rn;
    const int64_t stride = a.stride;

    enum { kIn = 1, kLive = 2 };  // this lane reports a row of the index / that row is a candidate
    double best = 0.0;
    panel_walk<SPACE, QT, PW, NW, 0, /*NT=*/true>(
        a.X, a.ld, a.total, nblk, qs, qinv,
        [&](int64_t row, bool in) {
            const bool live = panel_row_live(rn, row, in);
            best = __builtin_inf();
            if (live && best_in) best = best_in[row];
            return (in ? kIn : 0) | (live ? kLive : 0);
        },
        [&](int t, int st, double dist, int32_t row) {
            if (t >= nvalid || !(st & kIn)) return;  // (t: unrolled, block-uniform)
            const double c = dist > 0.0 ? dist : 0.0;  // (a NaN compares false)
            const double p = c < best ? c : best;
            plane0[(int64_t)t * stride + row] = (st & kLive) ? p : 0.0;
        });
}

// Leaves x .. x + 3 (x a multiple of 4) of one tree: the plane's values, or 1.0 per candidate off the norms; +0.0 from
// `total` on.  A plane starts at a multiple of 4 doubles, so x + 3 lies inside it whenever x < total.
__device__ __forceinline__ void seed_leaves4(const double* __restrict__ plane, const float* __restrict__ rn, int64_t x,
                                             int64_t total, double (&v)[4]) {
    if (plane) {
        double2 lo = {0.0, 0.0}, hi = {0.0, 0.0};
        if (x < total) {
            lo = *reinterpret_cast<const double2*>(plane + x);
            hi = *reinterpret_cast<const double2*>(plane + x + 2);
        }
        v[0] = lo.x;
        v[1] = lo.y;
        v[2] = hi.x;
        v[3] = hi.y;
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (x + i >= total) v[i] = 0.0;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = 0.0;
        if (x + i < total) {
            const float nrm = rn[x + i];
            v[i] = nrm == nrm ? 1.0 : 0.0;
        }
    }
}

// grid (ceil(blocks / 4), planes), one wave per block of kSeedBlock labels
__global__ __launch_bounds__(256) void seed_block_sums_kernel(const double* __restrict__ planes, const float* __restrict__ rn,
                                                              const int64_t total, const int64_t stride, const int64_t blocks,
                                                              const int64_t heap_size, double* __restrict__ heap) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blk = (int64_t)blockIdx.x * 4 + wave;
    if (blk >= blocks) return;  // (wave-uniform; no barrier below)
    double v[4];
    seed_leaves4(planes ? planes + (int64_t)blockIdx.y * stride : nullptr, rn, blk * kSeedBlock + lane * 4, total, v);
    double s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o);
    if (lane == 0) heap[(int64_t)blockIdx.y * heap_size + blocks + blk] = s;
}

// grid (width / fan, planes) with fan = min(width, kSeedFan): the nodes width + [b fan, (b + 1) fan) of a heap -> their
// log2(fan) levels of ancestors.  A local heap in LDS: the loaded nodes at [fan, 2 fan), node i from 2 i and 2 i + 1.
__global__ __launch_bounds__(kSeedFan) void seed_upper_tree_kernel(double* __restrict__ heap, const int64_t heap_size,
                                                                   const int64_t width) {
    __shared__ double lv[2 * kSeedFan];
    const int tid = threadIdx.x;
    const int fan = width < kSeedFan ? (int)width : kSeedFan;
    double* const hp = heap + (int64_t)blockIdx.y * heap_size;
    if (tid < fan) lv[fan + tid] = hp[width + (int64_t)blockIdx.x * fan + tid];
    __syncthreads();
    for (int w = fan >> 1; w >= 1; w >>= 1) {  // (block-uniform)
        if (tid < w) {
            const double s = lv[2 * (w + tid)] + lv[2 * (w + tid) + 1];
            lv[w + tid] = s;
            hp[(width / fan) * w + (int64_t)blockIdx.x * w + tid] = s;  // the level of (width / fan) w nodes
        }
        __syncthreads();
    }
}

// One step of descend(): true = right, r moved on by the left sum.
__device__ __forceinline__ bool seed_go_right(double a, double b, double& r) {
    if (b == 0.0) return false;
    if (a == 0.0) return true;
    if (r < a) return false;
    r = r - a;
    return true;
}

__global__ __launch_bounds__(256) void seed_pick_kernel(const double* __restrict__ heap, const double* __restrict__ planes,
                                                        const double* __restrict__ heap1, const float* __restrict__ rn,
                                                        const int64_t total, const int64_t stride, const int64_t blocks,
                                                        const int64_t heap_size, const int32_t nslots,
                                                        const double* __restrict__ u, const int32_t ndraw, const int32_t step,
                                                        SeedState* st, int64_t* __restrict__ out_labels,
                                                        double* __restrict__ out_potential) {
    __shared__ double tree[4][2 * kSeedBlock];  // per wave: the heap of the block its draw ends in
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the winner: every thread reads the same few roots
    int32_t win = 0;
    double phi = 0.0;
    for (int32_t t = 0; t < nslots; ++t) {
        const double p = heap[(int64_t)t * heap_size + 1];
        if (t == 0 || p < phi) {
            phi = p;
            win = t;
        }
    }
    const int64_t won = nslots > 0 ? st->trial[win] : -1;  // (read by all before any draw overwrites it: the barrier below)
    const bool own = nslots > 0 && phi > 0.0;               // otherwise T1: every candidate coincides with a pick, or step 0
    const double* const hp = own ? heap + (int64_t)win * heap_size : heap1;
    const double* const plane = own ? planes + (int64_t)win * stride : nullptr;
    __syncthreads();
    if (threadIdx.x == 0 && nslots > 0) {
        out_labels[step] = won;
        out_potential[step] = phi;
        st->winner = win;
    }
    double* const tr = tree[wave];
    for (int i = 0; i < kSeedMaxTrials / 4; ++i) {  // (block-uniform: every wave meets every barrier)
        const int t = wave + 4 * i;
        const bool mine = t < ndraw;  // (wave-uniform)
        double r = 0.0;
        int64_t blk = 0;
        if (mine) {
            r = u[t] * hp[1];
            int64_t node = 1;
            while (node < blocks) {
                const double a = hp[2 * node], b = hp[2 * node + 1];
                node = 2 * node + (seed_go_right(a, b, r) ? 1 : 0);
            }
            blk = node - blocks;
            double v[4];
            seed_leaves4(plane, rn, blk * kSeedBlock + lane * 4, total, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) tr[kSeedBlock + lane * 4 + j] = v[j];
        }
        __syncthreads();
        for (int w = kSeedBlock >> 1; w >= 1; w >>= 1) {
            if (mine)
                for (int k = lane; k < w; k += 64) tr[w + k] = tr[2 * (w + k)] + tr[2 * (w + k) + 1];
            __syncthreads();
        }
        if (mine && lane == 0) {
            int k = 1;
            while (k < kSeedBlock) k = 2 * k + (seed_go_right(tr[2 * k], tr[2 * k + 1], r) ? 1 : 0);
            const int64_t label = blk * kSeedBlock + (k - kSeedBlock);
            st->trial[t] = label < total ? label : 0;  // (a leaf of weight > 0 is a row; the staging reads this address)
        }
        __syncthreads();  // the next turn overwrites the wave's heap
    }
}

__global__ __launch_bounds__(256) void seed_commit_kernel(const double* __restrict__ planes, const int64_t stride,
                                                          const int64_t total, const SeedState* __restrict__ st,
                                                          double* __restrict__ best) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < total) best[x] = planes[(int64_t)st->winner * stride + x];
}

// ------------------------------------------------------------------------------ host side
hipError_t launch_seed_scan(const SeedScanArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.total <= 0) return hipSuccess;
    if (a.first < 0 || a.first >= a.nslots || a.first % p.qt != 0) return hipErrorInvalidValue;  // (tiles start at multiples of p.qt)
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = seed_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        const size_t lds = (size_t)p.qt * a.ld * sizeof(double);  // the query image alone (within kQueryImageMaxLds)
        if (hipError_t e = ensure_instance_lds<kern>(lds, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<p.nblk, p.threads, lds, s>>>(a, p.nblk);
        return hipGetLastError();
    });
}

hipError_t launch_seed_tree(const double* planes, const float* rn, int64_t total, const SeedGeometry& g, int32_t nplanes,
                            double* heap, hipStream_t s) {
    if (nplanes < 1 || (!planes && nplanes != 1)) return hipErrorInvalidValue;
    seed_block_sums_kernel<<<dim3((unsigned)((g.blocks + 3) / 4), (unsigned)nplanes), 256, 0, s>>>(planes, rn, total, g.stride,
                                                                                                 g.blocks, g.heap, heap);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    for (int64_t width = g.blocks; width > 1;) {
        const int64_t fan = std::min<int64_t>(width, kSeedFan);
        seed_upper_tree_kernel<<<dim3((unsigned)(width / fan), (unsigned)nplanes), kSeedFan, 0, s>>>(heap, g.heap, width);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        width /= fan;
    }
    return hipSuccess;
}

hipError_t launch_seed_pick(const double* heap, const double* planes, const double* heap1, const float* rn, int64_t total,
                            const SeedGeometry& g, int32_t nslots, const double* u, int32_t ndraw, int32_t step,
                            SeedState* st, int64_t* out_labels, double* out_potential, hipStream_t s) {
    if (nslots < 0 || nslots > kSeedMaxTrials || ndraw < 0 || ndraw > kSeedMaxTrials) return hipErrorInvalidValue;
    seed_pick_kernel<<<1, 256, 0, s>>>(heap, planes, heap1, rn, total, g.stride, g.blocks, g.heap, nslots, u, ndraw, step, st,
                                       out_labels, out_potential);
    return hipGetLastError();
}

hipError_t launch_seed_commit(const double* planes, int64_t stride, int64_t total, const SeedState* st, double* best,
                              hipStream_t s) {
    if (total <= 0) return hipSuccess;
    seed_commit_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(planes, stride, total, st, best);
    return hipGetLastError();
}

}  // namespace mlvdb
