// List-valued attribute columns (include/mlvdb_list.h): the repack of a value pool and the CSR read-back of a row range.
// Both are one computation -- the lengths of n slots, their exclusive scan, one copy of every list to its new place -- in
// three launches: per-block sums, a scan of the sums by one block, and the move, which scans inside its block again.  One
// row per thread and one block per kListBlock rows: no grid cap, no stride loop.  A row's copy is a loop of <= 255
// elements on one lane; lists are a few values long and the repack runs once per compaction.
#include "internal.h"

namespace mlvdb {

namespace {
__device__ __forceinline__ int slot_len(int64_t slot) { return slot == INT64_MIN ? 0 : (int)(slot & 0xff); }

// Inclusive scan of one value per thread over the block (kListBlock threads), Hillis-Steele in LDS; returns the inclusive
// prefix of this thread.  Every thread of the block must call it.
__device__ __forceinline__ int64_t block_inclusive_scan(int64_t v, int64_t* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < kListBlock; d <<= 1) {
        const int64_t add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    return lds[t];
}
}  // namespace

__global__ __launch_bounds__(kListBlock) void list_block_sums_kernel(const int64_t* __restrict__ slots,
                                                                      const float* __restrict__ rn, int64_t n,
                                                                      int64_t* __restrict__ sums) {
    __shared__ int64_t lds[kListBlock];
    const int64_t i = (int64_t)blockIdx.x * kListBlock + threadIdx.x;
    int64_t len = 0;
    if (i < n && (!rn || rn[i] == rn[i])) len = slot_len(slots[i]);
    const int64_t incl = block_inclusive_scan(len, lds);
    if (threadIdx.x == kListBlock - 1) sums[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kListBlock) void list_scan_sums_kernel(int64_t* __restrict__ sums, int64_t nblocks) {
    __shared__ int64_t lds[kListBlock];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nblocks; b0 += kListBlock) {  // b0 uniform over the block (barriers)
        const int64_t b = b0 + threadIdx.x;
        const int64_t v = b < nblocks ? sums[b] : 0;
        const int64_t incl = block_inclusive_scan(v, lds);
        if (b < nblocks) sums[b] = carry + incl - v;
        carry += lds[kListBlock - 1];
        __syncthreads();  // lds is rewritten by the next round
    }
    if (threadIdx.x == 0) sums[nblocks] = carry;
}

// (slots and out_slots may be the same memory: each thread reads its own slot before it writes it)
__global__ __launch_bounds__(kListBlock) void list_move_kernel(const int64_t* slots, int64_t n,
                                                                const int64_t* __restrict__ sums,
                                                                const int64_t* __restrict__ pool,
                                                                int64_t* __restrict__ out_pool, int64_t* out_slots,
                                                                int64_t* __restrict__ out_offsets,
                                                                uint8_t* __restrict__ out_present) {
    __shared__ int64_t lds[kListBlock];
    const int64_t i = (int64_t)blockIdx.x * kListBlock + threadIdx.x;
    const int64_t slot = i < n ? slots[i] : INT64_MIN;
    const int len = slot_len(slot);
    const int64_t at = sums[blockIdx.x] + block_inclusive_scan(len, lds) - len;
    if (i >= n) return;
    const int64_t* src = pool + (slot >> 8);  // (never read when len == 0)
    for (int j = 0; j < len; ++j) out_pool[at + j] = src[j];
    if (out_slots) out_slots[i] = slot == INT64_MIN ? INT64_MIN : ((at << 8) | len);
    if (out_offsets) {
        out_offsets[i] = at;
        if (i == n - 1) out_offsets[n] = at + len;
    }
    if (out_present) out_present[i] = slot == INT64_MIN ? 0 : 1;
}

hipError_t launch_list_block_sums(const int64_t* slots, const float* rn, int64_t n, int64_t* sums, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    list_block_sums_kernel<<<(unsigned)((n + kListBlock - 1) / kListBlock), kListBlock, 0, s>>>(slots, rn, n, sums);
    return hipGetLastError();
}

hipError_t launch_list_scan_sums(int64_t* sums, int64_t nblocks, hipStream_t s) {
    list_scan_sums_kernel<<<1, kListBlock, 0, s>>>(sums, nblocks);
    return hipGetLastError();
}

hipError_t launch_list_move(const int64_t* slots, int64_t n, const int64_t* sums, const int64_t* pool, int64_t* out_pool,
                            int64_t* out_slots, int64_t* out_offsets, uint8_t* out_present, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    list_move_kernel<<<(unsigned)((n + kListBlock - 1) / kListBlock), kListBlock, 0, s>>>(slots, n, sums, pool, out_pool,
                                                                                       out_slots, out_offsets, out_present);
    return hipGetLastError();
}

}  // namespace mlvdb
