#include <hip/hip_runtime.h>
#include <cstdio>
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// Does `buffer_load_dwordx4 ... offen lds` deliver to an LDS address >= 64 KiB through M0?  One workgroup of 8 waves with
// 160 KiB of dynamic LDS; wave w sends its 1 KiB piece (64 lanes x 16 B) to M0 = 96 KiB + w KiB.  If M0 carried only 16 bits
// the pieces would land at 32 KiB + w KiB instead.  Both windows are pre-filled with a pattern and read back; every address
// involved lies inside the allocation, whatever the answer.
constexpr unsigned kLds = 160 * 1024, kHigh = 96 * 1024, kLow = 32 * 1024, kWin = 8 * 1024;

__global__ __launch_bounds__(512) void k(const unsigned* in, unsigned* out) {
    extern __shared__ unsigned lds[];
    for (unsigned i = threadIdx.x; i < kWin / 4; i += blockDim.x) {
        lds[kHigh / 4 + i] = 0xdeadbeefu;
        lds[kLow / 4 + i] = 0xdeadbeefu;
    }
    __syncthreads();
    u32x4 srd;
    const unsigned long long b = (unsigned long long)in;
    srd[0] = __builtin_amdgcn_readfirstlane((unsigned)b);
    srd[1] = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32) & 0xffff);
    srd[2] = kWin;
    srd[3] = 0x00020000;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned voff = threadIdx.x * 16;  // this lane's 16 bytes of the source: wave * 1024 + lane * 16
    const unsigned dst = __builtin_amdgcn_readfirstlane(kHigh + wave * 1024);
    asm volatile("s_nop 4\n\t"
                 "s_mov_b32 m0, %[m]\n\t"
                 "s_nop 0\n\t"
                 "buffer_load_dwordx4 %[voff], %[srd], 0 offen lds\n\t"
                 "s_waitcnt vmcnt(0)\n\t" ::[m] "s"(dst), [voff] "v"(voff), [srd] "s"(srd)
                 : "memory", "m0");
    __syncthreads();
    for (unsigned i = threadIdx.x; i < kWin / 4; i += blockDim.x) {
        out[i] = lds[kHigh / 4 + i];
        out[kWin / 4 + i] = lds[kLow / 4 + i];
    }
}

int main() {
    unsigned *din, *dout;
    static unsigned h[kWin / 4], o[2 * kWin / 4];
    for (unsigned i = 0; i < kWin / 4; ++i) h[i] = i;
    if (hipMalloc(&din, kWin) != hipSuccess || hipMalloc(&dout, 2 * kWin) != hipSuccess) return 2;
    if (hipMemcpy(din, h, kWin, hipMemcpyHostToDevice) != hipSuccess) return 2;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, kLds) != hipSuccess) return 3;
    k<<<1, 512, kLds>>>(din, dout);
    if (hipMemcpy(o, dout, 2 * kWin, hipMemcpyDeviceToHost) != hipSuccess) return 4;
    unsigned high_ok = 0, low_ok = 0, high_touched = 0, low_touched = 0;
    for (unsigned i = 0; i < kWin / 4; ++i) {
        high_ok += o[i] == i;
        low_ok += o[kWin / 4 + i] == i;
        high_touched += o[i] != 0xdeadbeefu;
        low_touched += o[kWin / 4 + i] != 0xdeadbeefu;
    }
    printf("window at 96 KiB: %u of %u words hold the source (%u changed); window at 32 KiB: %u (%u changed)\n", high_ok, kWin / 4,
           high_touched, low_ok, low_touched);
    printf("M0 %s LDS addresses >= 64 KiB for buffer_load ... lds\n",
           high_ok == kWin / 4 && low_touched == 0 ? "REACHES" : (low_ok == kWin / 4 ? "DOES NOT reach (16 bits: wrapped to 32 KiB)" : "gives neither pattern at"));
    return 0;
}
