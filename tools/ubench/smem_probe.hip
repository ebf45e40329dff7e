// smem_probe.hip — what one round trip to the scalar data cache costs a wave on gfx950 (measurement tool;
// hipcc --offload-arch=gfx950 -O2 smem_probe.hip -o smem_probe).  The trace kernels read TraceParams from the kernarg segment by s_load;
// where the compiler has no scalar registers left it sinks those loads to their uses, and a wave's set-up becomes a chain of
// load-and-wait groups (tools/scalar_side_report.py counts them).  This probe times such a chain: every load's offset is the dword the
// load before it returned, each followed by s_waitcnt lgkmcnt(0), over a 1.5 KiB buffer (the size of TraceParams: it stays in the
// 16 KiB scalar cache), as one dword per trip and as one s_load_dwordx16 per trip (what a batched phase would issue instead of up to
// sixteen single ones).  1-7 waves per SIMD: 256-thread workgroups, one wave per SIMD each, as many per CU as an LDS request lets fit.
// Ticks are s_memtime's over a wave's own loop, printed beside the 100 MHz counter.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(16))) unsigned u32x16;
constexpr unsigned kBytes = 1536;

#define LD1 "s_load_dword %0, %1, %0\n s_waitcnt lgkmcnt(0)\n"
#define LD1x8 LD1 LD1 LD1 LD1 LD1 LD1 LD1 LD1

template <int MODE>
__global__ __launch_bounds__(256) void probe(const unsigned *buf, unsigned long long *out, int iters) {
    extern __shared__ unsigned lds_hold[]; // sized by the host so that exactly `waves per SIMD` workgroups fit a CU
    if (iters < 0) lds_hold[threadIdx.x] = 0;
    unsigned off = 0;
    const unsigned long long t0 = __builtin_readcyclecounter(); // s_memtime
    const unsigned long long r0 = wall_clock64();             // s_memrealtime: 100 MHz
    for (int i = 0; i < iters; i++) {
        if (MODE == 0) asm volatile(LD1x8 LD1x8 : "+s"(off) : "s"(buf));
        if (MODE == 1) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                u32x16 v;
                asm volatile("s_load_dwordx16 %0, %1, %2\n s_waitcnt lgkmcnt(0)\n" : "=&s"(v) : "s"(buf), "s"(off));
                off = v.x;
            }
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    const unsigned long long r1 = wall_clock64();
    if (off == 0x7fffffffu) out[3] = 1;
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(out, t1 - t0); // sum of the waves' loop times
        atomicAdd(out + 2, r1 - r0);
    }
}

template <int MODE>
static void run(const char *label, const unsigned *buf, unsigned long long *d) {
    const int iters = 2000, per_iter = 16;
    const int lds_kb[8] = {0, 96, 64, 48, 36, 32, 26, 22}; // k workgroups of this size fit a CU's 160 KiB, k + 1 do not
    for (int k = 1; k <= 7; k++) {
        const size_t lds = (size_t)lds_kb[k] * 1024;
        hipFuncSetAttribute(reinterpret_cast<const void *>(&probe<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        probe<MODE><<<256 * k, 256, lds>>>(buf, d, 10);
        hipMemsetAsync(d, 0, 32);
        probe<MODE><<<256 * k, 256, lds>>>(buf, d, iters);
        if (hipDeviceSynchronize() != hipSuccess) {
            printf("launch failed\n");
            exit(1);
        }
        unsigned long long sums[4] = {0, 0, 0, 0};
        hipMemcpy(sums, d, 32, hipMemcpyDeviceToHost);
        const double waves = 256.0 * 4.0 * k, loads = (double)iters * per_iter;
        printf("%-28s %d waves/SIMD: %7.1f ticks per load-and-wait (%.1f ns by the 100 MHz counter)\n", label, k, (double)sums[0] / waves / loads,
               (double)sums[2] / waves / loads * 10.0);
    }
}

int main() {
    // the chains: dword i holds the byte offset of dword (i + 91) % 384 (one cycle through all 384); of those, the first dword of
    // every 64-byte slot j is overwritten for the x16 chain with the offset of slot (j + 7) % 24 — two buffers, one per mode
    std::vector<unsigned> one(kBytes / 4), wide(kBytes / 4, 0u);
    for (unsigned i = 0; i < kBytes / 4; i++) one[i] = ((i + 91u) % (kBytes / 4)) * 4u;
    for (unsigned j = 0; j < kBytes / 64; j++) wide[j * 16] = ((j + 7u) % (kBytes / 64)) * 64u;
    unsigned *b0, *b1;
    unsigned long long *d;
    hipMalloc(&b0, kBytes);
    hipMalloc(&b1, kBytes);
    hipMalloc(&d, 32);
    hipMemcpy(b0, one.data(), kBytes, hipMemcpyHostToDevice);
    hipMemcpy(b1, wide.data(), kBytes, hipMemcpyHostToDevice);
    run<0>("dependent s_load_dword", b0, d);
    run<1>("dependent s_load_dwordx16", b1, d);
    return 0;
}
