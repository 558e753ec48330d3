// tools/ldsbench.hip — LDS read forms of the 64k kernels on gfx950 (diagnostic): one 1024-thread workgroup per CU
// (4 waves per SIMD), the exchange plane's 136-byte row pitch, the 8 KiB twiddle table behind it.
//   row16xb64      every lane reads its own plane row as 16 x ds_read_b64            (what the plane-at-a-time transposes read; the pipelined ones read 32 x ds_read_b64 at a 264-byte pitch, not covered here)
//   row8xread2     the same 128 bytes as 8 x ds_read2_b64                            (what the compiler merges it into)
//   tab_product    31 x ds_read_b64 of T[r][lo], lanes on consecutive 8-byte entries (product-indexed table)
//   tab_lo_r2      31 x ds_read_b64 of w1024[lo * r2]                                (stride 2 r2 dwords: gcd(r2, 32)-way)
//   tab_read2      T[r][lo] fetched as ds_read2_b64 pairs                            (what the compiler merges tab_product into)
// Every group of reads ends with s_waitcnt lgkmcnt(0) inside the same asm statement.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ldsbench.hip -o tools/bin/ldsbench && tools/bin/ldsbench
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
constexpr int ITER = 2048;
constexpr int kPitchBytes = 136, kPlaneBytes = 1024 * kPitchBytes, kLdsBytes = kPlaneBytes + 8192;

#define RD(i, off) "ds_read_b64 %" #i ", %16 offset:" #off "\n"
#define RD2(i, o0, o1) "ds_read2_b64 %" #i ", %8 offset0:" #o0 " offset1:" #o1 "\n"
#define RDA(i, j) "ds_read_b64 %" #i ", %" #j "\n"
#define OUT8(T, v) "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
#define OUT16(v) OUT8(f2, v), "=&v"(v[8]), "=&v"(v[9]), "=&v"(v[10]), "=&v"(v[11]), "=&v"(v[12]), "=&v"(v[13]), "=&v"(v[14]), "=&v"(v[15])

template<int MODE> __global__ __launch_bounds__(1024) void k(float *out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    for (int i = threadIdx.x; i < kLdsBytes / 4; i += 1024) lds[i] = (float) i;
    __syncthreads();
    const unsigned row = threadIdx.x * kPitchBytes;                         // LDS byte addresses (the dynamic array starts at 0)
    const unsigned lo = threadIdx.x & 31;
    const unsigned tab = kPlaneBytes + lo * 8;
    unsigned a[16];
    f2 v[16];
    f4 q[8];
    float s = 0.f;
    for (int it = 0; it < ITER; ++it) {
        if (MODE == 0) {
            asm volatile(RD(0, 0) RD(1, 8) RD(2, 16) RD(3, 24) RD(4, 32) RD(5, 40) RD(6, 48) RD(7, 56) RD(8, 64) RD(9, 72) RD(10, 80)
                         RD(11, 88) RD(12, 96) RD(13, 104) RD(14, 112) RD(15, 120) "s_waitcnt lgkmcnt(0)" : OUT16(v) : "v"(row) : "memory");
        } else if (MODE == 1) {
            asm volatile(RD2(0, 0, 1) RD2(1, 2, 3) RD2(2, 4, 5) RD2(3, 6, 7) RD2(4, 8, 9) RD2(5, 10, 11) RD2(6, 12, 13) RD2(7, 14, 15)
                         "s_waitcnt lgkmcnt(0)" : OUT8(f4, q) : "v"(row) : "memory");
        } else if (MODE == 2) {                                             // r = 1..16, then r = 17..31
            asm volatile(RD(0, 256) RD(1, 512) RD(2, 768) RD(3, 1024) RD(4, 1280) RD(5, 1536) RD(6, 1792) RD(7, 2048) RD(8, 2304) RD(9, 2560)
                         RD(10, 2816) RD(11, 3072) RD(12, 3328) RD(13, 3584) RD(14, 3840) RD(15, 4096) "s_waitcnt lgkmcnt(0)" : OUT16(v) : "v"(tab) : "memory");
            asm volatile(RD(0, 4352) RD(1, 4608) RD(2, 4864) RD(3, 5120) RD(4, 5376) RD(5, 5632) RD(6, 5888) RD(7, 6144) RD(8, 6400) RD(9, 6656)
                         RD(10, 6912) RD(11, 7168) RD(12, 7424) RD(13, 7680) RD(14, 7936) "s_waitcnt lgkmcnt(0)" : OUT16(v) : "v"(tab) : "memory");
        } else if (MODE == 3) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int i = 0; i < 16; ++i) a[i] = kPlaneBytes + lo * (half * 16 + i + 1) * 8;      // r2 = 1..16, 17..32 (the last is not issued)
                if (half == 0)
                    asm volatile(RDA(0, 16) RDA(1, 17) RDA(2, 18) RDA(3, 19) RDA(4, 20) RDA(5, 21) RDA(6, 22) RDA(7, 23) RDA(8, 24) RDA(9, 25) RDA(10, 26)
                                 RDA(11, 27) RDA(12, 28) RDA(13, 29) RDA(14, 30) RDA(15, 31) "s_waitcnt lgkmcnt(0)"
                                 : OUT16(v) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
                                   "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]) : "memory");
                else
                    asm volatile(RDA(0, 16) RDA(1, 17) RDA(2, 18) RDA(3, 19) RDA(4, 20) RDA(5, 21) RDA(6, 22) RDA(7, 23) RDA(8, 24) RDA(9, 25) RDA(10, 26)
                                 RDA(11, 27) RDA(12, 28) RDA(13, 29) RDA(14, 30) "s_waitcnt lgkmcnt(0)"
                                 : OUT16(v) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
                                   "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]) : "memory");
            }
        } else {                                                            // rows (1,2) (3,4) .. (15,16); (17,18) .. (29,30), 31: offsets in 8 B
            asm volatile(RD2(0, 32, 64) RD2(1, 96, 128) RD2(2, 160, 192) RD2(3, 224, 0) RD2(4, 32, 64) RD2(5, 96, 128) RD2(6, 160, 192) RD2(7, 224, 0)
                         "s_waitcnt lgkmcnt(0)" : OUT8(f4, q) : "v"(tab) : "memory");
            asm volatile(RD2(0, 32, 64) RD2(1, 96, 128) RD2(2, 160, 192) RD2(3, 224, 0) RD2(4, 32, 64) RD2(5, 96, 128) RD2(6, 160, 192) RD2(7, 224, 0)
                         "s_waitcnt lgkmcnt(0)" : OUT8(f4, q) : "v"(tab) : "memory");
        }
    }
    if (MODE == 1 || MODE == 4) { for (int i = 0; i < 8; ++i) s += q[i].x + q[i].w; }
    else { for (int i = 0; i < 16; ++i) s += v[i].x + v[i].y; }
    out[blockIdx.x * 1024 + threadIdx.x] = s;
}

template<int MODE> int run(const char *name, int reads_b64) {
    float *out; CK(hipMalloc(&out, 256 * 1024 * 4));
    CK(hipFuncSetAttribute((const void *) k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(k<MODE>, dim3(256), dim3(1024), kLdsBytes, 0, out);
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k<MODE>, dim3(256), dim3(1024), kLdsBytes, 0, out);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    const double cyc = ms * 1e6 * 2.4 / ((double) ITER * 16 * reads_b64);  // CU cycles @2.4 GHz per wave and 8 bytes per lane read
    printf("%-12s %.3f ms -> %.2f cycles per wave per 8 B/lane read (%d x 8 B per pass, %.0f B/clk/CU)\n", name, ms, cyc, reads_b64, 512.0 / cyc);
    CK(hipFree(out));
    return 0;
}
int main() {
    return run<0>("row16xb64", 16) | run<1>("row8xread2", 16) | run<2>("tab_product", 31) | run<3>("tab_lo_r2", 31) | run<4>("tab_read2", 32);
}
