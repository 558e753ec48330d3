// fft_r2c_64k.hip — 65536-point real FFT (f32) with the whole transform resident in registers.
//
// Replaces, for this size, the reference's per-line loop  gather -> dsc_real_fft -> scatter
// (dsc/src/dsc.cpp:2102-2171, dsc/include/dsc_fft.h:57-103, 178-238) by ONE pass over HBM:
// 4 B/sample in, 8 B/sample out, nothing else touches memory.
//
// Why registers: the packed transform is M = 32768 complex = 256 KiB per row, more than the
// 160 KiB of LDS but half of a CU's 512 KiB vector register file.  One 1024-thread workgroup
// (16 waves, 4 per SIMD, <= 128 VGPRs each) owns one row: 32 complex per thread.
//
//   M = 32 x 32 x 32,   j = 1024 j1 + 32 j2 + j3   (input),   k = k1 + 32 k2 + 1024 k3   (output)
//
//   load    thread t = 32 j2 + j3 reads z[1024 j1 + t], j1 = 0..31       (coalesced 8 B / lane)
//   pass 1  32-point DFT over j1 in registers, times W_1024^{j2 k1}
//   xchg 1  transpose j2 <-> k1 through LDS: complex values, one class of register groups at a time through a 132 KiB
//           buffer, pipelined behind the butterflies of the next group (see exchange())
//   pass 2  32-point DFT over j2, times W_32768^{j3 (k1 + 32 k2)}
//   xchg 2  transpose j3 <-> k2 the same way; the reader picks the column k' = k1 + 32 k2 so
//           that lane l and lane 63-l of a wave hold columns k' and 1024-k'
//   pass 3  32-point DFT over j3: Z[k' + 1024 k3]
//   post    packed-real untangling (dsc_fft.h:199-225) needs Z[k] and Z[M-k]: the partner
//           lane holds it, fetched with ds_bpermute (no LDS storage); each lane finishes 16
//           bin pairs and stores X[k] and X[M-k]                            (8 B / lane)
//
// In-register DFTs are radix-2, decimation in time, with compile-time twiddles (output index bit-reversed in
// the register number, which is free: every register index is a constant).  Inter-pass
// twiddles come from an 8 KiB LDS table indexed by the two factors of the exponent,
// T[r][h] = W_1024^{r h} (r = register, a constant; h = per-thread), and two per-thread constants.
// The inverse kernel (dsc_irfft, dsc_fft.h:194-236) is the same pipeline run backwards.
// The passes, the transposes and the store tail are in fft_64k_common.h, shared with fft_c2c_32k.hip; here are the three
// kernels with their real passes, the table builder and the launchers.
#include "fft_64k_common.h"

#include <cmath>

namespace {

// How much of the NEXT row a kernel requests before its last pass (see irfft64k_kernel); the two numbers a build can override.
// irfft64k_kernel, pairs: measured 0 / 4 / 6 / 8 -> 0.914 / 0.868 / 0.879 / 0.920 ms.  With pass 3 pinned, as it is, 4 / 6 / 8
// pairs need 116 / 121 / 128 VGPRs without spills and measure 0.868 / 0.870 / 0.884 ms: what pays is the rebalanced tail
// (8 + 16 + 9 loads instead of 17 + 16), not more prefetch.
#ifndef DSC_IRFFT_EARLY_PAIRS
#define DSC_IRFFT_EARLY_PAIRS 4
#endif
#ifndef DSC_FILTER_EARLY_LOADS
#define DSC_FILTER_EARLY_LOADS 4      // measured 0 / 4 / 12 / 16: 0.669 / 0.662 / 0.664 / 0.673 ms (the kernel is ALU bound; +1 %)
#endif

// Diagnostic builds (tools/probe64k.hip) add an `io_on` argument: 0 gives every buffer
// descriptor zero records, i.e. all global accesses are dropped while the instruction stream
// stays the same (compute-only timing).
#ifdef DSC_R2C64K_PROBE
#define PROBE_ARGS , int io_on
#define PROBE_NULL , 1
#define IO_ON io_on
#else
#define PROBE_ARGS
#define PROBE_NULL
#define IO_ON 1
#endif

// ------------------------------------------------------------------------------------------
// forward: x [batch][65536] f32  ->  X [batch][32769] c32
// in_pitch: floats between input rows; in_len <= 65536: valid samples per row — the rest of the transform length reads
// as zero (dsc_rfft's zero padding, dsc.cpp:2125-2133) through the range check of the row's buffer descriptor.
__global__ __launch_bounds__(1024) void rfft64k_kernel(const float *__restrict__ x, f2 *__restrict__ X, int batch,
                                                       const f2 *__restrict__ aux, int in_pitch, int in_len PROBE_ARGS) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *plane = lds;
    f2 *T = (f2 *) (lds + kPlaneFloats);
    fill_twiddle_table(T, aux);

    const int wave_sgpr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // The row loop is software pipelined on the loads: row r+1's 32 loads per lane are issued
    // in the tail of row r, as soon as the spectrum has left the registers for the LDS staging
    // area and BEFORE row r's stores are issued, so that (vmcnt retires in order) pass 1 of
    // the next row never waits behind the previous row's stores.
    cf v[32];
    {
        const int row0 = blockIdx.x;
        const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(
            (void *) (x + (size_t) row0 * in_pitch), 0, row0 < batch ? in_len * 4 * IO_ON : 0, 0x00020000);
        const int load_off = thread_id(wave_sgpr) * 8;
#pragma unroll
        for (int j1 = 0; j1 < 32; ++j1) v[j1] = load_c(r0, load_off, j1 * 8192);
    }

    for (int row = blockIdx.x; row < batch; row += gridDim.x) {
        // row descriptors: wave-uniform base, per-lane 32-bit byte offset, SGPR/immediate steps.
        // The next row's descriptor has zero records past the end of the batch: loads return 0.
        const int next_row = row + gridDim.x;
        const __amdgpu_buffer_rsrc_t rnext = __builtin_amdgcn_make_buffer_rsrc(
            (void *) (x + (size_t) next_row * in_pitch), 0, next_row < batch ? in_len * 4 * IO_ON : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rout =
            __builtin_amdgcn_make_buffer_rsrc((void *) (X + (size_t) row * (kM + 1)), 0, (kM + 1) * 8 * IO_ON, 0x00020000);

        const int cw = spectrum_wave(wave_sgpr);          // this wave holds the spectrum columns column_of(cw, lane)
        three_passes<false, kDit>(v, plane, T, aux, wave_sgpr, cw, false, true); // v[p] = Z[k' + 1024 br5(p)]
        // (Requesting part of the next row before pass 3, as irfft64k_kernel does, was tried here too: it needs pass 3's results
        // pinned — the compiler otherwise sinks the butterflies into the post-pass and the merged region takes all 128
        // registers — and then fits 4 loads, which measured 0.842-0.849 ms against 0.845-0.849 ms: nothing.)

        // ---- packed-real post-pass.  Rows 0..15 of this column pair with rows 31..16 of the
        // partner column (odd registers there); fetch them, finish both bins of each pair:
        // xk[k3] = X[k], xm[k3] = X[M-k], k = k' + 1024 k3.
        const int t4 = thread_id(wave_sgpr);
        const int lane = t4 & 63, wave = t4 >> 6;
        const int kp = column_of(cw, lane);
        const int partner_addr = partner_byte_addr(cw, lane);
        cf xk[16], xm[16];
        const cf zmid = v[br5(16)];                        // Z[M/2] in column 0
        if (cw == 0) {                                     // = wave 0
            // Column 0 (lane 0, its own partner) pairs row k3 with row 32 - k3 of ITSELF, not 31 - k3: shift its rows 17 .. 31
            // down by one (and row 0 into row 31) BEFORE the exchange, so that the general fetch below is right for it too and
            // the sent rows die with their ds_bpermute — fixing the fetched values up afterwards kept all 32 of them alive
            // across the exchange, in every wave.
#pragma unroll
            for (int r = 16; r < 31; ++r) v[br5(r)] = lane == 0 ? v[br5(r + 1)] : v[br5(r)];
            v[br5(31)] = lane == 0 ? v[br5(0)] : v[br5(31)];
        }
#pragma unroll
        for (int k3 = 0; k3 < 16; ++k3) {
            const int src = 31 - br5(k3);                  // = br5(31 - k3)
            xm[k3].x = bperm(partner_addr, v[src].x);
            xm[k3].y = bperm(partner_addr, v[src].y);
        }
        {
            const cf wpost = to_cf(aux[kAuxW65536 + kp]);
            const cf post_base = cf{0.5f * wpost.y, -0.5f * wpost.x};          // -(i/2) W_65536^{k'}
#pragma unroll
            for (int k3 = 0; k3 < 16; ++k3) {
                const cf c = cf{root64f_re(k3), root64f_im(k3)};                 // W_64^{k3} = W_65536^{1024 k3}
                const cf w = k3 == 0 ? post_base : cmul(post_base, c);
                real_pair(v[br5(k3)], xm[k3], w, 0.5f, xk[k3], xm[k3]);
            }
        }

        // ---- store.  Output rows are 32769 bins long, so a row starts 8 * (row mod 16) bytes
        // past a 128-B line; storing each lane's bins where the FFT left them would cut every
        // 256-B piece across three lines (measured: ~20 % of the HBM rate lost to partial
        // lines).  Instead the spectrum goes through the (now idle) LDS plane half a row at a
        // time and is stored as whole, 128-B aligned lines, 16 B per lane.
        f2 *stage = (f2 *) plane;
        const int skew = (int) ((((size_t) (X + (size_t) row * (kM + 1))) >> 3) & 15);     // bins past a line start
        // half 1: bins [0, 16384 - skew)
        lds_barrier();                                     // the last readers of the second transpose have left the plane
#pragma unroll
        for (int k3 = 0; k3 < 16; ++k3) stage[kp + 1024 * k3] = to_f2(xk[k3]);
        const cf xk15 = xk[15];
        const int load_off = thread_id(wave_sgpr) * 8;
#pragma unroll
        for (int j1 = 0; j1 < 16; ++j1) v[j1] = load_c(rnext, load_off, j1 * 8192);      // xk[] is dead: next row, first half (20 + 12 instead of 16 + 16: measured equal)
        lds_barrier();
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int k = 2 * (t4 + 1024 * m) - skew;       // first bin of this lane's 16-B chunk
            if (m > 0 || k >= 0) {                          // only the row's first chunk can start before bin 0
                const f2 lo2 = lds_read_b64(stage + k), hi2 = lds_read_b64(stage + k + 1);
                const f4 q = f4{lo2.x, lo2.y, hi2.x, hi2.y};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, q), rout, k * 8, 0, kStream);
            } else if (m == 0 && k == -1) {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, stage[0]), rout, 0, 0, kStream);
            }
            if (m & 1) __builtin_amdgcn_sched_barrier(0);       // at most two chunks of staging reads in flight (VGPR budget)
        }
        lds_barrier();
        // half 2: bins [16384 - skew, 32768], staged at index bin - kStage2
        constexpr int kStage2 = kM / 2 - 16;
#pragma unroll
        for (int k3 = 0; k3 < 16; ++k3) stage[(kM - kStage2) - kp - 1024 * k3] = to_f2(xm[k3]);
        if (kp >= 1009) stage[kp + 15 * 1024 - kStage2] = to_f2(xk15);         // bins 16369..16383
        if (t4 == 0) stage[kM / 2 - kStage2] = f2{zmid.x, -zmid.y};            // bin M/2 = conj Z[M/2] (dsc_fft.h:218)
#pragma unroll
        for (int j1 = 16; j1 < 32; ++j1) v[j1] = load_c(rnext, load_off, j1 * 8192);     // xm[] is dead: next row, second half
        lds_barrier();
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            if (m == 8 && wave != 0) break;                // bins past 32768 + 15 do not exist
            const int k = kM / 2 + 2 * (t4 + 1024 * m) - skew;
            if (m < 8 || k + 1 <= kM) {                     // only the row's last chunks can run past bin M
                const f2 lo2 = lds_read_b64(stage + k - kStage2), hi2 = lds_read_b64(stage + k + 1 - kStage2);
                const f4 q = f4{lo2.x, lo2.y, hi2.x, hi2.y};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, q), rout, k * 8, 0, kStream);
            } else if (m == 8 && k == kM) {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, stage[k - kStage2]), rout, k * 8, 0, kStream);
            }
            if (m & 1) __builtin_amdgcn_sched_barrier(0);
        }                                                  // (the next row's first transpose waits for these reads itself)
    }
}

// ------------------------------------------------------------------------------------------
// inverse: X [batch][32769] c32  ->  x [batch][65536] f32        (dsc_irfft, dsc_fft.h:194-236)
//
// The forward pipeline run backwards.  Each lane reads its column's first 16 rows AND their pairing partners (rows 31..16
// of the mirror column), the packed-real pre-pass completes the pairs and exchanges only the results through ds_bpermute, and three
// conjugate-twiddle passes end with thread t holding z[t + 1024 r]: the time samples leave as
// aligned, coalesced 8-B stores.  The 2/(2n) scale is folded into the pre-pass constants.
// in_pitch: bins between input rows; in_len <= 32769 bins per row are used, missing ones read as zero (dsc.cpp:2149-2157)
__global__ __launch_bounds__(1024) void irfft64k_kernel(const f2 *__restrict__ X, float *__restrict__ x, int batch,
                                                        const f2 *__restrict__ aux, int in_pitch, int in_len PROBE_ARGS) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *plane = lds;
    f2 *T = (f2 *) (lds + kPlaneFloats);
    fill_twiddle_table(T, aux);

    const int wave_sgpr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // Software pipelined like the forward kernel: the time samples leave through the LDS
    // staging area (whole lines, 16 B per lane) and the next row's bins are requested as soon
    // as the staging writes have freed the registers, ahead of this row's stores.
    // Loads keep the default cache policy: spectrum rows are skewed by 8 B x row, so neighbouring
    // waves share their boundary lines (nt loads measured 5 % slower on this kernel).
    // Register convention at the top of a row: v[a] = Y[c + 1024 a], v[16 + a] = Y[M - c - 1024 a] (a < 16): see inverse_prepass_direct.
    cf v[32];
    cf y_mid = cf{0.f, 0.f};
    {
        const int row0 = blockIdx.x;
        const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(
            (void *) (X + (size_t) row0 * in_pitch), 0, row0 < batch ? in_len * 8 * IO_ON : 0, 0x00020000);
        const int t0 = thread_id(wave_sgpr);
        const int c = column_of(t0 >> 6, t0 & 63);
        const int pv = (kM - c - 15 * 1024) * 8;                                     // Y[M - c - 1024 a] = pv + (15 - a) * 8192
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            v[a] = load_c_cached(r0, c * 8, a * 8192);
            v[16 + a] = load_c_cached(r0, pv, (15 - a) * 8192);
        }
        if (c == 0) y_mid = load_c_cached(r0, (kM / 2) * 8, 0);
    }

    for (int row = blockIdx.x; row < batch; row += gridDim.x) {
        const int next_row = row + gridDim.x;
        const __amdgpu_buffer_rsrc_t rnext = __builtin_amdgcn_make_buffer_rsrc(
            (void *) (X + (size_t) next_row * in_pitch), 0, next_row < batch ? in_len * 8 * IO_ON : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rout =
            __builtin_amdgcn_make_buffer_rsrc((void *) (x + (size_t) row * 65536), 0, 65536 * 4 * IO_ON, 0x00020000);

        inverse_prepass_direct(v, y_mid, aux, wave_sgpr);
        // The next row's first kEarly pairs (the ones the pre-pass consumes first) are requested BEFORE pass 3 — from the second
        // exchange on only v[] is live, which leaves room for them — the next eight when the first half of this row has left for
        // the staging area, the rest after the second half.  (kEarly = 0: everything in the tail, as the forward kernel does.)
        constexpr int kEarly = DSC_IRFFT_EARLY_PAIRS;
        cf early[kEarly > 0 ? 2 * kEarly : 1];
        three_passes<true, kDit>(v, plane, T, aux, wave_sgpr, wave_sgpr, true, false, [&]() {      // v[p] = z[t + 1024 br5(p)], t = reader_column
            if constexpr (kEarly > 0) {
                const int t3 = thread_id(wave_sgpr);
                const int c3 = column_of(t3 >> 6, t3 & 63);
                const int pv3 = (kM - c3 - 15 * 1024) * 8;
#pragma unroll
                for (int a = 0; a < kEarly; ++a) {
                    early[2 * a] = load_c_cached(rnext, c3 * 8, a * 8192);
                    early[2 * a + 1] = load_c_cached(rnext, pv3, (15 - a) * 8192);
                }
            }
        });

        // pass 3 complete here (the compiler otherwise sinks its butterflies towards the staging writes, where they overlap the
        // loads' registers)
        pin(v);
        const int t4 = thread_id(wave_sgpr);
        const int c = column_of(t4 >> 6, t4 & 63);
        const int pv = (kM - c - 15 * 1024) * 8;
        staged_time_store(v, plane, rout, wave_sgpr, [&](bool first_half) {
            // consumption order of the pre-pass: the pairs in ascending order (and bin M/2 with the first)
            if (first_half) {
                y_mid = cf{0.f, 0.f};
                if (c == 0) y_mid = load_c_cached(rnext, (kM / 2) * 8, 0);
#pragma unroll
                for (int i = 0; i < 8; ++i) {              // the even registers are free now
                    v[2 * i] = load_c_cached(rnext, c * 8, (kEarly + i) * 8192);
                    v[16 + 2 * i] = load_c_cached(rnext, pv, (15 - kEarly - i) * 8192);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8 - kEarly; ++i) {     // the odd ones
                    v[2 * i + 1] = load_c_cached(rnext, c * 8, (kEarly + 8 + i) * 8192);
                    v[17 + 2 * i] = load_c_cached(rnext, pv, (7 - kEarly - i) * 8192);
                }
            }
        });
        {   // back to the convention above (a renaming, every index is a constant)
            cf nxt[32];
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                if (a < kEarly)          { nxt[a] = early[2 * a];             nxt[16 + a] = early[2 * a + 1]; }
                else if (a < kEarly + 8) { nxt[a] = v[2 * (a - kEarly)];      nxt[16 + a] = v[16 + 2 * (a - kEarly)]; }
                else                     { nxt[a] = v[2 * (a - kEarly - 8) + 1]; nxt[16 + a] = v[17 + 2 * (a - kEarly - 8)]; }
            }
#pragma unroll
            for (int a = 0; a < 32; ++a) v[a] = nxt[a];
        }
    }
}

// ------------------------------------------------------------------------------------------
// fused README filterFFT (README.md:113-135): y = irfft(rfft(s) * H), H [32769] c32 shared by
// all rows.  The reference runs rfft, mul, irfft as three passes over memory with two
// materialised spectra; here the spectrum never leaves the register file: forward passes,
// post-pass pairs (X[k], X[M-k]), times (H[k], H[M-k]) read from L2, inverse pre-pass on the
// same pair in the same lane, inverse passes.  4 B/sample in, 4 B/sample out.
__global__ __launch_bounds__(1024) void filter64k_kernel(const float *__restrict__ x, const f2 *__restrict__ H,
                                                         float *__restrict__ y, int batch, const f2 *__restrict__ aux, int in_pitch,
                                                         int in_len) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *plane = lds;
    f2 *T = (f2 *) (lds + kPlaneFloats);
    fill_twiddle_table(T, aux);

    const int wave_sgpr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void *) H, 0, (kM + 1) * 8, 0x00020000);
    constexpr float kScale = 1.0f / (float) kM;

    cf v[32];                                              // software pipelined like the other two kernels
    {
        const int row0 = blockIdx.x;
        const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(
            (void *) (x + (size_t) row0 * in_pitch), 0, row0 < batch ? in_len * 4 : 0, 0x00020000);
        const int load_off = thread_id(wave_sgpr) * 8;
#pragma unroll
        for (int j1 = 0; j1 < 32; ++j1) v[j1] = load_c(r0, load_off, j1 * 8192);
    }
    for (int row = blockIdx.x; row < batch; row += gridDim.x) {
        const int next_row = row + gridDim.x;
        const __amdgpu_buffer_rsrc_t rnext = __builtin_amdgcn_make_buffer_rsrc(
            (void *) (x + (size_t) next_row * in_pitch), 0, next_row < batch ? in_len * 4 : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rout =
            __builtin_amdgcn_make_buffer_rsrc((void *) (y + (size_t) row * 65536), 0, 65536 * 4, 0x00020000);
        const int cw = spectrum_wave(wave_sgpr);          // this wave holds the spectrum columns column_of(cw, lane)
        three_passes<false, kDit>(v, plane, T, aux, wave_sgpr, cw, false, true); // v[p] = Z[c + 1024 br5(p)]

        // ---- post-pass, multiply by H, pre-pass: all on the pair (k, M-k) held by this lane.
        // In place: register br5(r) holds row r of the column before (Z) and after (Z'/M).
        {
            const int t1 = thread_id(wave_sgpr);
            const int lane = t1 & 63, wave = cw;
            const int c = column_of(wave, lane);
            const int partner_addr = partner_byte_addr(wave, lane);
            const cf wc = to_cf(aux[kAuxW65536 + c]);
            const cf post_base = cf{0.5f * wc.y, -0.5f * wc.x};                 // -(i/2) W^c
            const cf pre_base = cf{0.5f * kScale * wc.y, 0.5f * kScale * wc.x}; // (i/2M) conj(W^c)
            if (wave == 0) {                               // column 0, row 16: bin M/2 pairs with itself
                const cf zmid = v[br5(16)];
                const cf hmid = load_c_cached(rh, (kM / 2) * 8, 0);
                const cf pmid = cmul(cf{zmid.x, -zmid.y}, hmid);               // X[M/2] H[M/2]
                v[br5(16)] = lane == 0 ? cf{kScale * pmid.x, -kScale * pmid.y} : v[br5(16)];
            }
            // Column 0 pairs row a with row 32 - a of itself (row 0 with itself: X[0], X[M] both come
            // from Z[0]).  Shift its rows 17..31 down by one so that the general "row 31 - a" applies;
            // its own row 16 result (above) is parked meanwhile.
            cf park = v[br5(16)];
            if (wave == 0) {
#pragma unroll
                for (int r = 16; r < 31; ++r) v[br5(r)] = lane == 0 ? v[br5(r + 1)] : v[br5(r)];
                v[br5(31)] = lane == 0 ? v[br5(0)] : v[br5(31)];
            }
#pragma unroll
            for (int part = 0; part < 8; ++part) {         // eight batches of 2 pairs: VGPR budget
                cf q[2], zm[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int a = part * 2 + i;
                    q[i].x = bperm(partner_addr, v[br5(31 - a)].x);
                    q[i].y = bperm(partner_addr, v[br5(31 - a)].y);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int a = part * 2 + i;
                    const cf w64 = cf{root64f_re(a), root64f_im(a)};
                    cf xk, xm;
                    real_pair(v[br5(a)], q[i], a == 0 ? post_base : cmul(post_base, w64), 0.5f, xk, xm);
                    // bins k = c + 1024 a and M - k, times the filter
                    const cf hk = load_c_cached(rh, c * 8, a * 8192);
                    const cf hm = load_c_cached(rh, (kM - 15 * 1024 - c) * 8, (15 - a) * 8192);
                    cf pk = cmul(xk, hk), pm = cmul(xm, hm);
                    if (a == 0) {                          // dsc_fft.h:227-228: bins 0 and M enter irfft through their real parts
                        pk.y = (c == 0) ? 0.f : pk.y;
                        pm.y = (c == 0) ? 0.f : pm.y;
                    }
                    const cf w64c = cf{root64f_re(a), -root64f_im(a)};
                    real_pair(pk, pm, a == 0 ? pre_base : cmul(pre_base, w64c), 0.5f * kScale, v[br5(a)], zm[i]);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {              // Z'[M-k] belongs to the partner's row 31 - a
                    const int a = part * 2 + i;
                    v[br5(31 - a)].x = bperm(partner_addr, zm[i].x);
                    v[br5(31 - a)].y = bperm(partner_addr, zm[i].y);
                }
                __builtin_amdgcn_sched_barrier(0);         // keep the next batch's H loads and bpermutes out of this one
            }
            if (wave == 0) {                               // undo the shift of column 0
#pragma unroll
                for (int r = 31; r > 16; --r) v[br5(r)] = lane == 0 ? v[br5(r - 1)] : v[br5(r)];
                v[br5(16)] = lane == 0 ? park : v[br5(16)];
            }
        }
        cf z[32];                                          // inverse input in natural row order (a renaming)
#pragma unroll
        for (int r = 0; r < 32; ++r) z[r] = v[br5(r)];
        // the next row's first kEarlyX loads are requested before the inverse transform's last pass (see irfft64k_kernel)
        constexpr int kEarlyX = DSC_FILTER_EARLY_LOADS;
        cf early[kEarlyX > 0 ? kEarlyX : 1];
        three_passes<true, kDit>(z, plane, T, aux, wave_sgpr, cw, true, false, [&]() {  // z[p] = y[2(t + 1024 br5(p)) .. +1], t = reader_column
            if constexpr (kEarlyX > 0) {
                const int off = thread_id(wave_sgpr) * 8;
#pragma unroll
                for (int j1 = 0; j1 < kEarlyX; ++j1) early[j1] = load_c(rnext, off, j1 * 8192);
            }
        });
        {
            const int load_off = thread_id(wave_sgpr) * 8;
            staged_time_store(z, plane, rout, wave_sgpr, [&](bool first_half) {
                if (first_half) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) z[2 * i] = load_c(rnext, load_off, (kEarlyX + i) * 8192);
                } else {
#pragma unroll
                    for (int i = 0; i < 16 - kEarlyX; ++i) z[2 * i + 1] = load_c(rnext, load_off, (kEarlyX + 16 + i) * 8192);
                }
            });
#pragma unroll
            for (int j1 = 0; j1 < 32; ++j1) v[j1] = j1 < kEarlyX ? early[j1] : j1 < kEarlyX + 16 ? z[2 * (j1 - kEarlyX)] : z[2 * (j1 - kEarlyX - 16) + 1];
        }
    }
}


}  // namespace

size_t dsc_r2c64k_table_bytes() { return (size_t) kAuxEntries * sizeof(float) * 2; }

void dsc_r2c64k_build_tables(void *host_dst) {
    float *o = (float *) host_dst;
    auto put = [&](int at, long long k, long long n) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double) k / (long double) n;
        o[2 * at] = (float) cosl(a);
        o[2 * at + 1] = (float) sinl(a);
    };
    for (int m = 0; m < kTabEntries; ++m) {
        put(kAuxW1024 + m, m, 1024);
        put(kAuxW32768 + m, m, 32768);
        put(kAuxW65536 + m, m, 65536);
    }
    // exact values on the axes (bin M/2 relies on W_65536^{16384 * ...} only through constants,
    // but keep the tables clean too)
    o[2 * (kAuxW1024 + 256)] = 0.f;  o[2 * (kAuxW1024 + 256) + 1] = -1.f;
    o[2 * (kAuxW1024 + 512)] = -1.f; o[2 * (kAuxW1024 + 512) + 1] = 0.f;
    o[2 * (kAuxW1024 + 768)] = 0.f;  o[2 * (kAuxW1024 + 768) + 1] = 1.f;
}

void dsc_launch_rfft64k(const float *x, void *X, int batch, int in_pitch, int in_len, const void *aux, int n_cu, hipStream_t stream) {
    launch_rows<rfft64k_kernel>(batch, n_cu, stream, x, (f2 *) X, batch, (const f2 *) aux, in_pitch, in_len PROBE_NULL);
}
void dsc_launch_irfft64k(const void *X, float *x, int batch, int in_pitch, int in_len, const void *aux, int n_cu, hipStream_t stream) {
    launch_rows<irfft64k_kernel>(batch, n_cu, stream, (const f2 *) X, x, batch, (const f2 *) aux, in_pitch, in_len PROBE_NULL);
}
void dsc_launch_filter64k(const float *s, const void *H, float *y, int batch, int in_pitch, int in_len, const void *aux, int n_cu,
                          hipStream_t stream) {
    launch_rows<filter64k_kernel>(batch, n_cu, stream, s, (const f2 *) H, y, batch, (const f2 *) aux, in_pitch, in_len);
}
