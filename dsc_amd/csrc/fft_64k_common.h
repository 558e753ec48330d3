// fft_64k_common.h — what the kernels of fft_r2c_64k.hip (rfft64k, irfft64k, filter64k) and fft_c2c_32k.hip (c2c32k) are made of:
// the three passes of the 32768-point complex transform with their LDS transposes (see the header of fft_r2c_64k.hip), the
// packed-real pair step, the staged store tail and the launch helper.  The butterflies, the complex type, the LDS-only barrier
// and the cache policies come from fft_regs_common.h.  Header-only, everything in an anonymous namespace.
#pragma once

#include "dispatch.h"
#include "fft_regs_common.h"

namespace {

// Arithmetic is done on plain scalar pairs, and these files are built with -fno-slp-vectorize:
// v_pk_*_f32 issues at half the rate of the scalar forms on gfx950 (measured, tools/valubench.hip:
// ~6 vs ~3 cycles per wave-instruction), cannot take literal constants (every twiddle constant
// would occupy a VGPR pair for the whole kernel) and needs v_mov shuffles to line operands up.
// f2 is the memory-op type only (8-B loads / stores / LDS).
using cf = cpx<float>;
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ cf to_cf(f2 a) { return cf{a.x, a.y}; }
__device__ __forceinline__ f2 to_f2(cf a) { return f2{a.x, a.y}; }

constexpr int kM = 32768;            // complex points per row
constexpr int kPlaneFloats = 1024 * 34;                     // 136 KiB: the transposes' step buffer (132 KiB) and the store staging area (128 KiB + 16 bins)
constexpr int kLdsBytes = kPlaneFloats * 4 + 1024 * 8;      // plane + twiddle table T
constexpr int kTabEntries = 1024;

// aux table layout (f2 entries): [0,1024) W_1024^m | [1024,2048) W_32768^m | [2048,3072) W_65536^m
constexpr int kAuxW1024 = 0, kAuxW32768 = 1024, kAuxW65536 = 2048, kAuxEntries = 3072;

__host__ __device__ constexpr int br5(int x) { return brev(x, 5); }

// The W_64 constants of the post-pass and the pre-pass, exp(-2 pi i q / 64) = (cos, -sin) for q in [0, 64), from a FLOAT table of
// the first quadrant.  With the values cast from the double table of fft_regs_common.h instead, filter64k_kernel comes out with
// the two multiplicands of 32 v_fma / v_fmac swapped (profiles/64k_refactor.md): the table stays, so that the device code stays
// what was measured.
__device__ constexpr float kCos64f[17] = {
    1.0f, 0.99518472667219688624f, 0.98078528040323044913f, 0.95694033573220886494f,
    0.92387953251128675613f, 0.88192126434835502971f, 0.83146961230254523708f, 0.77301045336273696081f,
    0.70710678118654752440f, 0.63439328416364549822f, 0.55557023301960222474f, 0.47139673682599764856f,
    0.38268343236508977173f, 0.29028467725446236764f, 0.19509032201612826785f, 0.09801714032956060199f,
    0.0f};
__device__ constexpr float root64f_re(int q) {
    q &= 63;
    return q <= 16 ? kCos64f[q] : q <= 32 ? -kCos64f[32 - q] : q <= 48 ? -kCos64f[q - 32] : kCos64f[64 - q];
}
__device__ constexpr float root64f_im(int q) {      // -sin(2 pi q / 64)
    q &= 63;
    return q <= 16 ? -kCos64f[16 - q] : q <= 32 ? -kCos64f[q - 16] : q <= 48 ? kCos64f[48 - q] : kCos64f[q - 48];
}

// The same products with the contraction spelled out: the first product of each component rounded, the second fused — where
// hipcc, left to -ffp-contract=fast, fuses the first of a difference.  The four outputs of the DIT dft32 that are sums only
// (bins 0, 8, 16, 24) took this form in pass 2 while the transposes moved one float component at a time (the compiler kept
// them as vector values); spelling it out keeps the results of rfft, irfft and the fused filter bit-identical to that version
// (profiles/exchange_pipeline_64k.md, section 6).  It is a special case whose only purpose is that identity: dropping it is a
// numeric change (last bits, the same error against float64) to be made on purpose and recorded, not a simplification — compare
// the sha256 of `bench.py --dump-outputs` before and after.
template<bool INV>
__device__ __forceinline__ cf twiddle_mul_second_fused(cf a, cf w) {
    if (INV) return cf{__builtin_fmaf(a.y, w.y, a.x * w.x), __builtin_fmaf(-a.x, w.y, a.y * w.x)};
    return cf{__builtin_fmaf(-a.y, w.y, a.x * w.x), __builtin_fmaf(a.y, w.x, a.x * w.y)};
}

// 32-point DFT of fft_regs_common.h, natural order in; v[p] returns bin br5(p).  DIF: kDit, the Linzer-Feig form (388 VALU
// instructions against 456: the fused filter, six of them per row, is bound by the vector ALUs), or kDif, which c2c32k_kernel
// keeps (0.824 against 0.835 ms).
template<bool INV, bool DIF>
__device__ __forceinline__ void dft32(cf (&v)[32]) { dft_n<float, INV, 32, 0, DIF>(v); }

// The same graph cut after stage 2: the four quarters v[8 Q .. 8 Q + 7] are then independent 8-point transforms.
template<bool INV, bool DIF>
__device__ __forceinline__ void dft32_head(cf (&v)[32]) {
    dft_stage<float, INV, 32, 1, 0, DIF>(v, std::integer_sequence<int, 0>{});
    dft_stage<float, INV, 32, 2, 0, DIF>(v, std::integer_sequence<int, 0, 1>{});
}
template<bool INV, bool DIF, int Q>
__device__ __forceinline__ void dft32_quarter(cf (&v)[32]) {
    dft_stage<float, INV, 32, 3, 0, DIF>(v, std::integer_sequence<int, Q>{});
    dft_stage<float, INV, 32, 4, 0, DIF>(v, std::integer_sequence<int, 2 * Q, 2 * Q + 1>{});
    dft_stage<float, INV, 32, 5, 0, DIF>(v, std::integer_sequence<int, 4 * Q, 4 * Q + 1, 4 * Q + 2, 4 * Q + 3>{});
}

// One 8-byte LDS read that stays one ds_read_b64.  hipcc fuses neighbouring 8-byte reads of one base into ds_read2_b64,
// which moves half as much per clock (tools/ldsbench.hip: 4.15 against 2.40 cycles per wave and 8 B/lane), and the row
// reads of a plane sit between two barriers with nothing to hide behind: 0.830-0.838 -> 0.820-0.823 ms on the rfft kernel
// (profiles/lds_read_forms_64k.md).  The access is volatile IN the LDS address space (a generic volatile pointer would turn
// it into a flat load); the compiler counts it in lgkmcnt like any other LDS read.  The twiddle table reads do NOT go through
// here: they are interleaved with arithmetic and with the plane writes, where the fixed order of volatile accesses costs
// more (0.827-0.829 ms) than the fused reads do.
__device__ __forceinline__ f2 lds_read_b64(const f2 *p) { return *(const volatile __attribute__((address_space(3))) f2 *) p; }

__device__ __forceinline__ float bperm(int byte_addr, float x) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(x)));
}

// Column of the output spectrum a lane owns in pass 3 / post-pass (see the header of fft_r2c_64k.hip).
__device__ __forceinline__ int column_of(int wave, int lane) {
    int kp = lane < 32 ? 32 * wave + lane : 1024 - 32 * wave - (63 - lane);
    return kp == 1024 ? 512 : kp;
}

// Values derived from threadIdx are loop invariant; hipcc hoists every address built from
// them out of the persistent row loop (dozens of VGPRs) and then spills them, and every
// scratch reload drains vmcnt, i.e. waits for all outstanding global stores.  The thread id
// is therefore rebuilt where it is needed from the wave number (an SGPR) and the hardware
// lane count, behind an opaque zero that keeps the two mbcnt from being hoisted.
__device__ __forceinline__ int thread_id(int wave_sgpr) {
    int zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
    const int lane = __builtin_amdgcn_mbcnt_hi(-1, __builtin_amdgcn_mbcnt_lo(-1, zero));
    return (wave_sgpr << 6) | lane;
}

// Row data is touched exactly once: non-temporal (kStream, aux = 2, `nt`) loads and stores keep it from
// displacing the tables and the next rows in L2 (measured +3.8 % on the rfft kernel).
__device__ __forceinline__ cf load_c(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return buf_load<kStream>(r, voff, soff, float{}); }
// The filter spectrum H is re-read by every row and stays on the default policy (kCached).  So do the spectrum rows of the
// inverse kernel (skewed by 8 B x row; see irfft64k_kernel), by measurement: default policy 0.911 ms; sc0 0.911, nt 0.930,
// sc0 nt 0.929, sc1 0.937, sc0 sc1 0.936, sc1 nt 0.929.
__device__ __forceinline__ cf load_c_cached(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return buf_load<kCached>(r, voff, soff, float{}); }

// The inter-pass twiddle table.  Both twiddle loops of three_passes() need W_1024^{r h} with r the register number (a
// constant, 1..31) and h a 5-bit per-thread value, so the table is laid out by the two factors: T[r][h] = W_1024^{r h}, 32 x 32
// entries — the same 8 KiB and the same floats as a linear W_1024^m table, but every read is ONE per-thread base (8 h) plus an
// immediate (256 r): no index arithmetic, and the 32 values of h a wave reads lie in consecutive entries (conflict free; the
// linear table read at stride r was gcd(r, 32)-way conflicted).  Filled once per workgroup.
__device__ __forceinline__ void fill_twiddle_table(f2 *T, const f2 *aux) {
    const int t = threadIdx.x;
    T[t] = aux[kAuxW1024 + (t >> 5) * (t & 31)];
    __syncthreads();
}

// ---- LDS transposes, pipelined behind the butterflies ------------------------------------------------------------------------
// A transpose sends register p of a writer (bin k = br5(p) of its 32-point DFT) to the reader thread whose coordinate is k,
// so the registers of one CLASS of bins deliver all 32 inputs to one class of reader threads and nothing to the others.  The
// two classes are k mod 4 in {0, 3} and k mod 4 in {1, 2}: after stage 2 of dft32 the quarters v[8 Q .. 8 Q + 7] are independent
// and hold the bins = {0, 2, 1, 3}[Q] mod 4, i.e. class 0 is quarters 0 and 3, class 1 quarters 1 and 2.  (Pairs a, 3 - a because
// the mirrored lanes l and 63 - l of the forward kernel hold coordinates k and 31 - k: both land in one class.)  A transpose is
// two steps through ONE buffer of 512 reader rows x 32 COMPLEX values (132 KiB, inside the old float plane):
//
//      finish class 0 (stages 3-5 of its quarters, twiddles) | barrier: buffer free | write class 0 | barrier
//      class-0 readers issue their 32 reads;  EVERY wave finishes class 1 meanwhile             | barrier: reads drained
//      write class 1 | barrier | class-1 readers read;  class-0 readers are already in their next DFT
//
// Reader classes are whole waves (but for one lane, see reader_of), two of each on every SIMD: while one wave of a SIMD waits for
// the LDS another one has butterflies to run.  The plane-at-a-time form before this had every wave in the same LDS phase at
// once: five of the twelve barrier intervals of a row held no vector arithmetic at all.
constexpr int kCPitch = 33;          // complex per buffer row: ds_write_b64 (16-lane groups) and ds_read_b64 (32-lane groups) conflict free
static_assert(512 * kCPitch * 8 <= kPlaneFloats * 4, "the step buffer lives inside the plane");

__host__ __device__ constexpr int class_of(int k) { return (k ^ (k >> 1)) & 1; }                  // k mod 4: 0, 3 -> 0;  1, 2 -> 1
__host__ __device__ constexpr int index_in_class(int k) { return ((k >> 2) << 1) | (k & 1); }     // 0 .. 15 within its class
static_assert(class_of(br5(0)) == 0 && class_of(br5(7)) == 0 && class_of(br5(24)) == 0 && class_of(br5(31)) == 0 &&
              class_of(br5(8)) == 1 && class_of(br5(23)) == 1, "class 0 = quarters 0 and 3 of a dft32 output");

// Which (32-row block, lane) a thread READS in a transpose with natural-order readers, as row / column number
// 32 k + (t & 31): the two class bits of k are the two high bits of the wave number, so that a class is made of whole waves —
// waves 0-3 and 12-15 against 4-11 — and every SIMD (wave mod 4) holds two waves of each.
__device__ __forceinline__ int reader_column(int t) {
    const int a = t >> 5;
    return (t & 31) | ((((a >> 3) | ((a & 7) << 2))) << 5);
}
// The same for the mirrored spectrum side (column_of): the wave that holds the columns of `wave` there.  Wave 0 stays wave 0.
__device__ __forceinline__ int spectrum_wave(int wave_sgpr) { return (wave_sgpr >> 2) | ((wave_sgpr & 3) << 2); }

// Quarter Q of a dft32 output to the step buffer of its class: register p (bin k = br5(p)) goes to row block index_in_class(k), at
// wbase = (row within the block) * kCPitch + (column), in complex units.  Two bases cover the 16 blocks with 16-bit
// immediates; the second is opaque so that the compiler does not fold it back and build one address per write.
template<int Q>
__device__ __forceinline__ void quarter_write(f2 *buf, int wbase, const cf (&v)[32]) {
    int wbase_hi = wbase + 8 * (32 * kCPitch);
    asm("" : "+v"(wbase_hi));
    f2 *lo8 = buf + wbase;
    f2 *hi8 = buf + wbase_hi;
#pragma unroll
    for (int p = 8 * Q; p < 8 * Q + 8; ++p)
        if (index_in_class(br5(p)) < 8) lo8[index_in_class(br5(p)) * (32 * kCPitch)] = to_f2(v[p]);
#pragma unroll
    for (int p = 8 * Q; p < 8 * Q + 8; ++p)
        if (index_in_class(br5(p)) >= 8) hi8[(index_in_class(br5(p)) - 8) * (32 * kCPitch)] = to_f2(v[p]);
}

// A reader's 32 inputs: one buffer row, single ds_read_b64 (see lds_read_b64).  Row numbers are far below 2^24: their
// products with the pitch take the full-rate 24-bit multiply; v_mul_lo_u32 issues at a quarter of the rate.
__device__ __forceinline__ void step_read(const f2 *buf, int row, cf (&dst)[32]) {
    const f2 *r = buf + __mul24(row, kCPitch);
#pragma unroll
    for (int m = 0; m < 32; ++m) dst[m] = to_cf(lds_read_b64(r + m));
}

// The values of v[] exist here, in program order: left alone the compiler sinks the butterflies that only a later group needs
// down to that group, across the barriers, and keeps their inputs alive instead (spills).
__device__ __forceinline__ void pin(cf (&v)[32]) {
#pragma unroll
    for (int p = 0; p < 32; p += 8)
        asm volatile("" : "+v"(v[p].x), "+v"(v[p].y), "+v"(v[p + 1].x), "+v"(v[p + 1].y), "+v"(v[p + 2].x), "+v"(v[p + 2].y), "+v"(v[p + 3].x),
                     "+v"(v[p + 3].y), "+v"(v[p + 4].x), "+v"(v[p + 4].y), "+v"(v[p + 5].x), "+v"(v[p + 5].y), "+v"(v[p + 6].x), "+v"(v[p + 6].y),
                     "+v"(v[p + 7].x), "+v"(v[p + 7].y));
}

// One transpose.  finish(std::integral_constant<int, Q>) completes quarter Q of src (the rest of its DFT and its twiddles);
// rclass / rrow: the class this thread reads in and its row there (coordinate k: index_in_class(k) * 32 + row within block).
// The barrier that frees the buffer after the class-1 reads is the first one of whatever writes the plane next.
template<typename Finish>
__device__ __forceinline__ void exchange(f2 *buf, int wbase, int rclass, int rrow, cf (&src)[32], cf (&dst)[32], Finish finish) {
    pin(src);
    lds_barrier();                                         // buffer free
    finish(std::integral_constant<int, 0>{});
    quarter_write<0>(buf, wbase, src);
    finish(std::integral_constant<int, 3>{});
    quarter_write<3>(buf, wbase, src);
    lds_barrier();
    cf r[32];                                              // fresh registers: whatever dst held before must not stay alive for the lanes that skip a read
    if (rclass == 0) step_read(buf, rrow, r);
    finish(std::integral_constant<int, 1>{});
    lds_barrier();                                         // class-0 reads drained (one quarter's twiddles in flight at a time: the readers' 64 registers are live here)
    quarter_write<1>(buf, wbase, src);
    finish(std::integral_constant<int, 2>{});
    quarter_write<2>(buf, wbase, src);
    lds_barrier();
    if (rclass != 0) step_read(buf, rrow, r);
#pragma unroll
    for (int m = 0; m < 32; ++m) dst[m] = r[m];
}

// Three passes of the 32768-point complex DFT (forward, or INV = conjugate twiddles), with the butterflies of form DIF (see dft32).
//   in : v[i] = element 1024 i + col of the input sequence, i = 0..31; col = t, the thread id (forward: time samples z[j]),
//        or with mirrored_in col = column_of(col_wave, lane) (inverse: bins Z[k]); the exchange routes by column
//   out: v[p] = element col_out + 1024 br5(p) of the output sequence; col_out = reader_column(t), or with mirrored_out
//        column_of(col_wave, lane).
//   The buffer is the caller's again after a barrier (the class-1 readers of the second transpose may still be reading).
struct no_hook { __device__ __forceinline__ void operator()() const {} };

// `before_pass3` runs between the second exchange and the last 32-point DFT: from there to the end of the row only v[] (64
// VGPRs) is live, which leaves room to request part of the NEXT row that early (irfft64k_kernel does).
template<bool INV, bool DIF, typename Hook = no_hook>
__device__ __forceinline__ void three_passes(cf (&v)[32], float *plane, const f2 *T, const f2 *aux, int wave_sgpr, int col_wave,
                                             bool mirrored_in, bool mirrored_out, Hook before_pass3 = Hook{}) {
    f2 *buf = (f2 *) plane;
    // readers with natural-order coordinates: the class is a property of the wave (a scalar: the reads sit behind a branch)
    const int wave_class = ((wave_sgpr >> 2) ^ (wave_sgpr >> 3)) & 1;
    // ---- pass 1 (over the slow index) and twiddle W_1024^{hi r1}, hi = col >> 5
    dft32_head<INV, DIF>(v);
    cf u[32];
    {
        const int t = thread_id(wave_sgpr);
        const int col = mirrored_in ? column_of(col_wave, t & 63) : t;
        const int hi = col >> 5;
        const f2 *th = T + hi;                            // T[r1][hi]: hi takes two (mirrored: three) values per wave, the reads broadcast
        // exchange 1: (hi, lo)[r1] -> thread (r1, lo), registers [hi];  buffer row = (r1 within its class) * 32 + lo, col = hi
        const int rc = reader_column(t);
        exchange(buf, __mul24(col & 31, kCPitch) + hi, wave_class, (index_in_class(rc >> 5) << 5) | (rc & 31), v, u, [&](auto Q) {
            constexpr int kQ = decltype(Q)::value;
            dft32_quarter<INV, DIF, kQ>(v);
#pragma unroll
            for (int p = 8 * kQ; p < 8 * kQ + 8; ++p) {
                if (p == 0) continue;
                const cf w = to_cf(th[32 * br5(p)]);
                v[p] = INV ? cmulc(v[p], w) : cmul(v[p], w);
            }
        });
    }
    // ---- pass 2 (over the middle index) and twiddle W_32768^{lo r1} W_1024^{lo r2}
    dft32_head<INV, DIF>(u);
    {
        const int t = thread_id(wave_sgpr);
        const int rc = reader_column(t);
        const int hi = rc >> 5, lo = rc & 31;            // (r1, lo)
        const cf tw2_base = to_cf(aux[kAuxW32768 + __mul24(hi, lo)]);
        const f2 *tl = T + lo;                            // T[r2][lo]: the lanes read consecutive entries
        // exchange 2: (r1, lo)[r2] -> output column r1 + 32 r2, registers [lo];  buffer row = (r2 within its class) * 32 + r1
        const int col_out = mirrored_out ? column_of(col_wave, t & 63) : rc;
        const int k2 = col_out >> 5;
        // mirrored: lanes l and 63 - l hold k2 and 31 - k2, one class — but for lane 63 (k2 = 32 - col_wave), which reads
        // with the other class when col_wave is odd: a per-lane class there
        const int rclass = mirrored_out ? class_of(k2) : wave_class;
        exchange(buf, __mul24(hi, kCPitch) + lo, rclass, (index_in_class(k2) << 5) | (col_out & 31), u, v, [&](auto Q) {
            constexpr int kQ = decltype(Q)::value;
            dft32_quarter<INV, DIF, kQ>(u);
            constexpr bool kSumsOnly = !DIF;               // registers 0 .. 3: bins 0, 16, 8, 24 (see twiddle_mul_second_fused)
#pragma unroll
            for (int p = 8 * kQ; p < 8 * kQ + 8; ++p) {
                const cf w = p == 0 ? tw2_base : cmul(tw2_base, to_cf(tl[32 * br5(p)]));
                if (kSumsOnly && p < 4) u[p] = twiddle_mul_second_fused<INV>(u[p], w);
                else u[p] = INV ? cmulc(u[p], w) : cmul(u[p], w);
            }
        });
    }
    before_pass3();
    // ---- pass 3 (over the fast index)
    dft32<INV, DIF>(v);
}

// Packed-real relations on one pair of bins (dsc_fft.h:199-228), p = in[k], q = in[M-k]:
//   s = p + conj q,  d = p - conj q,  out[k] = hs s + wq d,  out[M-k] = conj(hs s - wq d)
// forward: hs = 1/2, wq = -(i/2) W^k;  inverse: hs = 1/(2M), wq = (i/2M) conj(W^k).
__device__ __forceinline__ void real_pair(cf p, cf q, cf wq, float hs, cf &out_k, cf &out_mk) {
    const cf s = cf{p.x + q.x, p.y - q.y};
    const cf d = cf{p.x - q.x, p.y + q.y};
    const cf wd = cmul(d, wq);
    out_k = cf{hs * s.x + wd.x, hs * s.y + wd.y};
    out_mk = cf{hs * s.x - wd.x, wd.y - hs * s.y};
}

// Lane layout of the spectrum side (forward post-pass / inverse pre-pass): lane l and lane
// 63-l of a wave hold columns c and 1024-c; rows a of c pair with rows 31-a of 1024-c.
// Column 0 (wave 0, lane 0) pairs with itself shifted by one row, column 512 (wave 0, lane 63)
// with itself; both use themselves as ds_bpermute partner.
__device__ __forceinline__ int partner_byte_addr(int wave, int lane) {
    return ((wave == 0 && (lane == 63 || lane == 0)) ? lane : 63 - lane) * 4;
}


// Inverse packed-real pre-pass with the partner bins LOADED by the lane itself: on entry v[a] = Y[k], v[16 + a] = Y[M - k] for
// the lane's first 16 rows, k = c + 1024 a (Y[M - k] is row 31 - a of the partner column 1024 - c: the same 32 loads per
// lane as reading one's own 32 rows, but the pair is complete without a ds_bpermute).  Each pair gives Z[k] — this lane's
// row a — and Z[M - k] — the PARTNER's row 31 - a, which is the only thing exchanged (32 ds_bpermute instead of 64).
// On exit v[r] = Z[c + 1024 r] / M in natural row order.  y_mid = bin M/2 (column 0 only).
__device__ __forceinline__ void inverse_prepass_direct(cf (&v)[32], cf y_mid, const f2 *aux, int wave_sgpr) {
    constexpr float kScale = 1.0f / (float) kM;            // 2/(2n), dsc_fft.h:232
    const int t1 = thread_id(wave_sgpr);
    const int lane = t1 & 63, wave = t1 >> 6;
    const int c = column_of(wave, lane);
    const int partner_addr = partner_byte_addr(wave, lane);
    if (wave == 0 && lane == 0) { v[0].y = 0.f; v[16].y = 0.f; }          // bins 0 and M: real parts only (dsc_fft.h:227-228)
    const cf wpre = to_cf(aux[kAuxW65536 + c]);
    const cf wq_base = cf{0.5f * kScale * wpre.y, 0.5f * kScale * wpre.x};      // (i/2) conj(W^c) / M
#pragma unroll
    for (int half = 0; half < 2; ++half) {                 // two batches of 8 pairs: VGPR budget, and batch 0 only needs the
        cf zm[8];                                          // loads the pipeline issues first
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int a = half * 8 + i;
            const cf cj = cf{root64f_re(a), -root64f_im(a)}; // conj(W_64^a)
            const cf wq = a == 0 ? wq_base : cmul(wq_base, cj);
            real_pair(v[a], v[16 + a], wq, 0.5f * kScale, v[a], zm[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {                      // the partner's Z[M - k] of its pair a is my row 31 - a
            const int a = half * 8 + i;
            v[16 + a].x = bperm(partner_addr, zm[i].x);
            v[16 + a].y = bperm(partner_addr, zm[i].y);
        }
    }
    cf w[32];
#pragma unroll
    for (int r = 0; r < 16; ++r) { w[r] = v[r]; w[16 + r] = v[31 - r]; }  // v[16 + a] holds row 31 - a
    if (wave == 0) {
        // Column 0 pairs row a with row 32 - a of ITSELF (and row 0 with bin M): what came back as "row 31 - a" is row
        // 32 - a.  Shift up by one; row 16 = bin M/2 pairs with itself: Z[M/2] = conj Y[M/2] (dsc_fft.h:218).
#pragma unroll
        for (int r = 31; r > 16; --r) w[r] = lane == 0 ? w[r - 1] : w[r];
        w[16] = lane == 0 ? cf{kScale * y_mid.x, -kScale * y_mid.y} : w[16];
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) v[r] = w[r];
}

// Half a row (16384 complex) from the staging area to the row's bins BASE ..: whole lines, 16 B per lane, by thread id.
template<int BASE>
__device__ __forceinline__ void store_staged_half(const f2 *stage, int t4, __amdgpu_buffer_rsrc_t rout) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = 2 * (t4 + 1024 * m);
        const f2 lo2 = lds_read_b64(stage + k), hi2 = lds_read_b64(stage + k + 1);
        const f4 q = f4{lo2.x, lo2.y, hi2.x, hi2.y};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, q), rout, (BASE + k) * 8, 0, kStream);
        if (m & 1) __builtin_amdgcn_sched_barrier(0);       // at most two chunks of staging reads in flight (VGPR budget)
    }
}

// Tail shared by the inverse, the fused and the complex kernels: v[p] = z[t + 1024 br5(p)] (time samples of
// one aligned row) leaves through the LDS staging area, half a row at a time; as soon as a half has left the registers
// the next row's loads are issued into them (`issue_next(first_half)`), ahead of this row's stores.  Register p holds
// row br5(p): even p = rows 0..15 = first half.  On return the even registers hold what
// issue_next(true) loaded, the odd ones what issue_next(false) loaded.  The thread's column t is reader_column(thread id),
// as three_passes leaves it; the stores go by thread id.
template<typename IssueNext>
__device__ __forceinline__ void staged_time_store(cf (&v)[32], float *plane, __amdgpu_buffer_rsrc_t rout, int wave_sgpr,
                                                  IssueNext issue_next) {
    f2 *stage = (f2 *) plane;
    const int t4 = thread_id(wave_sgpr);
    const int c4 = reader_column(t4);
    lds_barrier();                                         // the last readers of the second transpose have left the plane
#pragma unroll
    for (int p = 0; p < 32; p += 2) stage[c4 + 1024 * br5(p)] = to_f2(v[p]);
    issue_next(true);
    lds_barrier();
    store_staged_half<0>(stage, t4, rout);
    lds_barrier();
#pragma unroll
    for (int p = 1; p < 32; p += 2) stage[c4 + 1024 * (br5(p) - 16)] = to_f2(v[p]);
    issue_next(false);
    lds_barrier();
    store_staged_half<kM / 2>(stage, t4, rout);            // (the next row's first transpose waits for these reads itself)
}

// The pipelined loads land rows 0..15 in the even registers and rows 16..31 in the odd ones:
// back to natural row order (a renaming, every index is a constant).
__device__ __forceinline__ void unzip_rows(cf (&v)[32]) {
    cf nxt[32];
#pragma unroll
    for (int a = 0; a < 16; ++a) { nxt[a] = v[2 * a]; nxt[16 + a] = v[2 * a + 1]; }
#pragma unroll
    for (int a = 0; a < 32; ++a) v[a] = nxt[a];
}

// How each of the kernels is launched: persistent, one workgroup of 1024 per CU, or per row where there are fewer; no rows, no launch.
template<auto Kernel, typename... Args>
void launch_rows(int batch, int n_cu, hipStream_t stream, Args... args) {
    if (batch <= 0) return;
    dsc_launch_dyn_lds<Kernel>(batch < n_cu ? batch : n_cu, 1024, kLdsBytes, stream, args...);
}

}  // namespace
