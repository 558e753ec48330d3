// fft_2d.hip — 2-D transforms of small images in ONE pass: dsc_fft2 / dsc_ifft2 for N0, N1 in {32, 64, 128} and dsc_rfft2 for
// N0 in {32, 64, 128}, N1 in {64, 128, 256} (include/dsc_mi355x.h, Section F).
//
// An image of P = N0 x M complex points (M = N1, or N1 / 2 packed sample pairs of a real image) lives in the registers of T = P / 32
// threads, 32 complex each; a workgroup owns G = NT / T whole images.  One HBM round trip, no twiddle between the two dimensions:
//
//   N0 = 32 B0, M = 32 B1.  LDS holds one component (re, then im) of the image at a time as A[row][col], row pitch M + 1.
//   load    thread (t0, c) = x[t0 + B0 j][c], j < 32            lanes run along c: coalesced rows
//   col 1   dft32 over j -> q1,  x W_N0^{t0 q1}                 exchange (only if B0 > 1)
//   col 2   32 / B0 dft_B0 over t0 -> row bin q1 + 32 q2        exchange: columns -> rows
//   row 1   thread (t1, row) = A[row][t1 + B1 j]; dft32 over j -> k1,  x W_M^{t1 k1}      exchange
//   row 2   thread (rg, k1) = 32 / B1 rows, dft_B1 over t1 -> column bin k1 + 32 k2      lanes run along k1: 256-B runs of a row
//   store   natural [k0][k1] order
//
// The column transform runs first because a 2-D transform is separable and this order makes both the loads and the stores run along
// rows; the result is the one of "rows, then columns" up to rounding.  Zero padding: a row index >= h or a column index >= w is a
// lane whose offset lies outside the descriptor's range (reads zero); cropping never forms the offset; images past the end of the
// batch read zero and drop their stores.  Barriers order LDS only.
//
// Real input (rfft2): the image is loaded as N0 x N1/2 complex values z = (x[r][2m], x[r][2m + 1]) and transformed as above; with
// Z' = conj(Z[-q][-k]) (indices mod N0, mod M; fetched through one more exchange) E = (Z + Z') / 2 and O = -i (Z - Z') / 2 are the
// 2-D spectra of the even and the odd columns, and X[q][k] = E + W_N1^k O for k < M, X[q][M] = E[q][0] - O[q][0].  The columns 0 and
// N1 / 2 need no special treatment in this form: they fall out of the same formula.  Spectrum rows have the odd pitch M + 1.
//
// The inverse real transform (dsc_irfft2) is not fused: fft2.cpp composes it from dsc_ifft and dsc_irfft.
#include "dispatch.h"

#include <hip/hip_runtime.h>

#include <utility>

#include "fft_regs_common.h"

namespace {

// cos(2 pi q / 256), q = 0 .. 64
__device__ constexpr double kCos256[65] = {
    1.0, 0.9996988186962042201158, 0.9987954562051723927148, 0.9972904566786902161356,
    0.9951847266721968862448, 0.9924795345987099981568, 0.9891765099647809734517, 0.985277642388941244774,
    0.9807852804032304491262, 0.9757021300385285444604, 0.970031253194543992604, 0.9637760657954398666865,
    0.9569403357322088649358, 0.9495281805930366671959, 0.9415440651830207784125, 0.9329927988347388877117,
    0.9238795325112867561282, 0.914209755703530654635, 0.9039892931234433315862, 0.8932243011955153203424,
    0.8819212643483550297128, 0.8700869911087114186523, 0.8577286100002720699023, 0.8448535652497070732596,
    0.8314696123025452370788, 0.8175848131515836965049, 0.8032075314806449098067, 0.7883464276266062620092,
    0.7730104533627369608109, 0.7572088465064845475755, 0.7409511253549590911756, 0.7242470829514669209411,
    0.7071067811865475244008, 0.6895405447370669246167, 0.6715589548470184006254, 0.6531728429537767640842,
    0.6343932841636454982152, 0.6152315905806268454849, 0.595699304492433343467, 0.575808191417845300746,
    0.5555702330196022247428, 0.5349976198870972106631, 0.5141027441932217265937, 0.492898192229784036873,
    0.4713967368259976485564, 0.4496113296546066000463, 0.427555093430282094321, 0.4052413140049898709085,
    0.3826834323650897717285, 0.3598950365349881487751, 0.3368898533922200506893, 0.3136817403988914766565,
    0.2902846772544623676362, 0.2667127574748983863253, 0.2429801799032638899483, 0.2191012401568697972277,
    0.1950903220161282678483, 0.1709618887603012263636, 0.1467304744553617516589, 0.1224106751992161984987,
    0.0980171403295606019942, 0.07356456359966742352947, 0.04906767432741801425495, 0.02454122852291228803173,
    0.0};

// W_256^q = exp(-2 pi i q / 256)
template<typename R>
__device__ __forceinline__ cpx<R> root256(int q) {
    q &= 255;
    double c, s;
    if (q <= 64)       { c = kCos256[q];        s = -kCos256[64 - q]; }
    else if (q <= 128) { c = -kCos256[128 - q]; s = -kCos256[q - 64]; }
    else if (q <= 192) { c = -kCos256[q - 128]; s = kCos256[192 - q]; }
    else               { c = kCos256[256 - q];  s = kCos256[q - 192]; }
    return cpx<R>{(R) c, (R) s};
}

// N0 rows, M complex columns (REAL: M = N1 / 2 sample pairs)
template<typename R, int N0, int M> struct fft2_cfg {
    static constexpr bool DP = sizeof(R) == 8;
    static constexpr int B0 = N0 / 32, B1 = M / 32;
    static constexpr int T = N0 * M / 32;                       // threads per image
    static constexpr int NT_MIN = DP ? 128 : 256;
    static constexpr int NT = T > NT_MIN ? T : NT_MIN;          // threads per workgroup
    static constexpr int G = NT / T;                            // images per workgroup
    static constexpr int PW = M + 1;                            // LDS row pitch (values): odd
    static constexpr int IMG = N0 * PW;
    static constexpr int PLANE = (G * IMG + 3) & ~3;
    static constexpr int TABLE = 256;                           // W_256^m
    static constexpr size_t LDS = ((size_t) PLANE + 2 * TABLE) * sizeof(R);
};

// One exchange through the plane, one component at a time: register m goes to A[wr(m)], u[m] comes from A[rd(m)].  Ends with a
// barrier: the plane is free on return.
template<typename R, typename FW, typename FR>
__device__ __forceinline__ void exchange(const cpx<R> (&v)[32], cpx<R> (&u)[32], R *img, FW wr, FR rd) {
#pragma unroll
    for (int m = 0; m < 32; ++m) img[wr(m)] = v[m].x;
    lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; ++m) u[m].x = img[rd(m)];
    lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; ++m) img[wr(m)] = v[m].y;
    lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; ++m) u[m].y = img[rd(m)];
    lds_barrier();
}
template<typename R, typename FW, typename FR>
__device__ __forceinline__ void exchange(cpx<R> (&v)[32], R *img, FW wr, FR rd) {
    cpx<R> u[32];
    exchange(v, u, img, wr, rd);
#pragma unroll
    for (int m = 0; m < 32; ++m) v[m] = u[m];
}

// The same, reading back only the N registers lo .. lo + N - 1 (into u[0 .. N)): the partner fetch of the real split, which keeps v.
template<int N, typename R, typename FW, typename FR>
__device__ __forceinline__ void exchange_part(const cpx<R> (&v)[32], cpx<R> (&u)[N], int lo, R *img, FW wr, FR rd) {
#pragma unroll
    for (int m = 0; m < 32; ++m) img[wr(m)] = v[m].x;
    lds_barrier();
#pragma unroll
    for (int i = 0; i < N; ++i) u[i].x = img[rd(lo + i)];
    lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; ++m) img[wr(m)] = v[m].y;
    lds_barrier();
#pragma unroll
    for (int i = 0; i < N; ++i) u[i].y = img[rd(lo + i)];
    lds_barrier();
}

// in: [n_img][h][w] (complex; reals if in_real or REAL), out: [n_img][N0][M] complex (REAL: [n_img][N0][M + 1]).
// pairs (REAL): w is even and `in` aligned, so that every sample pair is one aligned 8- / 16-byte load.
// in and out may be the same memory (complex, h = N0, w = M): a group stores only after all its loads have been consumed.
template<typename R, int N0, int M, bool REAL, bool INV>
__global__ __launch_bounds__((fft2_cfg<R, N0, M>::NT)) void fft2_kernel(const void *in, void *out, long long n_img, int h, int w, int in_real,
                                                                         int pairs, R scale) {
    using C = cpx<R>;
    using cfg = fft2_cfg<R, N0, M>;
    constexpr int B0 = cfg::B0, B1 = cfg::B1, T = cfg::T, G = cfg::G, NT = cfg::NT, PW = cfg::PW;
    constexpr int LOGB0 = ilog2(B0), LOGB1 = ilog2(B1);
    constexpr int CB = (int) sizeof(C), RB = (int) sizeof(R);
    constexpr int OP = REAL ? M + 1 : M;                           // output row pitch
    constexpr int kOut = 0x7f000000;
    static_assert(!REAL || !INV, "the packed-real form is forward only");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    R *plane = (R *) lds_raw;
    C *wtab = (C *) (plane + cfg::PLANE);

    const int tid = threadIdx.x;
    const int g = T >= 64 ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;      // image within the group
    const int t = tid - g * T;
    const long long img0 = (long long) blockIdx.x * G;
    const long long left = n_img - img0;
    const int n_valid = left < G ? (int) left : G;                 // images past the end read zeros, their stores are dropped
    const int EB = (REAL || in_real) ? RB : CB;
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void *) ((const char *) in + img0 * h * w * EB), 0,
                                                                         n_valid * h * w * EB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void *) ((char *) out + img0 * N0 * OP * CB), 0,
                                                                          n_valid * N0 * OP * CB, 0x00020000);
    R *img = plane + g * cfg::IMG;

    // ---- load: thread (t0, c) takes rows t0 + B0 j of column c
    const int t0 = t / M, c = t % M;
    C v[32];
    if constexpr (REAL) {
        if (pairs) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int r = t0 + B0 * j;
                v[j] = buf_load<kCached>(rin, (r < h && 2 * c < w) ? ((g * h + r) * w + 2 * c) * RB : kOut, 0, R{});
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int r = t0 + B0 * j;
                const int base = ((g * h + r) * w + 2 * c) * RB;
                v[j] = C{buf_load_real<kCached>(rin, (r < h && 2 * c < w) ? base : kOut, 0, R{}).x,
                         buf_load_real<kCached>(rin, (r < h && 2 * c + 1 < w) ? base + RB : kOut, 0, R{}).x};
            }
        }
    } else {
        if (in_real) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int r = t0 + B0 * j;
                v[j] = buf_load_real<kStream>(rin, (r < h && c < w) ? ((g * h + r) * w + c) * RB : kOut, 0, R{});
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int r = t0 + B0 * j;
                v[j] = buf_load<kStream>(rin, (r < h && c < w) ? ((g * h + r) * w + c) * CB : kOut, 0, R{});
            }
        }
    }
    for (int i = tid; i < cfg::TABLE; i += NT) wtab[i] = root256<R>(i);
    lds_barrier();

    // ---- columns, pass 1: dft32 over j, twiddle W_N0^{t0 q1}
    dft_n<R, INV, 32>(v);                                           // v[m] = bin q1 = brev(m)
    if constexpr (B0 > 1) {
#pragma unroll
        for (int m = 1; m < 32; ++m) {
            const C tw = wtab[(256 / N0) * t0 * brev(m, 5)];
            v[m] = INV ? cmulc(v[m], tw) : cmul(v[m], tw);
        }
        // rows t0 + B0 q1 -> thread (t0', c) takes rows 32 t0' .. 32 t0' + 31: register m = (q1 = 32 / B0 t0' + m / B0, t0 = m % B0)
        exchange(v, img, [&](int m) { return (t0 + B0 * brev(m, 5)) * PW + c; }, [&](int m) { return (32 * t0 + m) * PW + c; });
        dft_columns<R, INV, B0>(v, std::make_integer_sequence<int, 32 / B0>{});
    }
    // register m holds row bin rb(m) of column c
    auto rb = [&](int m) { return B0 > 1 ? (32 / B0) * t0 + m / B0 + 32 * brev(m % B0, LOGB0) : brev(m, 5); };

    // ---- columns -> rows: thread (t1, row) takes columns t1 + B1 j of its row
    const int row1 = t % N0, t1 = t / N0;
    exchange(v, img, [&](int m) { return rb(m) * PW + c; }, [&](int m) { return row1 * PW + t1 + B1 * m; });

    // ---- rows, pass 1: dft32 over j, twiddle W_M^{t1 k1}
    dft_n<R, INV, 32>(v);                                           // v[m] = bin k1 = brev(m)
    if constexpr (B1 > 1) {
#pragma unroll
        for (int m = 1; m < 32; ++m) {
            const C tw = wtab[(256 / M) * t1 * brev(m, 5)];
            v[m] = INV ? cmulc(v[m], tw) : cmul(v[m], tw);
        }
    }
    // columns t1 + B1 k1 -> thread (rg, kk) takes, of the rows rg + RG i (i < 32 / B1), the B1 values of k1 = kk: register
    // m = (i = m / B1, t1 = m % B1).  B1 = 1: the same exchange turns "a thread per row" into "lanes along the row" for the stores.
    constexpr int RG = T / 32;
    const int kk = t % 32, rg = t / 32;
    exchange(v, img, [&](int m) { return row1 * PW + t1 + B1 * brev(m, 5); },
             [&](int m) { return (rg + RG * (m / B1)) * PW + (m % B1) + B1 * kk; });
    if constexpr (B1 > 1) dft_columns<R, INV, B1>(v, std::make_integer_sequence<int, 32 / B1>{});
    // register m holds bin (row(m), cb(m))
    auto row = [&](int m) { return rg + RG * (m / B1); };
    auto cb = [&](int m) { return kk + 32 * brev(m % B1, LOGB1); };

    if constexpr (!REAL) {
#pragma unroll
        for (int m = 0; m < 32; ++m)
            buf_store<kStream>(C{v[m].x * scale, v[m].y * scale}, rout, ((g * N0 + row(m)) * OP + cb(m)) * CB, 0);
    } else {
        // ---- the partner Z[-q][-k] of every value, then the split (see the file header).  f64 fetches the partners in two halves:
        // v and all 32 partners together are 256 registers of f64 data alone.
        constexpr int PARTS = sizeof(R) == 8 ? 2 : 1, PN = 32 / PARTS;
#pragma unroll
        for (int part = 0; part < PARTS; ++part) {
            C p[PN];
            exchange_part<PN>(v, p, part * PN, img, [&](int m) { return row(m) * PW + cb(m); },
                              [&](int m) { return ((N0 - row(m)) & (N0 - 1)) * PW + ((M - cb(m)) & (M - 1)); });
#pragma unroll
            for (int i = 0; i < PN; ++i) {
                const int m = part * PN + i;
                const C tw = wtab[(128 / M) * cb(m)];              // W_N1^k
                const R ex = (R) 0.5 * (v[m].x + p[i].x), ey = (R) 0.5 * (v[m].y - p[i].y);
                const R ox = (R) 0.5 * (v[m].y + p[i].y), oy = (R) -0.5 * (v[m].x - p[i].x);
                const int vo = ((g * N0 + row(m)) * OP + cb(m)) * CB;
                buf_store<kCached>(C{(ex + (tw.x * ox - tw.y * oy)) * scale, (ey + (tw.x * oy + tw.y * ox)) * scale}, rout, vo, 0);
                if (m % B1 == 0)                                    // k = 0 also yields the column N1 / 2
                    buf_store<kCached>(C{(ex - ox) * scale, (ey - oy) * scale}, rout, kk == 0 ? vo + M * CB : kOut, 0);
            }
        }
    }
}

// side of the window -> N0 or M of fft2_kernel; a size without a kernel ends the process
template<typename F> void with_fft2_len(int n, F f) {
    switch (n) {
        case 32:  return f(int_c<32>{});
        case 64:  return f(int_c<64>{});
        case 128: return f(int_c<128>{});
    }
    no_kernel("fft_2d.hip", "window side", n);
}

constexpr bool is_fused_dim(int n) { return n == 32 || n == 64 || n == 128; }

}  // namespace

bool dsc_fft2_regs_supports(int N0, int N1, dsc_fft_mode mode) {
    if (mode == DSC_MODE_C2R_PACKED) return false;
    return is_fused_dim(N0) && (mode == DSC_MODE_R2C_PACKED ? (N1 % 2 == 0 && is_fused_dim(N1 / 2)) : is_fused_dim(N1));
}

int dsc_fft2_regs_group(int N0, int N1, dsc_fft_mode mode, bool single_precision) {
    const int T = N0 * (mode == DSC_MODE_R2C_PACKED ? N1 / 2 : N1) / 32, nt_min = single_precision ? 256 : 128;
    return T > nt_min ? 1 : nt_min / T;
}

void dsc_launch_fft2_regs(const void *in, void *out, long long n_img, int N0, int N1, int h, int w, dsc_fft_mode mode, bool inverse,
                          bool single_precision, double scale, hipStream_t stream) {
    if (n_img <= 0) return;
    const int M = mode == DSC_MODE_R2C_PACKED ? N1 / 2 : N1;
    const bool real = mode == DSC_MODE_R2C_PACKED;                 // R2C_CAST: the C2C kernel, widening while it loads
    if (mode == DSC_MODE_C2R_PACKED) no_kernel("fft_2d.hip", "transform mode", mode);
    with_real(single_precision, [&](auto r) { with_fft2_len(N0, [&](auto n0) { with_fft2_len(M, [&](auto m) {
        with_mode(real ? DSC_MODE_R2C_PACKED : DSC_MODE_C2C, inverse, [&](auto md, auto inv) {
            using R = decltype(r);
            using cfg = fft2_cfg<R, decltype(n0)::value, decltype(m)::value>;
            static_assert(cfg::LDS <= 160 * 1024, "one image plane and the table fit the LDS of a CU");
            dsc_launch_dyn_lds<fft2_kernel<R, decltype(n0)::value, decltype(m)::value, decltype(md)::value == DSC_MODE_R2C_PACKED, decltype(inv)::value>>(
                (unsigned) ((n_img + cfg::G - 1) / cfg::G), cfg::NT, cfg::LDS, stream, in, out, n_img, h, w, mode == DSC_MODE_C2C ? 0 : 1,
                ((w & 1) == 0 && ((size_t) in & (2 * sizeof(R) - 1)) == 0) ? 1 : 0, (R) scale);
        });
    }); }); });
}
