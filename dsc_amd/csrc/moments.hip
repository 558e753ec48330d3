// moments.hip — centred moments along one axis: sumsq / rms, var / std, vdot and detrend (include/dsc_mi355x.h, Section K; host side
// moments.cpp).  The tensor is viewed as [outer][n][inner], as reduce.hip and scan.hip view it.
//
// Arithmetic, the same on every route.  Every sum is a double, for f32 / c32 data too (the product of two floats is exact there), and a
// result is rounded once to its dtype.  With m = (sum x) / n:
//   sumsq    sum |x|^2                                 rms   sqrt(sumsq / n)
//   var      sum |x - m|^2 / (n - ddof), centred on the computed mean (two passes)           std   its square root
//   vdot     sum conj(a) b
//   detrend  t[j] = j - (n - 1) / 2, b = sum t x / (n (n^2 - 1) / 12), out[j] = x[j] - m - b t[j] (b = 0 for the constant form and for
//            n == 1), per component of complex data
// No atomics: a thread adds its elements in ascending order, the threads of a wave are combined by a butterfly of shuffles (every lane
// gets the same bits), the waves, tiles and segments after them in index order.  Two identical calls give identical bits.
//
//   inner == 1   moment_seg_kernel.  G threads (a wave of 64, or a workgroup of 256) own a SEGMENT of a row and walk it in chunks of
//                G x 8 packs of 16 bytes.  Three uses of the one kernel:
//                  FUSED   segment = whole row (moment_rows / detrend_rows).  A row of at most one chunk — 32 KiB per workgroup, 8 KiB
//                          per wave: dsc_moment_tile_len() elements — stays in registers between the mean and the centred pass: one HBM
//                          read (and one write for detrend).  A longer row is read a second time by the same workgroup.
//                  PART0   segment = tile of one chunk (moment_tiles / detrend_tiles): the tile's sums to scratch
//                  PART1   the centred pass of a tile with its row's statistic: var's sum to scratch, detrend's output to memory
//                moment_combine_kernel adds the partial sums of an output in index order (a lane a contiguous run of them, then the
//                butterfly) and forms the statistic or the result.  Plain launches in stream order: no workgroup waits on another.
//                Rows whose length or address rules out 16-byte packs take the same kernel with one element per pack.
//   inner > 1    moment_cols_kernel: one thread per (outer, inner) element walks the axis (twice for var and detrend), neighbouring
//                threads on neighbouring addresses.  With too few outputs to fill the chip the axis is cut into segments
//                (moment_cols_seg_kernel, PART0 / PART1 as above) combined in order by moment_combine_kernel.
#include "stream_common.h"

namespace {

enum { K_SUMSQ = 0, K_VDOT = 1, K_VAR = 2, K_DETREND_C = 3, K_DETREND_L = 4 };
enum { FUSED = 0, PART0 = 1, PART1 = 2 };
constexpr int kThreads = 256, kPacks = 8, kAcc = 4;

// Sums and statistics travel as four doubles.  Pass 0: sumsq {S}; vdot {re, im}; var / detrend {sum re, sum t re, sum im, sum t im}.
// Statistic of var / detrend: {m re, b re, m im, b im}.  Pass 1 (var): {sum |x - m|^2}.
template<int OP, typename In, int PASS> constexpr bool acc_used(int k) {
    constexpr bool c = elem<In>::cplx;
    if (PASS == 1 || OP == K_SUMSQ) return k == 0;
    if (OP == K_VDOT) return k == 0 || (c && k == 1);
    if (OP == K_DETREND_L) return k < 2 || c;
    return k == 0 || (c && k == 2);
}
template<int OP> constexpr bool two_pass() { return OP >= K_VAR; }
template<int OP> constexpr bool is_detrend() { return OP >= K_DETREND_C; }
template<int OP, typename In> struct out_of { using type = typename elem<In>::real; };
template<typename In> struct out_of<K_VDOT, In> { using type = In; };
template<typename In> struct out_of<K_DETREND_C, In> { using type = In; };
template<typename In> struct out_of<K_DETREND_L, In> { using type = In; };

template<typename In> __device__ __forceinline__ double re_of(In v) { if constexpr (elem<In>::cplx) return (double) v.x; else return (double) v; }
template<typename In> __device__ __forceinline__ double im_of(In v) { if constexpr (elem<In>::cplx) return (double) v.y; else return 0.0; }

// one element into the sums; t = j - (n - 1) / 2 (exact), st = the statistic (pass 1)
template<int OP, typename In, int PASS>
__device__ __forceinline__ void accumulate(double (&a)[kAcc], In x, In y, double t, const double (&st)[kAcc]) {
    constexpr bool c = elem<In>::cplx;
    const double xr = re_of(x), xi = im_of(x);
    if constexpr (PASS == 1) {
        const double dr = xr - st[0], di = xi - st[2];
        a[0] += c ? fma(di, di, dr * dr) : dr * dr;
    } else if constexpr (OP == K_SUMSQ) {
        a[0] += c ? fma(xi, xi, xr * xr) : xr * xr;
    } else if constexpr (OP == K_VDOT) {
        const double yr = re_of(y), yi = im_of(y);
        a[0] = fma(xr, yr, a[0]);
        if (c) {
            a[0] = fma(xi, yi, a[0]);
            a[1] = fma(xr, yi, a[1]);
            a[1] = fma(-xi, yr, a[1]);
        }
    } else {
        a[0] += xr;
        if (c) a[2] += xi;
        if (OP == K_DETREND_L) {
            a[1] = fma(t, xr, a[1]);
            if (c) a[3] = fma(t, xi, a[3]);
        }
    }
}

// the statistic from the sums of pass 0: the mean, and for the linear form the slope over sum t^2 = n (n^2 - 1) / 12
template<int OP, typename In>
__device__ __forceinline__ void stat_of(const double (&a)[kAcc], int n, double (&st)[kAcc]) {
    const double dn = (double) n;
    st[0] = a[0] / dn;
    st[2] = elem<In>::cplx ? a[2] / dn : 0.0;
    st[1] = st[3] = 0.0;
    if (OP == K_DETREND_L && n > 1) {
        const double d = dn * (dn * dn - 1.0) / 12.0;
        st[1] = a[1] / d;
        if (elem<In>::cplx) st[3] = a[3] / d;
    }
}

template<int OP, typename In>
__device__ __forceinline__ In detrend_out(In x, double t, const double (&st)[kAcc]) {
    using R = typename elem<In>::real;
    const double r = fma(-st[1], t, re_of(x) - st[0]);
    if constexpr (elem<In>::cplx) return In{(R) r, (R) fma(-st[3], t, im_of(x) - st[2])};
    else return (R) r;
}

// the result of a reduction from its sums (var: those of pass 1); root: rms / std
template<int OP, typename In>
__device__ __forceinline__ void write_result(void *out, long long o, const double (&a)[kAcc], int n, int ddof, bool root) {
    using R = typename elem<In>::real;
    if constexpr (OP == K_VDOT) {
        if constexpr (elem<In>::cplx) ((In *) out)[o] = In{(R) a[0], (R) a[1]};
        else ((In *) out)[o] = (R) a[0];
    } else {
        double v = a[0];
        if (OP == K_VAR) v = v / (double) (n - ddof);
        else if (root) v = v / (double) n;
        ((R *) out)[o] = (R) (root ? sqrt(v) : v);
    }
}

// every lane of the wave gets the sum of the 64 values: a + b == b + a bit for bit, so the butterfly leaves one set of bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the sums of the G threads that share a segment, in every one of them.  G == 256: the four waves through LDS, added in wave order; the
// caller alternates buf, so one barrier per call is enough
template<int OP, typename In, int PASS, int G>
__device__ __forceinline__ void group_sum(double (&a)[kAcc], double (*part)[kThreads / 64][kAcc], int buf) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k)
        if (acc_used<OP, In, PASS>(k)) a[k] = wave_sum(a[k]);
    if constexpr (G == kThreads) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kAcc; ++k)
                if (acc_used<OP, In, PASS>(k)) part[buf][w][k] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kAcc; ++k)
            if (acc_used<OP, In, PASS>(k)) a[k] = ((part[buf][0][k] + part[buf][1][k]) + part[buf][2][k]) + part[buf][3][k];
    }
}

template<typename In, int V> struct chunk_regs { packed<In, V> p[kPacks]; };

// the calling thread's packs of the chunk that starts at position j0 of the row; positions from jend on are not read.  Pack u of
// thread g of the group is pack u G + g of the chunk.  Positions are unsigned: a row has fewer than 2^31 elements, and a position
// past its end stays below 2^32
template<typename In, int V, int G>
__device__ __forceinline__ void load_chunk(const In *__restrict__ row, unsigned j0, unsigned jend, int g, chunk_regs<In, V> &r) {
#pragma unroll
    for (int u = 0; u < kPacks; ++u) {
        const unsigned j = j0 + (unsigned) ((u * G + g) * V);
        if (j < jend) {
            r.p[u] = *(const packed<In, V> *) (row + j);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) r.p[u].e[k] = In{};
        }
    }
}

// t of the thread's first element of the chunk; element k of pack u is (u G V + k) further on.  Integers and half-integers below 2^32:
// every step is exact
template<int V> __device__ __forceinline__ double t_first(unsigned j0, int g, double tc) { return ((double) j0 - tc) + (double) (g * V); }

template<int OP, typename In, int PASS, int V, int G>
__device__ __forceinline__ void chunk_sums(double (&a)[kAcc], const chunk_regs<In, V> &cx_, const chunk_regs<In, V> &cy_, unsigned j0,
                                           unsigned jend, int g, double tc, const double (&st)[kAcc]) {
    const double tg = t_first<V>(j0, g, tc);
#pragma unroll
    for (int u = 0; u < kPacks; ++u) {
        const unsigned j = j0 + (unsigned) ((u * G + g) * V);
        if (j < jend) {
#pragma unroll
            for (int k = 0; k < V; ++k) accumulate<OP, In, PASS>(a, cx_.p[u].e[k], cy_.p[u].e[k], tg + (double) (u * G * V + k), st);
        }
    }
}

template<int OP, typename In, int V, int G>
__device__ __forceinline__ void chunk_detrend(typename out_of<OP, In>::type *__restrict__ orow, const chunk_regs<In, V> &c, unsigned j0,
                                              unsigned jend, int g, double tc, const double (&st)[kAcc]) {
    if constexpr (is_detrend<OP>()) {
        const double tg = t_first<V>(j0, g, tc);
#pragma unroll
        for (int u = 0; u < kPacks; ++u) {
            const unsigned j = j0 + (unsigned) ((u * G + g) * V);
            if (j < jend) {
                packed<In, V> o;
#pragma unroll
                for (int k = 0; k < V; ++k) o.e[k] = detrend_out<OP, In>(c.p[u].e[k], tg + (double) (u * G * V + k), st);
                *(packed<In, V> *) (orow + j) = o;
            }
        }
    }
}

// Segment `seg` is positions [t tile_len, min((t + 1) tile_len, n)) of row seg / tiles_per_row, t = seg % tiles_per_row; G threads own
// it, kThreads / G segments per workgroup at a time.  FUSED (tiles_per_row == 1): both passes and the result.  PART0: partial[seg] = the
// sums of pass 0.  PART1: the centred pass with stats[row]: partial[seg] (var) or the output (detrend).  V > 1: n, tile_len and the base
// addresses are multiples of a pack.
template<int OP, typename In, int V, int G, int MODE>
__global__ __launch_bounds__(kThreads) void moment_seg_kernel(const In *__restrict__ x, const In *__restrict__ y, void *__restrict__ out,
                                                              double *__restrict__ partial, const double *__restrict__ stats,
                                                              long long n_seg, int n, int tile_len, int tiles_per_row, int ddof, bool root) {
    using Out = typename out_of<OP, In>::type;
    constexpr int CH = G * kPacks * V, GROUPS = kThreads / G;
    constexpr int P0 = 0, P1 = 1;
    __shared__ double part[2][kThreads / 64][kAcc];
    const int g = threadIdx.x % G, grp = threadIdx.x / G;
    const double tc = 0.5 * (double) (n - 1);
    int buf = 0;

    // G == kThreads: seg is the same in every thread of the workgroup, which the barriers of group_sum need
    for (long long seg = (long long) blockIdx.x * GROUPS + grp; seg < n_seg; seg += (long long) gridDim.x * GROUPS) {
        const long long row = seg / tiles_per_row;
        const unsigned start = (unsigned) (seg - row * tiles_per_row) * (unsigned) tile_len;
        const unsigned end = start + (unsigned) tile_len < (unsigned) n ? start + (unsigned) tile_len : (unsigned) n;
        const In *xrow = x + row * n, *yrow = OP == K_VDOT ? y + row * n : nullptr;
        Out *orow = is_detrend<OP>() ? (Out *) out + row * n : nullptr;
        chunk_regs<In, V> first, more, ys;
        double a[kAcc] = {0.0, 0.0, 0.0, 0.0}, st[kAcc] = {0.0, 0.0, 0.0, 0.0};

        load_chunk<In, V, G>(xrow, start, end, g, first);
        if constexpr (MODE != PART1) {
            if constexpr (OP == K_VDOT) load_chunk<In, V, G>(yrow, start, end, g, ys);
            chunk_sums<OP, In, P0, V, G>(a, first, OP == K_VDOT ? ys : first, start, end, g, tc, st);
            for (unsigned j0 = start + CH; j0 < end; j0 += CH) {
                load_chunk<In, V, G>(xrow, j0, end, g, more);
                if constexpr (OP == K_VDOT) load_chunk<In, V, G>(yrow, j0, end, g, ys);
                chunk_sums<OP, In, P0, V, G>(a, more, OP == K_VDOT ? ys : more, j0, end, g, tc, st);
            }
            group_sum<OP, In, P0, G>(a, part, buf);
            buf ^= 1;
            if constexpr (MODE == PART0) {
                if (g == 0) {
#pragma unroll
                    for (int k = 0; k < kAcc; ++k) partial[seg * kAcc + k] = a[k];
                }
                continue;
            } else if constexpr (!two_pass<OP>()) {
                if (g == 0) write_result<OP, In>(out, row, a, n, ddof, root);
                continue;
            } else {
                stat_of<OP, In>(a, n, st);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kAcc; ++k) st[k] = stats[row * kAcc + k];
        }

        if constexpr (two_pass<OP>()) {
            // the centred pass: the first chunk is still in registers, the chunks after it are read again
            if constexpr (is_detrend<OP>()) {
                chunk_detrend<OP, In, V, G>(orow, first, start, end, g, tc, st);
                for (unsigned j0 = start + CH; j0 < end; j0 += CH) {
                    load_chunk<In, V, G>(xrow, j0, end, g, more);
                    chunk_detrend<OP, In, V, G>(orow, more, j0, end, g, tc, st);
                }
            } else {
                double s[kAcc] = {0.0, 0.0, 0.0, 0.0};
                chunk_sums<OP, In, P1, V, G>(s, first, first, start, end, g, tc, st);
                for (unsigned j0 = start + CH; j0 < end; j0 += CH) {
                    load_chunk<In, V, G>(xrow, j0, end, g, more);
                    chunk_sums<OP, In, P1, V, G>(s, more, more, j0, end, g, tc, st);
                }
                group_sum<OP, In, P1, G>(s, part, buf);
                buf ^= 1;
                if (g == 0) {
                    if constexpr (MODE == PART1) {
#pragma unroll
                        for (int k = 0; k < kAcc; ++k) partial[seg * kAcc + k] = s[k];
                    } else {
                        write_result<OP, In>(out, row, s, n, ddof, root);
                    }
                }
            }
        }
    }
}

// One wave per output o: its n_seg partial sums partial[(o n_seg + s) kAcc ..] added in index order — lane l the run
// [l per, (l + 1) per) from left to right, then the butterfly.  PASS 0 of var / detrend: stats[o] = the statistic; else the result.
template<int OP, typename In, int PASS>
__global__ __launch_bounds__(kThreads) void moment_combine_kernel(const double *__restrict__ partial, double *__restrict__ stats,
                                                                  void *__restrict__ out, long long n_out, int n_seg, int n, int ddof,
                                                                  bool root) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int per = (n_seg + 63) / 64;
    for (long long o = (long long) blockIdx.x * (kThreads / 64) + w; o < n_out; o += (long long) gridDim.x * (kThreads / 64)) {
        double a[kAcc] = {0.0, 0.0, 0.0, 0.0};
        const int s1 = (lane + 1) * per < n_seg ? (lane + 1) * per : n_seg;
        for (int s = lane * per; s < s1; ++s) {
#pragma unroll
            for (int k = 0; k < kAcc; ++k)
                if (acc_used<OP, In, PASS>(k)) a[k] += partial[(o * n_seg + s) * kAcc + k];
        }
#pragma unroll
        for (int k = 0; k < kAcc; ++k)
            if (acc_used<OP, In, PASS>(k)) a[k] = wave_sum(a[k]);
        if (lane == 0) {
            if constexpr (PASS == 0 && two_pass<OP>()) {
                double st[kAcc];
                stat_of<OP, In>(a, n, st);
#pragma unroll
                for (int k = 0; k < kAcc; ++k) stats[o * kAcc + k] = st[k];
            } else {
                write_result<OP, In>(out, o, a, n, ddof, root);
            }
        }
    }
}

// inner > 1, one thread per output element (oo, ii): the whole axis, both passes
template<int OP, typename In>
__global__ __launch_bounds__(kThreads) void moment_cols_kernel(const In *__restrict__ x, const In *__restrict__ y, void *__restrict__ out,
                                                               long long outer, int n, long long inner, int ddof, bool root) {
    using Out = typename out_of<OP, In>::type;
    const long long n_out = outer * inner;
    const double tc = 0.5 * (double) (n - 1);
    for (long long o = (long long) blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += (long long) gridDim.x * blockDim.x) {
        const long long oo = o / inner, ii = o - oo * inner;
        const long long base = oo * n * inner + ii;
        double a[kAcc] = {0.0, 0.0, 0.0, 0.0}, st[kAcc] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int j = 0; j < n; ++j) {
            const long long at = base + (long long) j * inner;
            accumulate<OP, In, 0>(a, x[at], OP == K_VDOT ? y[at] : In{}, (double) j - tc, st);
        }
        if constexpr (!two_pass<OP>()) {
            write_result<OP, In>(out, o, a, n, ddof, root);
        } else {
            stat_of<OP, In>(a, n, st);
            if constexpr (is_detrend<OP>()) {
#pragma unroll 8
                for (int j = 0; j < n; ++j) {
                    const long long at = base + (long long) j * inner;
                    ((Out *) out)[at] = detrend_out<OP, In>(x[at], (double) j - tc, st);
                }
            } else {
                double s[kAcc] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
                for (int j = 0; j < n; ++j) accumulate<OP, In, 1>(s, x[base + (long long) j * inner], In{}, 0.0, st);
                write_result<OP, In>(out, o, s, n, ddof, root);
            }
        }
    }
}

// ... positions [seg seg_len, (seg + 1) seg_len) of the axis only, seg = blockIdx.y.  PASS 0: the sums to partial[(o n_seg + seg)];
// PASS 1: with stats[o], var's sum to partial or detrend's output to memory
template<int OP, typename In, int PASS>
__global__ __launch_bounds__(kThreads) void moment_cols_seg_kernel(const In *__restrict__ x, const In *__restrict__ y, void *__restrict__ out,
                                                                   double *__restrict__ partial, const double *__restrict__ stats,
                                                                   long long outer, int n, long long inner, int seg_len, int n_seg) {
    using Out = typename out_of<OP, In>::type;
    const long long n_out = outer * inner;
    const double tc = 0.5 * (double) (n - 1);
    const int seg = blockIdx.y;
    const int j0 = seg * seg_len, j1 = j0 + seg_len < n ? j0 + seg_len : n;
    for (long long o = (long long) blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += (long long) gridDim.x * blockDim.x) {
        const long long oo = o / inner, ii = o - oo * inner;
        const long long base = oo * n * inner + ii;
        double a[kAcc] = {0.0, 0.0, 0.0, 0.0}, st[kAcc] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (PASS == 1) {
#pragma unroll
            for (int k = 0; k < kAcc; ++k) st[k] = stats[o * kAcc + k];
        }
        if constexpr (PASS == 1 && is_detrend<OP>()) {
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const long long at = base + (long long) j * inner;
                ((Out *) out)[at] = detrend_out<OP, In>(x[at], (double) j - tc, st);
            }
        } else {
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const long long at = base + (long long) j * inner;
                accumulate<OP, In, PASS>(a, x[at], OP == K_VDOT ? y[at] : In{}, (double) j - tc, st);
            }
#pragma unroll
            for (int k = 0; k < kAcc; ++k) partial[(o * n_seg + seg) * kAcc + k] = a[k];
        }
    }
}

template<typename In> constexpr int tile_len_of() { return kThreads * kPacks * (16 / (int) sizeof(In)); }

template<int OP, typename In, int G, int MODE>
void launch_seg(const In *x, const In *y, void *out, double *partial, const double *stats, long long n_seg, int n, int tile_len,
                int tiles_per_row, int ddof, bool root, hipStream_t s) {
    constexpr int VP = 16 / (int) sizeof(In);
    const bool packs = VP > 1 && n % VP == 0 && tile_len % VP == 0 && aligned_to(x, 16) && (y == nullptr || aligned_to(y, 16)) &&
                       (!is_detrend<OP>() || aligned_to(out, 16));
    const long long groups = (n_seg + kThreads / G - 1) / (kThreads / G), cap = (long long) dsc_cu_count() * 8;
    const dim3 grid((unsigned) (groups < cap ? groups : cap));
    with_bool(packs, [&](auto pk) {
        DSC_LAUNCH((moment_seg_kernel<OP, In, decltype(pk)::value ? VP : 1, G, MODE>), grid, dim3(kThreads), 0, s, x, y, out, partial, stats,
                   n_seg, n, tile_len, tiles_per_row, ddof, root);
    });
}

template<int OP, typename In, int PASS>
void launch_combine(const double *partial, double *stats, void *out, long long n_out, int n_seg, int n, int ddof, bool root, hipStream_t s) {
    long long blocks = (n_out + kThreads / 64 - 1) / (kThreads / 64);
    if (blocks > 256 * 8) blocks = 256 * 8;
    DSC_LAUNCH((moment_combine_kernel<OP, In, PASS>), dim3((unsigned) blocks), dim3(kThreads), 0, s, partial, stats, out, n_out, n_seg, n,
               ddof, root);
}

// (operator code, dtype) -> (OP, In)
template<typename F> void with_moment_types(int op, int dtype, F f) {
    with_index<5>("moments.hip", "operator", op, [&](auto opc) { with_dtype(dtype, [&](auto in) { f(opc, in); }); });
}

}  // namespace

int dsc_moment_tile_len(int dtype) {
    int len = 0;
    with_dtype(dtype, [&](auto in) { len = tile_len_of<decltype(in)>(); });
    return len;
}

size_t dsc_moment_scratch_bytes(long long n_out, long long n_seg) {
    return scratch_block_bytes(n_out * n_seg, kAcc * sizeof(double)) + scratch_block_bytes(n_out, kAcc * sizeof(double));
}

void dsc_launch_moment_rows(const void *x, const void *y, void *out, int op, int dtype, long long rows, int n, int ddof, bool root,
                            hipStream_t stream) {
    if (rows <= 0 || n <= 0) return;
    with_moment_types(op, dtype, [&](auto opc, auto in) {
        constexpr int OP = decltype(opc)::value;
        using In = decltype(in);
        // many rows that fit a wave's registers: a wave per row, no barrier
        if (rows >= 1024 && n <= tile_len_of<In>() / (kThreads / 64))
            launch_seg<OP, In, 64, FUSED>((const In *) x, (const In *) y, out, nullptr, nullptr, rows, n, n, 1, ddof, root, stream);
        else
            launch_seg<OP, In, kThreads, FUSED>((const In *) x, (const In *) y, out, nullptr, nullptr, rows, n, n, 1, ddof, root, stream);
    });
}

void dsc_launch_moment_tiles(const void *x, const void *y, void *out, int op, int dtype, long long rows, int n, int ddof, bool root,
                             void *scratch, hipStream_t stream) {
    if (rows <= 0 || n <= 0) return;
    with_moment_types(op, dtype, [&](auto opc, auto in) {
        constexpr int OP = decltype(opc)::value;
        using In = decltype(in);
        constexpr int tile_len = tile_len_of<In>();
        const int tiles_per_row = (n + tile_len - 1) / tile_len;
        const long long n_seg = rows * tiles_per_row;
        double *partial = (double *) scratch, *stats = (double *) ((char *) scratch + scratch_block_bytes(n_seg, kAcc * sizeof(double)));
        const In *xp = (const In *) x, *yp = (const In *) y;
        launch_seg<OP, In, kThreads, PART0>(xp, yp, out, partial, nullptr, n_seg, n, tile_len, tiles_per_row, ddof, root, stream);
        launch_combine<OP, In, 0>(partial, stats, out, rows, tiles_per_row, n, ddof, root, stream);
        if constexpr (two_pass<OP>()) {
            launch_seg<OP, In, kThreads, PART1>(xp, yp, out, partial, stats, n_seg, n, tile_len, tiles_per_row, ddof, root, stream);
            if constexpr (!is_detrend<OP>()) launch_combine<OP, In, 1>(partial, stats, out, rows, tiles_per_row, n, ddof, root, stream);
        }
    });
}

int dsc_moment_cols_segments(long long n_out, int n, size_t scratch_bytes) {
    // one thread per output fills the chip from 65536 outputs on; below that, segments of at least 32 positions
    if (n_out >= 256 * 256 || n < 128) return 1;
    long long n_seg = (512 * 256 + n_out - 1) / n_out;
    if (n_seg > n / 32) n_seg = n / 32;
    if (n_seg > 4096) n_seg = 4096;                 // grid.y
    while (n_seg >= 2 && dsc_moment_scratch_bytes(n_out, n_seg) > scratch_bytes) n_seg /= 2;
    if (n_seg < 2) return 1;
    const int seg_len = (int) ((n + n_seg - 1) / n_seg);
    return (n + seg_len - 1) / seg_len;
}

void dsc_launch_moment_cols(const void *x, const void *y, void *out, int op, int dtype, long long outer, int n, long long inner, int ddof,
                            bool root, int n_seg, void *scratch, hipStream_t stream) {
    const long long n_out = outer * inner;
    if (n_out <= 0 || n <= 0) return;
    with_moment_types(op, dtype, [&](auto opc, auto in) {
        constexpr int OP = decltype(opc)::value;
        using In = decltype(in);
        const In *xp = (const In *) x, *yp = (const In *) y;
        if (n_seg < 2) {
            DSC_LAUNCH((moment_cols_kernel<OP, In>), stream_grid(n_out), dim3(kThreads), 0, stream, xp, yp, out, outer, n, inner, ddof, root);
            return;
        }
        const int seg_len = (n + n_seg - 1) / n_seg;
        double *partial = (double *) scratch, *stats = (double *) ((char *) scratch + scratch_block_bytes(n_out * n_seg, kAcc * sizeof(double)));
        const dim3 grid((unsigned) ((n_out + kThreads - 1) / kThreads), (unsigned) n_seg);
        DSC_LAUNCH((moment_cols_seg_kernel<OP, In, 0>), grid, dim3(kThreads), 0, stream, xp, yp, out, partial, (const double *) nullptr,
                   outer, n, inner, seg_len, n_seg);
        launch_combine<OP, In, 0>(partial, stats, out, n_out, n_seg, n, ddof, root, stream);
        if constexpr (two_pass<OP>()) {
            DSC_LAUNCH((moment_cols_seg_kernel<OP, In, 1>), grid, dim3(kThreads), 0, stream, xp, yp, out, partial, (const double *) stats,
                       outer, n, inner, seg_len, n_seg);
            if constexpr (!is_detrend<OP>()) launch_combine<OP, In, 1>(partial, stats, out, n_out, n_seg, n, ddof, root, stream);
        }
    });
}
