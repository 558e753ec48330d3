// scan.hip — prefix scans along one axis: cumsum, unwrap, phase (= unwrap of angle, fused) and the element-wise diff
// (include/dsc_mi355x.h, Section I; host side scan.cpp).  The tensor is viewed as [outer][n][inner], as reduce.hip views it.
//
// What is scanned is the element itself (cumsum: f32 / f64, complex component-wise) or the int32 count m of whole periods between a
// sample and the one before it (unwrap / phase).  The counts make unwrap independent of the order of the scan: K[j] = m[1] + .. + m[j]
// is an exact integer on every route, and out[j] = x[j] - K[j] 2 pi is formed from it in one place (unwrap_out).
//
//   inner == 1   scan_seg_kernel.  A 1024-thread workgroup walks a SEGMENT of a row in chunks of 1024 x U packs of 16 bytes: the
//                thread scans its packs in registers, the wave scans the pack totals with __shfl_up, the 16 wave totals go through
//                LDS (one barrier per chunk, two buffers), and the running value of the segment stays in a register.  The loads of
//                the next chunk — across the end of a segment too — are issued before the current chunk is scanned.  The grid is
//                persistent over the segments.  Three uses of the one kernel:
//                  scan_rows    segment = whole row, one launch, one HBM round trip
//                  scan_tiles   segment = tile of one chunk: (1) TOTALS: the tile's total to scratch, nothing else stored; (2) the
//                               totals of each row scanned by the rows form of the kernel; (3) the tiles scanned with their carry-in.
//                               Plain launches in stream order: no workgroup waits on another.
//                Rows whose length or address rules out 16-byte packs take the same kernel with one element per pack.
//   inner > 1    scan_cols_kernel: one thread per (outer, inner) element walks the axis; neighbouring threads read neighbouring
//                addresses.  cumsum in numpy's own left-to-right order.  The axis is not segmented: few columns are slow.
//   diff         scan_diff_kernel: out[o][j][i] = x[o][j + 1][i] - x[o][j][i], flat over the output.
#include "stream_common.h"

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr double kTwoPi = 6.283185307179586, kPi = 3.141592653589793;


template<typename S> struct is_cx : std::false_type {};
template<typename T> struct is_cx<cx<T>> : std::true_type {};

// OP: 0 cumsum, 1 unwrap, 2 phase.  In: the element read; S: what is scanned; Out: the element written; R: the real type of Out
template<int OP, typename In> struct scan_types { using S = In; using Out = In; };
template<typename In> struct scan_types<1, In> { using S = int; using Out = In; };
template<typename In> struct scan_types<2, In> { using S = int; using Out = decltype(In{}.x); };
// phase recomputes one atan2 per wave and chunk: longer chunks, where the registers allow (the f64 atan2 needs most of them)
template<int OP, typename In> constexpr int packs_per_thread() { return OP == 2 && sizeof(In) == 8 ? 4 : 2; }

// the identity is -0: -0 + x = x for every x, so element 0 of a cumsum is a bit-for-bit copy
template<typename S> __device__ __forceinline__ S s_zero() {
    if constexpr (is_cx<S>::value) { using T = decltype(S{}.x); return S{(T) -0.0, (T) -0.0}; }
    else return (S) -0.0;
}
template<typename S> __device__ __forceinline__ S s_add(S a, S b) {
    if constexpr (is_cx<S>::value) return S{a.x + b.x, a.y + b.y};
    else return a + b;
}
template<typename S> __device__ __forceinline__ S s_sub(S a, S b) {
    if constexpr (is_cx<S>::value) return S{a.x - b.x, a.y - b.y};
    else return a - b;
}
template<typename S> __device__ __forceinline__ S s_shfl_up(S v, int d) {
    if constexpr (is_cx<S>::value) return S{__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)};
    else return __shfl_up(v, d, 64);
}
template<typename S> __device__ __forceinline__ S s_shfl(S v, int lane) {
    if constexpr (is_cx<S>::value) return S{__shfl(v.x, lane, 64), __shfl(v.y, lane, 64)};
    else return __shfl(v, lane, 64);
}

// the sample unwrap works on: x itself, or for phase the angle exactly as dsc_angle's functor forms it (elementwise.hip)
template<int OP, typename In>
__device__ __forceinline__ typename scan_types<OP, In>::Out sample_of(In v) {
    if constexpr (OP == 2) { using R = decltype(In{}.x); const R re = v.x, im = v.y; return atan2(im, re); }
    else return v;
}

// m of the header: whole periods between a sample and its predecessor; 0 for a step of at most pi and for one that is not finite
__device__ __forceinline__ int wrap_step(double cur, double prev) {
    const double d = cur - prev, ad = fabs(d);
    if (!(ad > kPi) || !(ad < (double) INFINITY)) return 0;
    const double q = d / kTwoPi;
    double r = q > 0 ? ceil(q - 0.5) : floor(q + 0.5);                 // nearest, ties toward zero
    r = fmin(fmax(r, -2147483647.0), 2147483647.0);
    return (int) r;
}

// out = x - K 2 pi in double, rounded once; K = 0 is a copy
template<typename R> __device__ __forceinline__ R unwrap_out(R a, int K) {
    if (K == 0) return a;
    return (R) fma(-(double) K, kTwoPi, (double) a);
}

template<typename In, int V, int U> struct chunk_regs { packed<In, V> p[U]; In halo; };

// the calling thread's packs of the chunk that starts at position j0 of the row xrow; positions from jend on do not belong to the
// segment.  Pack u of lane l of wave w is pack (w U + u) 64 + l of the chunk: a wave owns U 64 consecutive packs.
template<int OP, typename In, int V, int U>
__device__ __forceinline__ void load_chunk(const In *__restrict__ xrow, long long j0, long long jend, chunk_regs<In, V, U> &r) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long j = j0 + (long long) (((w * U + u) * 64 + lane) * V);
        if (j < jend) {
            r.p[u] = *(const packed<In, V> *) (xrow + j);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) r.p[u].e[k] = s_zero<In>();
        }
    }
    r.halo = s_zero<In>();
    if (OP != 0 && lane == 0) {                                          // the sample in front of the wave's first one
        const long long j = j0 + (long long) (w * U * 64 * V);
        if (j > 0 && j < jend) r.halo = xrow[j - 1];
    }
}

struct seg_geom { long long row, start, end; };
__device__ __forceinline__ seg_geom geom_of(long long seg, int n, int tile_len, int tiles_per_row) {
    const long long row = seg / tiles_per_row, t = seg - row * tiles_per_row;
    const long long start = t * tile_len, end = start + tile_len < n ? start + tile_len : n;
    return {row, start, end};
}
template<typename S>
__device__ __forceinline__ S carry_of(const S *__restrict__ carry_in, long long seg, int tiles_per_row) {
    return carry_in != nullptr && seg % tiles_per_row != 0 ? carry_in[seg - 1] : s_zero<S>();
}

// Segment `seg` is positions [t tile_len, min((t + 1) tile_len, n)) of row seg / tiles_per_row, t = seg % tiles_per_row; its scan
// starts from carry_in[seg - 1] (t > 0, carry_in given) or from the identity.  TOTALS: nothing is stored but totals[seg] = the
// segment's last scanned value.  V > 1: n, tile_len and both base addresses are multiples of a pack.
template<int OP, typename In, int V, bool TOTALS>
__global__ __launch_bounds__(kThreads) void scan_seg_kernel(const In *__restrict__ x, typename scan_types<OP, In>::Out *__restrict__ out,
                                                            const typename scan_types<OP, In>::S *__restrict__ carry_in,
                                                            typename scan_types<OP, In>::S *__restrict__ totals, long long n_seg, int n,
                                                            int tile_len, int tiles_per_row) {
    using S = typename scan_types<OP, In>::S;
    using Out = typename scan_types<OP, In>::Out;
    constexpr int U = packs_per_thread<OP, In>(), CH = kThreads * U * V;
    __shared__ S wave_total[2][kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;

    long long seg = blockIdx.x;
    if (seg >= n_seg) return;
    int c = 0, buf = 0;
    seg_geom g = geom_of(seg, n, tile_len, tiles_per_row);
    chunk_regs<In, V, U> cur, nxt;
    load_chunk<OP, In, V, U>(x + g.row * n, g.start, g.end, cur);
    S carry = carry_of<S>(carry_in, seg, tiles_per_row);

    for (;;) {
        // where the workgroup goes next, and that chunk's loads
        long long seg_n = seg;
        int c_n = c + 1;
        seg_geom g_n = g;
        if (g.start + (long long) c_n * CH >= g.end) {
            seg_n = seg + gridDim.x;
            c_n = 0;
            if (seg_n < n_seg) g_n = geom_of(seg_n, n, tile_len, tiles_per_row);
        }
        const bool has_next = seg_n < n_seg;
        S carry_n = s_zero<S>();
        if (has_next) {
            load_chunk<OP, In, V, U>(x + g_n.row * n, g_n.start + (long long) c_n * CH, g_n.end, nxt);
            if (c_n == 0) carry_n = carry_of<S>(carry_in, seg_n, tiles_per_row);
        }

        // the values to scan
        const long long j0 = g.start + (long long) c * CH;
        long long j[U];
        S p[U][V];
        Out a[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) j[u] = j0 + (long long) (((w * U + u) * 64 + lane) * V);
        if constexpr (OP == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < V; ++k) p[u][k] = cur.p[u].e[k];
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < V; ++k) a[u][k] = sample_of<OP, In>(cur.p[u].e[k]);
            const Out halo = sample_of<OP, In>(cur.halo);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Out prev = __shfl_up(a[u][V - 1], 1, 64);
                const Out wave_prev = u == 0 ? halo : __shfl(a[u == 0 ? 0 : u - 1][V - 1], 63, 64);
                if (lane == 0) prev = wave_prev;
                const bool valid = j[u] < g.end;
                p[u][0] = valid && j[u] > 0 ? wrap_step((double) a[u][0], (double) prev) : 0;
#pragma unroll
                for (int k = 1; k < V; ++k) p[u][k] = valid ? wrap_step((double) a[u][k], (double) a[u][k - 1]) : 0;
            }
        }

        // thread: inclusive over each pack.  wave: inclusive over the pack totals, then over the wave's U groups of 64 packs
        S excl[U], run[U];
        S wave_sum = s_zero<S>();
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 1; k < V; ++k) p[u][k] = s_add(p[u][k - 1], p[u][k]);
            S incl = p[u][V - 1];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const S below = s_shfl_up(incl, d);
                if (lane >= d) incl = s_add(below, incl);
            }
            excl[u] = s_shfl_up(incl, 1);
            if (lane == 0) excl[u] = s_zero<S>();
            run[u] = wave_sum;
            wave_sum = s_add(wave_sum, s_shfl(incl, 63));
        }
        if (lane == 0) wave_total[buf][w] = wave_sum;
        __syncthreads();                                                 // the only barrier of the chunk: wave_total has two buffers
        S before = carry, upto = carry;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) {
            if (v == w) before = upto;
            upto = s_add(upto, wave_total[buf][v]);
        }
        carry = upto;                                                    // the same sum in every thread

        if constexpr (!TOTALS) {
            Out *orow = out + g.row * n;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j[u] < g.end) {
                    const S base = s_add(s_add(before, run[u]), excl[u]);
                    packed<Out, V> o;
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const S sc = s_add(base, p[u][k]);
                        if constexpr (OP == 0) o.e[k] = sc;
                        else                   o.e[k] = unwrap_out<Out>(a[u][k], sc);
                    }
                    *(packed<Out, V> *) (orow + j[u]) = o;
                }
            }
        } else {
            if (seg_n != seg && threadIdx.x == 0) totals[seg] = carry;
        }

        if (!has_next) break;
        cur = nxt;
        if (c_n == 0) carry = carry_n;
        seg = seg_n;
        c = c_n;
        g = g_n;
        buf ^= 1;
    }
}

template<int OP, typename In>
__global__ void scan_cols_kernel(const In *__restrict__ x, typename scan_types<OP, In>::Out *__restrict__ out, long long outer, int n,
                                 long long inner) {
    using Out = typename scan_types<OP, In>::Out;
    const long long n_thr = outer * inner;
    for (long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x; t < n_thr; t += (long long) gridDim.x * blockDim.x) {
        const long long oo = t / inner, ii = t - oo * inner;
        const long long base = oo * n * inner + ii;
        if constexpr (OP == 0) {
            In acc = x[base];
            out[base] = acc;
#pragma unroll 8
            for (int j = 1; j < n; ++j) {
                acc = s_add(acc, x[base + (long long) j * inner]);
                out[base + (long long) j * inner] = acc;
            }
        } else {
            Out prev = sample_of<OP, In>(x[base]);
            out[base] = prev;
            int K = 0;
#pragma unroll 4
            for (int j = 1; j < n; ++j) {
                const Out a = sample_of<OP, In>(x[base + (long long) j * inner]);
                K += wrap_step((double) a, (double) prev);
                out[base + (long long) j * inner] = unwrap_out<Out>(a, K);
                prev = a;
            }
        }
    }
}

// pack p = outputs [p V, p V + V) of the flat output [outer][n - 1][inner]; row_len = (n - 1) inner.  V > 1: inner is a multiple of V
template<typename E, int V>
__global__ void scan_diff_kernel(const E *__restrict__ x, E *__restrict__ out, unsigned n_packs, unsigned row_len, unsigned inner) {
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < n_packs; p += gridDim.x * blockDim.x) {
        const unsigned o = p * V, q = o / row_len;
        const long long i = (long long) o + (long long) q * inner;
        const packed<E, V> lo = *(const packed<E, V> *) (x + i), hi = *(const packed<E, V> *) (x + i + inner);
        packed<E, V> r;
#pragma unroll
        for (int k = 0; k < V; ++k) r.e[k] = s_sub(hi.e[k], lo.e[k]);
        *(packed<E, V> *) (out + o) = r;
    }
}

template<int OP, typename In, bool TOTALS>
void launch_seg(const In *x, typename scan_types<OP, In>::Out *out, const typename scan_types<OP, In>::S *carry_in,
                typename scan_types<OP, In>::S *totals, long long n_seg, int n, int tile_len, int tiles_per_row, hipStream_t s) {
    using Out = typename scan_types<OP, In>::Out;
    constexpr int VP = 16 / (int) sizeof(In);
    const bool packs = VP > 1 && n % VP == 0 && tile_len % VP == 0 && aligned_to(x, 16) && aligned_to(out, sizeof(Out) * VP);
    const long long cus = dsc_cu_count();
    const dim3 grid((unsigned) (n_seg < cus ? n_seg : cus));
    with_bool(packs, [&](auto pk) {
        DSC_LAUNCH((scan_seg_kernel<OP, In, decltype(pk)::value ? VP : 1, TOTALS>), grid, dim3(kThreads), 0, s, x, out, carry_in, totals, n_seg, n, tile_len, tiles_per_row);
    });
}

template<int OP, typename In> constexpr int tile_len_of() { return kThreads * packs_per_thread<OP, In>() * (16 / (int) sizeof(In)); }

// (op, dtype of the input) -> (OP, In); the gate of the host side keeps every other pair away
template<typename F> void with_scan_types(int op, int dtype, F f) {
    if (op == 0 && dtype == 0) return f(int_c<0>{}, float{});
    if (op == 0 && dtype == 1) return f(int_c<0>{}, double{});
    if (op == 0 && dtype == 2) return f(int_c<0>{}, cx<float>{});
    if (op == 0 && dtype == 3) return f(int_c<0>{}, cx<double>{});
    if (op == 1 && dtype == 0) return f(int_c<1>{}, float{});
    if (op == 1 && dtype == 1) return f(int_c<1>{}, double{});
    if (op == 2 && dtype == 2) return f(int_c<2>{}, cx<float>{});
    if (op == 2 && dtype == 3) return f(int_c<2>{}, cx<double>{});
    no_kernel("scan.hip", "operator and dtype", op * 10 + dtype);
}

}  // namespace

int dsc_scan_tile_len(int op, int dtype) {
    int len = 0;
    with_scan_types(op, dtype, [&](auto opc, auto in) { len = tile_len_of<decltype(opc)::value, decltype(in)>(); });
    return len;
}

size_t dsc_scan_tiles_scratch_bytes(int op, int dtype, long long rows, int n) {
    const int tile_len = dsc_scan_tile_len(op, dtype);
    const long long n_seg = rows * ((n + tile_len - 1) / tile_len);
    return 2 * scratch_block_bytes(n_seg, 16);
}

void dsc_launch_scan_rows(const void *x, void *out, int op, int dtype, long long rows, int n, hipStream_t stream) {
    if (rows <= 0 || n <= 0) return;
    with_scan_types(op, dtype, [&](auto opc, auto in) {
        constexpr int OP = decltype(opc)::value;
        using In = decltype(in);
        launch_seg<OP, In, false>((const In *) x, (typename scan_types<OP, In>::Out *) out, nullptr, nullptr, rows, n, n, 1, stream);
    });
}

void dsc_launch_scan_tiles(const void *x, void *out, int op, int dtype, long long rows, int n, void *scratch, hipStream_t stream) {
    if (rows <= 0 || n <= 0) return;
    with_scan_types(op, dtype, [&](auto opc, auto in) {
        constexpr int OP = decltype(opc)::value;
        using In = decltype(in);
        using S = typename scan_types<OP, In>::S;
        constexpr int tile_len = tile_len_of<OP, In>();
        const int tiles_per_row = (n + tile_len - 1) / tile_len;
        const long long n_seg = rows * tiles_per_row;
        S *totals = (S *) scratch, *scanned = (S *) ((char *) scratch + scratch_block_bytes(n_seg, 16));
        launch_seg<OP, In, true>((const In *) x, nullptr, nullptr, totals, n_seg, n, tile_len, tiles_per_row, stream);
        launch_seg<0, S, false>(totals, scanned, nullptr, nullptr, rows, tiles_per_row, tiles_per_row, 1, stream);
        launch_seg<OP, In, false>((const In *) x, (typename scan_types<OP, In>::Out *) out, scanned, nullptr, n_seg, n, tile_len, tiles_per_row, stream);
    });
}

void dsc_launch_scan_cols(const void *x, void *out, int op, int dtype, long long outer, int n, long long inner, hipStream_t stream) {
    if (outer * inner <= 0 || n <= 0) return;
    with_scan_types(op, dtype, [&](auto opc, auto in) {
        constexpr int OP = decltype(opc)::value;
        using In = decltype(in);
        long long blocks = (outer * inner + 255) / 256;
        if (blocks > 256 * 16) blocks = 256 * 16;
        DSC_LAUNCH((scan_cols_kernel<OP, In>), dim3((unsigned) blocks), dim3(256), 0, stream, (const In *) x,
                   (typename scan_types<OP, In>::Out *) out, outer, n, inner);
    });
}

void dsc_launch_scan_diff(const void *x, void *out, int dtype, long long outer, int n, long long inner, hipStream_t stream) {
    const long long n_out = outer * (n - 1) * inner;
    if (n_out <= 0) return;
    with_scan_types(0, dtype, [&](auto, auto in) {
        using E = decltype(in);
        constexpr int VP = 16 / (int) sizeof(E);
        const bool packs = VP > 1 && inner % VP == 0 && aligned_to(x, 16) && aligned_to(out, 16);
        const long long n_packs = packs ? n_out / VP : n_out;
        long long blocks = (n_packs + 255) / 256;
        if (blocks > 256 * 32) blocks = 256 * 32;
        const unsigned row_len = (unsigned) ((n - 1) * inner);
        with_bool(packs, [&](auto pk) {
            DSC_LAUNCH((scan_diff_kernel<E, decltype(pk)::value ? VP : 1>), dim3((unsigned) blocks), dim3(256), 0, stream, (const E *) x, (E *) out, (unsigned) n_packs, row_len, (unsigned) inner);
        });
    });
}
