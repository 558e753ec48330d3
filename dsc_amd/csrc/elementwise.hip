// elementwise.hip — the HBM-bound streaming kernels that compute per element: dtype cast, the broadcast binary operators (add, sub,
// mul, div, pow; operands of one dtype or of two, promoted in registers), the unary functions (abs .. clip) and arange.
// The kernels that only move elements (slices, transposes) are in layout.hip.
//
// Reference: dsc_cast (dsc/src/dsc.cpp:536-597, cast_op dsc/include/dsc_ops.h:12-44) and
// binary_op (dsc/src/dsc.cpp:1186-1245) with mul_op & co. (dsc_ops.h:46-90).  The reference
// walks two dsc_broadcast_iterators per element (dsc_iter.h:67-95); here the output's flat
// index is decomposed once per element and each operand offset is a dot product with its
// broadcast strides (0 on broadcast dims), so equal-shape, row-broadcast and scalar operands
// all stream at the same rate.
#include "stream_common.h"

namespace {

// Grid of the PACKED kernels (16 bytes per thread in their widest stream): one pack per thread, no loop in practice —
// workgroups are dispatched in address order and end right after their store, so the whole chip sweeps one window of memory:
// 6.2 TB/s for a copy against 4.7 TB/s for 2048 grid-striding workgroups (tools/membench2.hip; mul c32 of equal shapes
// 62.8 -> 81.4 % of the roofline).  With 4 or 8 bytes per thread the same launch is SLOWER than the capped grid (measured:
// abs c32 69.5 -> 66 %, cast f32 -> c32 67.7 -> 55.8 %), hence the packs.  2^23 blocks keep the 32-bit strides at <= 2^31.
inline dim3 pack_grid(long long npack) {
    long long blocks = (npack + 255) / 256;
#ifdef DSC_STREAM_GRID_CAPPED
    if (blocks > 256 * 8) blocks = 256 * 8;
#endif
    if (blocks > (1 << 23)) blocks = 1 << 23;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned) blocks);
}

template<typename A, typename B> constexpr int pack_width() { return 16 / (int) (sizeof(A) > sizeof(B) ? sizeof(A) : sizeof(B)); }

// cast_op (dsc_ops.h:12-44): complex -> real keeps .real; real -> complex sets imag = 0
template<typename Tin, typename Tout>
__device__ __forceinline__ Tout cast_one(Tin v) {
    using Rout = typename elem<Tout>::real;
    if constexpr (elem<Tout>::cplx) {
        if constexpr (elem<Tin>::cplx) return Tout{(Rout) v.x, (Rout) v.y};
        else                           return Tout{(Rout) v, (Rout) 0};
    } else {
        if constexpr (elem<Tin>::cplx) return (Rout) v.x;
        else                           return (Rout) v;
    }
}

template<typename Tin, typename Tout>
__global__ void cast_kernel(const Tin *in, Tout *out, long long ne) {
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (long long) gridDim.x * blockDim.x)
        out[i] = cast_one<Tin, Tout>(in[i]);
}

// V consecutive elements per thread, 16 bytes in the wider of the two streams
template<typename Tin, typename Tout, int V>
__global__ void cast_pack_kernel(const Tin *in, Tout *out, unsigned npack) {
    const packed<Tin, V> *pi = (const packed<Tin, V> *) in;
    packed<Tout, V> *po = (packed<Tout, V> *) out;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npack; i += gridDim.x * blockDim.x) {
        const packed<Tin, V> x = pi[i];
        packed<Tout, V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) r.e[j] = cast_one<Tin, Tout>(x.e[j]);
        po[i] = r;
    }
}

template<typename Tin, typename Tout>
void cast_to(const Tin *x, Tout *out, long long ne, hipStream_t s) {
    constexpr int V = pack_width<Tin, Tout>();
    long long done = 0;
    if (ne >= V && aligned_to(x, sizeof(Tin) * V) && aligned_to(out, sizeof(Tout) * V)) {
        const long long npack = ne / V;
        DSC_LAUNCH((cast_pack_kernel<Tin, Tout, V>), pack_grid(npack), dim3(256), 0, s, x, out, (unsigned) npack);
        done = npack * V;
    }
    if (done < ne) DSC_LAUNCH((cast_kernel<Tin, Tout>), stream_grid(ne - done), dim3(256), 0, s, x + done, out + done, ne - done);
}

// ---- transcendental functions of dsc_ops.h:92-229, generic over the four element types.  Real parts go to ocml's ACCURATE
// functions (sinf / sin, expf / exp, ...; never the __sinf-style intrinsics); complex values use the reference's own formulas
// (cos z = (cos a cosh b, -sin a sinh b), ...), not std::complex or ocml's complex functions.
__device__ __forceinline__ float  m_sin(float x)             { return sinf(x); }
__device__ __forceinline__ double m_sin(double x)            { return sin(x); }
__device__ __forceinline__ float  m_cos(float x)             { return cosf(x); }
__device__ __forceinline__ double m_cos(double x)            { return cos(x); }
__device__ __forceinline__ float  m_sinh(float x)            { return sinhf(x); }
__device__ __forceinline__ double m_sinh(double x)           { return sinh(x); }
__device__ __forceinline__ float  m_cosh(float x)            { return coshf(x); }
__device__ __forceinline__ double m_cosh(double x)           { return cosh(x); }
__device__ __forceinline__ float  m_exp(float x)             { return expf(x); }
__device__ __forceinline__ double m_exp(double x)            { return exp(x); }
__device__ __forceinline__ float  m_log(float x)             { return logf(x); }
__device__ __forceinline__ double m_log(double x)            { return log(x); }
__device__ __forceinline__ float  m_log2(float x)            { return log2f(x); }
__device__ __forceinline__ double m_log2(double x)           { return log2(x); }
__device__ __forceinline__ float  m_log10(float x)           { return log10f(x); }
__device__ __forceinline__ double m_log10(double x)          { return log10(x); }
__device__ __forceinline__ float  m_sqrt(float x)            { return sqrtf(x); }
__device__ __forceinline__ double m_sqrt(double x)           { return sqrt(x); }
__device__ __forceinline__ float  m_atan2(float y, float x)  { return atan2f(y, x); }
__device__ __forceinline__ double m_atan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float  m_pow(float a, float b)    { return powf(a, b); }
__device__ __forceinline__ double m_pow(double a, double b)  { return pow(a, b); }

// exp_op (dsc_ops.h:211-227)
template<typename T>
__device__ __forceinline__ T t_exp(T v) {
    if constexpr (elem<T>::cplx) {
        const auto f = m_exp(v.x);
        return T{f * m_cos(v.y), f * m_sin(v.y)};
    } else {
        return m_exp(v);
    }
}

// logn_op / log2_op / log10_op (dsc_ops.h:144-191), BASE 0 = e: complex log = (log_B sqrt(re^2 + im^2), atan2(im, re) / ln B);
// the factor is the reference's 1 / log(B) rounded to the real type
template<typename T, int BASE>
__device__ __forceinline__ T t_log(T v) {
    using R = typename elem<T>::real;
    auto lg = [](R x) { return BASE == 0 ? m_log(x) : BASE == 2 ? m_log2(x) : m_log10(x); };
    if constexpr (elem<T>::cplx) {
        const R fact = BASE == 0 ? (R) 1 : BASE == 2 ? (R) 1 / (R) 0.693147180559945309417232121458176568
                                                      : (R) 1 / (R) 2.302585092994045684017991454684364208;
        const R phase = m_atan2(v.y, v.x);
        return T{lg(m_sqrt((v.x * v.x) + (v.y * v.y))), BASE == 0 ? phase : fact * phase};
    } else {
        return lg(v);
    }
}

// add_op / sub_op / mul_op / div_op: dsc_ops.h:46-90; OP 4 = pow_op (dsc_ops.h:305-316): pow / powf on reals,
// exp(b * log a) on complex values — the reference's own composition of exp_op, mul_op and logn_op
template<typename T, int OP>
__device__ __forceinline__ T apply(T a, T b) {
    if constexpr (elem<T>::cplx) {
        if constexpr (OP == 0) return T{a.x + b.x, a.y + b.y};
        else if constexpr (OP == 1) return T{a.x - b.x, a.y - b.y};
        else if constexpr (OP == 2) return T{(a.x * b.x) - (a.y * b.y), (a.x * b.y) + (a.y * b.x)};
        else if constexpr (OP == 3) {
            const auto den = (b.x * b.x) + (b.y * b.y);
            return T{((a.x * b.x) + (a.y * b.y)) / den, ((a.y * b.x) - (a.x * b.y)) / den};
        } else {
            return t_exp(apply<T, 2>(b, t_log<T, 0>(a)));
        }
    } else {
        if constexpr (OP == 0) return a + b;
        else if constexpr (OP == 1) return a - b;
        else if constexpr (OP == 2) return a * b;
        else if constexpr (OP == 3) return a / b;
        else return m_pow(a, b);
    }
}

// fast index paths: tensors have at most 2^31 - 1 elements (int ne), so 32-bit arithmetic suffices
template<typename T, int OP, int FAST>
__global__ void binary_fast_kernel(const T *a, const T *b, T *out, unsigned ne, unsigned small_ne) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += gridDim.x * blockDim.x) {
        const unsigned ia = FAST == 3 ? i % small_ne : i;
        const unsigned ib = FAST == 2 ? i % small_ne : i;
        out[i] = apply<T, OP>(a[ia], b[ib]);
    }
}

template<typename T, int OP>
__global__ void binary_kernel(const T *a, const T *b, T *out, const dsc_bcast_args g) {
    const long long s3 = g.out_shape[3];
    const long long s23 = s3 * g.out_shape[2];
    const long long s123 = s23 * g.out_shape[1];
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < g.ne; i += (long long) gridDim.x * blockDim.x) {
        long long ia, ib;
        if (g.a_scalar)      { ia = 0; ib = i; }
        else if (g.b_scalar) { ia = i; ib = 0; }
        else {
            const long long i0 = i / s123, r0 = i - i0 * s123;
            const long long i1 = r0 / s23, r1 = r0 - i1 * s23;
            const long long i2 = r1 / s3, i3 = r1 - i2 * s3;
            ia = i0 * g.a_stride[0] + i1 * g.a_stride[1] + i2 * g.a_stride[2] + i3 * g.a_stride[3];
            ib = i0 * g.b_stride[0] + i1 * g.b_stride[1] + i2 * g.b_stride[2] + i3 * g.b_stride[3];
        }
        out[i] = apply<T, OP>(a[ia], b[ib]);
    }
}

// general broadcast with a long innermost axis: a block owns a piece of one innermost row of the RESULT — one division chain per
// block instead of one per element; along the row each operand advances by its own stride (1, or 0 where it is broadcast)
template<typename T, int OP>
__global__ void binary_rows_kernel(const T *a, const T *b, T *out, const dsc_bcast_args g, unsigned chunks_per_row) {
    const unsigned long long blk = blockIdx.x;
    const unsigned long long row = blk / chunks_per_row;
    const unsigned chunk = (unsigned) (blk - row * chunks_per_row);
    const unsigned long long i01 = row / (unsigned) g.out_shape[2];
    const long long i2 = (long long) (row - i01 * (unsigned) g.out_shape[2]);
    const long long i0 = (long long) (i01 / (unsigned) g.out_shape[1]), i1 = (long long) (i01 - (unsigned long long) i0 * (unsigned) g.out_shape[1]);
    const T *pa = a + (i0 * g.a_stride[0] + i1 * g.a_stride[1] + i2 * g.a_stride[2]);
    const T *pb = b + (i0 * g.b_stride[0] + i1 * g.b_stride[1] + i2 * g.b_stride[2]);
    T *po = out + (long long) row * g.out_shape[3];
    const long long sa = g.a_stride[3], sb = g.b_stride[3];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = chunk * 1024 + u * 256 + threadIdx.x;
        if (c >= g.out_shape[3]) return;
        po[c] = apply<T, OP>(pa[c * sa], pb[c * sb]);
    }
}

// equal shapes: 16 bytes per lane and operand (V = 16 / sizeof(T) elements), the widest global access
template<typename T, int OP>
__global__ void binary_same_vec_kernel(const T *a, const T *b, T *out, unsigned nvec) {
    constexpr int V = 16 / sizeof(T);
    struct alignas(16) pack { T e[V]; };
    const pack *pa = (const pack *) a, *pb = (const pack *) b;
    pack *po = (pack *) out;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += gridDim.x * blockDim.x) {
        typedef unsigned int u4v __attribute__((ext_vector_type(4)));
        const u4v xr = __builtin_nontemporal_load((const u4v *) (pa + i)), yr = __builtin_nontemporal_load((const u4v *) (pb + i));
        const pack x = __builtin_bit_cast(pack, xr), y = __builtin_bit_cast(pack, yr);      // touched once: streaming policy
        pack r;
#pragma unroll
        for (int j = 0; j < V; ++j) r.e[j] = apply<T, OP>(x.e[j], y.e[j]);
        __builtin_nontemporal_store(__builtin_bit_cast(u4v, r), (u4v *) (po + i));
    }
}

// One operand has the output's shape, the other is a scalar or spans the trailing dims (a [B, K] spectrum times a [K] filter):
// 16 bytes per thread of the large operand and of the result; the small operand is read per element (it lives in the caches),
// its index from ONE modulo per thread.  BIG_IS_A: out = big op small, else out = small op big.
template<typename T, int OP, bool BIG_IS_A>
__global__ void binary_small_pack_kernel(const T *big, const T *small, T *out, unsigned npack, unsigned small_ne) {
    constexpr int V = 16 / sizeof(T);
    const packed<T, V> *pbig = (const packed<T, V> *) big;
    packed<T, V> *po = (packed<T, V> *) out;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npack; i += gridDim.x * blockDim.x) {
        const packed<T, V> x = pbig[i];
        unsigned m = small_ne == 1 ? 0u : (unsigned) (((unsigned long long) i * V) % small_ne);
        packed<T, V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const T sv = small[m];
            r.e[j] = BIG_IS_A ? apply<T, OP>(x.e[j], sv) : apply<T, OP>(sv, x.e[j]);
            m = m + 1 >= small_ne ? 0u : m + 1;
        }
        po[i] = r;
    }
}

// The small operand spans the LEADING dims (a [B, K] tensor against a [B, 1] column): element e of the result takes small[e / per];
// one division per thread, then the index steps when a pack crosses a row end.
template<typename T, int OP, bool BIG_IS_A>
__global__ void binary_column_pack_kernel(const T *big, const T *small, T *out, unsigned npack, unsigned per) {
    constexpr int V = 16 / sizeof(T);
    const packed<T, V> *pbig = (const packed<T, V> *) big;
    packed<T, V> *po = (packed<T, V> *) out;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npack; i += gridDim.x * blockDim.x) {
        const packed<T, V> x = pbig[i];
        const unsigned long long e0 = (unsigned long long) i * V;
        unsigned q = (unsigned) (e0 / per), m = (unsigned) (e0 - (unsigned long long) q * per);
        packed<T, V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const T sv = small[q];
            r.e[j] = BIG_IS_A ? apply<T, OP>(x.e[j], sv) : apply<T, OP>(sv, x.e[j]);
            if (++m >= per) { m = 0; ++q; }
        }
        po[i] = r;
    }
}

template<typename T, int OP>
bool binary_fast(const T *pa, const T *pb, T *po, const dsc_bcast_args &g, hipStream_t s) {
    constexpr unsigned V = 16 / sizeof(T);
    if (g.fast >= 4 && !g.a_scalar && !g.b_scalar) {
        const bool big_is_a = g.fast == 4;
        const T *big = big_is_a ? pa : pb, *small = big_is_a ? pb : pa;
        if (g.ne % V != 0 || !aligned_to(big, 16) || !aligned_to(po, 16) || g.small_ne < (int) V) return false;
        const unsigned npack = (unsigned) (g.ne / V);
        with_bool(big_is_a, [&](auto big_a) {
            DSC_LAUNCH((binary_column_pack_kernel<T, OP, decltype(big_a)::value>), pack_grid(npack), dim3(256), 0, s, big, small, po, npack, (unsigned) g.small_ne);
        });
        return true;
    }
    if ((g.a_scalar || g.b_scalar || g.fast == 2 || g.fast == 3) && g.ne % V == 0) {
        const bool big_is_a = g.b_scalar || (!g.a_scalar && g.fast == 2);
        const T *big = big_is_a ? pa : pb, *small = big_is_a ? pb : pa;
        const unsigned sm = (g.a_scalar || g.b_scalar) ? 1u : (unsigned) g.small_ne;
        if (aligned_to(big, 16) && aligned_to(po, 16) && sm >= 1) {
            const unsigned npack = (unsigned) (g.ne / V);
            with_bool(big_is_a, [&](auto big_a) {
                DSC_LAUNCH((binary_small_pack_kernel<T, OP, decltype(big_a)::value>), pack_grid(npack), dim3(256), 0, s, big, small, po, npack, sm);
            });
            return true;
        }
    }
    if (g.a_scalar || g.b_scalar || g.fast == 0 || g.fast >= 4) return false;
    const unsigned ne = (unsigned) g.ne, sm = (unsigned) g.small_ne;
    if (g.fast == 1 && V > 1 && ne % V == 0 && (((size_t) pa | (size_t) pb | (size_t) po) & 15) == 0) {
        DSC_LAUNCH((binary_same_vec_kernel<T, OP>), pack_grid(ne / V), dim3(256), 0, s, pa, pb, po, ne / V);
        return true;
    }
    with_index<3>("elementwise.hip", "fast index path", g.fast - 1, [&](auto f) {          // g.fast is 1, 2 or 3 here
        DSC_LAUNCH((binary_fast_kernel<T, OP, decltype(f)::value + 1>), stream_grid(g.ne), dim3(256), 0, s, pa, pb, po, ne, sm);
    });
    return true;
}

// General broadcast, 16 bytes of the result per thread: along the innermost axis an operand either advances with the result
// (one 16-byte load) or is broadcast (one element); the outer indices come from one division chain per thread.  A block is no
// longer tied to one innermost row, so short rows (512 floats) fill their workgroups too.
template<typename T, int OP>
__global__ void binary_bcast_pack_kernel(const T *a, const T *b, T *out, const dsc_bcast_args g, unsigned packs_per_row, unsigned npack) {
    constexpr int V = 16 / sizeof(T);
    packed<T, V> *po = (packed<T, V> *) out;
    const unsigned s2 = (unsigned) g.out_shape[2], s1 = (unsigned) g.out_shape[1];
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npack; p += gridDim.x * blockDim.x) {
        const unsigned row = p / packs_per_row, c = (p - row * packs_per_row) * V;
        const unsigned t = row / s2, i2 = row - t * s2;
        const unsigned i0 = t / s1, i1 = t - i0 * s1;
        const T *ra = a + ((long long) i0 * g.a_stride[0] + (long long) i1 * g.a_stride[1] + (long long) i2 * g.a_stride[2]);
        const T *rb = b + ((long long) i0 * g.b_stride[0] + (long long) i1 * g.b_stride[1] + (long long) i2 * g.b_stride[2]);
        packed<T, V> x, y, r;
        if (g.a_stride[3]) x = *(const packed<T, V> *) (ra + c);
        else {
            const T v = ra[0];
#pragma unroll
            for (int j = 0; j < V; ++j) x.e[j] = v;
        }
        if (g.b_stride[3]) y = *(const packed<T, V> *) (rb + c);
        else {
            const T v = rb[0];
#pragma unroll
            for (int j = 0; j < V; ++j) y.e[j] = v;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) r.e[j] = apply<T, OP>(x.e[j], y.e[j]);
        po[p] = r;
    }
}

template<typename T, int OP>
bool binary_bcast_pack(const T *pa, const T *pb, T *po, const dsc_bcast_args &g, hipStream_t s) {
    constexpr int V = 16 / sizeof(T);
    if (g.a_scalar || g.b_scalar || g.out_shape[3] % V != 0 || !aligned_to(po, 16) || g.ne / V >= (1LL << 32)) return false;
    auto fits = [&](const T *p, const int *st) {
        if (st[3] == 0) return true;
        if (st[3] != 1 || !aligned_to(p, 16)) return false;
        for (int k = 0; k < 3; ++k) if (st[k] % V != 0) return false;
        return true;
    };
    if (!fits(pa, g.a_stride) || !fits(pb, g.b_stride)) return false;
    const unsigned ppr = (unsigned) (g.out_shape[3] / V), npack = (unsigned) (g.ne / V);
    DSC_LAUNCH((binary_bcast_pack_kernel<T, OP>), pack_grid(npack), dim3(256), 0, s, pa, pb, po, g, ppr, npack);
    return true;
}

template<typename T, int OP>
void binary_op(const T *pa, const T *pb, T *po, const dsc_bcast_args &g, hipStream_t s) {
    if (binary_fast<T, OP>(pa, pb, po, g, s)) return;
    if (binary_bcast_pack<T, OP>(pa, pb, po, g, s)) return;
    const long long rows = g.out_shape[3] > 0 ? g.ne / g.out_shape[3] : 0;
    const unsigned chunks = (unsigned) ((g.out_shape[3] + 1023) / 1024);
    if (!g.a_scalar && !g.b_scalar && g.out_shape[3] >= 64 && rows * chunks < (1LL << 31)) {
        DSC_LAUNCH((binary_rows_kernel<T, OP>), dim3((unsigned) (rows * chunks)), dim3(256), 0, s, pa, pb, po, g, chunks);
        return;
    }
    DSC_LAUNCH((binary_kernel<T, OP>), stream_grid(g.ne), dim3(256), 0, s, pa, pb, po, g);
}

// abs / angle / conj / real / imag: dsc/src/dsc.cpp:1480-1622, functors dsc_ops.h:242-303.
// OP: 0 abs, 1 angle, 2 conj, 3 real, 4 imag.  Tin real or complex, output real (conj: same as input).
// OP 5 .. 14 keep the input's dtype (dsc.cpp:1299-1440, 1640-1770; dsc_ops.h:92-229, 318-339):
//   5 cos, 6 sin, 7 sinc, 8 logn, 9 log2, 10 log10, 11 exp, 12 sqrt, 13 i0 (real only), 14 clip(lo, hi)
template<typename Tin, int OP> struct unary_out { using type = typename std::conditional<(OP >= 5), Tin, typename elem<Tin>::real>::type; };
template<typename R> struct unary_out<cx<R>, 2> { using type = cx<R>; };

struct unary_params { double lo, hi; };     // clip bounds (f64 in the ABI, cast to the tensor's real type as dsc.cpp:1740-1765)

// Modified Bessel function I0, Abramowitz & Stegun 9.8.1 (|x| < 3.75, t = x / 3.75) and 9.8.2 (|x| >= 3.75): the two
// polynomial approximations the reference evaluates (dsc.cpp:1625-1687), in the real type of the tensor.
template<typename R>
__device__ __forceinline__ R bessel_i0(R x) {
    const R ax = x >= 0 ? x : -x;
    if (ax < (R) 3.75) {
        R y = x / (R) 3.75;
        y *= y;
        return (R) 1 + y * ((R) 3.5156229 + y * ((R) 3.0899424 + y * ((R) 1.2067492 + y * ((R) 0.2659732 + y * ((R) 0.360768e-1 + y * (R) 0.45813e-2)))));
    }
    const R y = (R) 3.75 / ax;
    return (m_exp(ax) / m_sqrt(ax)) *
           ((R) 0.39894228 + y * ((R) 0.1328592e-1 + y * ((R) 0.225319e-2 + y * ((R) -0.157565e-2 + y * ((R) 0.916281e-2 +
            y * ((R) -0.2057706e-1 + y * ((R) 0.2635537e-1 + y * ((R) -0.1647633e-1 + y * (R) 0.392377e-2))))))));
}

template<typename Tin, int OP>
__device__ __forceinline__ typename unary_out<Tin, OP>::type unary_one(Tin v, const unary_params p) {
    using R = typename elem<Tin>::real;
    constexpr bool C = elem<Tin>::cplx;
    R re, im;
    if constexpr (C) { re = v.x; im = v.y; }
    else             { re = v; im = (R) 0; }
    if constexpr (OP == 0) {
        if constexpr (C) return sqrt((re * re) + (im * im));
        else             return re >= 0 ? re : -re;
    } else if constexpr (OP == 1) {
        return atan2(im, re);
    } else if constexpr (OP == 2) {
        if constexpr (C) return Tin{re, -im};
        else             return re;
    } else if constexpr (OP == 3) {
        return re;
    } else if constexpr (OP == 4) {
        return im;
    } else if constexpr (OP == 5) {                                       // cos_op
        if constexpr (C) return Tin{m_cos(re) * m_cosh(im), -m_sin(re) * m_sinh(im)};
        else             return m_cos(re);
    } else if constexpr (OP == 6 || OP == 7) {                            // sin_op; sinc_op = sin(pi x) / (pi x), 1 at 0
        constexpr R pi = (R) 3.14159265358979323846;
        const R a = OP == 7 ? pi * re : re, b = OP == 7 ? pi * im : im;
        if constexpr (C) {
            const Tin s{m_sin(a) * m_cosh(b), m_cos(a) * m_sinh(b)};
            if constexpr (OP == 6) return s;
            else return (re == (R) 0 && im == (R) 0) ? Tin{(R) 1, (R) 0} : apply<Tin, 3>(s, Tin{a, b});   // through div_op
        } else {
            if constexpr (OP == 6) return m_sin(a);
            else return re == (R) 0 ? (R) 1 : m_sin(a) / a;
        }
    } else if constexpr (OP == 8) {
        return t_log<Tin, 0>(v);
    } else if constexpr (OP == 9) {
        return t_log<Tin, 2>(v);
    } else if constexpr (OP == 10) {
        return t_log<Tin, 10>(v);
    } else if constexpr (OP == 11) {
        return t_exp(v);
    } else if constexpr (OP == 12) {                                      // sqrt_op: the sign of the imaginary part from im >= 0
        if constexpr (C) {
            const R abs = m_sqrt((re * re) + (im * im));
            const R sign = im >= 0 ? (R) 1 : (R) -1;
            return Tin{m_sqrt((R) 0.5 * (abs + re)), sign * m_sqrt((R) 0.5 * (abs - re))};
        } else {
            return m_sqrt(re);
        }
    } else if constexpr (OP == 13) {
        static_assert(!C, "i0 is real only");
        return bessel_i0(re);
    } else {                                                              // clip: min_op(max_op(x, lo), hi)
        const R lo = (R) p.lo, hi = (R) p.hi;
        if constexpr (C) {                                                // compare real parts; a bound comes back as (bound, 0)
            const Tin m = re > lo ? v : Tin{lo, (R) 0};
            return m.x > hi ? Tin{hi, (R) 0} : m;
        } else {                                                          // DSC_MAX / DSC_MIN (dsc.h:43-44): NaN -> lo
            const R m = re > lo ? re : lo;
            return m < hi ? m : hi;
        }
    }
}

template<typename Tin, int OP>
__global__ void unary_kernel(const Tin *in, void *out, long long ne, const unary_params p) {
    using Tout = typename unary_out<Tin, OP>::type;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (long long) gridDim.x * blockDim.x)
        ((Tout *) out)[i] = unary_one<Tin, OP>(in[i], p);
}

template<typename Tin, int OP, int V>
__global__ void unary_pack_kernel(const Tin *in, void *out, unsigned npack, const unary_params p) {
    using Tout = typename unary_out<Tin, OP>::type;
    const packed<Tin, V> *pi = (const packed<Tin, V> *) in;
    packed<Tout, V> *po = (packed<Tout, V> *) out;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npack; i += gridDim.x * blockDim.x) {
        const packed<Tin, V> x = pi[i];
        packed<Tout, V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) r.e[j] = unary_one<Tin, OP>(x.e[j], p);
        po[i] = r;
    }
}

template<typename Tin, int OP>
void unary_op(const Tin *x, void *out, long long ne, const unary_params p, hipStream_t s) {
    using Tout = typename unary_out<Tin, OP>::type;
    constexpr int V = pack_width<Tin, Tout>();
    long long done = 0;
    if (V > 1 && ne >= V && aligned_to(x, sizeof(Tin) * V) && aligned_to(out, sizeof(Tout) * V)) {
        const long long npack = ne / V;
        DSC_LAUNCH((unary_pack_kernel<Tin, OP, V>), pack_grid(npack), dim3(256), 0, s, x, out, (unsigned) npack, p);
        done = npack * V;
    }
    if (done < ne) {
        if (V == 1) DSC_LAUNCH((unary_kernel<Tin, OP>), pack_grid(ne), dim3(256), 0, s, x, out, ne, p);       // 16 bytes per element already
        else DSC_LAUNCH((unary_kernel<Tin, OP>), stream_grid(ne - done), dim3(256), 0, s, x + done, (void *) ((Tout *) out + done), ne - done, p);
    }
}

// arange (dsc.cpp:430-439, 477-499): the reference accumulates val += 1 in T, so an f32 (or c32 real part) saturates at
// 2^24 — 2^24 + 1 rounds back to 2^24 — and element i is min(i, 2^24); f64 is exact for every int n.
template<typename T>
__device__ __forceinline__ T arange_value(long long i) {
    using R = typename elem<T>::real;
    const R v = sizeof(R) == 4 ? (R) (i < (1LL << 24) ? i : (1LL << 24)) : (R) i;
    if constexpr (elem<T>::cplx) return T{v, (R) 0};
    else                         return v;
}

// one pack of V elements per thread (16-byte stores), the elements past n of the last pack written one by one
template<typename T, int V>
__global__ void arange_kernel(T *out, unsigned npack, long long n) {
    packed<T, V> *po = (packed<T, V> *) out;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npack; p += gridDim.x * blockDim.x) {
        const long long e0 = (long long) p * V;
        if (e0 + V <= n) {
            packed<T, V> r;
#pragma unroll
            for (int j = 0; j < V; ++j) r.e[j] = arange_value<T>(e0 + j);
            po[p] = r;
        } else {
            for (long long e = e0; e < n; ++e) out[e] = arange_value<T>(e);
        }
    }
}

template<typename T>
void arange_typed(void *out, long long n, hipStream_t s) {
    constexpr int V = 16 / sizeof(T);
    if (aligned_to(out, 16)) {
        const long long npack = (n + V - 1) / V;
        DSC_LAUNCH((arange_kernel<T, V>), pack_grid(npack), dim3(256), 0, s, (T *) out, (unsigned) npack, n);
    } else {
        DSC_LAUNCH((arange_kernel<T, 1>), pack_grid(n), dim3(256), 0, s, (T *) out, (unsigned) n, n);
    }
}

}  // namespace

// in_dtype != out_dtype: both callers return the tensor itself for an equal pair, so no copy kernel is compiled for one
void dsc_launch_cast(const void *in, int in_dtype, void *out, int out_dtype, long long ne, hipStream_t stream) {
    if (ne <= 0) return;
    with_dtype(in_dtype, [&](auto ti) {
        with_dtype(out_dtype, [&](auto to) {
            using Tin = decltype(ti);
            using Tout = decltype(to);
            if constexpr (std::is_same<Tin, Tout>::value) no_kernel("elementwise.hip", "cast to the input's own dtype", out_dtype);
            else cast_to<Tin, Tout>((const Tin *) in, (Tout *) out, ne, stream);
        });
    });
}

void dsc_launch_unary(const void *in, int in_dtype, void *out, int op, long long ne, hipStream_t stream, double lo, double hi) {
    if (ne <= 0) return;
    const unary_params p{lo, hi};
    with_dtype(in_dtype, [&](auto t) {
        with_index<15>("elementwise.hip", "unary op", op, [&](auto opc) {
            using Tin = decltype(t);
            constexpr int OP = decltype(opc)::value;
            if constexpr (OP == 13 && elem<Tin>::cplx) {
                fprintf(stderr, "dsc_launch_unary: i0 of a complex tensor\n");
                exit(EXIT_FAILURE);
            } else {
                unary_op<Tin, OP>((const Tin *) in, out, ne, p, stream);
            }
        });
    });
}

void dsc_launch_arange(void *out, int dtype, long long n, hipStream_t stream) {
    if (n <= 0) return;
    with_dtype(dtype, [&](auto t) { arange_typed<decltype(t)>(out, n, stream); });
}

// ---- operands of DIFFERENT dtypes and equal shapes: the casts of binary_op (dsc.cpp:1186-1223 casts both operands to the
// promoted type first) happen in registers — same expression per element (cast_one, then apply), no temporary in HBM.
namespace {
template<typename Ta, typename Tb> struct promoted {          // dsc_dtype.h:73-78
    static constexpr bool cplx = elem<Ta>::cplx || elem<Tb>::cplx;
    static constexpr bool wide = cplx ? (sizeof(Ta) == 16 || sizeof(Tb) == 16)
                                      : (sizeof(Ta) == 8 || sizeof(Tb) == 8);
    using real = typename std::conditional<wide, double, float>::type;
    using type = typename std::conditional<cplx, cx<real>, real>::type;
};

template<typename Ta, typename Tb, int OP>
__global__ void binary_mixed_pack_kernel(const Ta *a, const Tb *b, typename promoted<Ta, Tb>::type *out, unsigned npack) {
    using To = typename promoted<Ta, Tb>::type;
    constexpr int V = 16 / sizeof(To);
    const packed<Ta, V> *pa = (const packed<Ta, V> *) a;
    const packed<Tb, V> *pb = (const packed<Tb, V> *) b;
    packed<To, V> *po = (packed<To, V> *) out;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npack; i += gridDim.x * blockDim.x) {
        const packed<Ta, V> x = pa[i];
        const packed<Tb, V> y = pb[i];
        packed<To, V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) r.e[j] = apply<To, OP>(cast_one<Ta, To>(x.e[j]), cast_one<Tb, To>(y.e[j]));
        po[i] = r;
    }
}

template<typename Ta, typename Tb>
bool mixed_pair(const void *a, const void *b, void *out, int op, long long ne, hipStream_t s) {
    using To = typename promoted<Ta, Tb>::type;
    constexpr int V = 16 / sizeof(To);
    if (ne % V != 0 || !aligned_to(a, sizeof(Ta) * V) || !aligned_to(b, sizeof(Tb) * V) || !aligned_to(out, 16)) return false;
    const unsigned npack = (unsigned) (ne / V);
    const Ta *pa = (const Ta *) a; const Tb *pb = (const Tb *) b; To *po = (To *) out;
    with_index<5>("elementwise.hip", "binary op", op, [&](auto opc) {
        DSC_LAUNCH((binary_mixed_pack_kernel<Ta, Tb, decltype(opc)::value>), pack_grid(npack), dim3(256), 0, s, pa, pb, po, npack);
    });
    return true;
}
}  // namespace

bool dsc_launch_binary_mixed(const void *a, int a_dtype, const void *b, int b_dtype, void *out, int op, long long ne, hipStream_t stream) {
    if (ne <= 0 || a_dtype == b_dtype) return false;
    bool done = false;
    with_dtype(a_dtype, [&](auto ta) {
        with_dtype(b_dtype, [&](auto tb) {
            using Ta = decltype(ta);
            using Tb = decltype(tb);
            if constexpr (std::is_same<Ta, Tb>::value) no_kernel("elementwise.hip", "mixed operands of one dtype", a_dtype);   // returned above
            else done = mixed_pair<Ta, Tb>(a, b, out, op, ne, stream);
        });
    });
    return done;
}

void dsc_launch_binary(const void *a, const void *b, void *out, int dtype, int op, const dsc_bcast_args &g, hipStream_t stream) {
    if (g.ne <= 0) return;
    with_dtype(dtype, [&](auto t) {
        with_index<5>("elementwise.hip", "binary op", op, [&](auto opc) {
            using T = decltype(t);
            binary_op<T, decltype(opc)::value>((const T *) a, (const T *) b, (T *) out, g, stream);
        });
    });
}
