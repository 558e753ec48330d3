// layout.hip — kernels that move elements without looking at them: the slice gather / scatter of dsc_tensor_get_slice / set_slice
// and dsc_concat, and the three transposes (last two axes; any permutation that moves the last axis, scalar and 16-byte forms).
// Elements are opaque 4-, 8- or 16-byte words (with_elem_bytes of stream_common.h).
#include "stream_common.h"

// ---- slice regions: dsc_tensor_get_slice / set_slice (dsc.cpp:868-1169) ---------------------
// The reference walks a dsc_slice_iterator (dsc_iter.h:125-190) per element; here a block owns a piece of
// one innermost row of the region (one division chain per block), or — for narrow rows — a flat
// per-element decomposition.
namespace {

// elements per thread of region_rows_kernel: ONE 16-byte pack (the launch then sweeps memory in address order and every
// workgroup ends right after its store: x[:, :60000] 67 -> 73.5 % of the roofline), four of the narrower elements (with one
// per thread the strided x[:, ::2] drops from 49 to 35 %)
template<typename E> constexpr int region_u() { return sizeof(E) == 16 ? 1 : 4; }

template<typename E, bool SCATTER>
__global__ void region_rows_kernel(const E *src, E *dst, const dsc_region r, unsigned chunks_per_row, long long dense_ne) {
    const unsigned long long blk = blockIdx.x;
    const unsigned long long row = blk / chunks_per_row;
    const unsigned chunk = (unsigned) (blk - row * chunks_per_row);
    const unsigned long long i01 = row / r.count[2];
    const long long i2 = (long long) (row - i01 * r.count[2]);
    const long long i0 = (long long) (i01 / r.count[1]), i1 = (long long) (i01 - (unsigned long long) i0 * r.count[1]);
    const long long base = r.base + i0 * r.stride[0] + i1 * r.stride[1] + i2 * r.stride[2];
    const long long dense0 = (long long) row * r.count[3];
    constexpr int U = region_u<E>();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = chunk * (256 * U) + u * 256 + threadIdx.x;
        if (c >= r.count[3]) return;
        if (SCATTER) dst[base + c * r.stride[3]] = src[(dense0 + c) % dense_ne];
        else         dst[dense0 + c] = src[base + c * r.stride[3]];
    }
}

template<typename E, bool SCATTER>
__global__ void region_flat_kernel(const E *src, E *dst, const dsc_region r, long long dense_ne) {
    const long long s3 = r.count[3], s23 = s3 * r.count[2], s123 = s23 * r.count[1];
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < r.ne; i += (long long) gridDim.x * blockDim.x) {
        const long long i0 = i / s123, r0 = i - i0 * s123;
        const long long i1 = r0 / s23, r1 = r0 - i1 * s23;
        const long long i2 = r1 / s3, i3 = r1 - i2 * s3;
        const long long at = r.base + i0 * r.stride[0] + i1 * r.stride[1] + i2 * r.stride[2] + i3 * r.stride[3];
        if (SCATTER) dst[at] = src[i % dense_ne];
        else         dst[i] = src[at];
    }
}

template<typename E>
void region_typed(const void *src, void *dst, const dsc_region &r, bool scatter, long long dense_ne, hipStream_t s) {
    const E *ps = (const E *) src;
    E *pd = (E *) dst;
    const long long rows = r.ne / r.count[3];
    constexpr int per_block = 256 * region_u<E>();
    if (r.count[3] >= 128 && rows * ((r.count[3] + per_block - 1) / per_block) < (1LL << 31)) {
        const unsigned chunks = (unsigned) ((r.count[3] + per_block - 1) / per_block);
        const dim3 grid((unsigned) (rows * chunks));
        with_bool(scatter, [&](auto sc) { DSC_LAUNCH((region_rows_kernel<E, decltype(sc)::value>), grid, dim3(256), 0, s, ps, pd, r, chunks, dense_ne); });
    } else {
        with_bool(scatter, [&](auto sc) { DSC_LAUNCH((region_flat_kernel<E, decltype(sc)::value>), stream_grid(r.ne), dim3(256), 0, s, ps, pd, r, dense_ne); });
    }
}

}  // namespace

void dsc_launch_region_copy(const void *src, void *dst, int elem_bytes, const dsc_region &r, bool scatter, long long dense_ne,
                            hipStream_t stream) {
    if (r.ne <= 0) return;
    // contiguous innermost rows whose ends fall on 16-byte boundaries (x[:, :60000], x[::2], a crop after irfft ...): move 16 bytes
    // per lane instead of one element
    const int V = 16 / elem_bytes;
    if (V > 1 && r.stride[3] == 1 && dense_ne == r.ne && r.count[3] % V == 0 && r.base % V == 0 && (((size_t) src | (size_t) dst) & 15) == 0) {
        bool ok = true;
        for (int k = 0; k < 3; ++k) ok = ok && (r.count[k] == 1 || r.stride[k] % V == 0);
        if (ok) {
            dsc_region w = r;
            w.base = r.base / V;
            w.count[3] = r.count[3] / V;
            for (int k = 0; k < 3; ++k) w.stride[k] = r.stride[k] / V;
            w.ne = r.ne / V;
            region_typed<b16>(src, dst, w, scatter, dense_ne / V, stream);
            return;
        }
    }
    with_elem_bytes(elem_bytes, [&](auto e) { region_typed<decltype(e)>(src, dst, r, scatter, dense_ne, stream); });
}

// ---- dsc_transpose of the last two axes (dsc.cpp:764-827 walks a stride iterator per element) ----
namespace {

template<typename E>
__global__ void transpose_last2_kernel(const E *in, E *out, int rows, int cols, unsigned tiles_c, unsigned tiles_r) {
    __shared__ E tile[32][33];
    const unsigned long long blk = blockIdx.x;
    const unsigned long long per = (unsigned long long) tiles_c * tiles_r;
    const unsigned long long b = blk / per;
    const unsigned rem = (unsigned) (blk - b * per);
    const unsigned tr = rem / tiles_c, tc = rem - tr * tiles_c;
    const E *src = in + b * (unsigned long long) rows * cols;
    E *dst = out + b * (unsigned long long) rows * cols;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;              // 32 x 8 threads
    for (int k = ty; k < 32; k += 8) {
        const int r = tr * 32 + k, c = tc * 32 + tx;
        if (r < rows && c < cols) tile[k][tx] = src[(long long) r * cols + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = tc * 32 + k, r = tr * 32 + tx;
        if (r < rows && c < cols) dst[(long long) c * rows + r] = tile[tx][k];
    }
}

template<typename E>
void transpose_typed(const void *in, void *out, long long batch, int rows, int cols, hipStream_t s) {
    const unsigned tiles_c = (cols + 31) / 32, tiles_r = (rows + 31) / 32;
    const unsigned long long blocks = (unsigned long long) batch * tiles_c * tiles_r;
    DSC_LAUNCH((transpose_last2_kernel<E>), dim3((unsigned) blocks), dim3(256), 0, s, (const E *) in, (E *) out, rows, cols, tiles_c,
                       tiles_r);
}

}  // namespace

// ---- any permutation that moves the LAST axis (dsc_transpose with the reversed default, (2, 0, 1), ...): the plane spanned by the
// input's last axis (c, stride 1 in the input) and the input axis that becomes the output's last axis (a, stride 1 in the output) is
// transposed in 32 x 32 LDS tiles, both sides coalesced; the remaining (at most two) axes are a batch with their own strides.
namespace {

struct tr_plan {
    int na, nc;                 // extents along a and c
    long long sa_in, sc_out;    // input stride of a, output stride of c (elements)
    int nb0, nb1;               // batch extents
    long long b0_in, b0_out, b1_in, b1_out;
};

template<typename E>
__global__ void transpose_plane_kernel(const E *in, E *out, tr_plan p, unsigned tiles_a, unsigned tiles_c) {
    __shared__ E tile[32][33];
    unsigned long long blk = blockIdx.x;
    const unsigned tc = (unsigned) (blk % tiles_c); blk /= tiles_c;
    const unsigned ta = (unsigned) (blk % tiles_a); blk /= tiles_a;
    const unsigned i0 = (unsigned) (blk % (unsigned) p.nb0), i1 = (unsigned) (blk / (unsigned) p.nb0);
    const E *src = in + i0 * p.b0_in + i1 * p.b1_in;
    E *dst = out + i0 * p.b0_out + i1 * p.b1_out;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;              // 32 x 8 threads
    for (int k = ty; k < 32; k += 8) {
        const int a = ta * 32 + k, c = tc * 32 + tx;
        if (a < p.na && c < p.nc) tile[k][tx] = src[a * p.sa_in + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = tc * 32 + k, a = ta * 32 + tx;
        if (a < p.na && c < p.nc) dst[c * p.sc_out + a] = tile[tx][k];
    }
}

// The same plane transpose with 16-byte global accesses on BOTH sides (4- and 8-byte elements, V = 4 / 2 per access): a
// (16 V) x (16 V) tile, 16 x 16 threads; a thread loads V packs (rows ty + 16 k, columns tx V ..) and stores V packs (output
// rows ty + 16 k, elements tx V ..) gathered from V tile rows.  The 32 x 32 tiles move 128 bytes per row segment in f32
// (41-49 % of the roofline for [256, 512, 1024]); this form moves 256.  Needs na, nc, sa_in, sc_out and the batch strides to
// be multiples of V and 16-byte aligned bases: then a pack is never cut by the edge of the tensor.
template<typename E>
__global__ __launch_bounds__(256) void transpose_plane_vec_kernel(const E *in, E *out, tr_plan p, unsigned tiles_a, unsigned tiles_c) {
    constexpr int V = 16 / (int) sizeof(E), TD = 16 * V;
    __shared__ E tile[TD][TD + 1];
    unsigned long long blk = blockIdx.x;
    const unsigned tc = (unsigned) (blk % tiles_c); blk /= tiles_c;
    const unsigned ta = (unsigned) (blk % tiles_a); blk /= tiles_a;
    const unsigned i0 = (unsigned) (blk % (unsigned) p.nb0), i1 = (unsigned) (blk / (unsigned) p.nb0);
    const E *src = in + i0 * p.b0_in + i1 * p.b1_in;
    E *dst = out + i0 * p.b0_out + i1 * p.b1_out;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int la = ty + 16 * k, a = ta * TD + la, c = tc * TD + tx * V;
        if (a < p.na && c < p.nc) {
            const packed<E, V> q = *(const packed<E, V> *) (src + a * p.sa_in + c);
#pragma unroll
            for (int j = 0; j < V; ++j) tile[la][tx * V + j] = q.e[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int lc = ty + 16 * k, c = tc * TD + lc, a = ta * TD + tx * V;
        if (a < p.na && c < p.nc) {
            packed<E, V> q;
#pragma unroll
            for (int j = 0; j < V; ++j) q.e[j] = tile[tx * V + j][lc];
            *(packed<E, V> *) (dst + c * p.sc_out + a) = q;
        }
    }
}

template<typename E>
bool transpose_plane_vec(const void *in, void *out, const tr_plan &p, hipStream_t s) {
    constexpr int V = 16 / (int) sizeof(E), TD = 16 * V;
    if (V == 1 || !aligned_to(in, 16) || !aligned_to(out, 16)) return false;
    const long long must[] = {p.na, p.nc, p.sa_in, p.sc_out, p.nb0 > 1 ? p.b0_in : 0, p.nb0 > 1 ? p.b0_out : 0, p.nb1 > 1 ? p.b1_in : 0,
                              p.nb1 > 1 ? p.b1_out : 0};
    for (long long m : must) if (m % V != 0) return false;
    const unsigned tiles_a = (p.na + TD - 1) / TD, tiles_c = (p.nc + TD - 1) / TD;
    const unsigned long long blocks = (unsigned long long) tiles_a * tiles_c * p.nb0 * p.nb1;
    if (blocks == 0 || blocks > 0x7fffffffull) return false;
    DSC_LAUNCH((transpose_plane_vec_kernel<E>), dim3((unsigned) blocks), dim3(256), 0, s, (const E *) in, (E *) out, p, tiles_a, tiles_c);
    return true;
}

template<typename E>
void transpose_plane_typed(const void *in, void *out, const tr_plan &p, hipStream_t s) {
    if (transpose_plane_vec<E>(in, out, p, s)) return;
    const unsigned tiles_a = (p.na + 31) / 32, tiles_c = (p.nc + 31) / 32;
    const unsigned long long blocks = (unsigned long long) tiles_a * tiles_c * p.nb0 * p.nb1;
    DSC_LAUNCH((transpose_plane_kernel<E>), dim3((unsigned) blocks), dim3(256), 0, s, (const E *) in, (E *) out, p, tiles_a, tiles_c);
}

}  // namespace

// shape / in_stride: the INPUT's extents and element strides per axis (n_dim <= 4, dense); perm: result axis i = input axis perm[i],
// with perm[n_dim - 1] != n_dim - 1.  Returns false if the launch would not fit (the caller keeps the strided copy).
bool dsc_launch_transpose_moving_last(const void *in, void *out, int elem_bytes, int n_dim, const int *shape, const int *in_stride, const int *perm,
                                      hipStream_t stream) {
    long long out_stride[4] = {1, 1, 1, 1};
    for (int i = n_dim - 2; i >= 0; --i) out_stride[i] = out_stride[i + 1] * shape[perm[i + 1]];
    const int a_axis = perm[n_dim - 1], c_axis = n_dim - 1;            // input axes of the tile plane
    tr_plan p;
    p.na = shape[a_axis]; p.nc = shape[c_axis];
    p.sa_in = in_stride[a_axis];
    p.sc_out = 1;
    p.nb0 = p.nb1 = 1; p.b0_in = p.b0_out = p.b1_in = p.b1_out = 0;
    int nb = 0;
    for (int i = 0; i < n_dim; ++i) {                                   // result axis i <- input axis perm[i]
        const int ax = perm[i];
        if (ax == c_axis) { p.sc_out = out_stride[i]; continue; }
        if (ax == a_axis) continue;
        if (nb == 0) { p.nb0 = shape[ax]; p.b0_in = in_stride[ax]; p.b0_out = out_stride[i]; }
        else         { p.nb1 = shape[ax]; p.b1_in = in_stride[ax]; p.b1_out = out_stride[i]; }
        ++nb;
    }
    const unsigned long long blocks = (unsigned long long) ((p.na + 31) / 32) * ((p.nc + 31) / 32) * p.nb0 * p.nb1;
    if (blocks == 0) return true;
    if (blocks > 0x7fffffffull) return false;
    with_elem_bytes(elem_bytes, [&](auto e) { transpose_plane_typed<decltype(e)>(in, out, p, stream); });
    return true;
}

void dsc_launch_transpose_last2(const void *in, void *out, int elem_bytes, long long batch, int rows, int cols, hipStream_t stream) {
    if (batch <= 0 || rows <= 0 || cols <= 0) return;
    with_elem_bytes(elem_bytes, [&](auto e) {
        using E = decltype(e);
        if (batch < (1LL << 31)) {                                      // [batch][rows][cols] -> [batch][cols][rows] as a plane plan (not for 16-byte elements)
            tr_plan p;
            p.na = rows; p.nc = cols; p.sa_in = cols; p.sc_out = rows;
            p.nb0 = (int) batch; p.b0_in = p.b0_out = (long long) rows * cols;
            p.nb1 = 1; p.b1_in = p.b1_out = 0;
            if (transpose_plane_vec<E>(in, out, p, stream)) return;
        }
        transpose_typed<E>(in, out, batch, rows, cols, stream);
    });
}
