// remap.hip — the kernels of dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift / dsc_pad (remap.cpp): one pass of a plan
// out[j0, j1, j2, j3] = x[m0(j0), m1(j1), m2(j2), m3(j3)] or the plan's constant (remap_plan.h).  Elements are opaque
// 4-, 8- or 16-byte words (with_elem_bytes of stream_common.h); the index arithmetic is dsc_map_index of remap_plan.h, the same
// function the host tests run.
//   remap_rows   the last axis is the identity: a workgroup owns a piece of one output row, resolves the three outer source indices
//                once (they depend on blockIdx alone: scalar registers) and copies aligned 16-byte packs, one per thread
//   remap_packs  the last axis is mapped: the same workgroups; a thread stores ONE aligned 16-byte pack of V = 16 / element size
//                elements.  It maps the pack's first and last element: V consecutive sources in either direction are a run, read at
//                once (load_run) and swapped in registers when they descend; a pack that straddles a seam of the map (the roll's wrap
//                point, a pad boundary, a reflection point) gathers element by element
//   remap_elems  one element per thread in the flat form of layout.hip's region_flat_kernel: any size, any alignment
#include "stream_common.h"

namespace {

template<typename E> __device__ inline E remap_constant(const dsc_remap &p);
template<> __device__ inline unsigned int remap_constant<unsigned int>(const dsc_remap &p) { return (unsigned int) p.value[0]; }
template<> __device__ inline unsigned long long remap_constant<unsigned long long>(const dsc_remap &p) { return p.value[0]; }
template<> __device__ inline b16 remap_constant<b16>(const dsc_remap &p) { return b16{p.value[0], p.value[1]}; }

// Output row `row` = (j0 n1 + j1) n2 + j2 -> its source row, or false: one of the three outer indices falls into a constant region.
// Fewer than 2^31 rows on either side (ne fits an int), so the divisions are 32-bit; `row` comes from blockIdx: uniform.
__device__ inline bool remap_source_row(const dsc_remap &p, unsigned row, long long &src_row) {
    const unsigned n1 = (unsigned) p.ax[1].n_out, n2 = (unsigned) p.ax[2].n_out;
    const unsigned i01 = row / n2, j2 = row - i01 * n2;
    const unsigned j0 = i01 / n1, j1 = i01 - j0 * n1;
    const int s0 = dsc_map_index(p.ax[0], (int) j0), s1 = dsc_map_index(p.ax[1], (int) j1), s2 = dsc_map_index(p.ax[2], (int) j2);
    src_row = ((long long) s0 * p.ax[1].n_in + s1) * p.ax[2].n_in + s2;
    return (s0 | s1 | s2) >= 0;
}

// V consecutive elements from element `at` of x, an index that is no multiple of V in general: ONE 16-byte access of element alignment,
// which gfx950 performs as a single global_load_dwordx4 whatever the address (V element loads compile to the same instruction).
// Measured against the two aligned packs around the run and a select in registers, which lost on every misaligned run
// (profiles/remap_bench.txt).
template<typename E, int V> __device__ inline packed<E, V> load_run(const E *x, long long at) {
    struct __attribute__((packed, aligned(alignof(E)))) loose { E e[V]; };
    const loose w = *(const loose *) (x + at);
    packed<E, V> q;
#pragma unroll
    for (int k = 0; k < V; ++k) q.e[k] = w.e[k];
    return q;
}

// grid: rows * chunks workgroups of blockDim.x threads, chunks = ceil(ppr / blockDim.x); ppr = 16-byte packs per row
template<typename E>
__global__ __launch_bounds__(256) void remap_rows_kernel(const E *x, E *out, const dsc_remap p, unsigned ppr, unsigned chunks) {
    constexpr int V = 16 / (int) sizeof(E);
    using P = packed<E, V>;
    const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
    const unsigned c = chunk * blockDim.x + threadIdx.x;
    if (c >= ppr) return;
    long long src_row;
    P q;
    if (remap_source_row(p, row, src_row)) {
        q = ((const P *) x)[src_row * ppr + c];
    } else {
        const E cst = remap_constant<E>(p);
#pragma unroll
        for (int k = 0; k < V; ++k) q.e[k] = cst;
    }
    ((P *) out)[(long long) row * ppr + c] = q;
}

template<typename E>
__global__ __launch_bounds__(256) void remap_packs_kernel(const E *x, E *out, const dsc_remap p, unsigned ppr, unsigned chunks) {
    constexpr int V = 16 / (int) sizeof(E);
    using P = packed<E, V>;
    const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
    const unsigned c = chunk * blockDim.x + threadIdx.x;
    if (c >= ppr) return;
    const dsc_axis_map &m = p.ax[3];
    const E cst = remap_constant<E>(p);
    long long src_row;
    P q;
    if (remap_source_row(p, row, src_row)) {
        const E *src = x + src_row * m.n_in;
        const int j = (int) c * V;
        const int first = dsc_map_index(m, j), last = dsc_map_index(m, j + V - 1);
        // a run: every step of the map is +1 (or every step -1).  The maps that never descend have steps of 0 or +1 and downward jumps
        // only, so last - first == V - 1 proves a run for every kind; first - last == V - 1 proves one for the kinds without jumps
        const bool may_descend = m.kind == DSC_MAP_REVERSED || m.kind == DSC_MAP_REFLECT || m.kind == DSC_MAP_SYMMETRIC;
        if (first >= 0 && last - first == V - 1) {
            q = load_run<E, V>(x, src_row * m.n_in + first);
        } else if (may_descend && last >= 0 && first - last == V - 1) {
            const P r = load_run<E, V>(x, src_row * m.n_in + last);
#pragma unroll
            for (int k = 0; k < V; ++k) q.e[k] = r.e[V - 1 - k];
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int s = dsc_map_index(m, j + k);
                q.e[k] = s >= 0 ? src[s] : cst;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) q.e[k] = cst;
    }
    ((P *) out)[(long long) row * ppr + c] = q;
}

template<typename E>
__global__ void remap_elems_kernel(const E *x, E *out, const dsc_remap p) {
    const unsigned n1 = (unsigned) p.ax[1].n_out, n2 = (unsigned) p.ax[2].n_out, n3 = (unsigned) p.ax[3].n_out;
    const E cst = remap_constant<E>(p);
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < p.ne_out; i += (long long) gridDim.x * blockDim.x) {
        const unsigned i012 = (unsigned) i / n3, j3 = (unsigned) i - i012 * n3;
        const unsigned i01 = i012 / n2, j2 = i012 - i01 * n2;
        const unsigned j0 = i01 / n1, j1 = i01 - j0 * n1;
        const int s0 = dsc_map_index(p.ax[0], (int) j0), s1 = dsc_map_index(p.ax[1], (int) j1);
        const int s2 = dsc_map_index(p.ax[2], (int) j2), s3 = dsc_map_index(p.ax[3], (int) j3);
        const long long at = (((long long) s0 * p.ax[1].n_in + s1) * p.ax[2].n_in + s2) * p.ax[3].n_in + s3;
        E v = cst;
        if ((s0 | s1 | s2 | s3) >= 0) v = x[at];
        out[i] = v;
    }
}

template<typename E>
void remap_typed(const void *x, void *out, const dsc_remap &p, int route, hipStream_t s) {
    constexpr int V = 16 / (int) sizeof(E);
    const E *px = (const E *) x;
    E *po = (E *) out;
    if (route == DSC_REMAP_ELEMS) {
        DSC_LAUNCH((remap_elems_kernel<E>), stream_grid(p.ne_out), dim3(256), 0, s, px, po, p);
        return;
    }
    const dsc_axis_map &last = p.ax[DSC_REMAP_DIMS - 1];
    const unsigned ppr = (unsigned) (last.n_out / V);
    const unsigned threads = ppr >= 256 ? 256 : 64;                      // a row of a few packs gets one wave
    const unsigned chunks = (ppr + threads - 1) / threads;
    const long long blocks = p.ne_out / last.n_out * chunks;
    if (blocks >= (1LL << 31)) no_kernel("remap.hip", "workgroup count", blocks);
    if (route == DSC_REMAP_ROWS) {
        DSC_LAUNCH((remap_rows_kernel<E>), dim3((unsigned) blocks), dim3(threads), 0, s, px, po, p, ppr, chunks);
    } else if constexpr (V > 1) {
        DSC_LAUNCH((remap_packs_kernel<E>), dim3((unsigned) blocks), dim3(threads), 0, s, px, po, p, ppr, chunks);
    } else {
        no_kernel("remap.hip", "remap_packs element size", (long long) sizeof(E));
    }
}

}  // namespace

void dsc_launch_remap(const void *x, void *out, int elem_bytes, const dsc_remap &plan, int route, hipStream_t stream) {
    if (plan.ne_out <= 0) return;
    // the pack routes rest on what dsc_remap_route checks (aligned bases, rows of whole packs): never launch them on anything else
    if (route != DSC_REMAP_ELEMS && dsc_remap_route(plan, elem_bytes, aligned_to(x, 16) && aligned_to(out, 16)) != route)
        no_kernel("remap.hip", "route", route);
    with_elem_bytes(elem_bytes, [&](auto e) { remap_typed<decltype(e)>(x, out, plan, route, stream); });
}
