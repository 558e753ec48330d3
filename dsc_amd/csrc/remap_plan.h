// remap_plan.h — the plan of dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift / dsc_pad (remap.cpp, remap.hip):
// out[j0, j1, j2, j3] = x[m0(j0), m1(j1), m2(j2), m3(j3)] or a constant, one piecewise-affine map per axis.  Integer arithmetic only; the
// header needs nothing but itself, so that a stand-alone host program (tests/cpp_remap_plan.cpp) runs the very functions the host side
// plans with and the kernels index with.  kernels.h includes it next to dsc_region.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSC_REMAP_HD __host__ __device__
#else
#define DSC_REMAP_HD
#endif

#define DSC_REMAP_DIMS 4

// kinds of dsc_axis_map.  With j the output index along the axis and n = n_in:
//   AFFINE_MOD  (j + b) mod n, 0 <= b < n: roll by s (b = -s mod n), pad 'wrap' (b = -before mod n), the identity (b = 0, n_out == n)
//   REVERSED    n - 1 - j: flip
//   CLAMP       j + b clamped to [0, n - 1], b = -before: pad 'edge' (and 'reflect' of an axis of one element)
//   REFLECT     u = (j + b) mod a with a = 2 (n - 1), 0 <= b < a (b = -before mod a); u if u < n, else a - u
//   SYMMETRIC   u = (j + b) mod a with a = 2 n, 0 <= b < a; u if u < n, else a - 1 - u
//   CONSTANT    t = j + b, b = -before: t inside [0, n), else the plan's constant (index -1)
enum dsc_map_kind { DSC_MAP_AFFINE_MOD = 0, DSC_MAP_REVERSED = 1, DSC_MAP_CLAMP = 2, DSC_MAP_REFLECT = 3, DSC_MAP_SYMMETRIC = 4, DSC_MAP_CONSTANT = 5 };

struct dsc_axis_map { int n_in, n_out, kind; long long a, b; };
struct dsc_remap {
    dsc_axis_map ax[DSC_REMAP_DIMS];      // right-aligned in the four slots, like every shape here; the identity in front
    long long ne_out;                     // product of n_out
    unsigned long long value[2];          // the constant's bytes, one element of the tensor's dtype at the front
};

// pad modes of dsc_pad (include/dsc_mi355x.h)
enum { DSC_PAD_CONSTANT = 0, DSC_PAD_EDGE = 1, DSC_PAD_REFLECT = 2, DSC_PAD_SYMMETRIC = 3, DSC_PAD_WRAP = 4 };

// routes of a plan (dsc_last_fft_path): remap_rows, remap_packs, remap_elems
enum { DSC_REMAP_ROWS = 0, DSC_REMAP_PACKS = 1, DSC_REMAP_ELEMS = 2 };
// rows shorter than this many 16-byte packs are not worth a workgroup of their own: remap_elems
#define DSC_REMAP_MIN_PACKS 16

// (j + b) mod p for 0 <= j < 2^31, 0 <= b < p <= 2^32 - 2, with at most one 32-bit division
static inline DSC_REMAP_HD unsigned dsc_remap_mod(int j, long long b, long long p) {
    unsigned long long t = (unsigned long long) j + (unsigned long long) b;
    if (t >= (unsigned long long) p) {
        t -= (unsigned long long) p;                       // now below max(j, p): 32 bits
        if (t >= (unsigned long long) p) t = (unsigned) t % (unsigned) p;
    }
    return (unsigned) t;
}

// source index along the axis for output index j, 0 <= j < n_out; -1: the constant
static inline DSC_REMAP_HD int dsc_map_index(const dsc_axis_map &m, int j) {
    switch (m.kind) {
        case DSC_MAP_AFFINE_MOD: return (int) dsc_remap_mod(j, m.b, m.n_in);
        case DSC_MAP_REVERSED:   return m.n_in - 1 - j;
        case DSC_MAP_CLAMP: {
            const long long t = j + m.b;
            return t < 0 ? 0 : t >= m.n_in ? m.n_in - 1 : (int) t;
        }
        case DSC_MAP_REFLECT: {
            const unsigned u = dsc_remap_mod(j, m.b, m.a);
            return u < (unsigned) m.n_in ? (int) u : (int) ((unsigned) m.a - u);
        }
        case DSC_MAP_SYMMETRIC: {
            const unsigned u = dsc_remap_mod(j, m.b, m.a);
            return u < (unsigned) m.n_in ? (int) u : (int) ((unsigned) m.a - 1u - u);
        }
        default: {
            const long long t = j + m.b;
            return t < 0 || t >= m.n_in ? -1 : (int) t;
        }
    }
}

// x mod n in [0, n) for any sign and magnitude of x, n >= 1
static inline long long dsc_floor_mod(long long x, long long n) {
    const long long r = x % n;
    return r < 0 ? r + n : r;
}

static inline bool dsc_map_is_identity(const dsc_axis_map &m) {
    return m.n_in == m.n_out && (m.n_in == 1 || (m.kind == DSC_MAP_AFFINE_MOD && m.b == 0));
}

static inline dsc_axis_map dsc_map_identity(int n) { return dsc_axis_map{n, n, DSC_MAP_AFFINE_MOD, 1, 0}; }

// numpy.roll along one axis: out[j] = x[(j - shift) mod n]; an axis of no elements stays as it is
static inline dsc_axis_map dsc_map_roll(int n, long long shift) {
    return dsc_axis_map{n, n, DSC_MAP_AFFINE_MOD, 1, n > 0 ? dsc_floor_mod(-shift, n) : 0};
}

static inline dsc_axis_map dsc_map_flip(int n) {
    return n <= 1 ? dsc_map_identity(n) : dsc_axis_map{n, n, DSC_MAP_REVERSED, -1, (long long) n - 1};
}

// numpy.pad along one axis of n >= 1 elements, before, after >= 0; n_out is the caller's to check against INT_MAX first
static inline dsc_axis_map dsc_map_pad(int n, long long before, long long after, int mode) {
    const int n_out = (int) (n + before + after);
    if (before == 0 && after == 0) return dsc_map_identity(n);
    switch (mode) {
        case DSC_PAD_EDGE:      return dsc_axis_map{n, n_out, DSC_MAP_CLAMP, 1, -before};
        case DSC_PAD_REFLECT:
            if (n == 1) return dsc_axis_map{n, n_out, DSC_MAP_CLAMP, 1, -before};
            return dsc_axis_map{n, n_out, DSC_MAP_REFLECT, 2 * ((long long) n - 1), dsc_floor_mod(-before, 2 * ((long long) n - 1))};
        case DSC_PAD_SYMMETRIC: return dsc_axis_map{n, n_out, DSC_MAP_SYMMETRIC, 2 * (long long) n, dsc_floor_mod(-before, 2 * (long long) n)};
        case DSC_PAD_WRAP:      return dsc_axis_map{n, n_out, DSC_MAP_AFFINE_MOD, 1, dsc_floor_mod(-before, n)};
        default:                return dsc_axis_map{n, n_out, DSC_MAP_CONSTANT, 1, -before};
    }
}

// Neighbouring identity axes become one (their product fits an int because ne does), axes of one element disappear, and the rest
// moves back to the right: [4096, 64, 256] rolled on axis 0 is 4096 rows of 16384.  Sets ne_out.
static inline void dsc_remap_merge(dsc_remap &p) {
    dsc_axis_map kept[DSC_REMAP_DIMS];
    int n = 0;
    for (int i = 0; i < DSC_REMAP_DIMS; ++i) {
        const dsc_axis_map &m = p.ax[i];
        if (m.n_in == 1 && m.n_out == 1) continue;
        if (n > 0 && dsc_map_is_identity(m) && dsc_map_is_identity(kept[n - 1])) kept[n - 1] = dsc_map_identity(kept[n - 1].n_in * m.n_in);
        else kept[n++] = dsc_map_is_identity(m) ? dsc_map_identity(m.n_in) : m;
    }
    p.ne_out = 1;
    for (int i = 0; i < DSC_REMAP_DIMS; ++i) {
        const int k = i - (DSC_REMAP_DIMS - n);
        p.ax[i] = k >= 0 ? kept[k] : dsc_map_identity(1);
        p.ne_out *= p.ax[i].n_out;
    }
}

// The route of a merged plan.  bases_aligned: both tensors start on 16-byte boundaries.
//   remap_rows   the last axis is the identity and a row is whole 16-byte packs
//   remap_packs  the last axis is mapped, elements of 4 or 8 bytes, and an OUTPUT row is whole packs
//   remap_elems  everything else: odd row bytes, unaligned bases, 16-byte elements with a mapped last axis, rows of fewer than
//                DSC_REMAP_MIN_PACKS packs, more workgroups than a grid holds
static inline int dsc_remap_route(const dsc_remap &p, int elem_bytes, bool bases_aligned) {
    const dsc_axis_map &last = p.ax[DSC_REMAP_DIMS - 1];
    const long long row_bytes = (long long) last.n_out * elem_bytes;
    if (!bases_aligned || row_bytes % 16 != 0 || row_bytes / 16 < DSC_REMAP_MIN_PACKS) return DSC_REMAP_ELEMS;
    const long long packs = row_bytes / 16, rows = p.ne_out / last.n_out;
    if (rows * ((packs + 255) / 256) >= (1LL << 31)) return DSC_REMAP_ELEMS;
    if (dsc_map_is_identity(last)) return DSC_REMAP_ROWS;
    return elem_bytes < 16 ? DSC_REMAP_PACKS : DSC_REMAP_ELEMS;
}
