// polyphase.hip — the direct (non-FFT) polyphase FIR kernel of dsc_upfirdn / dsc_resample_poly / dsc_decimate (resample.cpp;
// include/dsc_mi355x.h, Section H).  One primitive, along the last axis of x [rows][T]:
//
//   y[r][m] = sum_i (h[t - i up] gain) x[r][i],   t = m down + t0,   over 0 <= i < T and 0 <= t - i up < M;   0 <= m < T_out.
//
// With i_hi = t / up and p = t % up this is a K-term dot product, K = ceil(M / up):
//   y[r][m] = sum_{j < K} hp[p][j] x[r][i_hi - j],   hp[p][j] = h[p + j up] gain (zero past M),   x zero outside [0, T):
// only the taps of phase p meet nonzero samples of the zero-stuffed row, and only every down-th output is formed.
//
// Tiling.  A workgroup (S active threads, launched as S rounded up to whole waves, at most 256) forms TILE = S R consecutive outputs of one row; the grid is the flattened
// (row, tile) index.  The taps are staged in LDS once per workgroup, multiplied by gain (one rounding, in the data's type), and so are
// the samples the tile needs — 16-byte loads wherever the row base allows, the unaligned head, the tail and everything that touches
// the ends of the row element by element, zeros outside [0, T) — so the tap loops have no bounds test.  R is 4, 2 or 1.
//
//   up > 1.  Thread u owns outputs o = u + r S, r < R; S is a multiple of up whenever R > 1, so a thread's outputs share the phase p,
//   each tap it reads is used R times, and its sample index steps by the integer S down / up from one output to the next.  For a fixed
//   r the lanes of a wave store consecutive outputs.  Taps are phase-major with K rounded up to a multiple of 4 (K4, zero filled: the
//   tap loop runs in steps of 4 without a remainder) and an odd pitch: the lanes of a wave hold phases (p0 + l down) mod up, and an
//   odd pitch puts phases that differ mod 32 on different banks.  x is staged linearly; lane l reads sample i_hi(l) - j with i_hi(l)
//   advancing by down / up per lane (the rate pair is reduced, so this is no multiple of a power of two; below 1 neighbouring lanes
//   share a word, which the LDS broadcasts).  (1 + R) / R LDS reads per FMA.
//
//   up == 1 (UP1: decimation and plain FIR).  Every lane uses the same tap: a wave-uniform LDS address served by the broadcast.  The
//   samples are staged DE-INTERLEAVED by down: sample s of the span sits in sub-row s % down at word s / down, so that
//       y[o] = sum_{c < down} sum_d g[c][d] xs[c][o + d],   g[c][d] = h[K4 - 1 - c - d down] gain  (zero outside [0, M))
//   — `down` short correlations along contiguous sub-rows, whatever the decimation factor.  Thread u owns the R CONSECUTIVE outputs
//   o = R u .. R u + R - 1 and walks each sub-row with a sliding register window: per R taps it reads R taps (one wave-uniform vector
//   read) and R new samples (one vector read, 16-byte aligned: the pitch and the taps per sub-row are multiples of 4, lanes read
//   consecutive vectors, conflict free) for R R FMAs: 2 / R LDS words, 2 / R^2 read instructions per FMA.  The R outputs are stored
//   as one vector where the row's base allows (consecutive lanes, consecutive 16 bytes), element by element otherwise.  The sub-row
//   pitch is = max(ceil(32 / down), R) mod 32, which spreads the sub-rows a wave writes to while staging over the banks.
//   The taps per sub-row are rounded up to a multiple of 4 with zeros.
//
// Padding taps are zeros that meet real samples just outside the filter's support: a non-finite sample spreads that much further than
// in an exact sum.  No atomics, every output written once, accumulation in a fixed order in the data's type: results are deterministic.
#include "dispatch.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kThreads = 256;

template<typename R>
struct pack_of {
    static constexpr int n = 16 / (int) sizeof(R);
    typedef R type __attribute__((ext_vector_type(16 / sizeof(R))));
};

// up == 1: pitch of a sub-row of `rowlen` words (a multiple of 4) in the de-interleaved layout: the smallest one >= rowlen that is
// = max(ceil(32 / down), rb) rounded up to a multiple of rb, mod 32
__host__ __device__ inline int xs_pitch(int rowlen, int down, int rb) {
    if (down == 1) return rowlen;
    const int q = (32 + down - 1) / down;
    const int target = ((q > rb ? q : rb) + rb - 1) / rb * rb;
    return rowlen + ((target - rowlen) % 32 + 32) % 32;
}

struct poly_args {
    const void *x;
    const void *h;
    void *y;
    double gain;
    long long n_tiles;      // tiles per row
    long long T, T_out, t0;
    int M, up, down;
    int K4;                 // taps per phase, rounded up to a multiple of 4
    int hp_pitch;           // elements between phases in LDS (odd); up == 1: taps per sub-row, a multiple of 4
    int S;                  // active threads = outputs per register slot
    int span;               // x samples staged per tile; up == 1: down sub-rows of rowlen = span / down words
    int step;               // S down / up: sample step between a thread's outputs (RB > 1)
    int hp_elems;           // LDS elements of the taps, a multiple of the 16-byte pack
};

template<typename R, int RB, bool UP1>
__global__ __launch_bounds__(kThreads) void polyphase_kernel(const poly_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    R *hp = (R *) lds_raw;
    R *xs = hp + a.hp_elems;
    const int tid = (int) threadIdx.x, nt = (int) blockDim.x;    // nt: S rounded up to whole waves
    const long long row = (long long) blockIdx.x / a.n_tiles;
    const long long tile = (long long) blockIdx.x - row * a.n_tiles;
    const long long m0 = tile * ((long long) a.S * RB);
    const long long tb = m0 * a.down + a.t0;                // t of the tile's first output
    const long long ib = tb / a.up;
    const int pb = (int) (tb - ib * a.up);
    const long long i_lo = ib - (a.K4 - 1);                 // first staged sample (may be negative)
    const int di = UP1 ? a.down : 1;
    const int pitch = UP1 ? xs_pitch(a.span / a.down, a.down, RB) : a.span;

    // ---- taps: hp[p][j] = h[p + j up] gain, zero past M; up == 1: g[c][d] = h[K4 - 1 - c - d down] gain, zero outside [0, M)
    {
        const R *h = (const R *) a.h;
        const R g = (R) a.gain;
        const int n = (UP1 ? a.down : a.up) * a.hp_pitch;
        for (int e = tid; e < a.hp_elems; e += nt) {
            R v = (R) 0;
            if (e < n) {
                const int p = e / a.hp_pitch, j = e - p * a.hp_pitch;
                const long long k = UP1 ? (long long) a.K4 - 1 - p - (long long) j * a.down : (long long) p + (long long) j * a.up;
                if ((UP1 || j < a.K4) && k >= 0 && k < a.M) v = h[k] * g;
            }
            hp[e] = v;
        }
    }

    // ---- samples: xs[pos(s)] = x[row][i_lo + s], zero outside the row
    {
        constexpr int V = pack_of<R>::n;
        typedef typename pack_of<R>::type pack;
        const R *xr = (const R *) a.x + row * a.T;
        const long long g0 = row * a.T + i_lo;              // element index of s = 0 from the (16-byte aligned) base of x
        const bool base_ok = ((uintptr_t) a.x & 15) == 0;
        const int head = (int) (((-g0) % V + V) % V);       // first s whose element is 16-byte aligned
        const int n_chunks = (a.span - head + V - 1) / V + 1;
        for (int c = tid; c < n_chunks; c += nt) {
            const int s0 = head - V + c * V;
            const long long i0 = i_lo + s0;
            R v[V];
            if (base_ok && s0 >= 0 && s0 + V <= a.span && i0 >= 0 && i0 + V <= a.T) {
                const pack q = *(const pack *) (xr + i0);
#pragma unroll
                for (int e = 0; e < V; ++e) v[e] = q[e];
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const long long i = i0 + e;
                    v[e] = (s0 + e >= 0 && s0 + e < a.span && i >= 0 && i < a.T) ? xr[i] : (R) 0;
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int s = s0 + e;
                if (s >= 0 && s < a.span) {
                    if (UP1 && di > 1) {
                        const int d = s / di;
                        xs[(s - d * di) * pitch + d] = v[e];     // sub-row s % down, word s / down
                    } else {
                        xs[s] = v[e];
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid >= a.S) return;

    R acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = (R) 0;

    if constexpr (UP1) {
        // R consecutive outputs o = RB tid + r; sub-row c: y[o + r] += g[c][d] xs[c][o + r + d], a window of 2 RB - 1 words sliding by RB
        // 16-byte alignment is all the LDS layout guarantees (the f64 vector of 4 is 32 bytes long)
        typedef R vec_n __attribute__((ext_vector_type(RB > 1 ? RB : 2)));
        typedef vec_n vec __attribute__((aligned((RB > 1 ? RB : 2) * sizeof(R) < 16 ? (RB > 1 ? RB : 2) * sizeof(R) : 16)));
        const R *xo = xs + RB * tid;
        for (int c = 0; c < di; ++c) {
            const R *xc = xo + c * pitch;
            const R *gc = hp + c * a.hp_pitch;
            R win[2 * RB];
            if constexpr (RB > 1) {
                const vec w0 = *(const vec *) xc;
#pragma unroll
                for (int e = 0; e < RB; ++e) win[e] = w0[e];
            } else {
                win[0] = xc[0];
            }
            for (int d = 0; d < a.hp_pitch; d += RB) {
                R t[RB];
                if constexpr (RB > 1) {
                    const vec t4 = *(const vec *) (gc + d);         // wave-uniform address: one broadcast read for RB taps
                    const vec w1 = *(const vec *) (xc + d + RB);
#pragma unroll
                    for (int e = 0; e < RB; ++e) { t[e] = t4[e]; win[RB + e] = w1[e]; }
                } else {
                    t[0] = gc[d];
                    win[1] = xc[d + 1];
                }
#pragma unroll
                for (int e = 0; e < RB; ++e)
#pragma unroll
                    for (int r = 0; r < RB; ++r) acc[r] += t[e] * win[e + r];
#pragma unroll
                for (int e = 0; e < RB; ++e) win[e] = win[RB + e];
            }
        }
    } else {
        long long tt = (long long) pb + (long long) tid * a.down;
        const int di_hi = (int) (tt / a.up);
        const int p = (int) (tt - (long long) di_hi * a.up);
        const R *hq = hp + p * a.hp_pitch;
        const R *xq = xs + (a.K4 - 1) + di_hi;
        if constexpr (RB > 1) {
            for (int j = 0; j < a.K4; j += 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const R t = hq[j + e];
#pragma unroll
                    for (int r = 0; r < RB; ++r) acc[r] += t * xq[r * a.step - (j + e)];
                }
            }
        } else {
            for (int j = 0; j < a.K4; j += 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[0] += hq[j + e] * xq[-(j + e)];
            }
        }
    }

    R *yr = (R *) a.y + row * a.T_out;
    if constexpr (UP1 && RB > 1) {
        typedef R vec __attribute__((ext_vector_type(RB)));
        typedef vec vec_a __attribute__((aligned(RB * sizeof(R) < 16 ? RB * sizeof(R) : 16)));
        const long long m = m0 + (long long) RB * tid;
        R *dst = yr + m;
        if (m + RB <= a.T_out && ((uintptr_t) dst & (sizeof(vec_a) < 16 ? sizeof(vec_a) - 1 : 15)) == 0) {
            vec v;
#pragma unroll
            for (int r = 0; r < RB; ++r) v[r] = acc[r];
            *(vec_a *) dst = v;
        } else {
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (m + r < a.T_out) dst[r] = acc[r];
        }
    } else {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const long long m = m0 + tid + (long long) r * a.S;
            if (m < a.T_out) yr[m] = acc[r];
        }
    }
}

constexpr size_t kLdsMax = (size_t) 160 << 10;            // the LDS of a CU: the most one workgroup can take
constexpr size_t kLdsTwo = kLdsMax / 2;                   // two workgroups per CU

// outputs per thread -> RB of polyphase_kernel; another count ends the process
template<typename F> void with_poly_rb(int RB, F f) {
    switch (RB) {
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        case 4: return f(int_c<4>{});
    }
    no_kernel("polyphase.hip", "outputs per thread", RB);
}

// LDS bytes of a tile of S * RB outputs; fills the tile fields of a.  0 = the sizes do not fit an int
size_t tile_bytes(poly_args &a, int S, int RB, size_t elem) {
    const int V = 16 / (int) elem;
    const long long tile = (long long) S * RB;
    long long span, hp, xs;
    if (a.up == 1) {
        const long long dmax = ((long long) a.K4 + a.down - 1) / a.down;
        const long long dmax4 = (dmax + 3) / 4 * 4;
        const long long rowlen = tile + dmax4;                  // words o + d + r the window loop reads, o < tile: a multiple of 4
        if (rowlen > (1 << 24) || dmax4 * a.down > (1 << 24) || rowlen * a.down > (1 << 24)) return 0;
        a.hp_pitch = (int) dmax4;
        hp = ((long long) a.down * dmax4 + V - 1) / V * V;
        span = rowlen * a.down;
        xs = (long long) a.down * xs_pitch((int) rowlen, a.down, RB);
    } else {
        span = ((long long) a.up - 1 + (tile - 1) * a.down) / a.up + a.K4;
        hp = ((long long) a.up * a.hp_pitch + V - 1) / V * V;
        if (span > (1 << 24) || hp > (1 << 24)) return 0;
        xs = span;
    }
    a.S = S;
    a.span = (int) span;
    a.step = RB > 1 ? (int) ((long long) S * a.down / a.up) : 0;
    a.hp_elems = (int) hp;
    return (size_t) (hp + xs) * elem;
}

}  // namespace

size_t dsc_polyphase_lds_limit() { return kLdsMax; }

bool dsc_launch_polyphase(const void *x, const void *h, void *y, long long rows, long long T, long long T_out, int M, int up, int down, long long t0,
                          double gain, bool single_precision, hipStream_t stream) {
    if (rows <= 0 || T_out <= 0) return true;
    const size_t elem = single_precision ? 4 : 8;
    poly_args a{};
    a.x = x; a.h = h; a.y = y; a.gain = gain;
    a.T = T; a.T_out = T_out; a.t0 = t0;
    a.M = M; a.up = up; a.down = down;
    const long long K = ((long long) M + up - 1) / up;
    a.K4 = (int) ((K + 3) / 4 * 4);
    a.hp_pitch = a.K4 | 1;                                  // up == 1: set with the tile

    // the tile: R = 4, 2, 1 outputs per thread (up > 1: S a multiple of up when a thread has more than one), the first that is not more
    // than the row needs and leaves room for two workgroups per CU, else the first that fits the LDS at all; then one output per thread
    // and ever fewer threads, down to 64
    int RB = 0;
    size_t lds = 0;
    for (const size_t budget : {kLdsTwo, kLdsMax}) {
        for (const int rb : {4, 2, 1}) {
            if (RB != 0) break;
            const int S = (rb > 1 && up > 1 && up <= kThreads) ? up * (kThreads / up) : kThreads;
            if (rb > 1 && (S % up != 0 || (long long) S * (rb / 2) >= T_out)) continue;
            const size_t b = tile_bytes(a, S, rb, elem);
            if (b != 0 && b <= budget) { RB = rb; lds = b; }
        }
    }
    for (int S = kThreads - 64; RB == 0 && S >= 64; S -= 64) {
        const size_t b = tile_bytes(a, S, 1, elem);
        if (b != 0 && b <= kLdsMax) { RB = 1; lds = b; }
    }
    if (RB == 0) return false;

    a.n_tiles = (T_out + (long long) a.S * RB - 1) / ((long long) a.S * RB);
    const long long blocks = rows * a.n_tiles;
    if (blocks > 0x7fffffffLL) {                          // cannot happen below the tensor size limit (tiles <= T_out)
        fprintf(stderr, "dsc_launch_polyphase: %lld workgroups exceed the grid limit\n", blocks);
        exit(EXIT_FAILURE);
    }
    const unsigned grid = (unsigned) blocks;
    // the LDS size differs from launch to launch: the kernel is opted in to the whole 160 KiB
    with_real(single_precision, [&](auto real) { with_poly_rb(RB, [&](auto rb) { with_bool(up == 1, [&](auto up1) {
        dsc_launch_var_lds<polyphase_kernel<decltype(real), decltype(rb)::value, decltype(up1)::value>, kLdsMax>(grid, (a.S + 63) / 64 * 64, lds, stream, a);
    }); }); });
    return true;
}
