"""The integer rules of dsc_amd/csrc/op_common.h — dsc_chunk_lines and dsc_fused_rows_per_launch — against the formulas they replaced.

A stand-alone host program includes the arithmetic part of the header alone (DSC_OP_COMMON_PURE: nothing but <cstddef>), reads queries
from its standard input and prints the answers.  The expected values are the chunk formulas that stft.cpp, conv.cpp and hilbert.cpp each
carried, and the rows-per-launch formulas of stft.cpp and conv.cpp, written out below from the source of the commit before the header
existed.  Equality is exact.

Likewise the rules of the axis operators: dsc_axis_view_on / dsc_axis_view_at against numpy's products around the axis,
dsc_reduced_shape against numpy.sum's shape and against the block that reduce_entry (dsc_capi.cpp) and moments.cpp each carried, and
dsc_route_index."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ALIGN = 256
CHUNK_CAP = 128 << 20
HUGE = (1 << 63) - 1

PROGRAM = r'''
#define DSC_OP_COMMON_PURE
#include "op_common.h"
#include <climits>
#include <cstdio>
int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'c') {            // fixed line reserve n_lines count capacity...: the rule, and the rule as hilbert.cpp bounds it
            unsigned long long fixed, line, reserve, capacity;
            long long n_lines, count;
            if (scanf("%llu %llu %llu %lld %lld", &fixed, &line, &reserve, &n_lines, &count) != 5) return 1;
            for (long long i = 0; i < count; ++i) {
                if (scanf("%llu", &capacity) != 1) return 1;
                long long rounded = dsc_chunk_lines(capacity, fixed, line, reserve, LLONG_MAX);
                if (rounded > 4) rounded &= ~3LL;
                if (rounded > n_lines) rounded = n_lines;
                printf("%lld %lld\n", dsc_chunk_lines(capacity, fixed, line, reserve, n_lines), rounded);
            }
        } else if (what == 'v') {     // s0 s1 s2 s3 n_dim axis: the view, slot n outer inner
            int s[4], n_dim, axis;
            if (scanf("%d %d %d %d %d %d", &s[0], &s[1], &s[2], &s[3], &n_dim, &axis) != 6) return 1;
            const dsc_axis_view v = dsc_axis_view_on(s, n_dim, axis);
            printf("%d %d %lld %lld\n", v.slot, v.n, v.outer, v.inner);
        } else if (what == 's') {     // s0 s1 s2 s3 n_dim slot keep_dims: the reduced shape, rank and four slots, and the view at the slot
            int s[4], n_dim, slot, keep, o[5] = {-7, -7, -7, -7, -7};
            if (scanf("%d %d %d %d %d %d %d", &s[0], &s[1], &s[2], &s[3], &n_dim, &slot, &keep) != 7) return 1;
            const int rank = dsc_reduced_shape(s, n_dim, slot, keep != 0, o);
            if (o[4] != -7) return 2;
            const dsc_axis_view v = dsc_axis_view_at(s, slot);
            printf("%d %d %d %d %d %d %d %lld %lld\n", rank, o[0], o[1], o[2], o[3], v.slot, v.n, v.outer, v.inner);
        } else if (what == 'n') {     // count value name...; "-" stands for the empty string
            char value[32], names[4][32];
            const char *list[4];
            int count;
            if (scanf("%d %31s", &count, value) != 2 || count > 4) return 1;
            for (int i = 0; i < count; ++i) { if (scanf("%31s", names[i]) != 1) return 1; list[i] = names[i]; }
            printf("%d\n", dsc_route_index(value[0] == '-' ? "" : value, list, count));
        } else {                      // limit row_bytes_in row_bytes_out rows odd_rows
            long long limit, in, out, rows;
            int odd;
            if (scanf("%lld %lld %lld %lld %d", &limit, &in, &out, &rows, &odd) != 5) return 1;
            printf("%lld\n", dsc_fused_rows_per_launch(limit, in, out, rows, odd != 0));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp('op_common')
    src, exe = str(d / 'op_common_sweep.cpp'), str(d / 'op_common_sweep')
    open(src, 'w').write(PROGRAM)
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-I' + os.path.join(ROOT, 'dsc_amd', 'csrc'), src, '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(lines):
        r = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-400:])
        return np.array(r.stdout.split(), dtype=np.int64)
    return ask


# ---- the chunk formulas of the parent commit, over arrays of capacities; 0 where the operator exited with "scratch arena too small" ------

def _chunk(cap, line, reserve):
    """the part the three copies spelled alike: cap = what the arena has left for the chunk and the inner routes"""
    chunk = np.maximum(np.minimum(cap // 2, CHUNK_CAP) // line, 1)
    return np.minimum(chunk, (cap - reserve) // line)


def stft_chunk_frames(capacity, frame_b, n_lines):
    """stft.cpp chunk_frames: nothing else pinned"""
    reserve = 2 * frame_b + 4 * ALIGN
    chunk = np.minimum(_chunk(capacity, frame_b, reserve), n_lines)
    return np.where(capacity < frame_b + reserve, 0, chunk)


def conv_chunk(capacity, pinned, frame_b, n_lines):
    """conv.cpp, composed route of dsc_correlate: `pinned` = H and the reversed taps (bins csz + M rb), two blocks per chunk line"""
    cap = capacity - (pinned + 2 * ALIGN)
    reserve = 2 * frame_b + 4 * ALIGN
    chunk = np.minimum(_chunk(cap, 2 * frame_b, reserve), n_lines)
    return np.where(capacity < pinned + 2 * ALIGN + 2 * frame_b + reserve, 0, chunk)


def hilbert_chunk(capacity, h_b, y_b, w_b, rows):
    """hilbert.cpp: H pinned, a line is a filtered row of y_b bytes and a widened one of w_b (0 unless widened)"""
    frame_b = y_b + w_b
    reserve = 2 * y_b + 4 * ALIGN
    chunk = _chunk(capacity - (h_b + 3 * ALIGN), frame_b, reserve)
    chunk = np.where(chunk > 4, chunk & ~3, chunk)
    chunk = np.minimum(chunk, rows)
    return np.where(capacity < h_b + 3 * ALIGN + frame_b + reserve, 0, chunk)


MIB = 1 << 20
CAPACITIES = list(range(0, MIB + 1, 128)) + [64 * MIB, 200 * MIB + 12345, 256 * MIB, 256 * MIB + 4872, 257 * MIB + 1, 513 * MIB, (1 << 30) - 1, 2 << 30]
LINES = [256, 4096, 8192, MIB]
FIXED = [0, 4104 + 768, MIB]
N_LINES = [1, 3, 7, 10 ** 6]


def test_chunk_lines_is_the_three_formulas(program):
    """Every combination of line_bytes, fixed, n_lines and the two reserves the operators use (two more lines, as stft and hilbert, and
    one more line, as conv with its two blocks per line and hilbert with its widened rows), over the capacities and the two capacities
    around each combination's exit threshold."""
    queries, expect = [], []
    for line in LINES:
        for reserve in (2 * line + 4 * ALIGN, line + 4 * ALIGN):
            for fixed in FIXED:
                for n_lines in N_LINES:
                    edge = fixed + line + reserve
                    caps = np.array(CAPACITIES + [edge - 1, edge], dtype=np.int64)
                    queries.append('c %d %d %d %d %d %s' % (fixed, line, reserve, n_lines, len(caps), ' '.join(map(str, caps))))
                    wants = []                                     # (column of the program's output, expected values)
                    if reserve == 2 * line + 4 * ALIGN:
                        if fixed == 0:
                            wants.append((0, stft_chunk_frames(caps, line, n_lines)))
                        wants.append((1, hilbert_chunk(caps, fixed - 3 * ALIGN, line, 0, n_lines)))
                    else:
                        wants.append((0, conv_chunk(caps, fixed - 2 * ALIGN, line // 2, n_lines)))
                        wants.append((1, hilbert_chunk(caps, fixed - 3 * ALIGN, line // 2, line // 2, n_lines)))
                    for w in wants:
                        assert w[1][-2] == 0 and w[1][-1] >= 1, (fixed, line, reserve, n_lines)      # the exit threshold itself
                    expect.append(wants)
    got = program(queries).reshape(len(queries), -1, 2)
    assert got.shape[1] == len(CAPACITIES) + 2
    for q, g, wants in zip(queries, got, expect):
        for col, want in wants:
            bad = np.nonzero(g[:, col] != want)[0]
            assert bad.size == 0, (q[:60], col, bad[:5], g[bad[:5], col], want[bad[:5]])


def test_chunk_lines_takes_a_capacity_below_fixed(program):
    """capacity < fixed is a legal input: 0, not a difference that wrapped"""
    got = program(['c %d 256 1792 7 3 0 4095 4096' % 4096]).reshape(-1, 2)
    assert got.tolist() == [[0, 0], [0, 0], [0, 0]]


# ---- the rows-per-launch formulas of the parent commit; 0 where the condition of the fused route failed -------------------------------

def stft_rows_per_launch(n_fft, T, rb, rows):
    rows_per = (0x7f000000 - n_fft * rb) // (T * rb) - 1
    if rows_per > 1:
        rows_per &= ~1
    launch_aligned = rows_per != 1 or rows == 1 or (T & 1) == 0
    return rows_per if rows_per >= 1 and launch_aligned else 0


def conv_rows_per_launch(T, T_out, rb, rows):
    lim = 0x7f000000 - 32768 * rb
    rows_per = min(lim // (T * rb) - 1, lim // (T_out * rb) - 1)
    if rows_per > 1:
        rows_per &= ~1
    launch_aligned = rows_per != 1 or rows == 1 or ((T | T_out) & 1) == 0
    return rows_per if rows_per >= 1 and launch_aligned else 0


# 180_000_000 and 180_000_001: f32 rows of which the limit holds two, one per launch after the spare row — the odd-row case
LENGTHS = [1, 2, 1023, 1024, (1 << 20) + 1, 1 << 28, (1 << 29) - 1, 180_000_000, 180_000_001]


def test_fused_rows_per_launch_is_the_two_formulas(program):
    queries, want = [], []
    for rb in (4, 8):
        for rows in (1, 2, 3):
            for T in LENGTHS:
                for n_fft in (64, 32768):                           # stft: no output limit
                    queries.append('r %d %d 0 %d %d' % (0x7f000000 - n_fft * rb, T * rb, rows, T & 1))
                    want.append(stft_rows_per_launch(n_fft, T, rb, rows))
                for T_out in LENGTHS:
                    queries.append('r %d %d %d %d %d' % (0x7f000000 - 32768 * rb, T * rb, T_out * rb, rows, (T | T_out) & 1))
                    want.append(conv_rows_per_launch(T, T_out, rb, rows))
    got = program(queries)
    assert got.tolist() == want
    assert 1 in want and 0 in want and max(want) > 1000               # every kind of answer occurs


# ---- the axis rules: a view along one axis, the shape of a reduction's result, a route name's index -------------------------------------

EXTENTS = (1, 2, 3, 5)
SHAPES = [s for n_dim in (1, 2, 3, 4) for s in np.ndindex(*(len(EXTENTS),) * n_dim)]
SHAPES = [tuple(EXTENTS[i] for i in s) for s in SHAPES]


def _slots(shape):
    return (1,) * (4 - len(shape)) + tuple(shape)


def _axis_slot(n_dim, axis):
    """dsc_axis_slot (dsc_internal.h)"""
    return 4 + axis if axis < 0 else 4 - n_dim + axis


def test_axis_view_is_numpys_outer_n_inner(program):
    """every rank, extents of 1, 2, 3 and 5, every axis from one below the valid range to one above it"""
    queries, want = [], []
    for shape in SHAPES:
        n_dim = len(shape)
        for axis in range(-n_dim - 1, n_dim + 1):
            queries.append('v %d %d %d %d %d %d' % (_slots(shape) + (n_dim, axis)))
            if -n_dim <= axis < n_dim:
                a = axis % n_dim
                want.append([_axis_slot(n_dim, axis), shape[a], int(np.prod(shape[:a], dtype=np.int64)), int(np.prod(shape[a + 1:], dtype=np.int64))])
            else:
                want.append([-1, 0, 0, 0])
    got = program(queries).reshape(-1, 4)
    assert got.tolist() == want
    assert sum(w[0] == -1 for w in want) == 2 * len(SHAPES)


def test_axis_view_refuses_a_rank_outside_1_to_4(program):
    got = program(['v 1 1 1 1 0 0', 'v 1 1 1 1 0 -1', 'v 2 2 2 2 5 0', 'v 2 2 2 2 5 4', 'v 2 2 2 2 -1 0']).reshape(-1, 4)
    assert got[:, 0].tolist() == [-1] * 5


def reduce_entry_shape(slots, n_dim, slot, keep_dims):
    """the keep-dims / drop-axis block of reduce_entry (dsc_capi.cpp) in the commit before the header had it"""
    out_shape = [None] * 4
    out_ndim = n_dim
    if keep_dims:
        out_shape = list(slots)
        out_shape[slot] = 1
    else:
        out_ndim -= 1
        lead = 4 - out_ndim
        for i in range(lead):
            out_shape[i] = 1
        oi = 0
        for xi in range(4 - n_dim, 4):
            if xi == slot:
                continue
            out_shape[lead + oi] = slots[xi]
            oi += 1
    return [out_ndim] + out_shape


def test_reduced_shape_is_numpys_and_reduce_entrys(program):
    """the same sweep over the valid axes, times keep_dims; the view at the slot is the view along the axis"""
    queries, cases = [], []
    for shape in SHAPES:
        n_dim = len(shape)
        for axis in range(-n_dim, n_dim):
            for keep in (0, 1):
                queries.append('s %d %d %d %d %d %d %d' % (_slots(shape) + (n_dim, _axis_slot(n_dim, axis), keep)))
                cases.append((shape, axis, keep))
    got = program(queries).reshape(-1, 9).tolist()
    for (shape, axis, keep), g in zip(cases, got):
        n_dim, slot = len(shape), _axis_slot(len(shape), axis)
        want = np.sum(np.empty(shape), axis, keepdims=bool(keep)).shape
        rank, out_shape = g[0], g[1:5]
        assert rank == len(want) and tuple(out_shape[4 - rank:]) == want and out_shape[:4 - rank] == [1] * (4 - rank), (shape, axis, keep, g)
        assert g[:5] == reduce_entry_shape(_slots(shape), n_dim, slot, keep), (shape, axis, keep, g)
        a = axis % n_dim
        assert g[5:] == [slot, shape[a], int(np.prod(shape[:a], dtype=np.int64)), int(np.prod(shape[a + 1:], dtype=np.int64))]


def test_reduced_shape_keeps_a_padding_slot(program):
    """the reductions accept an axis in a leading padding slot with keep_dims: the shape as it is, a view of n = 1 around that slot"""
    got = program(['s 1 1 2 64 2 1 1', 's 1 1 2 64 2 0 1']).reshape(-1, 9).tolist()
    assert got == [[2, 1, 1, 2, 64, 1, 1, 1, 128], [2, 1, 1, 2, 64, 0, 1, 1, 128]]


def test_route_index(program):
    queries = ['n 2 rows rows tiles', 'n 2 tiles rows tiles', 'n 1 elems elems',       # known names
               'n 2 fast rows tiles', 'n 1 rows elems',                                # unknown
               'n 2 - rows tiles', 'n 1 - elems',                                      # the empty string
               'n 2 row rows tiles', 'n 2 tile rows tiles', 'n 2 rowss rows tiles', 'n 1 e elems']      # a prefix of a name, a name as a prefix
    assert program(queries).tolist() == [0, 1, 0, -1, -1, -1, -1, -1, -1, -1, -1]
