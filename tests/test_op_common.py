"""The integer rules of dsc_amd/csrc/op_common.h — dsc_chunk_lines and dsc_fused_rows_per_launch — against the formulas they replaced.

A stand-alone host program includes the arithmetic part of the header alone (DSC_OP_COMMON_PURE: nothing but <cstddef>), reads queries
from its standard input and prints the answers.  The expected values are the chunk formulas that stft.cpp, conv.cpp and hilbert.cpp each
carried, and the rows-per-launch formulas of stft.cpp and conv.cpp, written out below from the source of the commit before the header
existed.  Equality is exact."""
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
