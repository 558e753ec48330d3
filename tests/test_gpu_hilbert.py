"""GPU tests of dsc_hilbert / dsc_envelope: every fused length (512 .. 32768, fft_regs_mid.hip) and a set of composed ones, both
dtypes, every row against the long-double reference ref_hilbert / ref_envelope of tests/test_hilbert_abi.py under that file's bound
hilbert_err with tests.test_filter_ref.TAU (f32 2e-6, f64 1e-14).

Calibration (worst err / bound per route over every case of this file, every row checked, on an MI355X):
    hilbert_regs        f32 0.160   f64 0.061
    envelope_regs       f32 0.380   f64 0.172
    hilbert_composed    f32 0.158   f64 0.064
    envelope_composed   f32 0.515   f64 0.257
The first run measured envelope_composed f32 1.34 and hilbert_composed f32 0.295, both at N = 131072 on the impulse row (one sample at
T / 3) of spiced_rows, the first in the element half of the envelope bound: there the bound is tau 8 ||x|| / sqrt(N) = 4.4e-8 at the
weak elements of a row whose largest values are 1 and 2 / pi, 0.37 ulp of 1.0, and an f32 transform of 17 stages does not give that (the
hand composition absolute(ifft(fft(x) * h)) measures 1.355 on the same row).  The composed route now filters f32 rows of N >= 131072 in
f64 and rounds y once (hilbert.cpp); those cases measure 0.02 since.  What is left above 0.5 is the same impulse row at
N = 65536 f32 through filter_64k_regs (0.36 on full and padded rows, 0.515 on rows of 65539 samples cropped to N): f32 rounding of a 65536-point kernel that the
existing filter tests hold to the same tau.

Every case asserts dsc.last_fft_path() (expect_path restates the routing), checks that the input is left bit for bit unchanged, that
the real part of hilbert is bit for bit the row as the transform read it, and repeats the call with out= the head of a larger
sentinel-filled buffer: the result must be bit-identical and nothing past it may change.  Steps that end a process (argument errors)
or need their own context (the tight arena) run in child processes."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import (CPX, F32, F64, assert_ends_the_process, assert_out_call, build_cpp_smoke, dsc, run_child,  # noqa: F401
                           sync_fixture)
from tests.test_filter_ref import TAU, used
from tests.test_hilbert_abi import FUSED_GROUP, KINDS, expect_path, hilbert_err, length_of, ref_envelope, ref_hilbert, spiced_rows

pytestmark = pytest.mark.gpu

FUSED_LENGTHS = sorted(FUSED_GROUP[F32])
SWITCH = 'DSC_NO_HILBERT_FUSED'
_sync = sync_fixture(SWITCH)


# ---------------------------------------------------------------------------------------------------- checks

def err_ratio(kind, yh, x, n, rows=None):
    """largest err / bound over the rows (all, or the listed ones)"""
    N = yh.shape[-1]
    y2, x2 = yh.reshape(-1, N), x.reshape(-1, x.shape[-1])
    if rows is not None:
        y2, x2 = y2[rows], x2[rows]
    xu = used(x2, N)
    tau = TAU[x.dtype]
    if kind == 'hilbert':
        return hilbert_err(y2.imag, ref_hilbert(x2, n).imag, xu, tau)
    return hilbert_err(y2, ref_envelope(x2, n), xu, tau, envelope=True)


def run_case(dsc, record_property, kind, x, n=None, rows=None, fused_off=False):
    """kind(x, n) on the GPU: the route, the shape and dtype, the input left alone, hilbert's real part the row itself, every (listed)
    row within the bound, and a second call into the head of a sentinel-filled buffer that must give the same bits and leave the
    tail alone.  Returns the result."""
    T = x.shape[-1]
    N = length_of(T, n)
    want_path = expect_path(kind, x.dtype, N, T, fused_off=fused_off)
    fn = getattr(dsc, kind)
    X = dsc.from_numpy(x)
    y = fn(X, n=n)
    path = dsc.last_fft_path()
    assert path == want_path, (kind, x.dtype, x.shape, n, path, want_path)
    yh = y.numpy()
    odt = CPX[x.dtype] if kind == 'hilbert' else x.dtype
    oshape = x.shape[:-1] + (N,)
    assert yh.shape == oshape and yh.dtype == odt, (yh.shape, yh.dtype, oshape, odt)
    assert X.numpy().tobytes() == x.tobytes(), 'the input changed'
    if kind == 'hilbert':
        assert np.ascontiguousarray(yh.real).tobytes() == used(x, N).tobytes(), 'the real part is not the row'
    del y

    def again(out):
        fn(X, n=n, out=out)
        assert dsc.last_fft_path() == want_path
    assert_out_call(dsc, again, oshape, odt, yh)

    r = err_ratio(kind, yh, x, n, rows)
    record_property(f'{want_path}:{x.dtype}', r)
    print(f'{want_path} {x.dtype} {x.shape} n={n}: err / bound = {r:.3g}')
    assert r <= 1, f'{want_path} {x.dtype} {x.shape} n={n}: err / bound = {r:.3g}'
    return yh


# ---------------------------------------------------------------------------------------------------- the fused lengths

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N', FUSED_LENGTHS)
def test_fused_lengths(dsc, record_property, kind, dt, N):
    """batches of 1, G - 1, G, G + 1 rows (G rows per workgroup) and one of more than two waves of workgroups over 256 CUs; every row
    of every batch against the reference"""
    rng = np.random.default_rng([KINDS.index(kind), dt.itemsize, N])
    G = FUSED_GROUP[dt][N]
    assert expect_path(kind, dt, N, N).endswith('_regs')
    for B in sorted({1, max(1, G - 1), G, G + 1, 7}):
        run_case(dsc, record_property, kind, spiced_rows(rng, B, N, dt))
    B = 2 * 256 * G * (2 if N <= 2048 else 1) + G + 1
    run_case(dsc, record_property, kind, spiced_rows(rng, B, N, dt))


# ---------------------------------------------------------------------------------------------------- padded and cropped

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N', [512, 2048, 4096, 32768])
def test_padded_and_cropped_with_explicit_n(dsc, record_property, kind, dt, N):
    """T one of N - 1, N / 2 + 1, N + 3 and 1 (odd and even row pitches: sample pairs that straddle the end of a row, rows that start on
    an odd element)"""
    rng = np.random.default_rng([KINDS.index(kind), dt.itemsize, N, 1])
    G = FUSED_GROUP[dt][N]
    for T in (N - 1, N // 2 + 1, N + 3, 1):
        run_case(dsc, record_property, kind, spiced_rows(rng, G + 6, T, dt), N)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_n_none_and_n_no_power_of_two(dsc, record_property, kind, dt):
    rng = np.random.default_rng([KINDS.index(kind), dt.itemsize, 2])
    for T in (1000, 3000):
        yh = run_case(dsc, record_property, kind, spiced_rows(rng, 9, T, dt), None)
        assert yh.shape[-1] == length_of(T)
        yh = run_case(dsc, record_property, kind, spiced_rows(rng, 9, T, dt), -1)
        assert yh.shape[-1] == length_of(T)
    assert run_case(dsc, record_property, kind, spiced_rows(rng, 9, 1000, dt), 600).shape[-1] == 1024
    assert run_case(dsc, record_property, kind, spiced_rows(rng, 9, 1000, dt), 5000).shape[-1] == 8192
    assert run_case(dsc, record_property, kind, spiced_rows(rng, 9, 300, dt), 100).shape[-1] == 128


# ---------------------------------------------------------------------------------------------------- composed lengths, batch shapes

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N', [2, 8, 64, 256, 65536, 131072])
def test_composed_lengths(dsc, record_property, kind, dt, N):
    rng = np.random.default_rng([KINDS.index(kind), dt.itemsize, N, 3])
    assert expect_path(kind, dt, N, N).endswith('_composed')
    rows = 11 if N <= 256 else 6
    run_case(dsc, record_property, kind, spiced_rows(rng, rows, N, dt))
    if N in (8, 256, 65536):                                   # padded and cropped, odd pitches
        run_case(dsc, record_property, kind, spiced_rows(rng, rows, N - 1, dt), N)
        run_case(dsc, record_property, kind, spiced_rows(rng, rows, N + 3, dt), N)


def test_composed_f32_65536_runs_the_fused_64k_filter(dsc):
    """the inner route of the composed f32 65536-point call is filter_64k_regs: the last path is overwritten by the operator, so it is
    looked at through the filter itself with the same H"""
    from tests.test_hilbert_abi import response
    N = 65536
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, N)).astype(np.float32)
    H = response(N).astype(np.complex64)
    y = dsc.filter_fft(dsc.from_numpy(x), dsc.from_numpy(H)).numpy()
    assert dsc.last_fft_path() == 'filter_64k_regs'
    z = dsc.hilbert(dsc.from_numpy(x)).numpy()
    assert dsc.last_fft_path() == 'hilbert_composed'
    assert z.imag.tobytes() == y.tobytes()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_batch_shapes(dsc, record_property, kind, dt):
    """[T], [B, T], [2, 3, T] and [2, 2, 3, T] on a fused and a composed length"""
    rng = np.random.default_rng([KINDS.index(kind), dt.itemsize, 5])
    for T in (1024, 64):
        for lead in ((), (5,), (2, 3), (2, 2, 3)):
            rows = int(np.prod(lead)) if lead else 1
            x = spiced_rows(rng, rows, T, dt).reshape(lead + (T,))
            run_case(dsc, record_property, kind, x)


# ---------------------------------------------------------------------------------------------------- known answers

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N', [64, 512, 4096, 32768, 65536])
def test_tones_have_known_answers(dsc, record_property, dt, N):
    """cos(2 pi m j / N) gives sin and a flat envelope of 1; a constant row c gives y = 0 and the envelope |c| within the bound; the
    all-zero row gives exactly zero"""
    j = np.arange(N)
    tones = [1, 5, N // 4, N // 2 - 1]
    x = np.zeros((len(tones) + 2, N), dt)
    for i, m in enumerate(tones):
        x[i] = np.cos(2 * np.pi * ((m * j) % N) / N)
    x[len(tones)] = -2.5
    z = run_case(dsc, record_property, 'hilbert', x)
    e = run_case(dsc, record_property, 'envelope', x)
    tol = 100 * np.finfo(dt).eps
    for i, m in enumerate(tones):
        assert np.max(np.abs(z[i].imag - np.sin(2 * np.pi * ((m * j) % N) / N))) <= tol, (dt, N, m)
        assert np.max(np.abs(e[i] - 1)) <= tol, (dt, N, m)
    assert not np.any(z[-1]) and not np.any(e[-1])


# ---------------------------------------------------------------------------------------------------- the switch, envelope against hilbert

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_switch_forces_the_composed_route(dsc, record_property, kind, dt):
    """DSC_NO_HILBERT_FUSED=1 is read at every call; both routes hold the bound, so they agree within twice of it"""
    rng = np.random.default_rng([KINDS.index(kind), dt.itemsize, 6])
    for N, T in ((512, 512), (4096, 4001), (32768, 32768)):
        x = spiced_rows(rng, 9, T, dt)
        fused = run_case(dsc, record_property, kind, x, N)
        os.environ[SWITCH] = '1'
        composed = run_case(dsc, record_property, kind, x, N, fused_off=True)
        os.environ.pop(SWITCH)
        xu = used(x, N)
        if kind == 'hilbert':
            assert hilbert_err(fused.imag, composed.imag.astype(np.longdouble), xu, 2 * TAU[dt]) <= 1
        else:
            assert hilbert_err(fused, composed.astype(np.longdouble), xu, 2 * TAU[dt], envelope=True) <= 1
        again = getattr(dsc, kind)(dsc.from_numpy(x), n=N)
        assert dsc.last_fft_path() == expect_path(kind, dt, N, T) and again.numpy().tobytes() == fused.tobytes()


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N,fused_off', [(512, False), (8192, False), (32768, False), (4096, True), (64, False), (65536, False)])
def test_envelope_against_absolute_of_hilbert(dsc, dt, N, fused_off):
    """the same route's two results: within the envelope bound (not bitwise: FMA contraction may differ between the two kernels)"""
    rng = np.random.default_rng([dt.itemsize, N, 7])
    x = spiced_rows(rng, 9, N, dt)
    if fused_off:
        os.environ[SWITCH] = '1'
    X = dsc.from_numpy(x)
    z = dsc.hilbert(X)
    assert dsc.last_fft_path() == expect_path('hilbert', dt, N, N, fused_off)
    a = dsc.absolute(z).numpy()
    e = dsc.envelope(X).numpy()
    assert dsc.last_fft_path() == expect_path('envelope', dt, N, N, fused_off)
    assert a.dtype == e.dtype == dt
    assert hilbert_err(e, a.astype(np.longdouble), x, TAU[dt], envelope=True) <= 1


# ---------------------------------------------------------------------------------------------------- child processes

TIGHT = r'''
import sys
import numpy as np
import dsc_amd as dsc
from scipy import signal
kind, dt, N, B = sys.argv[1], np.dtype(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
out_item = dt.itemsize * (2 if kind == 'hilbert' else 1)
dsc.init(B * N * dt.itemsize + B * N * out_item + (1 << 20), 1 << 20)
rng = np.random.default_rng(3)
x = rng.standard_normal((B, N)).astype(dt)
y = getattr(dsc, kind)(dsc.from_numpy(x))
print('path', dsc.last_fft_path())
yh = y.numpy()
want = signal.hilbert(x[:4].astype(np.float64), N)
if kind == 'envelope':
    want = np.abs(want)
err = np.linalg.norm(yh[:4] - want) / np.linalg.norm(want)
print('err', err)
assert err < (1e-5 if dt == np.dtype(np.float32) else 1e-12)
print('tight ok')
'''


@pytest.mark.parametrize('kind,dt,N', [('hilbert', 'float32', 4096), ('envelope', 'float32', 32768), ('hilbert', 'float64', 512),
                                       ('envelope', 'float64', 16384)])
def test_fused_route_needs_no_scratch(kind, dt, N):
    """a context with room for x, out and 1 MiB, and 1 MiB of scratch: the fused route runs; the composed one needs a chunk"""
    B = (32 << 20) // (N * np.dtype(dt).itemsize)
    r = run_child(TIGHT, args=(kind, dt, str(N), str(B)))
    assert r.returncode == 0 and 'tight ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    assert f'path {kind}_regs' in r.stdout


CHUNKS = r'''
import sys
import numpy as np
import dsc_amd as dsc
kind, scratch, src, dst = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
dsc.init(64 << 20, scratch)
y = getattr(dsc, kind)(dsc.from_numpy(np.load(src)))
print('path', dsc.last_fft_path())
np.save(dst, y.numpy())
print('chunks ok')
'''


def composed_chunk(capacity, N, T, dt):
    """rows per chunk of the composed route in a scratch arena of `capacity` bytes, before and after the rounding to a multiple of 4 and
    without the bound by the rows: hilbert.cpp's call of dsc_chunk_lines (op_common.h) restated.  Pinned next to the chunk: H, N / 2 + 1
    complex values, and 3 x 256 bytes of alignment slack; a line is a filtered row and, for f32 rows of 131072 points and more (filtered
    in f64), the widened row next to it; the inner routes keep two filtered rows and 1024 bytes."""
    frb = 8 if dt == F32 and N >= 131072 else dt.itemsize
    y_b = N * frb
    line = y_b + (min(T, N) + min(T, N) % 2) * frb * (frb != dt.itemsize)
    cap = capacity - ((N // 2 + 1) * 2 * frb + 768)
    reserve = 2 * y_b + 1024
    assert cap >= line + reserve
    chunk = max(1, min(min(cap // 2, 128 << 20) // line, (cap - reserve) // line))
    return chunk, chunk & ~3 if chunk > 4 else chunk


# (kind, dtype, N, rows, scratch bytes, rows per chunk before and after rounding).  N = 1024: capacity - (513 * 8 + 768) in
# [49152, 57344) for f32 and capacity - (513 * 16 + 768) in [98304, 114688) for f64 make half of it 6 rows of 4096 / 8192 bytes, rounded
# down to 4: chunks of 4, 4 and 3 rows.  N = 131072, f32: a line is 2 MiB (a filtered and a widened f64 row); capacity - (65537 * 16 +
# 768) = 9 MiB and a few bytes makes half of it 2 lines: chunks of 2, 2 and 1 rows.  About 5 MiB stay unpinned, less than the 8 MiB and more that the
# one-launch f64 transform of 131072 points asks for (dsc_fft_fused_l2_scratch_bytes), so the inner rfft / irfft take the two-pass route
# (r2c_2pass_regs / c2r_2pass_regs) with its one row of 65536 complex values, 1 MiB, per row of the chunk.
CHUNK_CASES = [('hilbert', F32, 1024, 11, 58112, (6, 4)), ('envelope', F32, 1024, 11, 58112, (6, 4)),
               ('hilbert', F64, 1024, 11, 115456, (6, 4)), ('envelope', F64, 1024, 11, 115456, (6, 4)),
               ('hilbert', F32, 131072, 5, 10486784, (2, 2))]


@pytest.mark.parametrize('kind,dt,N,rows,scratch,chunk', CHUNK_CASES, ids=str)
def test_composed_route_in_several_chunks(tmp_path, record_property, kind, dt, N, rows, scratch, chunk):
    """the composed route with fewer rows per chunk than rows: the q > 0 offsets into x, the widened chunk and out, the rounding of the chunk
    to a multiple of 4 and a shorter last chunk.  Every element of every row against the reference."""
    assert composed_chunk(scratch, N, N, dt) == chunk and chunk[1] < rows
    x = spiced_rows(np.random.default_rng([N, dt.itemsize, 11]), rows, N, dt)
    src, dst = str(tmp_path / 'x.npy'), str(tmp_path / 'y.npy')
    np.save(src, x)
    r = run_child(CHUNKS, env={SWITCH: '1'}, args=(kind, str(scratch), src, dst))
    assert r.returncode == 0 and 'chunks ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    assert f'path {kind}_composed' in r.stdout
    yh = np.load(dst)
    assert yh.shape == (rows, N) and yh.dtype == (CPX[dt] if kind == 'hilbert' else dt)
    ratio = err_ratio(kind, yh, x, None)
    record_property(f'{kind}_composed:{dt} (chunked)', ratio)
    print(f'{kind}_composed {dt} [{rows}, {N}] in chunks of {chunk[1]}: err / bound = {ratio:.3g}')
    assert ratio <= 1, ratio


ERRORS = {
    'hilbert_of_complex': ("dsc.hilbert(dsc.from_numpy(np.ones((2, 512), np.complex64)))", 'input must be real'),
    'envelope_of_complex': ("dsc.envelope(dsc.from_numpy(np.ones((2, 64), np.complex128)))", 'input must be real'),
    'one_sample': ("dsc.hilbert(dsc.from_numpy(np.ones((2, 1), np.float32)))", 'at least 2'),
    'n_is_one': ("dsc.envelope(dsc.from_numpy(np.ones((2, 512), np.float64)), n=1)", 'at least 2'),
    'out_shape': ("dsc.hilbert(dsc.from_numpy(np.ones((2, 512), np.float32)), out=dsc.from_numpy(np.ones((2, 256), np.complex64)))", 'out must have'),
    'out_dtype': ("dsc.hilbert(dsc.from_numpy(np.ones((2, 512), np.float32)), out=dsc.from_numpy(np.ones((2, 512), np.float32)))", 'out must have'),
    'envelope_out_dtype': ("dsc.envelope(dsc.from_numpy(np.ones((2, 64), np.float64)), out=dsc.from_numpy(np.ones((2, 64), np.float32)))",
                           'out must have'),
    'out_overlaps_x': ("X = dsc.from_numpy(np.ones((2, 512), np.float32))\ndsc.envelope(X, out=X)", 'out must not share memory with x'),
}


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_argument_errors_end_the_process(name):
    """like every operator: a message on stderr and exit status 1; nothing runs on the GPU after it"""
    assert_ends_the_process(*ERRORS[name], without_env=SWITCH)


def test_cpp_hilbert_smoke_on_the_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_hilbert_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'hilbert templates ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])


# ---------------------------------------------------------------------------------------------------- full size

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_full_size(dsc, dt):
    """x [8192, 32768] f32 (1 GiB; out 2 GiB) and the f64 half of it through hilbert_regs.  All rows: the real part bitwise, and Parseval
    in f64 on the host — sum y^2 = sum x^2 - ((sum x)^2 + (sum (-1)^j x_j)^2) / N, the energy of x without its bins 0 and N/2 — to the
    north-star tolerance; a seeded sample of rows including the first and last group against the reference."""
    N = 32768
    B = 8192 if dt == F32 else 4096
    rng = np.random.default_rng([dt.itemsize, 8])
    blk = spiced_rows(rng, 64, N, dt)
    gain = (1.0 + (np.arange(B) % 5) * 0.25).astype(dt)
    x = np.tile(blk, (B // 64, 1)) * gain[:, None]
    assert x.dtype == dt and x.nbytes == 1 << 30
    X = dsc.from_numpy(x)
    Z = dsc.hilbert(X)
    assert dsc.last_fft_path() == 'hilbert_regs'
    zh = Z.numpy()
    del Z
    assert zh.shape == (B, N) and zh.dtype == CPX[dt]
    sign = 1.0 - 2.0 * (np.arange(N) % 2)
    worst = 0.0
    for i in range(0, B, 256):
        xs = x[i:i + 256]
        assert np.ascontiguousarray(zh[i:i + 256].real).tobytes() == xs.tobytes(), 'the real part is not the input'
        x64, y64 = xs.astype(np.float64), zh[i:i + 256].imag.astype(np.float64)
        e_x = np.sum(x64 * x64, axis=-1)
        want = e_x - (np.sum(x64, axis=-1) ** 2 + np.sum(x64 * sign, axis=-1) ** 2) / N
        got = np.sum(y64 * y64, axis=-1)
        live = e_x > 0
        assert np.all(got[~live] == 0)
        worst = max(worst, float(np.max(np.abs(got[live] - want[live]) / e_x[live])))
    print(f'full size {dt}: Parseval {worst:.3g}')
    assert worst < (1e-5 if dt == F32 else 1e-12)
    rows = sorted({0, 1, 2, 3, 4, 5, 63, 64, B // 2 + 3, B - 2, B - 1} | set(int(i) for i in rng.integers(0, B, 8)))
    r = err_ratio('hilbert', zh, x, None, rows)
    print(f'full size {dt}: err / bound = {r:.3g}')
    assert r <= 1
    assert X.numpy().tobytes() == x.tobytes()
    del zh
    E = dsc.envelope(X)
    assert dsc.last_fft_path() == 'envelope_regs'
    eh = E.numpy()
    r = err_ratio('envelope', eh, x, None, rows)
    print(f'full size {dt}: envelope err / bound = {r:.3g}')
    assert r <= 1
