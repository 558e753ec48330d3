"""GPU tests of dsc_cumsum / dsc_diff / dsc_unwrap / dsc_phase (scan.hip, scan.cpp), every element checked, with the references and
checks of tests/test_scan_abi.py:
    cumsum   scan_rows / scan_tiles: |out[k] - ref[k]| <= gamma_k A[k] per component (cumsum_err), element 0 a copy, zero rows exactly
             zero; scan_cols: bitwise numpy.cumsum of the same dtype
    diff     bitwise numpy.diff
    unwrap   the exact integers K of the definition and |out - ref| <= u |ref| + 4 2^-53 (|x| + TWO_PI |K|) (unwrap_err), on inputs that
             assert_away_from_ties accepts; scan_rows, scan_tiles and the transposed scan_cols call give the same bits
    phase    bitwise dsc.unwrap(dsc.angle(z)) on every route; diff(phase(hilbert(x))) against numpy / scipy in double

Calibration (worst err / bound per operator and dtype over every case of this file, on an MI355X; none above 1):
    cumsum   f32 0.988   f64 0.998   c32 0.9996   c64 0.99996     (scan_tiles / scan_rows, [300, 4097] and [3, 65535])
    unwrap   f32 0.9996  f64 0.200                                (scan_tiles, [300, 4097])
    diff(phase(hilbert))   f32 0.838   f64 0.747 of the derived tolerance
Ratios this close to 1 are what the cumsum bound gives at small k: at k = 1 the one rounding of x[0] + x[1], at most u |x[0] + x[1]|,
stands against gamma_1 A[1] = u / (1 - u) (|x[0]| + |x[1]|), and the two meet when the terms have one sign and the rounding is a full
half unit, so more rows bring the maximum closer to 1.  The bound is rigorous for every order of summation: a correct scan cannot
exceed it, and a dropped carry misses it by orders of magnitude (tests/test_scan_abi.py).  The f32 unwrap ratio is the final rounding
to f32, the bound's first term; in f64 the one rounding of the FMA uses a fifth of what the bound allows a product and a subtraction.

Every case asserts dsc.last_fft_path(), checks that the input is left bit for bit unchanged, and repeats the call with out= the head of
a larger sentinel-filled buffer: the result must be bit-identical and nothing past it may change.  DSC_SCAN_ROUTE forces scan_rows or
scan_tiles on the inner == 1 shapes.  Argument errors end the process and run in child processes."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import assert_ends_the_process, build_cpp_smoke, device_view, dsc, sync_fixture  # noqa: F401
from tests.test_scan_abi import (C32, C64, F32, F64, UNIT, assert_away_from_ties, cumsum_err, cumsum_rows, multi_wrap_rows, ref_unwrap,
                                 smooth_rows, unwrap_err, wrapped_chirps)

pytestmark = pytest.mark.gpu

ROWS, TILES, COLS, DIFF = 'scan_rows', 'scan_tiles', 'scan_cols', 'scan_diff'
# every length around a power of two up to 2^16, and 70001: the pack, wave, chunk and tile boundaries of every dtype lie among them
T_LAST = sorted({t for k in range(17) for t in (2 ** k - 1, 2 ** k, 2 ** k + 1) if t >= 1} | {70001})
REAL_OF = {C32: F32, C64: F64}
_sync = sync_fixture('DSC_SCAN_ROUTE')


def force(route):
    if route in (ROWS, TILES):
        os.environ['DSC_SCAN_ROUTE'] = route[5:]
    else:
        os.environ.pop('DSC_SCAN_ROUTE', None)


def run(dsc, op, x, axis, path, forced=True):
    """getattr(dsc, op)(x, axis) on the GPU: the route, the shape and dtype, the input left alone, and a second call into the head of a
    sentinel-filled buffer that must give the same bits and leave the tail alone.  Returns the result."""
    force(path if forced else None)
    f = getattr(dsc, op)
    odt = REAL_OF[x.dtype] if op == 'phase' else x.dtype
    oshape = list(x.shape)
    if op == 'diff':
        oshape[axis] -= 1
        path = DIFF
    oshape = tuple(oshape)
    X = dsc.from_numpy(x)
    y = f(X, axis=axis)
    assert dsc.last_fft_path() == path, (op, x.shape, axis, dsc.last_fft_path(), path)
    yh = y.numpy()
    assert yh.shape == oshape and yh.dtype == odt, (op, yh.shape, yh.dtype, oshape)
    assert X.numpy().tobytes() == x.tobytes(), 'the input changed'
    del y
    extra = 1031
    size = int(np.prod(oshape))
    big = dsc.from_numpy(np.full(size + extra, -7.25, dtype=odt))
    out = device_view(dsc, big, oshape, odt)
    f(X, axis=axis, out=out)
    assert dsc.last_fft_path() == path
    whole = big.numpy()
    assert whole[:size].tobytes() == yh.tobytes(), 'two identical calls differ (or out= was not written)'
    assert np.all(whole[size:] == -7.25), 'bytes past the output changed'
    del out, big
    return yh


def check_cumsum(dsc, record_property, x, axis, path, forced=True):
    yh = run(dsc, 'cumsum', x, axis, path, forced)
    if path == COLS:
        assert yh.tobytes() == np.cumsum(x, axis=axis, dtype=x.dtype).tobytes(), (x.shape, axis)
        return yh
    r = cumsum_err(yh, x, axis)
    record_property(f'cumsum:{x.dtype}', r)
    print(f'cumsum {path} {x.dtype} {x.shape} axis={axis}: err / bound = {r:.4g}')
    assert r <= 1, f'cumsum {path} {x.dtype} {x.shape} axis={axis}: err / bound = {r:.4g}'
    return yh


def check_unwrap(dsc, record_property, x, axis, path, forced=True):
    assert_away_from_ties(x, axis)
    yh = run(dsc, 'unwrap', x, axis, path, forced)
    r = unwrap_err(yh, x, axis)
    record_property(f'unwrap:{x.dtype}', r)
    print(f'unwrap {path} {x.dtype} {x.shape} axis={axis}: err / bound = {r:.4g}')
    assert r <= 1, f'unwrap {path} {x.dtype} {x.shape} axis={axis}: err / bound = {r:.4g}'
    return yh


def check_phase(dsc, z, axis, path, forced=True):
    """bitwise the two-operator composition, forced onto the same route"""
    yh = run(dsc, 'phase', z, axis, path, forced)
    force(path if forced else None)
    want = dsc.unwrap(dsc.angle(dsc.from_numpy(z)), axis=axis)
    assert dsc.last_fft_path() == path
    assert yh.tobytes() == want.numpy().tobytes(), ('phase', z.dtype, z.shape, axis, path)
    return yh


def check_diff(dsc, x, axis):
    yh = run(dsc, 'diff', x, axis, DIFF)
    assert yh.tobytes() == np.diff(x, 1, axis=axis).tobytes(), ('diff', x.dtype, x.shape, axis)
    return yh


def phasors(rng, rows, T, dt, kind):
    """complex rows whose angle is a wrapped chirp or a walk of several periods per sample, moduli 0.5 .. 1.5"""
    true = {'chirps': wrapped_chirps, 'multi_wrap': multi_wrap_rows}[kind](rng, rows, T, F64)
    return np.ascontiguousarray((rng.uniform(0.5, 1.5, (rows, T)) * np.exp(1j * true)).astype(dt))


# ---------------------------------------------------------------------------------------------------- the last axis, every length

@pytest.mark.parametrize('route', [ROWS, TILES])
@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_cumsum_last_axis(dsc, record_property, dt, route):
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 1])
    for T in T_LAST:
        yh = check_cumsum(dsc, record_property, cumsum_rows(rng, 3, T, dt), -1, route)
        assert not np.any(yh[2]), 'a row of zeros must give exact zeros'


@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_diff_last_axis(dsc, dt):
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 2])
    for T in T_LAST:
        if T >= 2:
            check_diff(dsc, cumsum_rows(rng, 3, T, dt), -1)


@pytest.mark.parametrize('kind', ['chirps', 'multi_wrap', 'smooth'])
@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_unwrap_last_axis(dsc, record_property, dt, kind):
    """both forced routes and the transposed scan_cols call: the exact integers, the value bound, and one set of bits"""
    rng = np.random.default_rng([dt.itemsize, len(kind), 3])
    gen = {'chirps': wrapped_chirps, 'multi_wrap': multi_wrap_rows, 'smooth': smooth_rows}[kind]
    for T in T_LAST:
        x = gen(rng, 3, T, dt)
        a = check_unwrap(dsc, record_property, x, -1, ROWS)
        b = check_unwrap(dsc, record_property, x, -1, TILES)
        c = check_unwrap(dsc, record_property, np.ascontiguousarray(x.T), 0, COLS)
        assert a.tobytes() == b.tobytes() and a.tobytes() == np.ascontiguousarray(c.T).tobytes(), (kind, dt, T)
        if kind == 'smooth':
            assert a.tobytes() == x.tobytes(), 'rows without a jump must come back unchanged'


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_unwrap_passes_what_is_not_finite(dsc, record_property, dt):
    """a NaN and an Inf in the middle of a row: they come through, and the samples after them follow the definition (no NaN spreads)"""
    rng = np.random.default_rng([dt.itemsize, 4])
    for T in (300, 20001):
        x = multi_wrap_rows(rng, 3, T, dt)
        x[1, T // 3], x[1, T // 2], x[2, T - 2] = np.nan, np.inf, -np.inf
        outs = [check_unwrap(dsc, record_property, x, -1, route) for route in (ROWS, TILES)]
        outs.append(np.ascontiguousarray(check_unwrap(dsc, record_property, np.ascontiguousarray(x.T), 0, COLS).T))
        assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()
        assert np.isnan(outs[0][1, T // 3]) and np.all(np.isfinite(outs[0][1, T // 2 + 1:]))
        assert int(np.max(np.abs(ref_unwrap(x)[1][1, T // 2 + 2:]))) > 0


@pytest.mark.parametrize('route', [ROWS, TILES])
@pytest.mark.parametrize('kind', ['chirps', 'multi_wrap'])
@pytest.mark.parametrize('dt', [C32, C64], ids=str)
def test_phase_last_axis(dsc, dt, kind, route):
    rng = np.random.default_rng([dt.itemsize, len(kind), 5])
    for T in T_LAST:
        check_phase(dsc, phasors(rng, 3, T, dt, kind), -1, route)


# ---------------------------------------------------------------------------------------------------- rows

@pytest.mark.parametrize('rows', [1, 3, 300])
def test_row_counts(dsc, record_property, rows):
    """T = 4097 (odd: every row but the first starts off a pack boundary); 300 rows are more than the persistent grid has workgroups"""
    rng = np.random.default_rng([rows, 6])
    for route in (ROWS, TILES):
        for dt in (F32, F64, C32, C64):
            check_cumsum(dsc, record_property, cumsum_rows(rng, rows, 4097, dt), -1, route)
        for dt in (F32, F64):
            check_unwrap(dsc, record_property, multi_wrap_rows(rng, rows, 4097, dt), -1, route)
            check_unwrap(dsc, record_property, wrapped_chirps(rng, rows, 4096, dt), -1, route)          # ... and on the pack path
        for dt in (C32, C64):
            check_phase(dsc, phasors(rng, rows, 4097, dt, 'multi_wrap'), -1, route)
            check_phase(dsc, phasors(rng, rows, 4096, dt, 'chirps'), -1, route)
    check_diff(dsc, cumsum_rows(rng, rows, 4097, F32), -1)


def test_the_route_left_to_the_library(dsc, record_property):
    """few long rows take scan_tiles, rows of at most a tile and many rows take scan_rows"""
    rng = np.random.default_rng(7)
    check_cumsum(dsc, record_property, cumsum_rows(rng, 3, 70001, F32), -1, TILES, forced=False)
    check_cumsum(dsc, record_property, cumsum_rows(rng, 3, 4096, F64), -1, ROWS, forced=False)          # f64: a tile is 4096
    check_cumsum(dsc, record_property, cumsum_rows(rng, 300, 4097, C32), -1, ROWS, forced=False)
    check_unwrap(dsc, record_property, multi_wrap_rows(rng, 2, 70001, F64), -1, TILES, forced=False)
    check_phase(dsc, phasors(rng, 2, 70001, C32, 'chirps'), -1, TILES, forced=False)
    check_phase(dsc, phasors(rng, 2, 100, C64, 'chirps'), -1, ROWS, forced=False)


# ---------------------------------------------------------------------------------------------------- columns and other axes

@pytest.mark.parametrize('T', [1, 2, 65, 4097])
def test_columns(dsc, record_property, T):
    """[2, T, 5] on axis 1 and [T, 7] on axis 0 (scan_cols); [3, 1, T], [3, T, 1] and [T, 1]: inner == 1 reached through a unit axis"""
    rng = np.random.default_rng([T, 8])
    for shape, axis, path in (((2, T, 5), 1, COLS), ((T, 7), 0, COLS), ((3, 1, T), 2, ROWS), ((3, 1, T), 1, COLS), ((3, T, 1), 1, ROWS),
                              ((T, 1), 0, ROWS), ((T, 1), 0, TILES), ((3, T, 1), -2, TILES)):
        n = shape[axis]
        lead = int(np.prod(shape)) // n
        if path == COLS and int(np.prod(shape[axis % len(shape) + 1:])) == 1:
            path = ROWS                                             # T = 1: nothing is left behind the axis

        def lay(rows):                                              # rows [lead, n] -> the shape, the scanned axis in place
            return np.ascontiguousarray(np.moveaxis(rows.reshape([s for i, s in enumerate(shape) if i != axis % len(shape)] + [n]), -1, axis))

        for dt in (F32, F64, C32, C64):
            x = lay(cumsum_rows(rng, lead, n, dt))
            check_cumsum(dsc, record_property, x, axis, path)
            if n >= 2:
                check_diff(dsc, x, axis)
        for dt in (F32, F64):
            check_unwrap(dsc, record_property, lay(multi_wrap_rows(rng, lead, n, dt)), axis, path)
        for dt in (C32, C64):
            check_phase(dsc, lay(phasors(rng, lead, n, dt, 'multi_wrap')), axis, path)


@pytest.mark.parametrize('axis', [0, 1, 2, 3, -1, -4])
def test_four_dims(dsc, record_property, axis):
    rng = np.random.default_rng([axis + 4, 9])
    shape = (3, 4, 5, 6)
    path = ROWS if axis in (3, -1) else COLS
    n = shape[axis]

    def lay(rows):
        return np.ascontiguousarray(np.moveaxis(rows.reshape([s for i, s in enumerate(shape) if i != axis % 4] + [n]), -1, axis))

    for dt in (F32, F64, C32, C64):
        x = lay(cumsum_rows(rng, 360 // n, n, dt))
        check_cumsum(dsc, record_property, x, axis, path)
        check_diff(dsc, x, axis)
    for dt in (F32, F64):
        check_unwrap(dsc, record_property, lay(multi_wrap_rows(rng, 360 // n, n, dt)), axis, path)
    for dt in (C32, C64):
        check_phase(dsc, lay(phasors(rng, 360 // n, n, dt, 'multi_wrap')), axis, path)


# ---------------------------------------------------------------------------------------------------- the pipeline the operators are for

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_instantaneous_frequency_of_a_two_tone_row(dsc, dt):
    """diff(phase(hilbert(x))) of two-tone rows of 4096 samples against numpy.diff(numpy.unwrap(numpy.angle(scipy.signal.hilbert(x)))) in
    double, over samples 64 .. T - 64 (a finite row's analytic signal rings at its edges).

    The tolerance, from the element bound of tests/test_hilbert_abi.py on the imaginary part y of the analytic signal (its real part is a
    copy of x), E_k = tau (8 ||x||_2 / sqrt(N) + |y_k| + max_j |y_j| / 8) with tau = tests.test_filter_ref.TAU: the angle atan2(y, x) has
    the gradient (-y, x) / (x^2 + y^2), so an error of at most E_k in y alone moves it by at most E_k / (e_k - E_k), e_k the envelope
    sqrt(x_k^2 + y_k^2) >= the row's minimum envelope (0.6 here: tones of amplitude 1 and 0.4).  On top come the rounding of atan2 in the
    dtype (4 u pi: two units in the last place of an angle of at most pi), the one rounding of unwrap's result (u |phase_k|; its integers
    are exact inside, where no step comes within 1 rad of pi; a different integer at a ringing edge moves the whole phase by a
    constant and leaves the difference alone) and the rounding of the difference (u |f_k|).  For f_k = phase_{k+1} - phase_k:
        |f_k - ref_k| <= E_k / (e_k - E_k) + E_{k+1} / (e_{k+1} - E_{k+1}) + 8 u pi + u (|phase_k| + |phase_{k+1}|) + u |ref_k| + 4 2^-53 pi
    The last term is the reference's own: numpy's two angles, rounded in double.  Its unwrap is done by ref_unwrap (numpy.unwrap's
    integers, checked against it here, applied in long double): numpy's running sum of corrections rounds at 2^-53 |phase|, which for
    f64 data is as large as the error under test (with it as the reference the f64 ratio came to 1.51).
    Measured on an MI355X: err / tol = 0.838 (f32, largest tol 3.5e-4 rad per sample) and 0.747 (f64, 7.9e-13)."""
    from scipy import signal
    from tests.test_filter_ref import TAU
    T, rows = 4096, 2
    t = np.arange(T)
    rng = np.random.default_rng([dt.itemsize, 10])
    x = np.stack([np.cos(2 * np.pi * f1 * t / T + p1) + 0.4 * np.cos(2 * np.pi * f2 * t / T + p2)
                  for f1, f2, p1, p2 in ((200.37, 331.9, 0.3, 1.1), (411.5, 97.25, 2.0, -0.7))]).astype(dt)
    X = dsc.from_numpy(x)
    f = dsc.diff(dsc.phase(dsc.hilbert(X))).numpy()
    assert f.shape == (rows, T - 1) and f.dtype == dt
    z = signal.hilbert(x.astype(np.float64))
    env = np.abs(z)
    assert np.min(env[:, 64:T - 64]) >= 0.5
    ph, _ = ref_unwrap(np.angle(z))                                # numpy.unwrap with the integers applied exactly, in long double:
    ref = np.diff(ph, axis=-1)                                     # numpy's own sum of corrections would round at 2^-53 |phase| too
    assert np.max(np.abs(ph.astype(np.float64) - np.unwrap(np.angle(z), axis=-1))) < 1e-9
    assert np.max(np.abs(ref[:, 63:T - 63])) < np.pi - 1
    u, tau = UNIT[dt], TAU[dt]
    xn = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=-1, keepdims=True))
    E = tau * (8 * xn / np.sqrt(T) + np.abs(z.imag) + np.max(np.abs(z.imag), axis=-1, keepdims=True) / 8)
    dth = E / (env - E)
    tol = dth[:, :-1] + dth[:, 1:] + 8 * u * np.pi + u * (np.abs(ph[:, :-1]) + np.abs(ph[:, 1:])) + u * np.abs(ref) + 4 * 2.0 ** -53 * np.pi
    s = slice(64, T - 64)
    r = float(np.max(np.abs(f.astype(np.longdouble) - ref)[:, s] / tol[:, s]))
    print(f'diff(phase(hilbert)) {dt}: err / tol = {r:.3g}, max tol = {float(np.max(tol[:, s])):.3g}')
    assert r <= 1


# ---------------------------------------------------------------------------------------------------- child processes

ERRORS = {
    'unwrap_complex': ("dsc.unwrap(dsc.from_numpy(np.ones((2, 64), np.complex64)))", 'input must be real'),
    'phase_real': ("dsc.phase(dsc.from_numpy(np.ones((2, 64), np.float32)))", 'input must be complex'),
    'axis_too_large': ("dsc.cumsum(dsc.from_numpy(np.ones((2, 64), np.float32)), axis=2)", 'out of range'),
    'axis_too_small': ("dsc.diff(dsc.from_numpy(np.ones((2, 64), np.float32)), axis=-3)", 'out of range'),
    'diff_of_one': ("dsc.diff(dsc.from_numpy(np.ones((2, 1), np.float32)))", 'at least 2'),
    'out_shape': ("dsc.diff(dsc.from_numpy(np.ones((2, 64), np.float32)), out=dsc.from_numpy(np.ones((2, 64), np.float32)))", 'out must have'),
    'out_dtype': ("dsc.phase(dsc.from_numpy(np.ones((2, 64), np.complex64)), out=dsc.from_numpy(np.ones((2, 64), np.float64)))", 'out must have'),
    'out_overlaps_x': ("X = dsc.from_numpy(np.ones((2, 64), np.float32))\ndsc.cumsum(X, out=X)", 'out must not share memory'),
    'bad_route': ("import os\nos.environ['DSC_SCAN_ROUTE'] = 'fast'\ndsc.cumsum(dsc.from_numpy(np.ones((2, 64), np.float32)))", 'DSC_SCAN_ROUTE must be'),
}


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_argument_errors_end_the_process(name):
    """like every operator: a message on stderr and exit status 1; nothing runs on the GPU after it"""
    stmt, message = ERRORS[name]
    assert_ends_the_process(stmt, message, without_env='DSC_SCAN_ROUTE')


def test_cpp_scan_smoke_on_the_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_scan_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'scan templates ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
