"""GPU tests of dsc_sumsq / dsc_rms / dsc_var / dsc_std / dsc_vdot / dsc_detrend (moments.hip, moments.cpp): every output element against
the long-double references and the bounds of tests/test_moments_abi.py (class Moments; the bounds are stated in that file's docstring),
on every route: moment_rows / moment_tiles (DSC_MOMENT_ROUTE forces either on the inner == 1 shapes), moment_cols with and without the
segmented walk, and detrend_rows / detrend_tiles / detrend_cols.

Inputs: rows of unit noise on the offsets 0, 3, 1e3 and 1e6, one all-zero and one constant row, for detrend with added slopes.  Last-axis
lengths: the powers of two up to 2^16 and their neighbours, 70001, and the lengths either side of the limits of moments.hip — a row that
stays in registers and a tile are both dsc_moment_tile_len() = 8192 (f32), 4096 (f64, c32), 2048 (c64) elements for a workgroup, a
quarter of that for a wave (rows counts from 1024 on), 2048 / 512 where the length rules 16-byte packs out.

Every case asserts dsc.last_fft_path(), checks that the inputs are left bit for bit unchanged, and repeats the call with out= the head of
a larger sentinel-filled buffer: the result must be bit-identical and nothing past it may change.  No two routes are bit-identical by
construction: rows adds a thread's elements of the whole row and then the threads, tiles the threads of a tile and then the tiles, cols
one thread's walk (or its segments), so the same sum is associated three ways.  Each route is held to the same bounds instead, and
each is deterministic (the repeated call).  Argument errors end the process and run in child processes.

Calibration (worst err / bound per operator, dtype and route over every case of this file, on an MI355X; none above 1):
                sumsq    rms      var      std      vdot     detrend constant / linear
    f32         0.9957   0.9863   0.9954   0.9953   0.9945   0.9994 / 0.9994
    c32         0.9858   0.9346   0.9912   0.8923   0.9701   0.9998 / 0.9993
    f64         0.1704   0.2299   0.2779   0.2652   0.1568   0.2010 / 0.1502
    c64         0.4272   0.4961   0.2517   0.2264   0.4445   0.1398 / 0.1398
the largest over the routes; per route in profiles/moments_err.md (written when DSC_MOMENTS_REPORT names a file).
In f32 / c32 the final rounding to the dtype is the first term of every bound, and a rounding that falls halfway meets it: the ratios
near 1 are those.  In f64 / c64 the gamma terms allow n roundings in a row where the kernels' trees make about n / 256 + 12; the largest
ratios there come from axes of one to three elements."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import TOL, assert_ends_the_process, build_cpp_smoke, device_view, dsc, sync_fixture  # noqa: F401
from tests.test_moments_abi import C32, C64, F32, F64, LD, REAL_OF, Moments, gamma, lay, moment_rows, reduced_shape

pytestmark = pytest.mark.gpu

ROWS, TILES, COLS = 'rows', 'tiles', 'cols'
DTYPES = [F32, F64, C32, C64]
T_LAST = sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65537, 70001}
                | {511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193, 8196})
TILE_LEN = {F32: 8192, F64: 4096, C32: 4096, C64: 2048}
# (operator, ddof, keepdims) of the sweeps: both ddof and both keepdims on every shape
SWEEP = (('sumsq', 0, True), ('rms', 0, False), ('var', 0, True), ('var', 1, False), ('std', 1, True), ('std', 0, False), ('vdot', 0, True),
         ('detrend_constant', 0, True), ('detrend_linear', 0, True))
WORST = {}


_sync = sync_fixture('DSC_MOMENT_ROUTE')


@pytest.fixture(scope='module', autouse=True)
def _report(dsc):
    yield
    report = os.environ.get('DSC_MOMENTS_REPORT')                   # tools and job scripts: the table of profiles/moments_err.md
    if report:
        with open(report, 'w') as fh:
            fh.write('| operator | dtype | route | worst err / bound |\n|---|---|---|---|\n')
            for (op, dt, route), r in sorted(WORST.items()):
                fh.write(f'| {op} | {dt} | {route} | {r:.4g} |\n')


def force(route):
    if route in (ROWS, TILES):
        os.environ['DSC_MOMENT_ROUTE'] = route
    else:
        os.environ.pop('DSC_MOMENT_ROUTE', None)


def call(dsc, op, X, Y, axis, ddof, keepdims, out=None):
    if op in ('sumsq', 'rms'):
        return getattr(dsc, op)(X, out=out, axis=axis, keepdims=keepdims)
    if op in ('var', 'std'):
        return getattr(dsc, op)(X, out=out, axis=axis, ddof=ddof, keepdims=keepdims)
    if op == 'vdot':
        return dsc.vdot(X, Y, out=out, axis=axis, keepdims=keepdims)
    return dsc.detrend(X, axis=axis, type=op[8:], out=out)


class Case:
    """one input (and a second operand for vdot) on the device, with its references"""

    def __init__(self, dsc, x, y, axis=-1):
        self.x, self.y, self.axis = x, y, axis % x.ndim
        self.X, self.Y = dsc.from_numpy(x), dsc.from_numpy(y)
        self.M = Moments(x, axis)


def run(dsc, case, op, route, ddof=0, keepdims=True, forced=True):
    """the operator on the GPU: the route, the shape and dtype, the inputs left alone, a second call into the head of a sentinel-filled
    buffer that must give the same bits and leave the tail alone; then every element against its bound.  Returns the result."""
    x = case.x
    detrend = op.startswith('detrend')
    path = ('detrend_' if detrend else 'moment_') + route
    odt = x.dtype if detrend or op == 'vdot' else REAL_OF[x.dtype]
    oshape = x.shape if detrend else reduced_shape(x.shape, case.axis, keepdims)
    force(route if forced else None)
    y = call(dsc, op, case.X, case.Y, case.axis, ddof, keepdims)
    assert dsc.last_fft_path() == path, (op, x.shape, case.axis, dsc.last_fft_path(), path)
    yh = y.numpy()
    assert yh.shape == oshape and yh.dtype == odt, (op, yh.shape, yh.dtype, oshape, odt)
    assert case.X.numpy().tobytes() == x.tobytes(), 'the input changed'
    if op == 'vdot':
        assert case.Y.numpy().tobytes() == case.y.tobytes(), 'the second operand changed'
    del y
    extra = 1031
    size = int(np.prod(oshape))
    big = dsc.from_numpy(np.full(size + extra, -7.25, dtype=odt))
    out = device_view(dsc, big, oshape, odt)
    call(dsc, op, case.X, case.Y, case.axis, ddof, keepdims, out=out)
    assert dsc.last_fft_path() == path
    whole = big.numpy()
    assert whole[:size].tobytes() == yh.tobytes(), 'two identical calls differ (or out= was not written)'
    assert np.all(whole[size:] == -7.25), 'bytes past the output changed'
    del out, big

    M = case.M
    if op == 'vdot':
        r = M.vdot_err(yh, case.y)
    elif detrend:
        r = M.detrend_err(yh, op[8:])
    elif op in ('var', 'std'):
        r = getattr(M, op + '_err')(yh, ddof)
    else:
        r = getattr(M, op + '_err')(yh)
    key = (op, str(x.dtype), path)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f'{op} {path} {x.dtype} {x.shape} axis={case.axis} ddof={ddof}: err / bound = {r:.4g}')
    assert r <= 1, f'{op} {path} {x.dtype} {x.shape} axis={case.axis} ddof={ddof} keepdims={keepdims}: err / bound = {r:.4g}'
    return yh


def sweep(dsc, case, route, forced=True):
    n = case.x.shape[case.axis]
    for op, ddof, keepdims in SWEEP:
        if case.x.ndim == 1:
            keepdims = True
        run(dsc, case, op, route, ddof if n > 1 else 0, keepdims, forced)


def rows_case(dsc, rng, rows, T, dt):
    return Case(dsc, moment_rows(rng, rows, T, dt, slopes=True), moment_rows(rng, rows, T, dt))


# ---------------------------------------------------------------------------------------------------- the last axis, every length

@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_last_axis(dsc, dt):
    """six rows (four offsets, the zero row, the constant row) of every length, both forced routes"""
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 1])
    for T in T_LAST:
        case = rows_case(dsc, rng, 6, T, dt)
        for route in (ROWS, TILES):
            sweep(dsc, case, route)
            for op in ('var', 'std'):
                v = run(dsc, case, op, route)
                assert v[4] == 0 and v[5] == 0, 'a zero row and a constant row have no variance'
            assert not np.any(run(dsc, case, 'detrend_linear', route)[4]), 'a row of zeros must give exact zeros'


@pytest.mark.parametrize('rows', [1, 3, 300])
def test_row_counts(dsc, rows):
    """T = 4097 (odd: every row but the first starts off a pack boundary) and, for the few rows, 4100 (packs, longer than a c32 / f64
    tile); 300 rows are more than the chip has compute units"""
    rng = np.random.default_rng([rows, 2])
    for dt in DTYPES:
        for T in (4097, 4100) if rows < 300 else (4097,):
            case = rows_case(dsc, rng, rows, T, dt)
            for route in (ROWS, TILES):
                sweep(dsc, case, route)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_a_wave_per_row(dsc, dt):
    """1030 rows: rows of at most a quarter of a tile go to one wave each, four to a workgroup; one element more and a workgroup takes them"""
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 3])
    q = TILE_LEN[dt] // 4
    for T in (65, q, q + 1):
        sweep(dsc, rows_case(dsc, rng, 1030, T, dt), ROWS, forced=False)


def test_the_route_left_to_the_library(dsc):
    """fewer than 1024 rows longer than a tile take the tiles route; rows of at most a tile, and 1024 rows or more, the rows route"""
    rng = np.random.default_rng(4)
    for rows, T, dt, route in ((3, 70001, F32, TILES), (3, 8192, F32, ROWS), (3, 8196, F32, TILES), (300, 4100, C32, TILES),
                               (1023, 2052, C64, TILES), (1024, 2052, C64, ROWS), (2, 2048, C64, ROWS), (2, 2049, C64, TILES), (1, 100, F64, ROWS)):
        sweep(dsc, rows_case(dsc, rng, rows, T, dt), route, forced=False)


# ---------------------------------------------------------------------------------------------------- other axes

OTHER_AXES = (((2, 65, 5), 1), ((65, 7), 0), ((2, 3, 4, 5), 2), ((4097, 3), 0), ((3, 257, 8), 1))


@pytest.mark.parametrize('shape,axis', OTHER_AXES, ids=lambda v: str(v).replace(' ', ''))
def test_other_axes(dsc, shape, axis):
    """inner > 1: one thread per output walks the axis; [4097, 3] and [3, 257, 8] have few outputs on an axis of 128 or more and take
    the segmented walk"""
    rng = np.random.default_rng([len(shape), axis, 5])
    n = shape[axis]
    lead = int(np.prod(shape)) // n
    for dt in DTYPES:
        x = lay(moment_rows(rng, lead, n, dt, slopes=True), shape, axis)
        y = lay(moment_rows(rng, lead, n, dt), shape, axis)
        sweep(dsc, Case(dsc, x, y, axis), COLS, forced=False)


def test_unit_axes_reach_the_row_routes(dsc):
    """[3, T, 1] on axis 1 and [T, 1] on axis 0 are inner == 1; [3, 1, T] on axis 1 reduces an axis of one element per column"""
    rng = np.random.default_rng(6)
    T = 4100
    for dt in (F32, C64):
        rows = moment_rows(rng, 3, T, dt, slopes=True)
        other = moment_rows(rng, 3, T, dt)
        for shape, axis, route in (((3, T, 1), 1, ROWS), ((3, T, 1), -2, TILES), ((3, 1, T), 1, COLS)):
            sweep(dsc, Case(dsc, rows.reshape(shape), other.reshape(shape), axis), route, forced=route != COLS)
        sweep(dsc, Case(dsc, rows[:1].reshape(T, 1), other[:1].reshape(T, 1), 0), TILES)


# ---------------------------------------------------------------------------------------------------- identities

@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_identities(dsc, dt):
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 7])
    for T, route in ((4097, ROWS), (20001, TILES)):
        case = rows_case(dsc, rng, 6, T, dt)
        M = case.M
        # vdot(x, x).real is sumsq(x): both within their bounds of the one reference
        self_case = Case(dsc, case.x, case.x)
        d = run(dsc, self_case, 'vdot', route)
        q = run(dsc, case, 'sumsq', route)
        ref, bound = M.vdot_ref(case.x)[0]
        qb = (gamma(LD(T) + 2) + M.uo) * M.sumsq
        assert np.all(np.abs(d.real.reshape(-1).astype(LD) - q.reshape(-1).astype(LD)) <= bound + qb + np.abs(ref - M.sumsq))
        if dt.kind == 'c':
            assert np.all(np.abs(d.imag.reshape(-1)) <= M.vdot_ref(case.x)[1][1])
        # var(x) is var(x + c): each within its bound of its own reference, the references apart by the rounding of x + c
        shifted = Case(dsc, (case.x + np.asarray(17.5, dt)).astype(dt), case.y)
        for ddof in (0, 1):
            v0, v1 = run(dsc, case, 'var', route, ddof), run(dsc, shifted, 'var', route, ddof)
            (r0, b0), (r1, b1) = M.var_ref(ddof), shifted.M.var_ref(ddof)
            assert np.all(np.abs(v0.reshape(-1).astype(LD) - v1.reshape(-1).astype(LD)) <= b0 + b1 + np.abs(r0 - r1))
        # detrend(detrend(x)) is detrend(x): z = detrend(y) within its own bound, and, detrend being an orthogonal projection P,
        # z - y = -(I - P) (y - ref) + the error of z, so per row ||z - y||_2 <= ||bound of y||_2 + ||bound of z||_2
        for kind in ('constant', 'linear'):
            y = run(dsc, case, 'detrend_' + kind, route)
            again = Case(dsc, y, case.y)
            z = run(dsc, again, 'detrend_' + kind, route)
            for yc, zc, (_, by), (_, bz) in zip(*([a.real, a.imag] if dt.kind == 'c' else [a] for a in (y, z)), M.detrend_ref(kind),
                                               again.M.detrend_ref(kind)):
                lhs = np.sqrt(np.sum((zc.astype(LD) - yc.astype(LD)) ** 2, axis=-1))
                assert np.all(lhs <= np.sqrt(np.sum(by ** 2, axis=-1)) + np.sqrt(np.sum(bz ** 2, axis=-1))), kind


def test_parseval_of_rfft(dsc):
    """sum x^2 = (2 sumsq(rfft(x)) - X[0]^2 - |X[n / 2]|^2) / n on [3, 4096], at the transforms' tolerance"""
    rng = np.random.default_rng(8)
    n = 4096
    x = rng.standard_normal((3, n)).astype(F32)
    X = dsc.rfft(dsc.from_numpy(x))
    Xh = X.numpy()
    assert Xh.shape == (3, n // 2 + 1)
    q = dsc.sumsq(X).numpy().reshape(-1).astype(np.float64)
    energy = dsc.sumsq(dsc.from_numpy(x)).numpy().reshape(-1).astype(np.float64)
    spectral = (2 * q - np.abs(Xh[:, 0].astype(C64)) ** 2 - np.abs(Xh[:, -1].astype(C64)) ** 2) / n
    rel = np.abs(spectral - energy) / energy
    print(f'Parseval: relative difference {np.max(rel):.3g}')
    assert np.all(rel <= TOL[F32])
    assert np.all(np.abs(energy - np.sum(x.astype(np.float64) ** 2, axis=-1)) <= 2.0 ** -23 * energy)


# ---------------------------------------------------------------------------------------------------- child processes

ONES = "dsc.from_numpy(np.ones((2, 64), np.float32))"
ERRORS = {
    'ddof_too_large': (f"dsc.var({ONES}, ddof=64)", 'ddof must be'),
    'ddof_negative': (f"dsc.std({ONES}, ddof=-1)", 'ddof must be'),
    'ddof_of_one_element': ("dsc.var(dsc.from_numpy(np.ones((2, 1), np.float32)), ddof=1)", 'ddof must be'),
    'vdot_shapes': (f"dsc.vdot({ONES}, dsc.from_numpy(np.ones((2, 32), np.float32)))", 'one shape and dtype'),
    'vdot_dtypes': (f"dsc.vdot({ONES}, dsc.from_numpy(np.ones((2, 64), np.float64)))", 'one shape and dtype'),
    'axis_too_large': (f"dsc.sumsq({ONES}, axis=2)", 'out of range'),
    'axis_too_small': (f"dsc.detrend({ONES}, axis=-3)", 'out of range'),
    'out_shape': (f"dsc.rms({ONES}, out=dsc.from_numpy(np.ones((2, 64), np.float32)))", 'out must have'),
    'out_keepdims': (f"dsc.sumsq({ONES}, out=dsc.from_numpy(np.ones((2, 1), np.float32)), keepdims=False)", 'out must have'),
    'out_dtype_of_complex': ("dsc.var(dsc.from_numpy(np.ones((2, 64), np.complex64)), out=dsc.from_numpy(np.ones((2, 1), np.complex64)))", 'out must have'),
    'detrend_out_shape': (f"dsc.detrend({ONES}, out=dsc.from_numpy(np.ones((2, 1), np.float32)))", 'out must have'),
    'out_overlaps_x': (f"X = {ONES}\ndsc.detrend(X, out=X)", 'out must not share memory'),
    'out_overlaps_b': (f"from tests.helpers import device_view\nY = {ONES}\ndsc.vdot({ONES}, Y, out=device_view(dsc, Y, (2, 1), np.float32))", 'out must not share memory'),
    'detrend_type': (f"from dsc_amd import _bindings as B\nfrom dsc_amd.context import _get_ctx\nB.dsc_detrend(_get_ctx(), {ONES}._c_ptr, None, -1, 7)", 'type must be'),
    'bad_route': (f"import os\nos.environ['DSC_MOMENT_ROUTE'] = 'fast'\ndsc.sumsq({ONES})", 'DSC_MOMENT_ROUTE must be'),
}


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_argument_errors_end_the_process(name):
    """like every operator: a message on stderr and exit status 1; nothing runs on the GPU after it"""
    stmt, message = ERRORS[name]
    assert_ends_the_process(stmt, message, without_env='DSC_MOMENT_ROUTE')


def test_detrend_type_names(dsc):
    with pytest.raises(ValueError):
        dsc.detrend(dsc.from_numpy(np.ones((2, 8), np.float32)), type='quadratic')


def test_cpp_moments_smoke_on_the_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_moments_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'moment templates ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
