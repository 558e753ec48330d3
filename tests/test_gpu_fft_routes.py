"""GPU tests of dsc_rfft / dsc_irfft / dsc_fft / dsc_ifft on every kernel route of fft_driver.cpp (its `routes` table), every line against the
long-double reference of tests/test_fft_ref.py under the per-line bound an FFT obeys:
    per line  ||y - ref||_2 <= tau ||ref||_2,   |y_k - ref_k| <= tau (8 ||ref||_2 / sqrt(len) + |ref_k| + max |ref| / 8)
(cols_4step_real: ||ref|| and max |ref| of the pair of neighbouring columns it transforms as one complex column)
Every case asserts dsc.last_fft_path() (expect() below restates the `routes` table for a roomy context), checks that the input is left
bit for bit unchanged, and repeats the call with out= the start of a larger sentinel-filled buffer: the result must be bit-identical
and nothing past it may change.  Shapes: batch counts of 1, lines-per-workgroup +- 1 and more than one wave over 256 CUs; inner extents
ragged for every column tile width (8 .. 256); odd inner extents on the real four-step; 3-d / 4-d tensors and trailing unit
dimensions; zero padded and cropped lines (irfft: fewer and more bins than order + 1, imaginary parts in bins 0 and order); plain
noise plus lines with a large DC offset or one strong tone.  Routes behind an environment switch run in a child process, as do the
tight-context fallbacks of the axis four-step routes."""
import numpy as np
import pytest

from tests.helpers import C64, C128, CPX, F32, F64, assert_out_call, dsc, run_child, sync_fixture  # noqa: F401
from tests.test_fft_ref import TAU, fft_err, out_len, pow2, real_of, ref_fft

pytestmark = pytest.mark.gpu

LDS_MAX = {True: 8192, False: 4096}                     # dsc_fft_lds_max_len
_sync = sync_fixture()


# ------------------------------------------------------------------------------------- the routes table of fft_driver.cpp, restated

def _tile_width(L, sp):                                 # fft_regs_cols.hip cols_tile_width
    if L <= 32:
        return 256
    w = {64: 128, 128: 64, 256: 32}.get(L)
    if w:
        return w
    if sp:
        return 32 if L == 512 else 16 if L <= 2048 else 8
    return 16 if L <= 1024 else 8


def _split(n, sp, cols):                                # dsc_fft_cols_4step_split
    lg = n.bit_length() - 1
    if (1 << lg) != n or lg < 10:
        return None
    a = 1 << (lg // 2)
    b = n // a
    while _tile_width(a, sp) > cols and b >= 128 and a < 2048:
        a, b = a * 2, b // 2
    if a < 32 or b < 32 or a > 2048 or b > 2048:
        return None
    return a, b


def _last_axis(L, mode, sp, x_n, in_len):
    """route of contiguous lines (inner == 1) in a roomy context"""
    packed = mode in ('r2c', 'c2r')
    want = 2 * L if mode == 'r2c' else L + 1 if mode == 'c2r' else L
    full = in_len == want and x_n == want
    if sp and mode in ('c2c', 'cast') and L == 32768:
        return 'c2c_32k_regs'
    if sp and packed and L == 32768:
        return 'r2c_64k_regs' if mode == 'r2c' else 'c2r_64k_regs'
    if L == 65536 or L == 131072 or (L == 32768 and not sp):                   # dsc_fft_fused_l2_supports
        return {'r2c': 'r2c_fused_l2', 'c2r': 'c2r_fused_l2'}.get(mode, 'c2c_fused_l2')
    two_pass = L in (65536, 131072, 262144, 524288, 1048576) or (L == 32768 and not sp)
    if two_pass and (mode != 'cast' or L != 262144):
        if mode == 'cast':
            return 'c2c_2pass_regs'                      # widened into a complex temporary first
        return {'r2c': 'r2c_2pass_regs', 'c2r': 'c2r_2pass_regs'}.get(mode, 'c2c_2pass_regs')
    if two_pass:
        return 'c2c_2pass_regs'
    if L in (2, 4, 8, 16) and (full or x_n * 16 * 256 < (1 << 30)):
        return 'regs_tiny'
    if L in (32, 64, 128, 256) and (full or x_n * 16 * 256 < (1 << 30)):
        return 'regs_small'
    if 256 <= L <= 16384 and (full or x_n * 16 * 64 < (1 << 30)):
        return 'regs_mid'
    return 'generic_lds' if L <= LDS_MAX[sp] else 'generic_4step'


def expect(kind, x_dt, shape, n, axis):
    """the path dsc.last_fft_path() reports for kind(x, n, axis) in a roomy context (fft_driver.cpp, the route functions in the order of `routes`)"""
    x_dt = np.dtype(x_dt)
    axis = axis % len(shape)
    sp = real_of(x_dt) == F32
    x_n = shape[axis]
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    m = n if n > 0 else x_n
    if kind == 'rfft':
        L, mode = pow2(m) // 2, 'r2c'
        in_len, out_n = min(x_n, 2 * L), L + 1
    elif kind == 'irfft':
        L, mode = pow2(m - 1), 'c2r'
        in_len, out_n = min(x_n, L + 1), 2 * L
    else:
        L, mode = pow2(m), 'c2c' if x_dt.kind == 'c' else 'cast'
        in_len, out_n = min(x_n, L), L
    if inner == 1:
        return _last_axis(L, mode, sp, x_n, in_len)
    csz = 8 if sp else 16
    s = _split(L, sp, inner)
    if inner >= 8 and L >= 4096 and mode in ('c2c', 'cast') and x_n == L and in_len == L and out_n == L and L <= (1 << 22) and \
            (L > 4096 or inner >= 64) and s and L * inner * csz < 0x7f000000:
        return 'cols_4step'
    nn = 2 * L
    full = (x_n == nn and out_n == L + 1) if mode == 'r2c' else (x_n == L + 1 and out_n == nn) if mode == 'c2r' else False
    s = _split(nn, sp, 1 << 20)
    if full and inner >= 16 and inner % 2 == 0 and 8192 <= nn <= (1 << 22) and s and s[0] >= 64 and s[1] >= 64:
        return 'cols_4step_real'
    if L in (2, 4, 8, 16):
        return 'regs_tiny_cols'
    if L in (32, 64, 128, 256, 512, 1024, 2048) or (L == 4096 and sp and mode == 'c2c'):
        return 'regs_cols'
    last_axis_kernel = (256 <= L <= 16384) or (sp and L == 32768) or L in (65536, 131072) or (L == 32768 and not sp) or \
        ((mode != 'cast') and L in (262144, 524288, 1048576)) or (mode == 'cast' and L == 262144)
    if L >= 512 and last_axis_kernel:                   # transposed to the back: reported as the contiguous route
        return _last_axis(L, mode, sp, x_n, in_len)
    return 'generic_lds' if L <= LDS_MAX[sp] else 'generic_4step'


# ---------------------------------------------------------------------------------------------------- inputs and checks

def make_input(rng, kind, x_dt, shape, axis, spice=True):
    """standard normal lines; with spice, line 1 carries a large DC offset and line 2 one strong tone on top (for irfft, whose input
    is a spectrum: a strong bin 0 and a strong bin 5), so that the pairing of bins k and L - k in the packed-real passes is seen with
    one of the pair large"""
    x_dt = np.dtype(x_dt)
    x = rng.standard_normal(shape)
    if x_dt.kind == 'c':
        x = x + 1j * rng.standard_normal(shape)
    if spice:
        v = np.moveaxis(x, axis, -1).reshape(-1, shape[axis])
        m = v.shape[-1]
        if v.shape[0] >= 2:
            if kind == 'irfft':
                v[1, 0] += 20 * m
            else:
                v[1] += 20
        if v.shape[0] >= 3 and m >= 8:
            if kind == 'irfft':
                v[2, 5] += 20 * m
            else:
                v[2] += 20 * np.cos(2 * np.pi * 5 * np.arange(m) / m)
        x = np.moveaxis(v.reshape(np.moveaxis(x, axis, -1).shape), -1, axis)
    return np.ascontiguousarray(x.astype(x_dt))


def _out_dtype(kind, x_dt):
    x_dt = np.dtype(x_dt)
    if kind == 'irfft':
        return real_of(x_dt)
    return CPX[real_of(x_dt)]


def run_case(dsc, record_property, kind, x, n, axis):
    """kind(x, n, axis) on the GPU: the route, the input left alone, every line within the bound, and a second call into the start of
    a sentinel-filled buffer that must give the same bits and leave the tail alone.  Returns err / bound."""
    want_path = expect(kind, x.dtype, x.shape, n, axis)
    fn = getattr(dsc, kind)
    X = dsc.from_numpy(x)
    y = fn(X, n=n, axis=axis)
    path = dsc.last_fft_path()
    assert path == want_path, (kind, x.dtype, x.shape, n, axis, path, want_path)
    yh = y.numpy()
    odt = _out_dtype(kind, x.dtype)
    oshape = list(x.shape)
    oshape[axis % x.ndim] = out_len(kind, x.shape[axis], n)
    assert yh.shape == tuple(oshape) and yh.dtype == odt, (yh.shape, yh.dtype, oshape, odt)
    assert X.numpy().tobytes() == x.tobytes(), 'the input changed'
    del y

    def again(out):
        fn(X, out=out, n=n, axis=axis)
        assert dsc.last_fft_path() == want_path
    assert_out_call(dsc, again, oshape, odt, yh)

    # cols_4step_real: two neighbouring real columns go through one complex column, each carries rounding of the pair's size
    r = fft_err(yh, ref_fft(x, n, axis, kind), axis, TAU[real_of(x.dtype)], paired=want_path == 'cols_4step_real')
    record_property(f'{want_path}:{kind}:{x.dtype}', r)
    assert r <= 1, f'{want_path} {kind} {x.dtype} {x.shape} n={n} axis={axis}: err / bound = {r:.3g}'
    return r


def in_dtypes(kind, rdt):
    """input dtypes of kind at precision rdt: fft / ifft take complex and real (widened) tensors"""
    return {'rfft': (rdt,), 'irfft': (CPX[rdt],), 'fft': (CPX[rdt], rdt), 'ifft': (CPX[rdt], rdt)}[kind]


def natural(kind, L):
    """(input length along the axis, n) of a full line of complex transform length L"""
    return {'rfft': (2 * L, -1), 'irfft': (L + 1, -1)}.get(kind, (L, -1))


def fits(kind, L):
    """(label, input length, n): full, zero padded and cropped lines of complex transform length L; for irfft fewer and more bins
    than order + 1 (n = L + 1 gives order L)"""
    if kind == 'rfft':
        return [('full', 2 * L, -1), ('padded', max(1, 2 * L - 3), 2 * L), ('cropped', 2 * L + 5, 2 * L)]
    if kind == 'irfft':
        return [('full', L + 1, -1), ('fewer', max(2, L // 2 + 1), L + 1), ('more', L + 7, L + 1)]
    return [('full', L, -1), ('padded', max(1, L - 3), L), ('cropped', L + 5, L)]


KINDS = ('rfft', 'irfft', 'fft', 'ifft')


# ---------------------------------------------------------------------------------------------------- contiguous lines

LAST_L = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1048576, 1 << 21)


def _rows(L, fit):
    """batch counts: 1, lines-per-workgroup +- 1 for every power-of-two group size, and more than one wave over 256 CUs"""
    if L >= 65536:
        return (1, 3) if fit == 'full' and L <= 131072 else (2,)
    if L >= 8192:
        return (1, 17) + ((257 if L <= 16384 else 33,) if fit == 'full' else ())
    if L >= 256:
        return (1, 17, 257) + (((1 << 21) // L + 1,) if fit == 'full' else ())
    return (1, 63, 65) + (((1 << 18) // L + 1 if L >= 32 else 70001,) if fit == 'full' else ())


def _last_cases():
    cases = []
    for L in LAST_L:
        for rdt in (F32, F64):
            for kind in KINDS:
                if L == 1 and kind == 'irfft':
                    continue                                     # order >= 1: irfft has no 1-point form
                for x_dt in in_dtypes(kind, rdt):
                    for label, x_n, n in fits(kind, L):
                        if L >= (1 << 18) and label != 'full' and (kind == 'irfft' or rdt == F64):
                            continue                             # keep the host reference small at the longest lengths
                        if L == 1 and kind in ('fft', 'ifft'):
                            continue                             # a 1-point complex transform is a copy: no kernel
                        cases.append((kind, x_dt, L, label, x_n, n))
    return cases


@pytest.mark.parametrize('kind,x_dt,L,label,x_n,n', _last_cases(), ids=lambda v: str(v))
def test_last_axis(dsc, record_property, kind, x_dt, L, label, x_n, n):
    rng = np.random.default_rng([L, KINDS.index(kind), np.dtype(x_dt).num, x_n])
    for rows in _rows(L, label):
        x = make_input(rng, kind, x_dt, (rows, x_n), -1)
        run_case(dsc, record_property, kind, x, n, -1)


# 3-d / 4-d batches and trailing unit dimensions along the last real axis: the line count is the product of the leading extents
ND_L = (4, 64, 1024, 16384, 32768, 65536, 262144)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('L', ND_L)
def test_batched_shapes(dsc, record_property, kind, rdt, L):
    rng = np.random.default_rng([L, KINDS.index(kind), rdt.itemsize, 7])
    x_n, n = natural(kind, L)
    x_dt = in_dtypes(kind, rdt)[0]
    lead = (2, 3) if L <= 16384 else (1, 2)
    for shape, axis in (((*lead, x_n), -1), ((lead[0], 1, lead[1], x_n), 3), ((lead[1], x_n, 1), 1), ((2, x_n, 1, 1), 1)):
        x = make_input(rng, kind, x_dt, shape, axis)
        run_case(dsc, record_property, kind, x, n, axis)


# ---------------------------------------------------------------------------------------------------- strided lines

# inner extents: 3 (narrower than every tile), 70 and 300 (a ragged last tile for every tile width 8 .. 256)
COL_INNER = (3, 70, 300)


def _col_cases():
    cases = []
    for L in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        for rdt in (F32, F64):
            for kind in KINDS:
                if L == 1 and kind != 'rfft':
                    continue
                for x_dt in in_dtypes(kind, rdt):
                    for label, x_n, n in fits(kind, L):
                        for inner in COL_INNER:
                            if L >= 1024 and inner == 300 and label != 'full':
                                continue
                            cases.append((kind, x_dt, L, label, x_n, n, inner))
    return cases


@pytest.mark.parametrize('kind,x_dt,L,label,x_n,n,inner', _col_cases(), ids=lambda v: str(v))
def test_column_routes(dsc, record_property, kind, x_dt, L, label, x_n, n, inner):
    """[outer, x_n, inner] along axis 1 (outer 1 or 2) and [x_n, inner] along axis 0: regs_tiny_cols, regs_cols, the transpose route
    (real 4096-point and f64 lines) and the strided LDS kernel (one complex point)."""
    rng = np.random.default_rng([L, KINDS.index(kind), np.dtype(x_dt).num, x_n, inner])
    for shape, axis in (((x_n, inner), 0), ((2, x_n, inner), 1)):
        x = make_input(rng, kind, x_dt, shape, axis)
        run_case(dsc, record_property, kind, x, n, axis)


def _four_step_cases():
    cases = []
    for rdt in (F32, F64):
        # the complex four-step: full lines >= 4096 (4096 only from 64 columns); inner 8 and 70 / 300 ragged
        for L, inner in ((4096, 64), (4096, 300), (8192, 8), (8192, 70), (16384, 37), (65536, 8), (262144, 8)):
            for kind in ('fft', 'ifft'):
                for x_dt in in_dtypes(kind, rdt):
                    cases.append((kind, x_dt, L, inner, 'full'))
        # the real four-step: full lines of >= 8192 real points, an even number of columns >= 16; odd ones leave the route
        for L, inner in ((4096, 16), (4096, 70), (8192, 300), (32768, 16), (131072, 16), (4096, 17), (8192, 71)):
            for kind in ('rfft', 'irfft'):
                cases.append((kind, in_dtypes(kind, rdt)[0], L, inner, 'full'))
        # not full lines: the transpose route (reported as the contiguous route), for every kind
        for L, inner in ((8192, 16), (65536, 8)):
            for kind in KINDS:
                cases.append((kind, in_dtypes(kind, rdt)[0], L, inner, 'padded'))
    # the 1024- and 2048-point rows of the column tables, at the smallest shapes that reach them: 2^21 real points = 1024 x 2048 (split at
    # 1024, merge at 2048, column passes at both), and 2^21 complex points in eight columns, which widen the split to 2048 x 1024
    for kind in ('rfft', 'irfft'):
        cases.append((kind, in_dtypes(kind, F32)[0], 1 << 20, 16, 'full'))
    for kind in ('fft', 'ifft'):
        cases.append((kind, C128, 1 << 21, 8, 'full'))
    return cases


@pytest.mark.parametrize('kind,x_dt,L,inner,label', _four_step_cases(), ids=lambda v: str(v))
def test_axis_four_step_routes(dsc, record_property, kind, x_dt, L, inner, label):
    rng = np.random.default_rng([L, KINDS.index(kind), np.dtype(x_dt).num, inner])
    fit = {f[0]: f for f in fits(kind, L)}
    _, x_n, n = fit['full'] if label == 'full' else fit['fewer' if kind == 'irfft' else 'padded']
    outer = 2 if L * inner <= (1 << 20) else 1
    for shape, axis in (((x_n, inner), 0), ((outer, x_n, inner), 1)):
        x = make_input(rng, kind, x_dt, shape, axis)
        run_case(dsc, record_property, kind, x, n, axis)


def test_generic_four_step_strided(dsc, record_property):
    """zero padded lines of complex length 2^21 along axis 0: no register kernel, no four-step axis route"""
    rng = np.random.default_rng(21)
    for kind, x_dt, x_n, n in (('rfft', F32, (1 << 22) - 5, 1 << 22), ('fft', C64, (1 << 21) - 5, 1 << 21)):
        x = make_input(rng, kind, x_dt, (x_n, 2), 0)
        assert expect(kind, x_dt, x.shape, n, 0) == 'generic_4step'
        run_case(dsc, record_property, kind, x, n, 0)


# ---------------------------------------------------------------------------------------------------- routes behind a switch

SWITCHED = r'''
import sys, numpy as np
import dsc_amd as dsc
dsc.init(4 << 30, 1 << 30)
rng = np.random.default_rng(9)
for i, (kind, dt, shape, n, axis) in enumerate(CASES):
    x = np.asarray(rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if np.dtype(dt).kind == 'c' else 0)).astype(dt)
    X = dsc.from_numpy(x)
    y = getattr(dsc, kind)(X, n=n, axis=axis)
    np.save('%s/x%d.npy' % (OUT, i), x)
    np.save('%s/y%d.npy' % (OUT, i), y.numpy())
    assert X.numpy().tobytes() == x.tobytes()
    print('PATH', i, dsc.last_fft_path(), flush=True)
dsc.synchronize()
'''

SWITCH_CASES = {
    # the column kernels and the transposes switched off: strided lines take the LDS line kernel / the generic four-step
    'DSC_NO_COLS DSC_NO_TINY DSC_NO_AXIS_TRANSPOSE': [
        ('rfft', 'float32', (64, 70), -1, 0, 'generic_lds'), ('irfft', 'complex128', (9, 3, 5), -1, 1, 'generic_lds'),
        ('fft', 'complex64', (4000, 37), 4096, 0, 'generic_lds'), ('ifft', 'float64', (2, 4096, 3), -1, 1, 'generic_lds'),
        ('rfft', 'float64', (16000, 3), 16384, 0, 'generic_4step'), ('ifft', 'complex64', (32768, 2), -1, 0, 'generic_4step')],
    # the last-axis register kernels switched off
    'DSC_NO_TINY DSC_NO_REGS_MID': [
        ('rfft', 'float32', (5, 32), -1, -1, 'generic_lds'), ('irfft', 'complex64', (17, 1025), -1, -1, 'generic_lds'),
        ('fft', 'complex128', (3, 4096), -1, -1, 'generic_lds'), ('ifft', 'float32', (33, 8192), -1, -1, 'generic_lds'),
        ('fft', 'complex128', (2, 16384), -1, -1, 'generic_4step')],
    # no fused-L2 kernel, no two-pass route: the generic four-step on the longest rows
    'DSC_NO_FUSED_L2 DSC_NO_TWO_PASS': [
        ('rfft', 'float32', (3, 131072), -1, -1, 'generic_4step'), ('irfft', 'complex128', (2, 65537), -1, -1, 'generic_4step'),
        ('fft', 'float32', (2, 65536), -1, -1, 'generic_4step'), ('ifft', 'complex64', (2, 262144), -1, -1, 'generic_4step')],
}


@pytest.mark.parametrize('switches', list(SWITCH_CASES))
def test_switched_off_routes(record_property, tmp_path, switches):
    cases = SWITCH_CASES[switches]
    code = 'CASES = %r\nOUT = %r\n' % ([c[:5] for c in cases], str(tmp_path)) + SWITCHED
    r = run_child(code, env={k: '1' for k in switches.split()}, timeout=600, check=True)
    paths = [ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith('PATH')]
    assert paths == [c[5] for c in cases], paths
    for i, (kind, dt, shape, n, axis, path) in enumerate(cases):
        x, y = np.load(tmp_path / f'x{i}.npy'), np.load(tmp_path / f'y{i}.npy')
        rr = fft_err(y, ref_fft(x, n, axis, kind), axis, TAU[real_of(x.dtype)])
        record_property(f'{path}:{kind}:{x.dtype}', rr)
        assert rr <= 1, (kind, dt, shape, n, axis, rr)


# ---------------------------------------------------------------------------------------------------- tight contexts

TIGHT = r'''
import sys, numpy as np
import dsc_amd as dsc
from tests.test_fft_ref import TAU, fft_err, ref_fft
kind, rows, cols, dt, spare, roomy = KIND, ROWS, COLS, DT, SPARE, ROOMY
rng = np.random.default_rng(17)
x = rng.standard_normal((rows, cols))
if np.dtype(dt).kind == 'c':
    x = x + 1j * rng.standard_normal((rows, cols))
x = x.astype(dt)
dsc.init((1 << 30) if roomy else NEED + spare, 64 << 20)
X = dsc.from_numpy(x)
y = getattr(dsc, kind)(X, axis=0)
path = dsc.last_fft_path()
yh = y.numpy()
assert X.numpy().tobytes() == x.tobytes()
r = fft_err(yh, ref_fft(x, -1, 0, kind), 0, TAU[np.dtype(np.float32)])
assert r <= 1, r
dsc.synchronize()
print('OK', path, r, flush=True)
'''


def _tight(kind, rows, cols, dt, need, spare, roomy):
    code = TIGHT.replace('KIND', repr(kind)).replace('ROWS', str(rows)).replace('COLS', str(cols)).replace('DT', repr(dt)) \
        .replace('NEED', str(need)).replace('SPARE', str(spare)).replace('ROOMY', str(roomy))
    r = run_child(code, timeout=600)
    assert r.returncode == 0 and 'OK' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout.split('OK')[-1].split()


def test_real_axis_four_step_in_a_tight_context(record_property):
    """dsc_rfft along axis 0 of f32 [16384, 32]: cols_4step_real, whose tables include the 16384-point COMPLEX plan (not the 8192-point
    REAL plan geom_of makes for the job).  Main arena, 256-B aligned blocks, plans carved from the top:
        x      16384 * 32 * 4                      = 2097152
        out    8193 * 32 * 8                       = 2097408
        plan   REAL 8192, f32: 8192 * 8 + 8193 * 8 -> 65536 + 65792 = 131328
        work   16384 * 16 complex * 8              = 2097152
    and 65536 B to spare: less than the 16384-point complex table (131072 B) the route would add (with the 128-point one, 1024 B).
    Before the probe counted the tables, this exited in dsc_main_arena::alloc; now it falls back to the strided LDS kernel, which
    needs no more main memory.  With room it takes the four-step route."""
    need = 2097152 + 2097408 + 131328 + 2097152
    path, r = _tight('rfft', 16384, 32, 'float32', need, 65536, False)
    assert path == 'generic_lds', path
    record_property('generic_lds:rfft:float32 (tight)', float(r))
    path, r = _tight('rfft', 16384, 32, 'float32', need, 65536, True)
    assert path == 'cols_4step_real', path


def test_complex_axis_four_step_in_a_tight_context(record_property):
    """dsc_fft along axis 0 of c64 [16384, 16]: cols_4step with n1 = 256, n2 = 64 (16 columns widen the split), whose new tables are the
    256- and 64-point plans (2048 + 512 B); the 16384-point plan is the job's own (geom_of).  Main arena:
        x      16384 * 16 * 8  = 2097152
        out    16384 * 16 * 8  = 2097152
        plan   COMPLEX 16384   = 131072
        work   16384 * 16 * 8  = 2097152
    and 1024 B to spare, less than the 2560 B of the two tables.  It falls back to the generic four-step, whose 128-point table fits."""
    need = 2097152 * 3 + 131072
    path, r = _tight('fft', 16384, 16, 'complex64', need, 1024, False)
    assert path == 'generic_4step', path
    record_property('generic_4step:fft:complex64 (tight)', float(r))
    path, r = _tight('fft', 16384, 16, 'complex64', need, 1024, True)
    assert path == 'cols_4step', path
