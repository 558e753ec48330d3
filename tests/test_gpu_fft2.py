"""GPU tests of dsc_fft2 / dsc_ifft2 / dsc_rfft2 / dsc_irfft2: every size of the fused windows (fft_2d.hip) and a set of composed
sizes, every image against the long-double reference ref_fft2 of tests/test_fft2_abi.py under the per-line bound of
tests/test_fft_ref.py with the image flattened to one line and that file's TAU (f32 2e-6, f64 5e-15): a 2-D transform of P points
rounds like a 1-D Cooley-Tukey transform of P points, P <= 32768 here.

Calibration (first run on an MI355X; worst err / bound over 9 spiced images of every window size, per precision):
    hand composition, calls of the parent commit only:
      fft(fft(x, -1), -2), ifft likewise       f32 0.120   f64 0.106
      fft(rfft(x, -1), -2)                     f32 0.137   f64 0.101
      irfft(ifft(X, -2), -1)                   f32 0.102   f64 0.082
    fft2_regs (fft2 and ifft2)                 f32 0.137   f64 0.105
    rfft2_regs                                 f32 0.116   f64 0.113
    rfft2_composed                             f32 0.137   f64 0.101
    irfft2_composed                            f32 0.102   f64 0.082
Every route, old and new, is below 0.5, so TAU stays as it is.

Every case asserts dsc.last_fft_path() (expect_path restates the routing), checks that the input is left bit for bit unchanged, and
repeats the call with out= the head of a larger sentinel-filled buffer: the result must be bit-identical and nothing past it may
change.  Steps that end a process (argument errors) or need their own context (the tight arena) run in child processes."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import (C128, CPX, F32, F64, assert_ends_the_process, assert_out_call, build_cpp_smoke, dsc,  # noqa: F401
                           run_child, sync_fixture)
from tests.test_fft2_abi import FUSED_DIMS, FUSED_REAL_COLS, expect_path, fused_group, out_shape2, ref_fft2
from tests.test_fft_ref import TAU, fft_err, real_of

pytestmark = pytest.mark.gpu

KINDS2 = ('fft2', 'ifft2', 'rfft2', 'irfft2')
_sync = sync_fixture('DSC_NO_FFT2_FUSED')


# ---------------------------------------------------------------------------------------------------- inputs and checks

def in_dtype(kind, rdt, real_input=False):
    if kind == 'rfft2' or (real_input and kind in ('fft2', 'ifft2')):
        return rdt
    return CPX[rdt]


def make_images(rng, shape, dt, spice=True):
    """standard normal images (complex ones with imaginary parts everywhere); with spice, image 1 carries a large DC offset, image 2
    one strong 2-D tone and image 3 is all zero between non-zero neighbours"""
    dt = np.dtype(dt)
    x = rng.standard_normal(shape)
    if dt.kind == 'c':
        x = x + 1j * rng.standard_normal(shape)
    h, w = shape[-2], shape[-1]
    v = x.reshape(-1, h, w)
    if spice:
        if v.shape[0] >= 2:
            v[1] += 20
        if v.shape[0] >= 3:
            v[2] += 20 * np.cos(2 * np.pi * (3 * np.arange(h)[:, None] / h + 5 * np.arange(w)[None, :] / w))
        if v.shape[0] >= 5:
            v[3] = 0
    return np.ascontiguousarray(x.astype(dt))


def transform_sizes(kind, shape, s):
    """(N0, N1) the transform runs at (N1: the length along the last axis, for rfft2 / irfft2 the real length)"""
    o = out_shape2(kind, shape, s)
    return o[-2], (2 * (o[-1] - 1) if kind == 'rfft2' else o[-1])


def err_ratio(yh, x, s, kind, images=None):
    """largest err / bound over the images (all, or the listed ones), each flattened to one line"""
    oshape = yh.shape
    y3 = yh.reshape((-1,) + oshape[-2:])
    x3 = x.reshape((-1,) + x.shape[-2:])
    if images is not None:
        y3, x3 = y3[images], x3[images]
    ref = ref_fft2(x3, s, kind)
    assert ref.shape == y3.shape, (ref.shape, y3.shape)
    return fft_err(y3.reshape(y3.shape[0], -1), ref.reshape(ref.shape[0], -1), -1, TAU[real_of(x.dtype)])


def run_case(dsc, record_property, kind, x, s, images=None, fused_off=False):
    """kind(x, s) on the GPU: the route, the shape, the input left alone, every (listed) image within the bound, and a second call
    into the head of a sentinel-filled buffer that must give the same bits and leave the tail alone.  Returns the result."""
    N0, N1 = transform_sizes(kind, x.shape, s)
    want_path = expect_path(kind, x.dtype, N0, N1, x.shape[-2], x.shape[-1], fused_off=fused_off)
    fn = getattr(dsc, kind)
    X = dsc.from_numpy(x)
    y = fn(X, s=s)
    path = dsc.last_fft_path()
    assert path == want_path, (kind, x.dtype, x.shape, s, path, want_path)
    yh = y.numpy()
    odt = real_of(x.dtype) if kind == 'irfft2' else CPX[real_of(x.dtype)]
    oshape = out_shape2(kind, x.shape, s)
    assert yh.shape == oshape and yh.dtype == odt, (yh.shape, yh.dtype, oshape, odt)
    assert X.numpy().tobytes() == x.tobytes(), 'the input changed'
    del y

    def again(out):
        fn(X, out=out, s=s)
        assert dsc.last_fft_path() == want_path
    assert_out_call(dsc, again, oshape, odt, yh)

    r = err_ratio(yh, x, s, kind, images)
    record_property(f'{want_path}:{kind}:{x.dtype}', r)
    print(f'{want_path} {kind} {x.dtype} {x.shape} s={s}: err / bound = {r:.3g}')
    assert r <= 1, f'{want_path} {kind} {x.dtype} {x.shape} s={s}: err / bound = {r:.3g}'
    return yh


def natural_shape(kind, N0, N1):
    """input image of a full transform at N0 x N1"""
    return (N0, N1 // 2 + 1) if kind == 'irfft2' else (N0, N1)


# ---------------------------------------------------------------------------------------------------- the fused windows

def _window_cases():
    cases = []
    for rdt in (F32, F64):
        for N0 in FUSED_DIMS:
            for kind in ('fft2', 'ifft2'):
                cases += [(kind, rdt, N0, N1) for N1 in FUSED_DIMS]
            cases += [('rfft2', rdt, N0, N1) for N1 in FUSED_REAL_COLS]
    return cases


@pytest.mark.parametrize('kind,rdt,N0,N1', _window_cases(), ids=str)
def test_fused_windows(dsc, record_property, kind, rdt, N0, N1):
    """batches of 1, G - 1, G, G + 1 images (G images per workgroup) and more than one wave of workgroups over 256 CUs; the large
    batch is checked on its first and last groups and a seeded sample"""
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, N0, N1])
    G = fused_group(kind, rdt, N0, N1)
    dt = in_dtype(kind, rdt)
    assert expect_path(kind, dt, N0, N1).endswith('_regs')
    for B in sorted({1, max(1, G - 1), G, G + 1}):
        run_case(dsc, record_property, kind, make_images(rng, (B, N0, N1), dt), None)
    B = 2 * 256 * G * (2 if N0 * N1 <= 4096 else 1) + G + 1
    images = sorted(set(range(5)) | set(range(B - G - 1, B)) | set(int(i) for i in rng.integers(0, B, 6)))
    run_case(dsc, record_property, kind, make_images(rng, (B, N0, N1), dt), None, images=images)


@pytest.mark.parametrize('kind', ['fft2', 'ifft2'])
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1', [(32, 32), (64, 128), (128, 64), (128, 128)])
def test_real_input_is_widened(dsc, record_property, kind, rdt, N0, N1):
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, N0, N1, 1])
    G = fused_group(kind, rdt, N0, N1)
    run_case(dsc, record_property, kind, make_images(rng, (G + 5, N0, N1), rdt), None)


@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1', [(32, 64), (64, 64), (128, 256), (16, 64), (256, 256)])
def test_irfft2_is_composed(dsc, record_property, rdt, N0, N1):
    """random spectra: non-Hermitian, with imaginary parts in columns 0 and order that must not reach the result"""
    rng = np.random.default_rng([rdt.itemsize, N0, N1, 2])
    x = make_images(rng, (5, N0, N1 // 2 + 1), CPX[rdt])
    assert np.all(x[0, :, 0].imag != 0) and np.all(x[0, :, -1].imag != 0)
    run_case(dsc, record_property, 'irfft2', x, None)


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1', [(16, 64), (64, 16), (256, 256), (32, 1024), (1024, 32)])
def test_composed_sizes(dsc, record_property, kind, rdt, N0, N1):
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, N0, N1, 3])
    x = make_images(rng, (3,) + natural_shape(kind, N0, N1), in_dtype(kind, rdt))
    assert expect_path(kind, x.dtype, N0, N1).endswith('_composed')
    run_case(dsc, record_property, kind, x, None)


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
def test_batch_shapes(dsc, record_property, kind, rdt):
    """[h, w], [B, h, w] and [2, 3, h, w]"""
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, 4])
    for N0, N1 in ((64, 64), (32, 128)):
        img = natural_shape(kind, N0, N1)
        for lead in ((), (7,), (2, 3)):
            run_case(dsc, record_property, kind, make_images(rng, lead + img, in_dtype(kind, rdt)), None)


# ---------------------------------------------------------------------------------------------------- padded and cropped

def _fits(N):
    return (N - 1, N // 2 + 1, N + 3)


@pytest.mark.parametrize('kind', ['fft2', 'ifft2', 'rfft2'])
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1', [(32, 64), (64, 128), (128, 64)])
def test_padded_and_cropped_with_explicit_s(dsc, record_property, kind, rdt, N0, N1):
    """h and w each one of N - 1, N / 2 + 1, N + 3 (odd and even widths: both load forms of the real kernel)"""
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, N0, N1, 5])
    G = fused_group(kind, rdt, N0, N1)
    for h in _fits(N0):
        for w in _fits(N1):
            for real_input in ((False, True) if kind != 'rfft2' and (h, w) == (N0 - 1, N1 + 3) else (False,)):
                x = make_images(rng, (G + 2, h, w), in_dtype(kind, rdt, real_input))
                run_case(dsc, record_property, kind, x, (N0, N1))


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
def test_s_none_on_other_shapes(dsc, record_property, kind, rdt):
    """s=None rounds each axis up to a power of two; s that is no power of two is rounded too"""
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, 6])
    for h, w in ((50, 100), (33, 65), (100, 20), (3, 50)):
        run_case(dsc, record_property, kind, make_images(rng, (3, h, w), in_dtype(kind, rdt)), None)
    run_case(dsc, record_property, kind, make_images(rng, (3, 50, 100), in_dtype(kind, rdt)), (60, 70))
    run_case(dsc, record_property, kind, make_images(rng, (3, 50, 100), in_dtype(kind, rdt)), (20, 300))
    run_case(dsc, record_property, kind, make_images(rng, (3, 50, 100), in_dtype(kind, rdt)), (-1, 128))


# ---------------------------------------------------------------------------------------------------- known answers

@pytest.mark.parametrize('kind', ['fft2', 'ifft2', 'rfft2'])
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1', [(32, 64), (64, 128), (128, 128)])
def test_impulses_have_known_answers(dsc, record_property, kind, rdt, N0, N1):
    """a single impulse at each corner and at (N0 / 2, N1 / 2): every bin has modulus 1 (ifft2: 1 / (N0 N1)) and the phase of its
    position; image 0 (impulse at the origin) is constant"""
    spots = [(0, 0), (0, N1 - 1), (N0 - 1, 0), (N0 - 1, N1 - 1), (N0 // 2, N1 // 2)]
    x = np.zeros((len(spots), N0, N1), in_dtype(kind, rdt))
    for i, (r, c) in enumerate(spots):
        x[i, r, c] = 1
    yh = run_case(dsc, record_property, kind, x, None)
    cols = yh.shape[-1]
    sign, scale = (1, 1.0 / (N0 * N1)) if kind == 'ifft2' else (-1, 1.0)
    k0, k1 = np.arange(N0)[:, None], np.arange(cols)[None, :]
    tol = 100 * np.finfo(rdt).eps
    for i, (r, c) in enumerate(spots):
        want = scale * np.exp(sign * 2j * np.pi * ((k0 * r % N0) / N0 + (k1 * c % N1) / N1))
        assert np.max(np.abs(yh[i] - want)) <= tol * scale, (kind, rdt, spots[i])
    assert np.all(yh[0] == yh[0].flat[0])


# ---------------------------------------------------------------------------------------------------- in place, switch, round trips

@pytest.mark.parametrize('kind', ['fft2', 'ifft2'])
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1,fused_off', [(32, 32, False), (64, 128, False), (128, 128, False), (64, 64, True), (256, 64, False)])
def test_in_place(dsc, kind, rdt, N0, N1, fused_off):
    """out = x for a complex image of the transform's size, on the fused and the composed route: the bits of the out-of-place call"""
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, N0, N1, 7])
    G = fused_group(kind, rdt, min(N0, 128), N1)
    x = make_images(rng, (3 * G + 1, N0, N1), CPX[rdt])
    if fused_off:
        os.environ['DSC_NO_FFT2_FUSED'] = '1'
    want_path = expect_path(kind, x.dtype, N0, N1, fused_off=fused_off)
    fn = getattr(dsc, kind)
    want = fn(dsc.from_numpy(x)).numpy()
    assert dsc.last_fft_path() == want_path
    X = dsc.from_numpy(x)
    y = fn(X, out=X)
    assert dsc.last_fft_path() == want_path
    assert X.numpy().tobytes() == want.tobytes() and y.numpy().tobytes() == want.tobytes()
    assert err_ratio(want, x, None, kind) <= 1


@pytest.mark.parametrize('kind', ['fft2', 'ifft2', 'rfft2'])
@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
def test_switch_forces_the_composed_route(dsc, record_property, kind, rdt):
    """DSC_NO_FFT2_FUSED=1 is read at every call; both routes hold the bound, so they agree within twice of it"""
    rng = np.random.default_rng([KINDS2.index(kind), rdt.itemsize, 8])
    for N0, N1 in ((32, 64), (128, 128)):
        x = make_images(rng, (9, N0, N1), in_dtype(kind, rdt))
        fused = run_case(dsc, record_property, kind, x, None)
        os.environ['DSC_NO_FFT2_FUSED'] = '1'
        composed = run_case(dsc, record_property, kind, x, None, fused_off=True)
        os.environ.pop('DSC_NO_FFT2_FUSED')
        a, b = fused.reshape(9, -1), composed.reshape(9, -1)
        assert fft_err(a, b.astype(np.clongdouble), -1, 2 * TAU[rdt]) <= 1
        again = getattr(dsc, kind)(dsc.from_numpy(x))
        assert dsc.last_fft_path() == expect_path(kind, x.dtype, N0, N1) and again.numpy().tobytes() == fused.tobytes()


@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
@pytest.mark.parametrize('N0,N1', [(32, 32), (64, 128), (128, 128), (256, 64), (16, 32)])
def test_round_trips(dsc, rdt, N0, N1):
    """ifft2(fft2(x)) = x and irfft2(rfft2(x)) = x: two transforms, each within tau per image"""
    rng = np.random.default_rng([rdt.itemsize, N0, N1, 9])
    tau = 2 * TAU[rdt]
    xc = make_images(rng, (6, N0, N1), CPX[rdt], spice=False)
    back = dsc.ifft2(dsc.fft2(dsc.from_numpy(xc))).numpy()
    assert fft_err(back.reshape(6, -1), xc.reshape(6, -1).astype(np.clongdouble), -1, tau) <= 1
    xr = make_images(rng, (6, N0, 2 * N1), rdt, spice=False)
    X = dsc.rfft2(dsc.from_numpy(xr))
    back = dsc.irfft2(X).numpy()
    assert back.shape == xr.shape and back.dtype == rdt
    assert fft_err(back.reshape(6, -1), xr.reshape(6, -1).astype(np.longdouble), -1, tau) <= 1


# ---------------------------------------------------------------------------------------------------- child processes

TIGHT = r'''
import sys
import numpy as np
import dsc_amd as dsc
kind, dt, N0, N1, B = sys.argv[1], np.dtype(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
cols = N1 // 2 + 1 if kind == 'rfft2' else N1
cdt = np.dtype(np.complex64 if dt in (np.dtype(np.float32), np.dtype(np.complex64)) else np.complex128)
x_bytes, out_bytes = B * N0 * N1 * dt.itemsize, B * N0 * cols * cdt.itemsize
dsc.init(x_bytes + out_bytes + (1 << 20), 1 << 20)
rng = np.random.default_rng(3)
x = rng.standard_normal((B, N0, N1))
if dt.kind == 'c':
    x = x + 1j * rng.standard_normal((B, N0, N1))
x = x.astype(dt)
y = getattr(dsc, kind)(dsc.from_numpy(x))
print('path', dsc.last_fft_path())
yh = y.numpy()
want = getattr(np.fft, kind)(x[:4].astype(np.float64 if dt.kind == 'f' else np.complex128))
err = np.linalg.norm(yh[:4] - want) / np.linalg.norm(want)
print('err', err)
assert err < (1e-5 if cdt == np.dtype(np.complex64) else 1e-12)
print('tight ok')
'''


@pytest.mark.parametrize('kind,dt,N0,N1', [('fft2', 'complex64', 64, 64), ('ifft2', 'complex128', 128, 128), ('rfft2', 'float32', 128, 256),
                                           ('rfft2', 'float64', 32, 64)])
def test_fused_route_needs_no_intermediate(kind, dt, N0, N1):
    """a context with room for x and out and 1 MiB: the fused route runs; the composed one would need an intermediate of out's size"""
    B = (32 << 20) // (N0 * N1 * np.dtype(dt).itemsize)
    r = run_child(TIGHT, args=(kind, dt, str(N0), str(N1), str(B)))
    assert r.returncode == 0 and 'tight ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    assert ('path rfft2_regs' if kind == 'rfft2' else 'path fft2_regs') in r.stdout


ERRORS = {
    'rfft2_of_complex': ("dsc.rfft2(dsc.from_numpy(np.ones((2, 32, 64), np.complex64)))", 'RFFT2 input must be real'),
    'irfft2_of_real': ("dsc.irfft2(dsc.from_numpy(np.ones((2, 32, 33), np.float32)))", 'IRFFT2 input must be complex'),
    'one_dimension': ("dsc.fft2(dsc.from_numpy(np.ones(64, np.complex64)))", 'at least 2 dimensions'),
    'out_shape': ("dsc.fft2(dsc.from_numpy(np.ones((2, 32, 64), np.complex64)), out=dsc.from_numpy(np.ones((2, 32, 32), np.complex64)))",
                  'out must have'),
    'out_dtype': ("dsc.rfft2(dsc.from_numpy(np.ones((2, 32, 64), np.float64)), out=dsc.from_numpy(np.ones((2, 32, 33), np.complex64)))",
                  'out must have'),
}


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_argument_errors_end_the_process(name):
    """like every operator: a message on stderr and a non-zero exit; nothing runs on the GPU after it"""
    assert_ends_the_process(*ERRORS[name], without_env='DSC_NO_FFT2_FUSED')


def test_cpp_fft2_smoke_on_the_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_fft2_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'fft2 templates ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])


# ---------------------------------------------------------------------------------------------------- full size

@pytest.mark.parametrize('rdt', [F32, F64], ids=str)
def test_full_size(dsc, rdt):
    """about 2 GiB of complex 128 x 128 images through fft2_regs: a seeded sample of images against the reference, Parseval over
    every image (sum |X|^2 = N0 N1 sum |x|^2; summed on the host in f64, as tests/test_gpu_headline.py does for rows), the input
    unchanged"""
    N = 128
    B = (2 << 30) // (N * N * CPX[rdt].itemsize)
    rng = np.random.default_rng([rdt.itemsize, 10])
    blk = make_images(rng, (64, N, N), CPX[rdt])
    gain = (1.0 + (np.arange(B) % 5) * 0.25).astype(rdt)
    x = np.tile(blk, (B // 64, 1, 1)) * gain[:, None, None]
    assert x.dtype == CPX[rdt] and x.nbytes == 2 << 30
    X = dsc.from_numpy(x)
    Y = dsc.fft2(X)
    assert dsc.last_fft_path() == 'fft2_regs'

    yh = Y.numpy()
    del Y

    def energy(a):                                              # per image, in f64, a block of images at a time
        return np.concatenate([np.sum(np.abs(a[i:i + 512].astype(C128)) ** 2, axis=(1, 2)) for i in range(0, B, 512)])

    e_t, e_f = energy(x), energy(yh)
    live = e_t > 0
    assert np.all(e_f[~live] == 0) and np.count_nonzero(~live) == B // 64
    assert np.max(np.abs(e_f[live] / (N * N) - e_t[live]) / e_t[live]) < (1e-5 if rdt == F32 else 1e-12)
    images = sorted({0, 1, 2, 3, 63, 64, B // 2 + 3, B - 1} | set(int(i) for i in rng.integers(0, B, 8)))
    r = err_ratio(yh, x, None, 'fft2', images)
    print(f'full size {rdt}: err / bound = {r:.3g}')
    assert r <= 1
    # homogeneity: image i is gain[i] / gain[i % 64] times image i % 64, to rounding
    i = B - 7
    assert np.allclose(yh[i], yh[i % 64] * (gain[i] / gain[i % 64]), rtol=0, atol=1e-4 * np.abs(yh[i]).max() if rdt == F32 else 1e-12 * np.abs(yh[i]).max())
    assert X.numpy().tobytes() == x.tobytes()
