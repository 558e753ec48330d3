"""CPU checks of dsc_fft2 / dsc_ifft2 / dsc_rfft2 / dsc_irfft2 (include/dsc_mi355x.h, Section F): the four entry points exist in the
header, the library, the ctypes bindings and the package; the long-double reference ref_fft2 the GPU tests of tests/test_gpu_fft2.py
compare with — the compositions of the 1-D reference of tests/test_fft_ref.py that DEFINE the four calls — is pinned against
numpy.fft.*2 in long double on power-of-two shapes and against its own definition on padded / cropped ones; expect_path restates the
routing of fft2.cpp; the C++ smoke program compiles and links."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke
from tests.test_fft_ref import pow2, real_of, ref_fft

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NAMES = ('dsc_fft2', 'dsc_ifft2', 'dsc_rfft2', 'dsc_irfft2')
KINDS2 = ('fft2', 'ifft2', 'rfft2', 'irfft2')
FUSED_DIMS = (32, 64, 128)
FUSED_REAL_COLS = (64, 128, 256)


def ref_fft2(x, s, kind):
    """kind(x, s) over the last two axes as DSC defines it, in long double:
      fft2    fft(fft(x, n1, -1), n0, -2)            ifft2   ifft(ifft(x, n1, -1), n0, -2)
      rfft2   fft(rfft(x, n1, -1), n0, -2)           irfft2  irfft(ifft(x, n0, -2), n1, -1)
    s = (n0, n1) or None (the axis lengths).  The intermediate stays in long double, as the definition composes exact operators."""
    n0, n1 = (-1, -1) if s is None else s
    if kind == 'fft2':
        return ref_fft(ref_fft(x, n1, -1, 'fft'), n0, -2, 'fft')
    if kind == 'ifft2':
        return ref_fft(ref_fft(x, n1, -1, 'ifft'), n0, -2, 'ifft')
    if kind == 'rfft2':
        return ref_fft(ref_fft(x, n1, -1, 'rfft'), n0, -2, 'fft')
    assert kind == 'irfft2'
    return ref_fft(ref_fft(x, n0, -2, 'ifft'), n1, -1, 'irfft')


def out_shape2(kind, shape, s):
    """shape of kind(x, s) for x of the given shape"""
    n0, n1 = (-1, -1) if s is None else s
    h, w = shape[-2], shape[-1]
    N0 = pow2(n0 if n0 > 0 else h)
    m = n1 if n1 > 0 else w
    cols = pow2(m) // 2 + 1 if kind == 'rfft2' else 2 * pow2(m - 1) if kind == 'irfft2' else pow2(m)
    return tuple(shape[:-2]) + (N0, cols)


def fused_group(kind, dt, N0, N1):
    """images per workgroup of the fused kernel (fft_2d.hip fft2_cfg): 32 points per thread, groups of at least 256 (f32) / 128
    (f64) threads"""
    threads = N0 * (N1 // 2 if kind == 'rfft2' else N1) // 32
    nt_min = 256 if real_of(dt) == np.dtype(np.float32) else 128
    return max(1, nt_min // threads)


def expect_path(kind, dt, N0, N1, h=None, w=None, fused_off=False):
    """the path dsc.last_fft_path() reports for kind on images transformed at N0 x N1 (N1: the transform length along the last axis,
    for rfft2 the real length) from h x w inputs of dtype dt (fft2.cpp)"""
    if kind == 'irfft2':
        return 'irfft2_composed'
    h, w = N0 if h is None else h, N1 if w is None else w
    composed = 'rfft2_composed' if kind == 'rfft2' else 'fft2_composed'
    ok = N0 in FUSED_DIMS and (N1 in FUSED_REAL_COLS if kind == 'rfft2' else N1 in FUSED_DIMS)
    if fused_off or not ok:
        return composed
    if fused_group(kind, dt, N0, N1) * h * w * np.dtype(dt).itemsize >= 0x7f000000:
        return composed
    return 'rfft2_regs' if kind == 'rfft2' else 'fft2_regs'


def _rand(rng, shape, cplx):
    x = rng.standard_normal(shape).astype(np.longdouble)
    return x + 1j * rng.standard_normal(shape).astype(np.longdouble) if cplx else x


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---------------------------------------------------------------------------------------------------- the surface

def test_header_declares_the_four_prototypes():
    text = open(os.path.join(ROOT, 'include', 'dsc_mi355x.h')).read()
    for name in NAMES:
        assert re.search(r'dsc_tensor \*' + name + r'\s*\(dsc_ctx \*ctx, const dsc_tensor \*x, dsc_tensor \*out, int n0, int n1\);', text), name
    assert 'Section F' in text and 'DSC_NO_FFT2_FUSED' in text


def test_library_exports_and_bindings():
    from dsc_amd import _bindings as B
    lib = ctypes.CDLL(B.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in B.EXPORTS, name
        fn = getattr(B, name)
        assert fn.restype is not None and len(fn.argtypes) == 5 and fn.argtypes[3] is ctypes.c_int and fn.argtypes[4] is ctypes.c_int


def test_package_exposes_the_wrappers():
    import dsc_amd
    for name in KINDS2:
        assert callable(getattr(dsc_amd, name)) and name in dsc_amd.__all__
    api = open(os.path.join(ROOT, 'dsc_amd', 'api', 'dsc_api.h')).read()
    for name in NAMES:
        assert name + '(ctx, x.x_, nullptr, n0, n1)' in api


def test_switch_is_documented():
    assert 'DSC_NO_FFT2_FUSED' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


# ---------------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize('shape', [(32, 32), (3, 64, 128), (2, 3, 16, 256), (128, 8)], ids=str)
def test_reference_equals_numpy_on_power_of_two_shapes(shape):
    rng = np.random.default_rng([len(shape), shape[-1]])
    xc, xr = _rand(rng, shape, True), _rand(rng, shape, False)
    assert _rel(ref_fft2(xc, None, 'fft2'), np.fft.fft2(xc)) <= 1e-17
    assert _rel(ref_fft2(xr, None, 'fft2'), np.fft.fft2(xr.astype(np.clongdouble))) <= 1e-17
    assert _rel(ref_fft2(xc, None, 'ifft2'), np.fft.ifft2(xc)) <= 1e-17
    assert _rel(ref_fft2(xr, None, 'rfft2'), np.fft.rfft2(xr)) <= 1e-17
    # a non-Hermitian spectrum: numpy's irfft2 also inverts axis -2 first and drops what irfft drops
    X = _rand(rng, shape[:-1] + (shape[-1] // 2 + 1,), True)
    got = ref_fft2(X, None, 'irfft2')
    assert got.dtype == np.longdouble and got.shape == tuple(shape)
    assert _rel(got, np.fft.irfft2(X, s=shape[-2:])) <= 1e-17
    for kind, x in (('fft2', xc), ('ifft2', xc), ('rfft2', xr), ('irfft2', X)):
        assert ref_fft2(x, None, kind).shape == out_shape2(kind, x.shape, None)


@pytest.mark.parametrize('s', [None, (64, 64), (20, 300)], ids=str)
def test_reference_on_padded_and_cropped_shapes(s):
    """[3, 50, 100]: the definition spelled out with numpy on the explicitly cropped / zero padded image"""
    rng = np.random.default_rng(5)
    shape = (3, 50, 100)
    n0, n1 = (-1, -1) if s is None else s
    N0, N1 = pow2(n0 if n0 > 0 else 50), pow2(n1 if n1 > 0 else 100)

    def fitted(x, rows, cols):
        y = np.zeros(x.shape[:-2] + (rows, cols), x.dtype)
        r, c = min(rows, x.shape[-2]), min(cols, x.shape[-1])
        y[..., :r, :c] = x[..., :r, :c]
        return y

    xc, xr = _rand(rng, shape, True), _rand(rng, shape, False)
    assert _rel(ref_fft2(xc, s, 'fft2'), np.fft.fft2(fitted(xc, N0, N1))) <= 1e-17
    assert _rel(ref_fft2(xc, s, 'ifft2'), np.fft.ifft2(fitted(xc, N0, N1))) <= 1e-17
    assert _rel(ref_fft2(xr, s, 'rfft2'), np.fft.rfft2(fitted(xr, N0, N1))) <= 1e-17
    for kind, x in (('fft2', xc), ('ifft2', xc), ('rfft2', xr)):
        assert ref_fft2(x, s, kind).shape == out_shape2(kind, shape, s)


@pytest.mark.parametrize('b,n1', [(65, -1), (40, -1), (65, 40), (40, 65)])
def test_irfft2_reference_bins_and_dropped_imaginary_parts(b, n1):
    """b bins with n1: order = pow2((n1 or b) - 1); bins cropped / zero filled to order + 1; the imaginary parts of columns 0 and
    order of the INTERMEDIATE (after the inverse along axis -2) do not reach the result"""
    rng = np.random.default_rng([b, n1 + 1])
    X = _rand(rng, (2, 24, b), True)
    order = pow2((n1 if n1 > 0 else b) - 1)
    got = ref_fft2(X, (32, n1), 'irfft2')
    assert got.shape == (2, 32, 2 * order) == out_shape2('irfft2', X.shape, (32, n1))
    mid = np.fft.ifft(np.concatenate([X, np.zeros((2, 8, b), X.dtype)], axis=-2), axis=-2)
    bins = np.zeros((2, 32, order + 1), np.clongdouble)
    k = min(b, order + 1)
    bins[..., :k] = mid[..., :k]
    assert np.abs(bins[..., 0].imag).max() > 0.01
    bins[..., 0] = bins[..., 0].real
    bins[..., order] = bins[..., order].real
    assert _rel(got, np.fft.irfft(bins, 2 * order, axis=-1)) <= 1e-17


def test_expect_path_windows():
    f32, c64, f64 = np.dtype(np.float32), np.dtype(np.complex64), np.dtype(np.float64)
    for N0 in FUSED_DIMS:
        for N1 in FUSED_DIMS:
            assert expect_path('fft2', c64, N0, N1) == 'fft2_regs' == expect_path('ifft2', f64, N0, N1)
            assert expect_path('fft2', c64, N0, N1, fused_off=True) == 'fft2_composed'
        for N1 in FUSED_REAL_COLS:
            assert expect_path('rfft2', f32, N0, N1) == 'rfft2_regs'
        assert expect_path('rfft2', f32, N0, 32) == 'rfft2_composed' == expect_path('rfft2', f64, N0, 512)
    for N0, N1 in ((16, 64), (64, 16), (256, 256), (32, 1024), (1024, 32)):
        assert expect_path('fft2', c64, N0, N1) == 'fft2_composed'
    assert expect_path('irfft2', c64, 64, 64) == 'irfft2_composed'
    assert expect_path('fft2', c64, 32, 32, h=1 << 20, w=64) == 'fft2_composed'      # 8 images x 512 MiB: past 31-bit offsets
    assert fused_group('fft2', c64, 32, 32) == 8 and fused_group('fft2', np.dtype(np.complex128), 32, 32) == 4
    assert fused_group('rfft2', f32, 32, 64) == 8 and fused_group('fft2', c64, 128, 128) == 1


# ---------------------------------------------------------------------------------------------------- C++

def test_cpp_fft2_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_fft2_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout
