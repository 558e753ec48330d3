"""CPU tests of dsc_hilbert / dsc_envelope (include/dsc_mi355x.h, Section G): the prototypes are declared, exported, bound and wrapped;
the long-double reference ref_hilbert / ref_envelope — the oracle of tests/test_gpu_hilbert.py — is the textbook ifft(fft(x) * h) and
scipy.signal.hilbert; the bound hilbert_err is calibrated with numpy's native f32 / f64 transforms standing in for the kernel and shown
to catch one wrong element and a swapped sign; expect_path restates the routing of dsc_amd/csrc/hilbert.cpp.

The definition: N = pow2(n > 0 ? n : T), x_used = the row cropped or zero padded to N samples, H[0] = H[N/2] = 0 and H[k] = -i in between,
    y = irfft(rfft(x_used, N) * H, N),   hilbert = x_used + i y,   envelope = sqrt(x_used^2 + y^2).

The bound (largest per-row ratio, <= 1 passes), tau = tests.test_filter_ref.TAU (f32 2e-6, f64 1e-14: the fused filter's own, since this
is its arithmetic with max|H| = 1), the element form that of tests.test_fft_ref.fft_err:
    imaginary part   ||y - ref||_2 <= tau ||x_used||_2      |y_k - ref_k| <= tau (8 ||x_used||_2 / sqrt(N) + |ref_k| + max_j |ref_j| / 8)
    envelope         ||e - ref||_2 <= tau ||ref||_2         |e_k - ref_k| <= tau (8 ||x_used||_2 / sqrt(N) + |ref_k|)
A row whose bound is zero must come out exactly zero."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke
from tests.test_fft_ref import pow2
from tests.test_filter_ref import TAU, ref_filter, used

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'dsc_mi355x.h')
LIB = os.path.join(ROOT, 'dsc_amd', 'libdsc_mi355x.so')
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
KINDS = ('hilbert', 'envelope')
FUSED_MIN_N, FUSED_MAX_N = 512, 32768

# rows per workgroup of the fused kernel (mid_cfg<R, B, TWO, 1>::G of fft_regs_mid.hip), by N
FUSED_GROUP = {F32: {512: 16, 1024: 8, 2048: 4, 4096: 4, 8192: 2, 16384: 1, 32768: 1},
               F64: {512: 32, 1024: 16, 2048: 4, 4096: 2, 8192: 1, 16384: 1, 32768: 1}}


# ---- the reference -------------------------------------------------------------------------------------------------------------
def length_of(T, n=None):
    return pow2(n if n is not None and n > 0 else T)


def response(N):
    """H [N/2 + 1]: 0 at bins 0 and N/2, -i in between"""
    H = np.full(N // 2 + 1, -1j, dtype=np.clongdouble)
    H[0] = H[-1] = 0
    return H


def ref_hilbert(x, n=None):
    """[.., T] real -> [.., N] clongdouble, real part x_used exactly"""
    x = np.asarray(x)
    N = length_of(x.shape[-1], n)
    y = ref_filter(x, response(N), N)
    z = np.empty(y.shape, np.clongdouble)
    z.real = used(x, N).astype(np.longdouble)
    z.imag = y
    return z


def ref_envelope(x, n=None):
    z = ref_hilbert(x, n)
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def hilbert_err(y, ref, x_used, tau, envelope=False):
    """largest per-row ratio of the error to its bound; y: the imaginary part of the analytic signal (or the envelope), ref: the same of
    the reference, x_used: the rows as the transform read them"""
    N = ref.shape[-1]
    y = np.asarray(y).reshape(-1, N).astype(np.longdouble)
    ref = np.asarray(ref).reshape(-1, N).astype(np.longdouble)
    xu = np.asarray(x_used).reshape(-1, N).astype(np.longdouble)
    assert y.shape == ref.shape == xu.shape, (y.shape, ref.shape, xu.shape)
    d = np.abs(y - ref)
    a = np.abs(ref)
    xn = np.sqrt(np.sum(xu * xu, axis=-1))
    l2_scale = tau * (np.sqrt(np.sum(ref * ref, axis=-1)) if envelope else xn)
    zero = xn == 0
    if np.any(zero):                                     # an all-zero row: nothing may come out
        assert not np.any(d[zero]), 'nonzero output on a row whose bound is zero'
    l2_scale = np.where(l2_scale == 0, 1, l2_scale)
    el = tau * (8 * xn[:, None] / np.sqrt(N) + a + (0 if envelope else np.max(a, axis=-1)[:, None] / 8))
    el = np.where(el == 0, 1, el)
    l2 = np.sqrt(np.sum(d * d, axis=-1)) / l2_scale
    return float(max(np.max(l2), np.max(d / el)))


def expect_path(kind, dtype, N, T, fused_off=False):
    """dsc_last_fft_path of kind(x [.., T], n) at transform length N"""
    assert kind in KINDS and np.dtype(dtype) in (F32, F64)
    fused = not fused_off and FUSED_MIN_N <= N <= FUSED_MAX_N and T * 8 * 64 < (1 << 30)
    return kind + ('_regs' if fused else '_composed')


def spiced_rows(rng, rows, T, dt):
    """noise; row 1 + 20, row 2 + a strong tone, row 3 one impulse, row 4 all zero, row 5 a third of a row (as far as there are rows)"""
    x = rng.standard_normal((rows, T))
    if rows > 1:
        x[1] += 20
    if rows > 2:
        x[2] += 20 * np.cos(2 * np.pi * 5 * np.arange(T) / T)
    if rows > 3:
        x[3] = 0
        x[3, T // 3] = 1
    if rows > 4:
        x[4] = 0
    if rows > 5:
        x[5, T // 3:] = 0
    return np.ascontiguousarray(x.astype(dt))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared_exported_and_bound():
    text = open(HEADER).read()
    assert 'Section G' in text and 'DSC_NO_HILBERT_FUSED' in text
    for name in ('dsc_hilbert', 'dsc_envelope'):
        assert re.search(name + r' *\(dsc_ctx \*ctx, const dsc_tensor \*x, dsc_tensor \*out, int n\);', text), name
    lib = ctypes.CDLL(LIB)
    assert lib.dsc_hilbert and lib.dsc_envelope
    from dsc_amd import _bindings
    for name in ('dsc_hilbert', 'dsc_envelope'):
        assert name in _bindings.EXPORTS
        assert len(getattr(_bindings, name).argtypes) == 4
    import dsc_amd
    assert callable(dsc_amd.hilbert) and callable(dsc_amd.envelope)
    assert 'hilbert' in dsc_amd.__all__ and 'envelope' in dsc_amd.__all__


def test_cpp_wrappers_and_documents():
    api = open(os.path.join(ROOT, 'dsc_amd', 'api', 'dsc_api.h')).read()
    assert re.search(r'tensor<T> hilbert\(const tensor<T> &x, int n = -1\)', api)
    assert re.search(r'tensor<T> envelope\(const tensor<T> &x, int n = -1\)', api)
    assert 'DSC_NO_HILBERT_FUSED' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'hilbert' in readme and 'envelope' in readme


def test_cpp_hilbert_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_hilbert_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout


# ---- the reference is the textbook and scipy's ---------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 8, 64, 512, 4096])
def test_reference_is_the_textbook_analytic_signal(N):
    """ifft(fft(x_used) * h), h = 1, 2, .., 2, 1, 0, .., 0, in long double, on full, padded and cropped rows"""
    rng = np.random.default_rng(N)
    h = np.zeros(N, np.longdouble)
    h[0] = 1
    h[N // 2] = 1
    h[1:N // 2] = 2
    for T in sorted({N, max(1, N - 1), N // 2 + 1, N + 3}):
        x = rng.standard_normal((3, T))
        xu = used(x, N).astype(np.longdouble)
        want = np.fft.ifft(np.fft.fft(xu) * h)
        assert want.dtype == np.clongdouble
        got = ref_hilbert(x, N)
        assert got.shape == (3, N) and got.dtype == np.clongdouble
        assert np.all(got.real == xu)
        top = float(np.max(np.abs(want)))
        assert np.max(np.abs(got - want)) <= 1e-17 * top, (N, T)
        assert np.max(np.abs(ref_envelope(x, N) - np.abs(want))) <= 1e-17 * top


@pytest.mark.parametrize('N', [2, 16, 256, 2048, 65536])
def test_reference_is_scipy_hilbert(N):
    from scipy import signal
    rng = np.random.default_rng(N + 1)
    for T in sorted({N, max(1, N - 1), N // 2 + 1, N + 3}):
        x = rng.standard_normal((2, T)).astype(np.float32)
        want = signal.hilbert(x.astype(np.float64), N)
        got = ref_hilbert(x, N)
        top = float(np.max(np.abs(want)))
        assert np.max(np.abs(got - want)) <= 1e-13 * top, (N, T)
        assert np.max(np.abs(ref_envelope(x, N) - np.abs(want))) <= 1e-13 * top


def test_length_rule():
    assert [length_of(T) for T in (2, 3, 1000, 3000, 4096)] == [2, 4, 1024, 4096, 4096]
    assert length_of(1000, 600) == 1024 and length_of(10, 4097) == 8192 and length_of(5000, -1) == 8192
    x = np.arange(10.0)
    assert ref_hilbert(x, 6).shape == (8,) and ref_envelope(x).shape == (16,)


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def _stand_in(x, N, dt):
    """numpy's native transform of the dtype in the kernel's place"""
    cdt = np.complex64 if dt == F32 else np.complex128
    xu = used(x, N).astype(dt)
    P = np.fft.rfft(xu, N) * response(N).astype(cdt)
    assert P.dtype == cdt
    y = np.fft.irfft(P, N)
    assert y.dtype == dt
    return xu, y, np.sqrt(xu * xu + y * y)


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N', [512, 2048, 8192, 32768, 65536])
def test_bound_is_calibrated_on_native_transforms(dt, N):
    """Worst ratios seen here, N = 512 .. 65536: imaginary part 0.28 (f32) / 0.062 (f64), envelope 0.93 / 0.18, all on the impulse row at
    N = 65536; every other row stays below 0.08 / 0.05.  The impulse's ratio depends on where it sits: at sample 1 of 65536 the f32
    envelope ratio is 0.20, at sample 0 or N / 2 0.49, at N / 3 (spiced_rows) 0.93 — numpy's f32 transform, not the kernels'; the GPU
    figures are in tests/test_gpu_hilbert.py."""
    rng = np.random.default_rng([N, dt.itemsize])
    x = spiced_rows(rng, 8, N, dt)
    xu, y, env = _stand_in(x, N, dt)
    ref = ref_hilbert(x, N)
    r_im = hilbert_err(y, ref.imag, xu, TAU[dt])
    r_env = hilbert_err(env, ref_envelope(x, N), xu, TAU[dt], envelope=True)
    print(f'N = {N} {dt}: imaginary part {r_im:.3g}, envelope {r_env:.3g}')
    assert r_im <= 1 and r_env <= 1
    assert not np.any(y[4]) and not np.any(env[4])


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('N', [512, 65536])
def test_bound_catches_one_wrong_element_and_a_swapped_sign(dt, N):
    rng = np.random.default_rng([N, dt.itemsize, 1])
    x = rng.standard_normal((2, N)).astype(dt)
    xu, y, env = _stand_in(x, N, dt)
    ref, ref_env = ref_hilbert(x, N), ref_envelope(x, N)
    tau = TAU[dt]
    assert hilbert_err(y, ref.imag, xu, tau) <= 1 and hilbert_err(env, ref_env, xu, tau, envelope=True) <= 1
    off = 20 * tau * float(np.linalg.norm(xu[1].astype(np.float64))) / np.sqrt(N)
    for k in (0, N // 3, N - 1):
        bad = y.astype(np.longdouble)
        bad[1, k] += off
        assert hilbert_err(bad, ref.imag, xu, tau) > 1
        bad = env.astype(np.longdouble)
        bad[1, k] += off
        assert hilbert_err(bad, ref_env, xu, tau, envelope=True) > 1
    assert hilbert_err(-y, ref.imag, xu, tau) > 1


def test_zero_row_must_be_exact():
    x = np.zeros((2, 512), np.float32)
    x[1] = 1
    ref = ref_hilbert(x)
    y = np.zeros((2, 512), np.float32)
    assert hilbert_err(y, ref.imag, x, TAU[F32]) <= 1
    y[0, 7] = 1e-30
    with pytest.raises(AssertionError):
        hilbert_err(y, ref.imag, x, TAU[F32])


def test_expect_path():
    assert expect_path('hilbert', F32, 512, 512) == 'hilbert_regs' and expect_path('envelope', F64, 32768, 100) == 'envelope_regs'
    assert expect_path('hilbert', F32, 256, 256) == 'hilbert_composed' and expect_path('envelope', F32, 65536, 65536) == 'envelope_composed'
    assert expect_path('hilbert', F64, 4096, 4096, fused_off=True) == 'hilbert_composed'
    assert expect_path('hilbert', F32, 32768, 1 << 21) == 'hilbert_composed'
    assert set(FUSED_GROUP[F32]) == set(FUSED_GROUP[F64]) == {1 << k for k in range(9, 16)}
