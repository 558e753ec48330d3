"""The long-double reference of dsc.filter_fft (README filterFFT: y = irfft(rfft(s, n) * H)) and the error bound the GPU tests of
tests/test_gpu_filter.py hold it to.  CPU only: the tests here pin the reference itself against a direct convolution and against
the oracle's three-operator composition.

The reference runs numpy's FFT in long double (numpy >= 2.0 transforms np.longdouble natively).  It needs a long double that is
wider than f64 — x86-64's 80-bit format, eps 1.1e-19 — or the f64 kernels would be compared with something as coarse as themselves;
the module refuses to load otherwise."""
import numpy as np
import pytest

from oracle import port

assert np.finfo(np.longdouble).eps < 1e-18, 'the filter reference needs a long double wider than f64'

# FFT filter error grows like eps * log n * max|H| * ||s||_2, whatever the gain of H.  tau: 2.5x the README's measured 65536-point
# rfft rel-L2 error (3.9e-7) for forward plus inverse; the f64 value scaled the same way.  Never above the north star 1e-5 / 1e-12.
TAU = {np.dtype(np.float32): 2e-6, np.dtype(np.float64): 1e-14}


def used(s, n):
    """each row of s cropped or zero padded to n samples, as dsc_rfft(s, n) reads it"""
    s = np.asarray(s)
    ls = s.shape[-1]
    if ls >= n:
        return s[..., :n]
    return np.concatenate([s, np.zeros(s.shape[:-1] + (n - ls,), s.dtype)], axis=-1)


def ref_filter(s, H, n):
    """irfft(rfft(s, n) * H, n) in long double, from s and H exactly as passed to the GPU.  The imaginary parts of the products at
    bin 0 and bin n/2 are dropped, as irfft drops them."""
    H = np.asarray(H)
    assert H.shape == (n // 2 + 1,), (H.shape, n)
    s_ld = used(s, n).astype(np.longdouble)
    H_ld = H.astype(np.clongdouble)
    P = np.fft.rfft(s_ld, n) * H_ld
    assert P.dtype == np.clongdouble
    P[..., 0] = P[..., 0].real
    P[..., -1] = P[..., -1].real
    y = np.fft.irfft(P, n)
    assert y.dtype == np.longdouble
    return y


def filter_err(y, want, s, H, n, tau):
    """largest per-row ratio of the error to its bound (<= 1 passes):
        ||y - ref||_2  <= tau * max|H| * ||s_used||_2
        max |y - ref|  <= 8 * tau * max|H| * ||s_used||_2 / sqrt(n)"""
    y = np.asarray(y).reshape(-1, n).astype(np.longdouble)
    want = np.asarray(want).reshape(-1, n)
    su = used(s, n).reshape(-1, n).astype(np.longdouble)
    scale = tau * float(np.max(np.abs(np.asarray(H).astype(np.clongdouble)))) * np.sqrt(np.sum(su * su, axis=-1))
    d = np.abs(y - want)
    l2, mx = np.sqrt(np.sum(d * d, axis=-1)), np.max(d, axis=-1)
    if np.any(scale == 0):                           # a zero row or a zero filter: nothing may come out
        assert not np.any(d[scale == 0]), 'nonzero output where the bound is zero'
        scale = np.where(scale == 0, 1, scale)
    return float(max(np.max(l2 / scale), np.max(mx / (8 * scale / np.sqrt(n)))))


def test_longdouble_reference_is_wide():
    assert np.finfo(np.longdouble).eps < 1e-18
    x = np.arange(8, dtype=np.longdouble)
    assert np.fft.rfft(x).dtype == np.clongdouble and np.fft.irfft(np.fft.rfft(x), 8).dtype == np.longdouble


@pytest.mark.parametrize('n', [4, 64, 1024, 65536])
def test_reference_is_linear_convolution(n):
    """Real taps b (length lb), H = rfft(b, n): wherever ls + lb - 1 <= n the circular filter is the linear convolution, computed
    here directly in long double."""
    rng = np.random.default_rng(n)
    lb = max(1, min(61, n // 4))
    b = rng.standard_normal(lb).astype(np.longdouble)
    H = np.fft.rfft(b, n)                        # clongdouble: the reference keeps it
    for ls in sorted({1, 2, 3, n - lb, n - lb + 1}):
        if ls < 1:
            continue
        s = rng.standard_normal((2, ls)).astype(np.longdouble)
        y = ref_filter(s, H, n)
        want = np.zeros((2, n), np.longdouble)
        for r in range(2):
            want[r, :ls + lb - 1] = np.convolve(s[r], b)
        err = np.max(np.abs(y - want)) / (np.max(np.abs(want)))
        assert err < 1e-16 * np.log2(n), (n, ls, err)


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('n', [4, 512, 4096, 65536])
def test_reference_matches_oracle_composition(dt, n):
    """The reference against the oracle's irfft(mul(rfft(s, n), H)) in the oracle's precision, padded and cropped rows, an H whose
    DC and Nyquist bins carry imaginary parts that both must ignore."""
    rng = np.random.default_rng([n, np.dtype(dt).itemsize])
    cdt = np.complex64 if dt == np.float32 else np.complex128
    H = (rng.standard_normal(n // 2 + 1) + 1j * rng.standard_normal(n // 2 + 1)).astype(cdt)
    for ls in (n, n // 2 + 1, n + 3):
        s = rng.standard_normal((3, ls)).astype(dt)
        want = ref_filter(s, H, n)
        got = np.stack([port.irfft(port.mul(port.rfft(s[r], n), H)) for r in range(3)])
        assert got.dtype == dt
        assert filter_err(got, want, s, H, n, TAU[np.dtype(dt)]) <= 1


def test_bound_catches_a_wrong_bin():
    """The bound is tight enough to see one bin of a 65536-point f32 filter multiplied by the wrong factor."""
    n = 65536
    rng = np.random.default_rng(7)
    H = (rng.standard_normal(n // 2 + 1) + 1j * rng.standard_normal(n // 2 + 1)).astype(np.complex64)
    s = rng.standard_normal((2, n)).astype(np.float32)
    want = ref_filter(s, H, n)
    assert filter_err(want.astype(np.float32), want, s, H, n, TAU[np.dtype(np.float32)]) <= 1
    Hw = H.copy()
    Hw[n // 4] *= 1.5
    assert filter_err(ref_filter(s, Hw, n), want, s, H, n, TAU[np.dtype(np.float32)]) > 1
