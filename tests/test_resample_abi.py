"""CPU tests of dsc_upfirdn / dsc_resample_poly / dsc_decimate / dsc_firwin (include/dsc_mi355x.h, Section H): the prototypes are declared,
exported, bound and wrapped; the long-double reference ref_polyphase — the oracle of tests/test_gpu_resample.py — is scipy's upfirdn,
resample_poly and decimate; dsc_firwin_host (host only, called through ctypes) is scipy.signal.firwin; the bound polyphase_err is
calibrated with a sequential numpy stand-in of the data's precision and shown to catch one wrong element, a phase error, a reversed
filter and a nonzero output where nothing may come out.

The primitive: P(x, h, gain, up, down, t0, T_out), along the last axis,
    y[r][m] = sum_i (h[t - i up] gain) x[r][i],   t = m down + t0,   over 0 <= i < T and 0 <= t - i up < M;   0 <= m < T_out
    upfirdn        gain 1,  t0 0,         T_out = ceil(((T - 1) up + M) / down)
    resample_poly  gain up, t0 half_len,  T_out = ceil(T up / down), up and down reduced by their gcd (1 / 1: a copy); half_len =
                   10 max(up, down) with the designed Kaiser filter, (M - 1) // 2 with the caller's taps
    decimate       resample_poly(x, 1, q, firwin(n + 1, 1 / q, hamming)), n = 20 q by default

The bound, elementwise, K = ceil(M / up), u = 2^-24 (f32) or 2^-53 (f64), A[r][m] = sum |tap| |x| over the same terms:
    |y - ref| <= (K + 2) u A
the standard bound of a K-term dot product in any summation order, with or without FMA: |fl(dot) - dot| <= gamma_K A with
gamma_K = K u / (1 - K u) = K u + (K u)^2 / (1 - K u), and (K u)^2 = u (K^2 u) <= u while K^2 u <= 1, so gamma_K < (K + 2) u.  polyphase_err
asserts K^2 u <= 1: K <= 4096 in f32 (the 4096-tap cases at up = 1 sit exactly on it).  Where A = 0 the output must be exactly 0.

ref_polyphase zero-stuffs the row and runs np.convolve in long double.  by_phase=True forms the same sums without the stuffed zeros
(output t = p + n up is sample n of x convolved with the taps p, p + up, ..: the zeros contribute exact zeros) — T M instead of T up M
products, which keeps the largest GPU cases (up = 160, 4096 taps at up = 16) to a fraction of a second; the two agree to the rounding
of long double (test_by_phase_reference_is_the_stuffed_one)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'dsc_mi355x.h')
LIB = os.path.join(ROOT, 'dsc_amd', 'libdsc_mi355x.so')
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
UNIT = {F32: 2.0 ** -24, F64: 2.0 ** -53}
NAMES = ('dsc_upfirdn', 'dsc_resample_poly', 'dsc_decimate', 'dsc_firwin', 'dsc_firwin_host')
RATE_PAIRS = [(1, 2), (2, 1), (3, 2), (2, 3), (5, 7), (7, 5), (1, 4), (4, 1), (160, 147), (1, 8)]
WINDOWS = {'hamming': 0, 'kaiser': 1}


# ---- the reference -------------------------------------------------------------------------------------------------------------
def staged_taps(h, gain, dt):
    """the taps as the kernel stages them: h gain, the product formed (rounded once) in the data's dtype"""
    h = np.asarray(h)
    assert h.dtype == dt, (h.dtype, dt)
    return h * np.asarray(gain, dtype=dt)


def _polyphase_ld(x, taps, up, down, t0, T_out, by_phase=False):
    """[.., T] and [M] long double -> [.., T_out]: zero-stuff to T up, np.convolve, [t0::down][:T_out] zero-extended"""
    T = x.shape[-1]
    rows = x.reshape(-1, T)
    out = np.zeros((rows.shape[0], T_out), np.longdouble)
    for r in range(rows.shape[0]):
        if by_phase:
            full = np.zeros(T * up + len(taps) - 1 + up, np.longdouble)
            for p in range(min(up, len(taps))):
                c = np.convolve(rows[r], taps[p::up])
                full[p:p + up * len(c):up] = c
            full = full[:T * up + len(taps) - 1]
        else:
            z = np.zeros(T * up, np.longdouble)
            z[::up] = rows[r]
            full = np.convolve(z, taps)
        assert full.dtype == np.longdouble
        kept = full[t0::down][:T_out]
        out[r, :len(kept)] = kept
    return out.reshape(x.shape[:-1] + (T_out,))


def ref_polyphase(x, h, gain, up, down, t0, T_out, by_phase=False):
    """the primitive in long double, on the very taps the kernel staged"""
    x = np.asarray(x)
    return _polyphase_ld(x.astype(np.longdouble), staged_taps(h, gain, x.dtype).astype(np.longdouble), up, down, t0, T_out, by_phase)


def ref_magnitude(x, h, gain, up, down, t0, T_out, by_phase=False):
    """A = sum |tap| |x| over the terms of every output"""
    x = np.asarray(x)
    return _polyphase_ld(np.abs(x.astype(np.longdouble)), np.abs(staged_taps(h, gain, x.dtype).astype(np.longdouble)), up, down, t0, T_out,
                         by_phase)


def polyphase_err(y, ref, A, K, dt):
    """largest |y - ref| / ((K + 2) u A) over all elements (<= 1 passes); asserts an exact zero wherever A = 0"""
    y = np.asarray(y).astype(np.longdouble)
    assert y.shape == ref.shape == A.shape, (y.shape, ref.shape, A.shape)
    assert K * K * UNIT[np.dtype(dt)] <= 1, K
    zero = A == 0
    assert not np.any(y[zero]), 'nonzero output where no term contributes'
    bound = (K + 2) * np.longdouble(UNIT[np.dtype(dt)]) * A
    d = np.abs(y - ref)
    if np.all(zero):
        return 0.0
    return float(np.max(d[~zero] / bound[~zero]))


def upfirdn_plan(T, M, up, down):
    """(gain, up, down, t0, T_out) of upfirdn"""
    return 1, up, down, 0, -(-((T - 1) * up + M) // down)


def resample_plan(T, up, down, M=None):
    """(gain, up, down, t0, T_out) of resample_poly after the gcd reduction (None for 1 / 1: a copy); M: the caller's taps"""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down == 1:
        return None
    half_len = 10 * max(up, down) if M is None else (M - 1) // 2
    return up, up, down, half_len, -(-T * up // down)


def default_taps(up, down, dt):
    """the designed filter of resample_poly (after the reduction), in the dtype; scipy's own design, which dsc_firwin_host equals to 1e-14"""
    from scipy import signal
    g = math.gcd(up, down)
    r = max(up // g, down // g)
    return signal.firwin(20 * r + 1, 1.0 / r, window=('kaiser', 5.0)).astype(dt)


def decimate_taps(q, n, dt):
    from scipy import signal
    n = 20 * q if n is None or n <= 0 else n
    return signal.firwin(n + 1, 1.0 / q, window='hamming').astype(dt)


def spiced_rows(rng, rows, T, dt):
    """noise; row 1 + 20 (a DC offset), row 2 + a strong tone, row 3 one impulse, row 4 all zero, row 5 a third of a row"""
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
    assert 'Section H' in text and 'polyphase_direct' in text and 'polyphase_copy' in text
    protos = [r'dsc_upfirdn *\(dsc_ctx \*ctx, const dsc_tensor \*h, const dsc_tensor \*x, int up, int down, dsc_tensor \*out\);',
              r'dsc_resample_poly\(dsc_ctx \*ctx, const dsc_tensor \*x, int up, int down, const dsc_tensor \*taps, dsc_tensor \*out\);',
              r'dsc_decimate *\(dsc_ctx \*ctx, const dsc_tensor \*x, int q, int n, dsc_tensor \*out\);',
              r'dsc_firwin *\(dsc_ctx \*ctx, int numtaps, double cutoff, int window, double beta, dsc_dtype dtype\);',
              r'void +dsc_firwin_host *\(double \*taps, int numtaps, double cutoff, int window, double beta\);']
    for p in protos:
        assert re.search(p, text), p
    lib = ctypes.CDLL(LIB)
    from dsc_amd import _bindings
    for name, n_args in zip(NAMES, (6, 6, 5, 6, 5)):
        assert hasattr(lib, name), name
        assert name in _bindings.EXPORTS
        assert len(getattr(_bindings, name).argtypes) == n_args, name
    import dsc_amd
    for name in ('upfirdn', 'resample_poly', 'decimate', 'firwin'):
        assert callable(getattr(dsc_amd, name)) and name in dsc_amd.__all__, name


def test_cpp_wrappers_and_documents():
    api = open(os.path.join(ROOT, 'dsc_amd', 'api', 'dsc_api.h')).read()
    assert re.search(r'tensor<T> upfirdn\(const tensor<T> &h, const tensor<T> &x, int up = 1, int down = 1\)', api)
    assert re.search(r'tensor<T> resample_poly\(const tensor<T> &x, int up, int down\)', api)
    assert re.search(r'tensor<T> resample_poly\(const tensor<T> &x, int up, int down, const tensor<T> &taps\)', api)
    assert re.search(r'tensor<T> decimate\(const tensor<T> &x, int q, int n = 0\)', api)
    assert re.search(r'tensor<T> firwin\(int numtaps, double cutoff, int window = 0, double beta = 5.0\)', api)
    for doc in ('README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in ('upfirdn', 'resample_poly', 'decimate', 'firwin'):
            assert name in text, (doc, name)


def test_cpp_resample_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_resample_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout


# ---- the reference is scipy's ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 5, 97])
@pytest.mark.parametrize('up,down', RATE_PAIRS)
def test_reference_is_scipy_upfirdn(up, down, T):
    from scipy import signal
    rng = np.random.default_rng([up, down, T])
    x = rng.standard_normal((2, T)).astype(np.float32)
    for M in (1, 2, 11, 64):                                       # odd and even
        h = rng.standard_normal(M).astype(np.float32)
        want = signal.upfirdn(h.astype(np.float64), x.astype(np.float64), up, down, axis=-1)
        gain, u, d, t0, T_out = upfirdn_plan(T, M, up, down)
        got = ref_polyphase(x, h, gain, u, d, t0, T_out)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (up, down, T, M)


@pytest.mark.parametrize('T', [1, 5, 97])
@pytest.mark.parametrize('up,down', RATE_PAIRS)
def test_reference_is_scipy_resample_poly(up, down, T):
    """default taps and taps= of odd and even length; scipy in float64 on the same dtype-rounded taps (window=taps: scipy multiplies by
    up itself, in float64 — exactly the f32 product where up is a power of two, and one f32 rounding of the tap away elsewhere, which
    is why the comparison runs on f64 data)"""
    from scipy import signal
    rng = np.random.default_rng([up, down, T, 1])
    x = rng.standard_normal((2, T))
    for taps in (default_taps(up, down, F64), rng.standard_normal(20), rng.standard_normal(31)):
        want = signal.resample_poly(x, up, down, axis=-1, window=taps)
        plan = resample_plan(T, up, down, len(taps))
        if taps.shape[0] == 20 * max(up, down) + 1:
            assert plan == resample_plan(T, up, down)
            assert np.array_equal(want, signal.resample_poly(x, up, down, axis=-1))
        got = ref_polyphase(x, taps, *plan)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (up, down, T, len(taps))


@pytest.mark.parametrize('T', [1, 5, 97])
@pytest.mark.parametrize('q,n', [(2, None), (4, None), (8, None), (3, 30), (13, None)])
def test_reference_is_scipy_decimate(q, n, T):
    from scipy import signal
    rng = np.random.default_rng([q, T, 2])
    x = rng.standard_normal((2, T))
    want = signal.decimate(x, q, n, ftype='fir', axis=-1, zero_phase=True)
    taps = decimate_taps(q, n, F64)
    got = ref_polyphase(x, taps, *resample_plan(T, 1, q, len(taps)))
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (q, n, T)


@pytest.mark.parametrize('up,down', RATE_PAIRS + [(16, 15), (4, 6)])
def test_by_phase_reference_is_the_stuffed_one(up, down):
    rng = np.random.default_rng([up, down, 5])
    for T, M in ((1, 1), (5, 2), (97, 11), (40, 20 * max(up, down) + 1), (3, 64)):
        x = rng.standard_normal((2, T)).astype(np.float32)
        h = rng.standard_normal(M).astype(np.float32)
        for plan in (upfirdn_plan(T, M, up, down), resample_plan(T, up, down, M)):
            a, b = ref_polyphase(x, h, *plan), ref_polyphase(x, h, *plan, by_phase=True)
            A, B = ref_magnitude(x, h, *plan), ref_magnitude(x, h, *plan, by_phase=True)
            assert a.shape == b.shape and np.array_equal(A == 0, B == 0)
            assert np.all(np.abs(a - b) <= 1e-17 * A) and np.all(np.abs(A - B) <= 1e-17 * A), (up, down, T, M)


def test_gcd_rule_and_copy():
    assert resample_plan(100, 4, 6) == resample_plan(100, 2, 3) == (2, 2, 3, 30, 67)
    assert resample_plan(100, 5, 5) is None and resample_plan(7, 1, 1) is None
    assert upfirdn_plan(1000, 64, 4, 6) == (1, 4, 6, 0, 677)


# ---- the design ------------------------------------------------------------------------------------------------------------------
def firwin_host(numtaps, cutoff, window, beta=5.0):
    lib = ctypes.CDLL(LIB)
    lib.dsc_firwin_host.restype = None
    lib.dsc_firwin_host.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double]
    h = np.empty(numtaps, np.float64)
    lib.dsc_firwin_host(h.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), numtaps, cutoff, WINDOWS[window], beta)
    return h


@pytest.mark.parametrize('window', ['hamming', 'kaiser'])
@pytest.mark.parametrize('numtaps,r', [(20 * r + 1, r) for r in (2, 3, 7, 147, 160, 400)] + [(20, 2), (146, 7)])
def test_firwin_host_is_scipy_firwin(numtaps, r, window):
    """max|h - h_scipy| <= 1e-14 max|h_scipy| (scipy's own distance from a long-double design is 1e-16 .. 8.4e-16 of max|h| over these
    cases).  Measured here: at most 8.3e-16 of max|h| over the sixteen cases (kaiser, 3201 taps).  Rounded to f32 the two designs
    differ by at most one unit 2^-23 max|h|; they do differ, at the sinc's zero crossings, where both are about 1e-17."""
    from scipy import signal
    want = signal.firwin(numtaps, 1.0 / r, window=window if window == 'hamming' else ('kaiser', 5.0), pass_zero=True, scale=True)
    got = firwin_host(numtaps, 1.0 / r, window)
    top = float(np.max(np.abs(want)))
    d = float(np.max(np.abs(got - want))) / top
    print(f'firwin {window} {numtaps} taps, cutoff 1/{r}: max|h - h_scipy| / max|h| = {d:.3g}')
    assert d <= 1e-14
    assert np.max(np.abs(got.astype(np.float32).astype(np.float64) - want.astype(np.float32))) <= 2.0 ** -23 * top
    assert abs(float(np.sum(got)) - 1) <= 1e-13


def test_firwin_host_one_tap_and_bad_arguments():
    assert firwin_host(1, 0.5, 'hamming').tolist() == [1.0] and firwin_host(1, 0.25, 'kaiser').tolist() == [1.0]
    code = ('import ctypes; L = ctypes.CDLL(%r); L.dsc_firwin_host.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, '
            'ctypes.c_double]; b = (ctypes.c_double * 8)(); L.dsc_firwin_host(b, 8, %s, 0, 0.0); print("survived")')
    for cutoff in ('1.0', '0.0', '-0.5', '1.5'):
        r = subprocess.run([sys.executable, '-c', code % (LIB, cutoff)], capture_output=True, text=True)
        assert r.returncode == 1 and 'survived' not in r.stdout and 'cutoff must lie strictly between 0 and 1' in r.stderr, (cutoff, r.stderr)


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def stand_in(x, h, gain, up, down, t0, T_out):
    """the kernel's arithmetic in numpy: taps staged in the dtype, K products per output summed one after the other in the dtype"""
    dt = x.dtype
    taps = staged_taps(h, gain, dt)
    M, T = len(taps), x.shape[-1]
    K = -(-M // up)
    hp = np.zeros(K * up, dt)
    hp[:M] = taps
    m = np.arange(T_out, dtype=np.int64)
    t = m * down + t0
    i_hi, p = t // up, t % up
    y = np.zeros(x.shape[:-1] + (T_out,), dt)
    for j in range(K):
        i = i_hi - j
        ok = (i >= 0) & (i < T)
        xv = np.where(ok, x[..., np.clip(i, 0, T - 1)], dt.type(0))
        y = (y + hp[p + j * up] * xv).astype(dt)
    return y


def case_of(rng, kind, up, down, T, dt, rows=6):
    x = spiced_rows(rng, rows, T, dt)
    if kind == 'resample':
        h = default_taps(up, down, dt)
        plan = resample_plan(T, up, down)
    else:
        h = rng.standard_normal(kind).astype(dt)
        plan = upfirdn_plan(T, kind, up, down)
    return x, h, plan


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('up,down', RATE_PAIRS + [(8, 1)])
def test_bound_is_calibrated_on_a_sequential_stand_in(dt, up, down):
    """Worst ratios seen here over the eleven rate pairs (T = 300, designed taps, spiced rows): f32 0.20, f64 0.18 (both at (8, 1))."""
    rng = np.random.default_rng([up, down, dt.itemsize])
    x, h, plan = case_of(rng, 'resample', up, down, 300, dt)
    y = stand_in(x, h, *plan)
    K = -(-len(h) // plan[1])
    r = polyphase_err(y, ref_polyphase(x, h, *plan), ref_magnitude(x, h, *plan), K, dt)
    print(f'({up}, {down}) {dt}: err / bound = {r:.3g}')
    assert r <= 1
    assert not np.any(y[4])


def caught(y, ref, A, K, dt):
    """the check rejects y: an element over its bound, or a nonzero where A = 0"""
    try:
        return polyphase_err(y, ref, A, K, dt) > 1
    except AssertionError:
        return True


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_bound_has_teeth(dt):
    rng = np.random.default_rng([dt.itemsize, 3])
    for kind, up, down, T in (('resample', 3, 2, 200), ('resample', 1, 4, 200), (11, 4, 6, 150), (64, 1, 1, 100)):
        x, h, plan = case_of(rng, kind, up, down, T, dt)
        gain, u, d, t0, T_out = plan
        K = -(-len(h) // u)
        ref, A = ref_polyphase(x, h, *plan), ref_magnitude(x, h, *plan)
        y = stand_in(x, h, *plan)
        assert polyphase_err(y, ref, A, K, dt) <= 1
        for k in (0, T_out // 3, T_out - 1):                       # one element off by 4 times its bound
            bad = y.astype(np.longdouble)
            bad[1, k] = ref[1, k] + 4 * (K + 2) * UNIT[dt] * A[1, k]
            assert polyphase_err(bad, ref, A, K, dt) > 1
        assert caught(stand_in(x, h, gain, u, d, t0 + 1, T_out), ref, A, K, dt)                   # a phase error
        live = [0, 1, 2, 5]                                         # ... by the bound itself on the rows without exact zeros
        assert polyphase_err(stand_in(x[live], h, gain, u, d, t0 + 1, T_out), ref[live], A[live], K, dt) > 1
        assert np.array_equal(h, h[::-1]) or polyphase_err(stand_in(x[live], h[::-1].copy(), *plan), ref[live], A[live], K, dt) > 1
        bad = y.copy()
        bad[4, T_out // 2] = 1e-30                                  # row 4 is all zero: A = 0 there
        with pytest.raises(AssertionError):
            polyphase_err(bad, ref, A, K, dt)


def test_reversed_filter_is_caught_on_an_asymmetric_one():
    rng = np.random.default_rng(9)
    x, h, plan = case_of(rng, 11, 3, 2, 120, F32)
    assert not np.array_equal(h, h[::-1])
    ref, A = ref_polyphase(x, h, *plan), ref_magnitude(x, h, *plan)
    assert polyphase_err(stand_in(x, h[::-1].copy(), *plan), ref, A, 4, F32) > 1
