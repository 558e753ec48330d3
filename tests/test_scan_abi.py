"""CPU tests of dsc_cumsum / dsc_diff / dsc_unwrap / dsc_phase (include/dsc_mi355x.h, Section I): the prototypes are declared, exported,
bound and wrapped; a C++ translation unit that names the four wrappers of dsc_api.h compiles and links; the references of
tests/test_gpu_scan.py — ref_cumsum in long double and ref_unwrap, the integer definition of the header — are numpy.cumsum and
numpy.unwrap; and the checks cumsum_err and unwrap_err are calibrated on numpy stand-ins of the data's precision (a tiled scan with a
carry, the structure of the kernels) and shown to catch a K off by one, a dropped carry, a halo from the wrong row and a shifted result.

The definition of unwrap, TWO_PI = 6.283185307179586 and PI = 3.141592653589793 as doubles:
    d[j] = (double) x[j] - (double) x[j - 1];   m[j] = 0 when |d[j]| <= PI or d[j] is not finite, else the integer nearest to d[j] / TWO_PI,
    ties toward zero;   K[j] = m[1] + .. + m[j] (exact integers, K[0] = 0);   out[j] = x[j] - K[j] TWO_PI in double, rounded once.
m[j] is only defined away from its ties, so every input an exact-K check runs on goes through assert_away_from_ties first: every
|d| / TWO_PI at least 1e-9 from a half-integer and every |d| at least 1e-9 from PI.

The bounds, u = 2^-24 (f32, c32) or 2^-53 (f64, c64), per component:
    cumsum   |out[k] - ref[k]| <= gamma_k A[k],  gamma_k = k u / (1 - k u),  A[k] = |x[0]| + .. + |x[k]|: the standard bound of a sum of
             k + 1 terms in any order, and every output of a scan is such a sum tree.  Element 0 is exact and a row of zeros gives zeros.
    unwrap   rint(((double) x - out) / TWO_PI) == K exactly, and |out - ref| <= u |ref| + 4 2^-53 (|x| + TWO_PI |K|): the final rounding
             to the dtype, and the product and the subtraction in double."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'dsc_mi355x.h')
LIB = os.path.join(ROOT, 'dsc_amd', 'libdsc_mi355x.so')
F32, F64, C32, C64 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)
UNIT = {F32: 2.0 ** -24, F64: 2.0 ** -53, C32: 2.0 ** -24, C64: 2.0 ** -53}
NAMES = ('dsc_cumsum', 'dsc_diff', 'dsc_unwrap', 'dsc_phase')
TWO_PI, PI = 6.283185307179586, 3.141592653589793
LD = np.longdouble


# ---- the references and the checks -----------------------------------------------------------------------------------------------
def components(a):
    a = np.asarray(a)
    return [a.real, a.imag] if np.iscomplexobj(a) else [a]


def ref_cumsum(x, axis=-1):
    """numpy.cumsum in (complex) long double"""
    x = np.asarray(x)
    return np.cumsum(x.astype(np.clongdouble if np.iscomplexobj(x) else LD), axis=axis)


def cumsum_err(out, x, axis=-1):
    """largest |out - ref| / (gamma_k A[k]) over every element and component (<= 1 passes); asserts that element 0 along the axis is a
    bit-for-bit copy and that the output is exactly the reference wherever the bound is 0 (A = 0: nothing but zeros so far)"""
    out, x = np.asarray(out), np.asarray(x)
    assert out.shape == x.shape and out.dtype == x.dtype, (out.shape, out.dtype, x.shape, x.dtype)
    assert np.take(out, [0], axis).tobytes() == np.take(x, [0], axis).tobytes(), 'element 0 is not a copy'
    n = x.shape[axis]
    shape = [1] * x.ndim
    shape[axis] = n
    k = np.arange(n, dtype=LD).reshape(shape)
    u = LD(UNIT[x.dtype])
    assert n * UNIT[x.dtype] < 0.5
    gamma = k * u / (1 - k * u)
    worst = 0.0
    for oc, xc in zip(components(out), components(x)):
        ref = np.cumsum(xc.astype(LD), axis=axis)
        bound = gamma * np.cumsum(np.abs(xc).astype(LD), axis=axis)
        d = np.abs(oc.astype(LD) - ref)
        zero = bound == 0
        assert not np.any(d[zero]), 'inexact output where the bound is zero'
        if not np.all(zero):
            worst = max(worst, float(np.max(d[~zero] / bound[~zero])))
    return worst


def wrap_counts(x, axis=-1):
    """m of the definition along the axis (zeros in front), int64, with the steps d"""
    xd = np.moveaxis(np.asarray(x), axis, -1).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.diff(xd, axis=-1)
        q = d / TWO_PI
        m = np.where(q > 0, np.ceil(q - 0.5), np.floor(q + 0.5))
        m = np.where((np.abs(d) <= PI) | ~np.isfinite(d), 0.0, m)
    m = np.concatenate([np.zeros(xd.shape[:-1] + (1,)), m], axis=-1).astype(np.int64)
    return np.moveaxis(m, -1, axis), np.moveaxis(d, -1, axis)


def ref_unwrap(x, axis=-1):
    """the integer definition: (x - K TWO_PI in long double, K as int64)"""
    m, _ = wrap_counts(x, axis)
    K = np.cumsum(m, axis=axis)
    return np.asarray(x).astype(LD) - K.astype(LD) * LD(TWO_PI), K


def assert_away_from_ties(x, axis=-1, gap=1e-9):
    """the condition under which m is defined: returns the smallest distances seen (to a half-integer, to PI)"""
    _, d = wrap_counts(x, axis)
    d = np.abs(d[np.isfinite(d)])
    if d.size == 0:
        return np.inf, np.inf
    q = d / TWO_PI
    half = float(np.min(np.abs(q - np.floor(q) - 0.5)))
    at_pi = float(np.min(np.abs(d - PI)))
    assert half >= gap and at_pi >= gap, (half, at_pi)
    return half, at_pi


def unwrap_err(out, x, axis=-1):
    """asserts the exact integers, rint(((double) x - out) / TWO_PI) == K at every finite sample, and samples that are not finite
    passed through; returns the largest |out - ref| / (u |ref| + 4 2^-53 (|x| + TWO_PI |K|)) (<= 1 passes)"""
    out, x = np.asarray(out), np.asarray(x)
    assert out.shape == x.shape and out.dtype == x.dtype, (out.shape, out.dtype, x.shape, x.dtype)
    ref, K = ref_unwrap(x, axis)
    xd, od = x.astype(np.float64), out.astype(np.float64)
    finite = np.isfinite(xd)
    assert np.array_equal(od[~finite], xd[~finite], equal_nan=True), 'a sample that is not finite changed'
    got = np.rint((xd[finite] - od[finite]) / TWO_PI)
    bad = got != K[finite]
    assert not np.any(bad), f'{int(np.sum(bad))} of {bad.size} integers K differ, first at {int(np.argmax(bad))}'
    bound = LD(UNIT[x.dtype]) * np.abs(ref[finite]) + 4 * LD(2.0 ** -53) * (np.abs(xd[finite]).astype(LD) + LD(TWO_PI) * np.abs(K[finite]))
    d = np.abs(od[finite].astype(LD) - ref[finite])
    zero = bound == 0
    assert not np.any(d[zero])
    return float(np.max(d[~zero] / bound[~zero])) if not np.all(zero) else 0.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def wrapped_chirps(rng, rows, T, dt):
    """rows of linear chirps wrapped to (-pi, pi]: the true phase advances by 0.05 .. 2.6 rad per sample, scaled down on long rows so
    that it ends below 5040 rad (|K| <= 802, the range in which the definition was compared with numpy.unwrap)"""
    t = np.arange(T, dtype=np.float64)
    s = min(1.0, 2800.0 / T)
    f0 = rng.uniform(0.05, 1.0, (rows, 1)) * s
    f1 = rng.uniform(1.0, 2.6, (rows, 1)) * s
    true = rng.uniform(-3, 3, (rows, 1)) + f0 * t + (f1 - f0) * t * t / (2 * max(T - 1, 1))
    return np.ascontiguousarray(np.angle(np.exp(1j * true)).astype(dt))


def multi_wrap_rows(rng, rows, T, dt):
    """random walks with steps of up to +-20 rad per sample: several periods per jump, K in the hundreds on long rows"""
    return np.ascontiguousarray(np.cumsum(rng.uniform(-20, 20, (rows, T)), axis=1).astype(dt))


def smooth_rows(rng, rows, T, dt):
    """no step above 1.5 rad: unwrap must return these bit for bit; row 0 is constant"""
    x = np.cumsum(rng.uniform(-1.5, 1.5, (rows, T)), axis=1)
    x[0] = 2.75
    return np.ascontiguousarray(x.astype(dt))


def cumsum_rows(rng, rows, T, dt):
    """noise; row 1 with a DC offset (the sum grows), row 2 all zero when there are three rows or more"""
    dt = np.dtype(dt)
    x = rng.standard_normal((rows, T))
    if dt.kind == 'c':
        x = x + 1j * rng.standard_normal((rows, T))
    if rows > 1:
        x[1] += 3
    if rows > 2:
        x[2] = 0
    return np.ascontiguousarray(x.astype(dt))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared_exported_bound_and_wrapped():
    text = open(HEADER).read()
    assert 'Section I' in text
    for route in ('scan_rows', 'scan_tiles', 'scan_cols', 'scan_diff', 'DSC_SCAN_ROUTE'):
        assert route in text, route
    for name, arg in zip(NAMES, ('x', 'x', 'x', 'z')):
        assert re.search(r'dsc_tensor \*%s *\(dsc_ctx \*ctx, const dsc_tensor \*%s, dsc_tensor \*out, int axis\);' % (name, arg), text), name
    lib = ctypes.CDLL(LIB)
    from dsc_amd import _bindings
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _bindings.EXPORTS
        f = getattr(_bindings, name)
        assert f.argtypes == [_bindings._DscCtx, _bindings._DscTensor_p, _bindings._DscTensor_p, ctypes.c_int], name
        assert f.restype is _bindings._DscTensor_p
    import dsc_amd
    for name in ('cumsum', 'diff', 'unwrap', 'phase'):
        assert callable(getattr(dsc_amd, name)) and name in dsc_amd.__all__, name


def test_cpp_wrappers_and_documents():
    api = open(os.path.join(ROOT, 'dsc_amd', 'api', 'dsc_api.h')).read()
    for name, arg in (('cumsum', 'x'), ('diff', 'x'), ('unwrap', 'x'), ('phase', 'z')):
        assert re.search(r'tensor<T> %s\(const tensor<T> &%s, int axis = -1\)' % (name, arg), api), name
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in ('cumsum', 'diff', 'unwrap', 'phase'):
            assert name in text, (doc, name)


def test_cpp_scan_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_scan_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout


# ---- the references are numpy's ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_ref_cumsum_is_numpy_cumsum(dt):
    rng = np.random.default_rng([dt.itemsize, 1])
    for shape, axis in (((3, 1000), -1), ((2, 65, 5), 1), ((65, 7), 0), ((2, 3, 4, 5), 2)):
        x = cumsum_rows(rng, shape[0], int(np.prod(shape[1:])), dt).reshape(shape)
        want = np.cumsum(x.astype(C64 if dt.kind == 'c' else F64), axis=axis)
        got = ref_cumsum(x, axis)
        assert got.shape == want.shape and got.dtype in (LD, np.clongdouble)
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize('kind', ['chirps', 'multi_wrap', 'smooth'])
@pytest.mark.parametrize('T', [1, 2, 65, 4097, 70001])
def test_ref_unwrap_is_numpy_unwrap(kind, T):
    """in double.  numpy adds its corrections up in floating point where the definition multiplies once, so the two differ by numpy's own
    error: T additions, each rounding a partial sum of at most TWO_PI max|K| by at most 2^-53 of it, after a correction that carries the
    roundings of the mod (a few 2^-53 of a step of at most max|x| + TWO_PI max|K|) — tol = 4 T 2^-53 (TWO_PI max|K| + max|x|), 1.2e-7 for
    T = 70001 and |K| = 620, against the 6.28 of one wrong integer.  Measured here: at most 5.6e-11 (chirps, T = 70001, |K| up to 620);
    2.6e-11 on multi_wrap at T = 70001 (|K| up to 562).  On the smooth rows the two are equal."""
    rng = np.random.default_rng([T, len(kind)])
    x = {'chirps': wrapped_chirps, 'multi_wrap': multi_wrap_rows, 'smooth': smooth_rows}[kind](rng, 3, T, F64)
    assert_away_from_ties(x)
    ref, K = ref_unwrap(x)
    want = np.unwrap(x, axis=-1)
    d = float(np.max(np.abs(ref - want)))
    print(f'{kind} T = {T}: max |ref - numpy.unwrap| = {d:.3g}, max |K| = {int(np.max(np.abs(K)))}')
    assert d <= 4 * T * 2.0 ** -53 * (TWO_PI * float(np.max(np.abs(K))) + float(np.max(np.abs(x))))
    assert np.all(K[:, 0] == 0)
    if kind == 'smooth':
        assert not np.any(K) and np.array_equal(ref.astype(F64), x)
    if kind == 'chirps' and T > 65:
        assert np.max(np.abs(K)) > 3
    # the definition is closer to the exact x - 2 pi K than numpy's accumulated corrections
    exact = x.astype(LD) - K.astype(LD) * LD('6.283185307179586476925286766559')
    assert np.max(np.abs(ref.astype(F64).astype(LD) - exact)) <= np.max(np.abs(want.astype(LD) - exact)) + 1e-18


def test_ref_unwrap_along_other_axes_and_in_f32():
    rng = np.random.default_rng(5)
    x = multi_wrap_rows(rng, 6, 301, F64).reshape(2, 3, 301)
    assert_away_from_ties(x)
    for axis, perm in ((1, (0, 2, 1)), (0, (2, 1, 0))):
        xt = np.ascontiguousarray(np.transpose(x, perm))
        ref, K = ref_unwrap(xt, axis)
        ref2, K2 = ref_unwrap(x, -1)
        assert np.array_equal(np.transpose(ref, perm), ref2) and np.array_equal(np.transpose(K, perm), K2)
    x32 = multi_wrap_rows(rng, 3, 4097, F32)
    assert_away_from_ties(x32)
    ref, K = ref_unwrap(x32)
    assert np.max(np.abs(ref - np.unwrap(x32.astype(F64)))) <= 1e-9             # f32 data: the same integers, in double (bound as above: 2.5e-9)
    assert unwrap_err(ref.astype(F32), x32) <= 1


def test_ref_unwrap_does_not_spread_what_is_not_finite():
    rng = np.random.default_rng(6)
    x = multi_wrap_rows(rng, 2, 200, F64)
    clean = x.copy()
    x[0, 70], x[0, 130], x[1, 50] = np.nan, np.inf, -np.inf
    ref, K = ref_unwrap(x)
    m, _ = wrap_counts(x)
    assert not np.any(m[0, [70, 71, 130, 131]]) and not np.any(m[1, [50, 51]])
    m_clean, _ = wrap_counts(clean)
    keep = np.ones(200, bool)
    keep[[70, 71, 130, 131]] = False
    assert np.array_equal(m[0, keep], m_clean[0, keep])
    assert np.isnan(ref[0, 70]) and np.isinf(ref[0, 130]) and np.all(np.isfinite(ref[0, 131:]))


# ---- the bounds: calibrated on stand-ins of the data's precision, and with teeth ----------------------------------------------------------
def standin_cumsum(x, tile, drop_carry_at=None):
    """a tiled scan with a carry, every sum in the data's dtype; drop_carry_at: that tile starts from zero"""
    out = np.empty_like(x)
    carry = None
    for t, s in enumerate(range(0, x.shape[1], tile)):
        seg = np.cumsum(x[:, s:s + tile], axis=1, dtype=x.dtype)
        if carry is not None and t != drop_carry_at:
            seg = (carry[:, None] + seg).astype(x.dtype)
        out[:, s:s + tile] = seg
        carry = out[:, min(s + tile, x.shape[1]) - 1].copy()
    return out


def standin_unwrap(x, tile, k_off_from=None, drop_carry_at=None, wrong_halo_at=None):
    """the kernels' structure in numpy: m per tile with a one-sample halo, K = carry + the tile's integer scan, out = x - K TWO_PI in
    double rounded once.  k_off_from: K one too large from that sample on; drop_carry_at: that tile starts from K = 0; wrong_halo_at:
    that tile takes its halo from the row before"""
    rows, T = x.shape
    xd = x.astype(np.float64)
    K = np.zeros((rows, T), np.int64)
    carry = np.zeros(rows, np.int64)
    for t, s in enumerate(range(0, T, tile)):
        e = min(s + tile, T)
        if s == 0:
            ext = np.concatenate([xd[:, :1], xd[:, s:e]], axis=1)
        else:
            halo = xd[:, s - 1:s] if t != wrong_halo_at else np.roll(xd, 1, axis=0)[:, s - 1:s]
            ext = np.concatenate([halo, xd[:, s:e]], axis=1)
        m = wrap_counts(ext)[0][:, 1:]
        if t == drop_carry_at:
            carry = np.zeros(rows, np.int64)
        K[:, s:e] = carry[:, None] + np.cumsum(m, axis=1)
        carry = K[:, e - 1].copy()
    if k_off_from is not None:
        K[:, k_off_from:] += 1
    out = (xd - K.astype(np.float64) * TWO_PI).astype(x.dtype)
    return np.where(K == 0, x, out)


def caught(check, out, x):
    try:
        return check(out, x) > 1
    except AssertionError:
        return True


def shifted(out):
    bad = out.copy()
    bad[:, 1:] = out[:, :-1]
    return bad


@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_cumsum_bound_is_calibrated_and_has_teeth(dt):
    """Worst ratio of the stand-in seen here: 0.91 (c64, T = 70001), f32 0.77, f64 0.74, c32 0.91.  The largest ratios sit at small k, where the one rounding of
    x[0] + x[1] can nearly meet the bound of one addition; the bound is rigorous for every order of summation, so it cannot be exceeded
    by a correct scan, and a dropped carry misses it by orders of magnitude."""
    rng = np.random.default_rng([dt.itemsize, 2])
    for T, tile in ((4097, 64), (4097, 1000), (70001, 4096)):
        x = cumsum_rows(rng, 4, T, dt)
        out = standin_cumsum(x, tile)
        r = cumsum_err(out, x)
        print(f'cumsum stand-in {dt} T = {T} tile = {tile}: err / bound = {r:.3g}')
        assert r <= 1
        assert not np.any(out[2])
        n_tiles = -(-T // tile)
        for t in (1, n_tiles // 2, n_tiles - 1):                       # a carry dropped at one tile boundary
            assert caught(cumsum_err, standin_cumsum(x, tile, drop_carry_at=t)[[0, 1, 3]], x[[0, 1, 3]]), (T, tile, t)
        assert caught(cumsum_err, shifted(out), x)                     # a result shifted by one sample
        bad = out.copy()
        bad[2, T // 2] = 1e-30                                         # the zero row must stay exactly zero
        assert caught(cumsum_err, bad, x)
        bad = out.copy()
        bad[0, 0] = np.nextafter(bad[0, 0].real, np.inf)               # element 0 must be a copy
        assert caught(cumsum_err, bad, x)


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('kind', ['chirps', 'multi_wrap'])
def test_unwrap_check_is_calibrated_and_has_teeth(dt, kind):
    """Worst value ratio of the stand-in seen here: 0.999 (f32: the final rounding to f32 is the first term of the bound, and it is met
    almost exactly where a sample falls halfway between two floats) and 0.37 (f64)."""
    rng = np.random.default_rng([dt.itemsize, len(kind), 3])
    gen = {'chirps': wrapped_chirps, 'multi_wrap': multi_wrap_rows}[kind]
    for T, tile in ((4097, 64), (70001, 4096)):
        x = gen(rng, 3, T, dt)
        assert_away_from_ties(x)
        out = standin_unwrap(x, tile)
        r = unwrap_err(out, x)
        print(f'unwrap stand-in {kind} {dt} T = {T} tile = {tile}: err / bound = {r:.3g}')
        assert r <= 1
        n_tiles = -(-T // tile)
        for j in (1, T // 2, T - 1):                                   # one K off by one from some element on
            assert caught(unwrap_err, standin_unwrap(x, tile, k_off_from=j), x), (T, j)
        for t in (n_tiles // 2, n_tiles - 1):                          # a carry dropped at one tile boundary
            assert caught(unwrap_err, standin_unwrap(x, tile, drop_carry_at=t), x), (T, t)
        assert caught(unwrap_err, shifted(out), x)                     # a result shifted by one sample
        if kind == 'multi_wrap':                                       # a halo taken from the wrong row: rows that far apart differ in m
            hit = [caught(unwrap_err, standin_unwrap(x, tile, wrong_halo_at=t), x) for t in range(1, n_tiles)]
            assert all(hit), hit


def test_no_jump_rows_come_back_unchanged():
    rng = np.random.default_rng(4)
    for dt in (F32, F64):
        x = smooth_rows(rng, 3, 4097, dt)
        assert standin_unwrap(x, 64).tobytes() == x.tobytes() and unwrap_err(x, x) == 0
