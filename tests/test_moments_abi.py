"""CPU tests of dsc_sumsq / dsc_rms / dsc_var / dsc_std / dsc_vdot / dsc_detrend (include/dsc_mi355x.h, Section K): the prototypes are
declared, exported, bound and wrapped; a C++ translation unit that names the six wrappers of dsc_api.h compiles and links; the
references of tests/test_gpu_moments.py (class Moments, long double) are numpy.var / std / vdot, the residual of numpy.polyfit and
scipy.signal.detrend; and the bounds are calibrated on numpy stand-ins with the kernels' structure (tiles summed left to right in double,
combined in tile order, one rounding to the dtype) and shown to catch seven mutations.

The definition (every sum in double, one rounding to the result's dtype), n the length of the axis:
    m = (sum x[j]) / n      sumsq = sum |x[j]|^2      rms = sqrt(sumsq / n)      vdot = sum conj(a[j]) b[j]
    var = sum |x[j] - m|^2 / (n - ddof), centred on the computed mean      std = sqrt(var)
    detrend: t[j] = j - (n - 1) / 2, b = sum t[j] x[j] / (n (n^2 - 1) / 12) (0 for 'constant' and n == 1), out[j] = x[j] - m - b t[j],
    per component of complex data

The bounds, ua = 2^-53, uo = the unit of the result's dtype (2^-24 or 2^-53), gamma_k = k ua / (1 - k ua); where a bound is 0 the
output must equal the reference:
    sumsq    |out - ref| <= (gamma_{n+2} + uo) ref
    vdot     real part gamma_{2n+1} sum(|a_r b_r| + |a_i b_i|) + uo |ref|, imaginary part gamma_{2n+1} sum(|a_r b_i| + |a_i b_r|) + uo |ref|;
             real dtypes gamma_{n+1} sum |a b| + uo |ref|
    var      S = sum |x - m|^2, A = sum |x[j]|, e = gamma_n A / n + ua |m|, B_S = gamma_{n+2} S + (1 + gamma_{n+2}) n e^2:
             |out - ref| <= B_S / (n - ddof) + (2 ua + uo) ref
    std, rms sqrt(max(ref_v - B, 0)) (1 - eps) <= out <= sqrt(ref_v + B) (1 + eps), eps = ua + uo: B = var's bound without its uo term
             for std, gamma_{n+2} ref_v for rms (ref_v the variance, the mean square).  Reported as the distance from sqrt(ref_v) over
             the width of the side the output is on.
    detrend  per component |out[j] - ref[j]| <= e + |t[j]| e_b + 3 ua (|x[j]| + |m| + |b t[j]|) + uo |ref[j]|,
             e_b = gamma_{n+3} sum |t[j]| |x[j]| / sum t[j]^2 + 2 ua |b| (0 for 'constant' and n == 1)"""
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
REAL_OF = {F32: F32, F64: F64, C32: F32, C64: F64}
WIDE_OF = {F32: F64, F64: F64, C32: C64, C64: C64}
NAMES = ('dsc_sumsq', 'dsc_rms', 'dsc_var', 'dsc_std', 'dsc_vdot', 'dsc_detrend')
PY_NAMES = ('sumsq', 'rms', 'var', 'std', 'vdot', 'detrend')
LD = np.longdouble
UA = LD(2.0 ** -53)
OFFSETS = (0.0, 3.0, 1e3, 1e6)


def gamma(k):
    return k * UA / (1 - k * UA)


# ---- the references and the checks -----------------------------------------------------------------------------------------------
def components(a):
    a = np.asarray(a)
    return [a.real, a.imag] if np.iscomplexobj(a) else [a]


def ratio(d, bound):
    """largest d / bound (<= 1 passes); where the bound is 0 the output must be the reference"""
    zero = bound == 0
    assert not np.any(d[zero]), 'inexact output where the bound is zero'
    return float(np.max(d[~zero] / bound[~zero])) if not np.all(zero) else 0.0


def root_ratio(out, ref_v, B, eps):
    """out must lie in [sqrt(max(ref_v - B, 0)) (1 - eps), sqrt(ref_v + B) (1 + eps)]: its distance from sqrt(ref_v) over the width of
    its side of the interval (<= 1 passes)"""
    c = np.sqrt(ref_v)
    lo = np.sqrt(np.maximum(ref_v - B, 0)) * (1 - eps)
    hi = np.sqrt(ref_v + B) * (1 + eps)
    out = out.astype(LD)
    d = np.where(out >= c, out - c, c - out)
    return ratio(d, np.where(out >= c, hi - c, c - lo))


class Moments:
    """The long-double references and bounds of x along one axis (the axis is moved to the end; results have x's other axes)."""

    def __init__(self, x, axis=-1):
        self.x = np.asarray(x)
        self.dt = self.x.dtype
        self.axis = axis % self.x.ndim
        self.n = self.x.shape[self.axis]
        self.uo = LD(UNIT[self.dt])
        self._detrend = {}
        assert self.n * 2.0 ** -53 < 0.01
        self.c = [np.moveaxis(c, self.axis, -1).astype(LD) for c in components(self.x)]
        n = LD(self.n)
        self.t = np.arange(self.n, dtype=LD) - (n - 1) / 2
        self.sumsq = sum(np.sum(c * c, axis=-1) for c in self.c)
        self.mean = [np.sum(c, axis=-1) / n for c in self.c]
        self.S = sum(np.sum((c - m[..., None]) ** 2, axis=-1) for c, m in zip(self.c, self.mean))
        self.A = np.sum(np.sqrt(sum(c * c for c in self.c)), axis=-1)
        self.m_abs = np.sqrt(sum(m * m for m in self.mean))
        self.e = gamma(n) * self.A / n + UA * self.m_abs
        self.B_S = gamma(n + 2) * self.S + (1 + gamma(n + 2)) * n * self.e ** 2

    def reduced(self, out):
        """a reduction's output, keepdims or not, as an array over x's other axes"""
        out = np.asarray(out)
        assert out.dtype == REAL_OF[self.dt], (out.dtype, self.dt)
        return out.reshape(self.sumsq.shape)

    def sumsq_err(self, out):
        return ratio(np.abs(self.reduced(out).astype(LD) - self.sumsq), (gamma(LD(self.n) + 2) + self.uo) * self.sumsq)

    def rms_err(self, out):
        ref_v = self.sumsq / self.n
        return root_ratio(self.reduced(out), ref_v, gamma(LD(self.n) + 2) * ref_v, UA + self.uo)

    def var_ref(self, ddof):
        """(reference, bound)"""
        ref = self.S / (self.n - ddof)
        return ref, self.B_S / (self.n - ddof) + (2 * UA + self.uo) * ref

    def var_err(self, out, ddof=0):
        ref, bound = self.var_ref(ddof)
        return ratio(np.abs(self.reduced(out).astype(LD) - ref), bound)

    def std_err(self, out, ddof=0):
        ref_v = self.S / (self.n - ddof)
        return root_ratio(self.reduced(out), ref_v, self.B_S / (self.n - ddof) + 2 * UA * ref_v, UA + self.uo)

    def vdot_ref(self, y):
        """per component of the result: (reference, bound)"""
        b = [np.moveaxis(c, self.axis, -1).astype(LD) for c in components(np.asarray(y))]
        a = self.c
        n = LD(self.n)
        if len(a) == 1:
            ref = np.sum(a[0] * b[0], axis=-1)
            return [(ref, gamma(n + 1) * np.sum(np.abs(a[0] * b[0]), axis=-1) + self.uo * np.abs(ref))]
        re = np.sum(a[0] * b[0] + a[1] * b[1], axis=-1)
        im = np.sum(a[0] * b[1] - a[1] * b[0], axis=-1)
        g = gamma(2 * n + 1)
        return [(re, g * np.sum(np.abs(a[0] * b[0]) + np.abs(a[1] * b[1]), axis=-1) + self.uo * np.abs(re)),
                (im, g * np.sum(np.abs(a[0] * b[1]) + np.abs(a[1] * b[0]), axis=-1) + self.uo * np.abs(im))]

    def vdot_err(self, out, y):
        out = np.asarray(out)
        assert out.dtype == self.dt, (out.dtype, self.dt)
        out = out.reshape(self.sumsq.shape)
        return max(ratio(np.abs(oc.astype(LD) - ref), bound) for oc, (ref, bound) in zip(components(out), self.vdot_ref(y)))

    def detrend_ref(self, kind):
        """per component, the axis last: (reference, bound); kept for the next call"""
        if kind in self._detrend:
            return self._detrend[kind]
        n, t = LD(self.n), self.t
        linear = kind == 'linear' and self.n > 1
        stt = np.sum(t * t)
        res = []
        for c, m in zip(self.c, self.mean):
            b = np.sum(t * c, axis=-1) / stt if linear else np.zeros_like(m)
            e = gamma(n) * np.sum(np.abs(c), axis=-1) / n + UA * np.abs(m)
            e_b = gamma(n + 3) * np.sum(np.abs(t) * np.abs(c), axis=-1) / stt + 2 * UA * np.abs(b) if linear else np.zeros_like(m)
            ref = c - m[..., None] - b[..., None] * t
            bound = (e[..., None] + np.abs(t) * e_b[..., None] + 3 * UA * (np.abs(c) + np.abs(m)[..., None] + np.abs(b[..., None] * t))
                     + self.uo * np.abs(ref))
            res.append((ref, bound))
        self._detrend[kind] = res
        return res

    def detrend_err(self, out, kind):
        out = np.asarray(out)
        assert out.shape == self.x.shape and out.dtype == self.dt, (out.shape, out.dtype, self.x.shape, self.dt)
        return max(ratio(np.abs(np.moveaxis(oc, self.axis, -1).astype(LD) - ref), bound)
                   for oc, (ref, bound) in zip(components(out), self.detrend_ref(kind)))


def reduced_shape(shape, axis, keepdims):
    shape = list(shape)
    if keepdims:
        shape[axis] = 1
    else:
        del shape[axis]
    return tuple(shape)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def moment_rows(rng, rows, T, dt, slopes=False):
    """rows of unit noise: row i on the offset OFFSETS[i % 4] (0, 3, 1e3, 1e6); with six rows or more row 4 is all zero and row 5
    constant (2.75); slopes: row i gains the ramp (i % 3 - 1) 0.01 j"""
    dt = np.dtype(dt)
    x = rng.standard_normal((rows, T))
    if dt.kind == 'c':
        x = x + 1j * rng.standard_normal((rows, T))
    x += np.array([OFFSETS[i % 4] for i in range(rows)])[:, None] * (1 - 0.5j if dt.kind == 'c' else 1)
    if slopes:
        x += (np.arange(rows)[:, None] % 3 - 1) * 0.01 * np.arange(T)[None, :] * (1 + 2j if dt.kind == 'c' else 1)
    if rows >= 6:
        x[4] = 0
        x[5] = 2.75
    return np.ascontiguousarray(x.astype(dt))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared_exported_bound_and_wrapped():
    text = open(HEADER).read()
    assert 'Section K' in text
    for route in ('moment_rows', 'moment_tiles', 'moment_cols', 'detrend_rows', 'detrend_tiles', 'detrend_cols', 'DSC_MOMENT_ROUTE'):
        assert route in text, route
    assert re.search(r'typedef enum \{ DSC_DETREND_CONSTANT = 0, DSC_DETREND_LINEAR = 1 \} dsc_detrend_type;', text)
    tail = {'dsc_sumsq': r'const dsc_tensor \*x, dsc_tensor \*out, int axis, bool keep_dims',
            'dsc_rms': r'const dsc_tensor \*x, dsc_tensor \*out, int axis, bool keep_dims',
            'dsc_var': r'const dsc_tensor \*x, dsc_tensor \*out, int axis, int ddof, bool keep_dims',
            'dsc_std': r'const dsc_tensor \*x, dsc_tensor \*out, int axis, int ddof, bool keep_dims',
            'dsc_vdot': r'const dsc_tensor \*a, const dsc_tensor \*b, dsc_tensor \*out, int axis, bool keep_dims',
            'dsc_detrend': r'const dsc_tensor \*x, dsc_tensor \*out, int axis, dsc_detrend_type type'}
    lib = ctypes.CDLL(LIB)
    from dsc_amd import _bindings as B
    T, I, Bo = B._DscTensor_p, ctypes.c_int, ctypes.c_bool
    argtypes = {'dsc_sumsq': [T, T, I, Bo], 'dsc_rms': [T, T, I, Bo], 'dsc_var': [T, T, I, I, Bo], 'dsc_std': [T, T, I, I, Bo],
                'dsc_vdot': [T, T, T, I, Bo], 'dsc_detrend': [T, T, I, I]}
    for name in NAMES:
        assert re.search(r'dsc_tensor \*%s *\(dsc_ctx \*ctx, %s\);' % (name, tail[name]), text), name
        assert hasattr(lib, name), name
        assert name in B.EXPORTS
        f = getattr(B, name)
        assert f.argtypes == [B._DscCtx] + argtypes[name], name
        assert f.restype is B._DscTensor_p
    import dsc_amd
    for name in PY_NAMES:
        assert callable(getattr(dsc_amd, name)) and name in dsc_amd.__all__, name
    import inspect
    for name in ('sumsq', 'rms'):
        p = inspect.signature(getattr(dsc_amd, name)).parameters
        assert list(p) == ['x', 'out', 'axis', 'keepdims'] and p['out'].default is None and p['axis'].default == -1 and p['keepdims'].default is True
    for name in ('var', 'std'):
        p = inspect.signature(getattr(dsc_amd, name)).parameters
        assert list(p) == ['x', 'out', 'axis', 'ddof', 'keepdims'] and p['ddof'].default == 0 and p['axis'].default == -1 and p['keepdims'].default is True
    p = inspect.signature(dsc_amd.vdot).parameters
    assert list(p) == ['a', 'b', 'out', 'axis', 'keepdims'] and p['axis'].default == -1 and p['keepdims'].default is True
    p = inspect.signature(dsc_amd.detrend).parameters
    assert list(p) == ['x', 'axis', 'type', 'out'] and p['type'].default == 'linear' and p['axis'].default == -1


def test_cpp_wrappers_and_documents():
    api = open(os.path.join(ROOT, 'dsc_amd', 'api', 'dsc_api.h')).read()
    for name in ('sumsq', 'rms'):
        assert re.search(r'tensor<T> %s\(const tensor<T> &x, int axis = -1, bool keep_dims = true\)' % name, api), name
    for name in ('var', 'std'):
        assert re.search(r'tensor<T> %s\(const tensor<T> &x, int axis = -1, int ddof = 0, bool keep_dims = true\)' % name, api), name
    assert re.search(r'tensor<T> vdot\(const tensor<T> &a, const tensor<T> &b, int axis = -1, bool keep_dims = true\)', api)
    assert re.search(r'tensor<T> detrend\(const tensor<T> &x, int axis = -1, dsc_detrend_type type = DSC_DETREND_LINEAR\)', api)
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in PY_NAMES:
            assert re.search(r'\b%s\b' % name, text), (doc, name)
    assert '4.12' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'bench_moments.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()


def test_cpp_moments_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_moments_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout


# ---- the references are numpy's ------------------------------------------------------------------------------------------------------
SHAPES = (((6, 1000), -1), ((2, 65, 5), 1), ((65, 7), 0), ((2, 3, 4, 5), 2))


def lay(rows, shape, axis):
    """rows [lead, n] -> the shape, the axis in place"""
    axis %= len(shape)
    return np.ascontiguousarray(np.moveaxis(rows.reshape([s for i, s in enumerate(shape) if i != axis] + [shape[axis]]), -1, axis))


@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_references_are_numpy(dt):
    """against numpy in double; the tolerance is numpy's own error: pairwise sums of n terms in double, a few hundred ua of the sum of
    magnitudes (1e-13 of it here), and for var the cancellation of its mean, n (ua offset)^2"""
    rng = np.random.default_rng([dt.itemsize, 1])
    wide = WIDE_OF[dt]
    for shape, axis in SHAPES:
        n = shape[axis]
        x = lay(moment_rows(rng, int(np.prod(shape)) // n, n, dt, slopes=True), shape, axis)
        y = lay(moment_rows(rng, int(np.prod(shape)) // n, n, dt), shape, axis)
        M = Moments(x, axis)
        xw, yw = x.astype(wide), y.astype(wide)
        mag2 = np.sum(np.abs(xw) ** 2, axis=axis)
        assert np.all(np.abs(M.sumsq - mag2) <= 1e-13 * mag2)
        for ddof in (0, 1):
            ref, _ = M.var_ref(ddof)
            want = np.var(xw, axis=axis, ddof=ddof)
            big = np.max(np.abs(xw), axis=axis)                         # numpy's x - mean rounds at 2^-53 max|x| per element
            assert np.all(np.abs(ref - want) <= 1e-12 * want + 1e-15 * big * np.sqrt(want)), (shape, ddof)
            assert np.all(np.abs(np.sqrt(ref) - np.std(xw, axis=axis, ddof=ddof)) <= 1e-12 * np.sqrt(want) + 1e-15 * big), (shape, ddof)
        parts = M.vdot_ref(y)
        want = np.sum(np.conj(xw) * yw, axis=axis)
        if axis in (-1, len(shape) - 1):
            flat_x, flat_y = xw.reshape(-1, n), yw.reshape(-1, n)
            by_vdot = np.array([np.vdot(a, b) for a, b in zip(flat_x, flat_y)]).reshape(want.shape)
            assert np.all(np.abs(by_vdot - want) <= 1e-12 * np.sum(np.abs(xw * yw), axis=axis))
        scale = np.sum(np.abs(xw * yw), axis=axis)
        for (ref, _), wc in zip(parts, components(want)):
            assert np.all(np.abs(ref - wc) <= 1e-13 * scale)
        t = np.arange(n, dtype=np.float64)
        for kind in ('constant', 'linear'):
            for (ref, _), xc in zip(M.detrend_ref(kind), components(np.moveaxis(xw, axis, -1))):
                flat = xc.reshape(-1, n)
                for row, r in zip(flat, ref.reshape(-1, n)):
                    fit = np.polyval(np.polyfit(t - (n - 1) / 2, row, 1 if kind == 'linear' else 0), t - (n - 1) / 2)
                    assert np.max(np.abs(r - (row - fit))) <= 1e-9 * max(np.max(np.abs(row)), 1.0), (shape, kind)


@pytest.mark.parametrize('kind', ['constant', 'linear'])
def test_detrend_reference_is_scipy(kind):
    signal = pytest.importorskip('scipy.signal')
    rng = np.random.default_rng([len(kind), 2])
    for shape, axis in SHAPES + (((3, 1), -1), ((3, 2), -1)):
        n = shape[axis]
        for dt in (F64, C64):
            x = lay(moment_rows(rng, int(np.prod(shape)) // n, n, dt, slopes=True), shape, axis)
            want = signal.detrend(x, axis=axis, type=kind)
            got = Moments(x, axis).detrend_ref(kind)
            for (ref, _), wc in zip(got, components(np.moveaxis(want, axis, -1))):
                assert np.max(np.abs(ref - wc)) <= 1e-9 * max(float(np.max(np.abs(x))), 1.0), (shape, dt, kind)


# ---- the bounds: calibrated on stand-ins of the kernels' structure, and with teeth -----------------------------------------------------
def ordered_sum(v, tile, drop=None):
    """tiles of v [rows, n] (double) summed left to right, the tile sums left to right; drop: that tile's sum is left out"""
    parts = [np.cumsum(v[:, s:s + tile], axis=1)[:, -1] for s in range(0, v.shape[1], tile)]
    if drop is not None and len(parts) > 1:
        parts[drop % len(parts)] = np.zeros_like(parts[0])
    return np.cumsum(np.stack(parts, axis=1), axis=1)[:, -1]


def standin(op, x, tile, y=None, ddof=0, kind='linear', mutate=None):
    """the kernels' arithmetic in numpy on x [rows, n]: double sums per tile, ordered combine, one rounding.  mutate: 'one_pass' (var as
    sum |x|^2 - n |m|^2), 'mean_f32' (the mean rounded to f32 before the subtraction), 'drop_tile' (tile 1's sums lost), 'neighbour'
    (the statistic of the row before), 'no_ddof', 't_half' (t centred at n / 2), 'shift' (the result one element on)"""
    rows, n = x.shape
    rdt = REAL_OF[x.dtype]
    xw = x.astype(WIDE_OF[x.dtype])
    drop = 1 if mutate == 'drop_tile' else None
    cs = components(xw)
    if op in ('sumsq', 'rms'):
        s = ordered_sum(sum(c * c for c in cs), tile, drop)
        out = (np.sqrt(s / n) if op == 'rms' else s).astype(rdt)
    elif op == 'vdot':
        yw = y.astype(WIDE_OF[x.dtype])
        prod = np.conj(xw) * yw
        parts = [ordered_sum(c, tile, drop) for c in components(prod)]
        out = (parts[0] + 1j * parts[1] if len(parts) == 2 else parts[0]).astype(x.dtype)
    else:
        m = [ordered_sum(c, tile, drop if op == 'detrend' else None) / n for c in cs]
        if mutate == 'mean_f32':
            m = [mc.astype(np.float32).astype(np.float64) for mc in m]
        if mutate == 'neighbour':
            m = [np.roll(mc, 1) for mc in m]
        if op in ('var', 'std'):
            if mutate == 'one_pass':
                S = ordered_sum(sum(c * c for c in cs), tile) - n * sum(mc * mc for mc in m)
            else:
                S = ordered_sum(sum((c - mc[:, None]) ** 2 for c, mc in zip(cs, m)), tile, drop)
            v = S / (n if mutate == 'no_ddof' else n - ddof)
            out = (np.sqrt(np.maximum(v, 0)) if op == 'std' else v).astype(rdt)
        else:
            t = np.arange(n, dtype=np.float64) - ((n / 2) if mutate == 't_half' else (n - 1) / 2)
            d = n * (float(n) * n - 1.0) / 12.0
            res = []
            for c, mc in zip(cs, m):
                b = ordered_sum(t * c, tile) / d if kind == 'linear' and n > 1 else np.zeros(rows)
                if mutate == 'neighbour':
                    b = np.roll(b, 1)
                res.append((c - mc[:, None]) - b[:, None] * t)
            out = (res[0] + 1j * res[1] if len(res) == 2 else res[0]).astype(x.dtype)
    if mutate == 'shift':
        out = np.roll(out, 1, axis=-1 if op == 'detrend' else 0)
    return out


def err_of(M, op, out, y=None, ddof=0, kind='linear'):
    if op == 'vdot':
        return M.vdot_err(out, y)
    if op == 'detrend':
        return M.detrend_err(out, kind)
    if op in ('var', 'std'):
        return getattr(M, op + '_err')(out, ddof)
    return getattr(M, op + '_err')(out)


def caught(M, op, out, **kw):
    try:
        return err_of(M, op, out, **kw) > 1
    except AssertionError:
        return True


CALIBRATION = ((65, 16), (4097, 1000), (70001, 8192))


@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_bounds_are_calibrated(dt):
    """Worst err / bound of the stand-in seen here, rows on the offsets 0, 3, 1e3, 1e6, a zero and a constant row, n up to 70001:
        f32   sumsq 0.77   rms 0.56   vdot 0.75    var 0.90   std 0.87   detrend 0.997
        c32   sumsq 0.93   rms 0.73   vdot 0.80    var 0.73   std 0.53   detrend 0.9992
        f64   sumsq 0.015  rms 0.019  vdot 0.009   var 0.019  std 0.018  detrend 0.027
        c64   sumsq 0.011  rms 0.036  vdot 0.005   var 0.025  std 0.026  detrend 0.026
    In f32 / c32 the final rounding to the dtype is the bound's first term, so the ratios near 1 are roundings that fall halfway; in
    double the gamma terms allow n roundings in a row where a tiled sum makes n / tile + tile of them."""
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 3])
    worst = {}
    for n, tile in CALIBRATION:
        x, y = moment_rows(rng, 6, n, dt, slopes=True), moment_rows(rng, 6, n, dt)
        M = Moments(x)
        for op, kw in (('sumsq', {}), ('rms', {}), ('vdot', {'y': y}), ('var', {'ddof': 0}), ('var', {'ddof': 1}), ('std', {'ddof': 1}),
                       ('detrend', {'kind': 'constant'}), ('detrend', {'kind': 'linear'})):
            out = standin(op, x, tile, **kw)
            r = err_of(M, op, out, **kw)
            worst[op] = max(worst.get(op, 0.0), r)
            assert r <= 1, (op, kw, n, r)
            if op != 'detrend':
                assert not np.any(out[4]) or op == 'vdot', 'the zero row'
            if op in ('var', 'std'):
                assert out[5] == 0, 'the constant row has no variance'
    print(f'stand-in worst err / bound {dt}: ' + '  '.join(f'{k} {v:.4g}' for k, v in worst.items()))


@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_checks_have_teeth(dt):
    """Each mutation must be caught on the rows where it changes the result by more than the result's rounding:
        one_pass   var / std: at the offsets 1e3 and 1e6 in f64 / c64 (cancellation ua offset^2 against a variance of 1), at 1e6 in f32 / c32
        mean_f32   detrend at the offsets 1e3 and 1e6 (the f32 mean is off by up to 3e-5 / 0.03); var / std where n delta^2 shows: at
                   1e6, and at 1e3 in f64 / c64
        drop_tile, neighbour, shift   every operator they apply to, every row with data that differs from its neighbour's
        no_ddof    var / std with ddof = 1        t_half   linear detrend of the rows with a slope"""
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 4])
    wide = dt in (F64, C64)
    for n, tile in CALIBRATION:
        sloped, y = moment_rows(rng, 6, n, dt, slopes=True), moment_rows(rng, 6, n, dt)
        level = moment_rows(rng, 6, n, dt)                             # var / std: a slope would be variance, and hide the offsets' cancellation

        def hit(op, mutate, rows, **kw):
            x = sloped if op == 'detrend' else level
            out = standin(op, x, tile, mutate=mutate, **kw)
            sel = list(rows)
            Ms = Moments(x[sel])
            kw2 = dict(kw)
            if 'y' in kw2:
                kw2['y'] = y[sel]
            assert caught(Ms, op, out[sel], **kw2), (dt, n, op, mutate, rows)

        for op in ('var', 'std'):
            for row in ((2, 3) if wide else (3,)):
                hit(op, 'one_pass', [row], ddof=0)
                hit(op, 'mean_f32', [row], ddof=0)
            hit(op, 'no_ddof', [0, 1, 2, 3], ddof=1)
            for row in (0, 1, 2, 3):
                hit(op, 'drop_tile', [row], ddof=0)
                hit(op, 'neighbour', [row], ddof=0)
        for kind in ('constant', 'linear'):
            for row in (2, 3):
                hit('detrend', 'mean_f32', [row], kind=kind)
            for row in (0, 1, 2, 3):
                hit('detrend', 'drop_tile', [row], kind=kind)
                hit('detrend', 'neighbour', [row], kind=kind)
                hit('detrend', 'shift', [row], kind=kind)
        for row in (0, 2, 3):                                          # the rows with a slope of -0.01 or 0.01 per sample
            hit('detrend', 't_half', [row], kind='linear')
        for op, kw in (('sumsq', {}), ('rms', {}), ('vdot', {'y': y})):
            for row in (0, 1, 2, 3):
                hit(op, 'drop_tile', [row], **kw)
            hit(op, 'shift', [0, 1, 2, 3], **kw)
        for op in ('var', 'std'):
            hit(op, 'shift', [0, 1, 2, 3, 4], ddof=0)                    # the zero row takes row 3's variance
