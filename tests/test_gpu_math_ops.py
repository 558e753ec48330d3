"""GPU tests of the math, creation and shape operators (cos .. sqrt, pow, clip, i0, arange, randn, reshape, concat) through the
Python package: every case of tests/golden/math.npz (outputs of the reference itself), the f32 saturation of arange, the scalar
tail and unaligned paths next to the packed kernels, 2^26-element runs against numpy in f64, out= / view semantics, the
counterparts of the reference's python/tests/test_ops.py cases, and a windowed-sinc FIR designed and applied on the device."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN, assert_ends_the_process, build_cpp_smoke, dsc, rel_l2, sync_fixture  # noqa: F401

pytestmark = pytest.mark.gpu

UNARY = ('cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt')
NP_UNARY = {'cos': np.cos, 'sin': np.sin, 'sinc': np.sinc, 'logn': np.log, 'log2': np.log2, 'log10': np.log10, 'exp': np.exp, 'sqrt': np.sqrt}
_sync = sync_fixture()


def assert_matches(got, want, rel, floor, what=''):
    """Element-wise |got - want| <= rel |want| + floor (complex: moduli); NaN and +-inf in the same places, component by component."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}'
    parts = (lambda a: (a.real, a.imag)) if np.iscomplexobj(want) else (lambda a: (a,))
    finite = np.ones(want.shape, bool)
    for g, w in zip(parts(got), parts(want)):
        bad = np.isnan(g) != np.isnan(w)
        assert not bad.any(), f'{what}: NaN positions differ at {np.flatnonzero(bad)[:8]}'
        inf = np.isinf(w)
        assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], w[inf]), f'{what}: inf positions differ'
        finite &= np.isfinite(w)
    d = np.abs(got[finite].astype(np.complex128 if np.iscomplexobj(want) else np.float64) - want[finite])
    lim = rel * np.abs(want[finite]).astype(np.float64) + floor
    worst = int(np.argmax(d - lim)) if d.size else 0
    assert d.size == 0 or (d <= lim).all(), f'{what}: |a-b| = {d[worst]:.3e} > {lim[worst]:.3e} at {worst} (want {want[finite][worst]}, got {got[finite][worst]})'


def tolerance(op, dtype):
    single = np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64))
    if op == 'pow' and np.iscomplexobj(np.zeros(1, dtype)):
        return (1e-5, 1e-30) if single else (1e-12, 1e-300)
    return (4e-6, 1e-30) if single else (1e-13, 1e-300)


def run_case(dsc, rec, xs):
    op = rec['op']
    t = [dsc.from_numpy(x) for x in xs]
    if op in UNARY:
        return getattr(dsc, op)(t[0])
    if op == 'pow':
        return dsc.power(t[0], t[1])
    if op == 'i0':
        return dsc.i0(t[0])
    if op == 'clip':
        return dsc.clip(t[0], rec['lo'], rec['hi'])
    if op == 'arange':
        return dsc.arange(rec['n'], dsc.Dtype[rec['dtype'].upper()])
    if op == 'randn':
        return dsc.randn(*rec['shape'], dtype=dsc.Dtype[rec['dtype'].upper()])
    if op == 'reshape':
        return t[0].reshape(*rec['dims'])
    if op == 'concat':
        return dsc.concat(t, axis=rec['axis'])
    raise ValueError(op)


EXACT = ('clip', 'arange', 'randn', 'reshape', 'concat')


def _generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_math', os.path.join(GOLDEN, 'make_golden_math.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()                         # inputs of the fixtures: seeded draws rebuilt from the manifest (make_golden_math.inputs)


@pytest.mark.parametrize('op', UNARY + ('pow', 'clip', 'i0') + ('arange', 'randn', 'reshape', 'concat'))
def test_golden_math(dsc, op):
    recs = [r for r in json.load(open(os.path.join(GOLDEN, 'math_manifest.json'))) if r['op'] == op]
    assert recs
    with np.load(os.path.join(GOLDEN, 'math.npz')) as z:
        for rec in recs:
            key = rec['key']
            xs = GEN.inputs(rec, z)
            want = z[f'{key}_y']
            got = run_case(dsc, rec, xs).numpy()
            if op in EXACT:
                assert got.shape == want.shape and got.dtype == want.dtype, key
                assert got.tobytes() == want.tobytes(), f'{key}: not bit-exact ({np.sum(got != want)} elements differ)'
            else:
                assert_matches(got, want, *tolerance(op, want.dtype), what=key)


def test_arange_f32_saturates_at_2_pow_24(dsc):
    n = (1 << 24) + 3
    got = dsc.arange(n, dsc.Dtype.F32).numpy()
    want = np.minimum(np.arange(n, dtype=np.int64), 1 << 24).astype(np.float32)
    assert np.array_equal(got, want)
    c = dsc.arange(n, dsc.Dtype.C32).numpy()
    assert np.array_equal(c.real, want) and not c.imag.any()
    assert np.array_equal(dsc.arange(n, dsc.Dtype.F64).numpy(), np.arange(n, dtype=np.float64))


# ---- odd counts and unaligned views: the scalar tail and the unpacked paths next to the packed kernels

class _Offset:
    """A dsc_tensor_from_device_ptr view whose data starts `offset` bytes into a buffer of the caller's own.  The entry point
    takes 8-byte aligned pointers only (peer.cpp): 8 bytes off a 256-byte aligned allocation is the most unaligned view there is,
    and it misses the 16-byte alignment of every packed kernel."""

    def __init__(self, dsc, x, offset):
        from dsc_amd import _bindings as B
        from dsc_amd.context import _get_ctx
        from dsc_amd.dtype import NP_TO_DTYPE
        self.B, self.ctx = B, _get_ctx()
        self.raw = B.dsc_device_alloc(self.ctx, x.nbytes + 256)
        assert self.raw
        shape = (ctypes.c_int * x.ndim)(*x.shape)
        self.t = dsc.Tensor(B.dsc_tensor_from_device_ptr(self.ctx, self.raw + offset, x.nbytes, x.ndim, shape, NP_TO_DTYPE[x.dtype].value))
        B.dsc_copy_from_host(self.ctx, self.t._c_ptr, x.ctypes.data, x.nbytes)

    def close(self, dsc):
        del self.t
        dsc.synchronize()
        self.B.dsc_device_free(self.ctx, self.raw)


@pytest.mark.parametrize('dtype,offset', [(np.float32, 8), (np.float64, 8), (np.complex64, 8), (np.float32, 24)])
def test_unaligned_and_odd_lengths(dsc, dtype, offset):
    rng = np.random.default_rng(7)
    for n in (1, 3, 1001, 4099):
        x = (rng.uniform(0.1, 4, n) + (1j * rng.uniform(-2, 2, n) if np.dtype(dtype).kind == 'c' else 0)).astype(dtype)
        view = _Offset(dsc, x, offset)
        try:
            aligned = dsc.from_numpy(x)
            rel, floor = tolerance('exp', dtype)
            for op in UNARY:
                want = getattr(dsc, op)(aligned).numpy()
                assert_matches(getattr(dsc, op)(view.t).numpy(), want, rel, floor, what=f'{op} n={n} +{offset}B')
            e = dsc.from_numpy(np.full(n, 1.5, dtype))
            assert_matches(dsc.power(view.t, e).numpy(), dsc.power(aligned, e).numpy(), *tolerance('pow', dtype), what=f'pow n={n}')
            assert_matches(dsc.power(view.t, 0.5).numpy(), dsc.power(aligned, 0.5).numpy(), *tolerance('pow', dtype), what=f'pow scalar n={n}')
            got = dsc.clip(view.t, 0.5, 2.0).numpy()
            assert got.tobytes() == dsc.clip(aligned, 0.5, 2.0).numpy().tobytes()
            if np.dtype(dtype).kind == 'f':
                assert_matches(dsc.i0(view.t).numpy(), dsc.i0(aligned).numpy(), rel, floor, what=f'i0 n={n}')
            r = view.t.reshape(1, n)
            assert r.shape == (1, n) and np.array_equal(r.numpy()[0], x)
            del r
        finally:
            view.close(dsc)


# ---- at scale: 2^26 elements per op family, f32 and c64, against numpy in f64

def _big_input(op, dtype, n, rng):
    lo, hi = {'logn': (1e-3, 1e3), 'log2': (1e-3, 1e3), 'log10': (1e-3, 1e3), 'sqrt': (0, 1e3), 'exp': (-20, 20), 'sinc': (-10, 10)}.get(op, (-100, 100))
    x = rng.uniform(lo, hi, n)
    if np.dtype(dtype).kind == 'c':
        # |im| >= 0.5: the reference's complex sqrt, sqrt(0.5 (|z| + re)), cancels near the negative real axis where numpy's does not
        x = x + 1j * rng.uniform(0.5, 3, n) * rng.choice([-1.0, 1.0], n)
    return x.astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.complex128])
def test_large_unary_against_numpy(dsc, dtype):
    n = 1 << 26
    rng = np.random.default_rng(26)
    rel = 2e-6 if dtype == np.float32 else 1e-12
    for op in UNARY:
        x = _big_input(op, dtype, n, rng)
        got = getattr(dsc, op)(dsc.from_numpy(x)).numpy()
        want = NP_UNARY[op](x.astype(np.complex128 if np.iscomplexobj(x) else np.float64))
        # f32: the output's own rounding (0.5 ulp) on top of the ~2 ulp of the function; relative to the result's size
        d = np.abs(got - want)
        assert (d <= rel * np.abs(want) + (1e-6 if op == 'sin' or op == 'cos' or op == 'sinc' else 0) * (dtype == np.float32)).all(), \
            f'{op} {np.dtype(dtype)}: worst {np.max(d / (np.abs(want) + 1e-300)):.3e}'
        del x, got, want


@pytest.mark.parametrize('dtype', [np.float32, np.complex128])
def test_large_pow_clip_i0_arange(dsc, dtype):
    n = 1 << 26
    rng = np.random.default_rng(27)
    if np.dtype(dtype).kind == 'c':
        a = (rng.uniform(0.1, 2, n) * np.exp(1j * rng.uniform(-3, 3, n))).astype(dtype)
        b = (rng.uniform(-2, 2, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    else:
        a, b = rng.uniform(0.1, 3, n).astype(dtype), rng.uniform(-3, 3, n).astype(dtype)
    ta, tb = dsc.from_numpy(a), dsc.from_numpy(b)
    wide = np.complex128 if np.iscomplexobj(a) else np.float64
    want = np.power(a.astype(wide), b.astype(wide))
    got = (ta ** tb).numpy()
    assert np.all(np.abs(got - want) <= (1e-5 if dtype == np.float32 else 1e-12) * np.abs(want)), 'pow'
    row = dsc.from_numpy(b[:4096].copy())
    got = dsc.power(ta.reshape(-1, 4096), row).numpy().reshape(-1)
    want = np.power(a.astype(wide).reshape(-1, 4096), b[:4096].astype(wide)).reshape(-1)
    assert np.all(np.abs(got - want) <= (1e-5 if dtype == np.float32 else 1e-12) * np.abs(want)), 'pow broadcast row'
    got = dsc.clip(ta, 0.5, 2.0).numpy()
    if np.iscomplexobj(a):
        want = np.where(a.real > 0.5, a, 0.5 + 0j)
        want = np.where(want.real > 2.0, 2.0 + 0j, want).astype(dtype)
    else:
        want = np.minimum(np.maximum(a, dtype(0.5)), dtype(2.0))
    assert got.tobytes() == want.tobytes(), 'clip'
    del ta, tb, got, want
    if np.dtype(dtype).kind == 'f':
        x = rng.uniform(-30, 30, n).astype(dtype)
        got = dsc.i0(dsc.from_numpy(x)).numpy()
        assert np.all(np.abs(got - np.i0(x.astype(np.float64))) <= 2e-6 * np.i0(x.astype(np.float64))), 'i0 (A&S: 1.9e-7 + f32 evaluation)'
        got = dsc.arange(n, dsc.Dtype.F32).numpy()
        assert np.array_equal(got, np.minimum(np.arange(n), 1 << 24).astype(np.float32)), 'arange'
    else:
        got = dsc.arange(n, dsc.Dtype.C64).numpy()
        assert np.array_equal(got, np.arange(n).astype(np.complex128)), 'arange'


# ---- out=, views, lifetimes

def _data_ptr(t):
    return t._c_ptr.contents.data


def test_out_writes_into_out_and_returns_a_view(dsc):
    x = dsc.from_numpy(np.linspace(0.1, 3, 1000).astype(np.float32))
    for op in UNARY:
        out = dsc.empty(1000, dsc.Dtype.F32)
        y = getattr(dsc, op)(x, out=out)
        assert _data_ptr(y) == _data_ptr(out) and y._c_ptr is not out._c_ptr
        assert np.array_equal(out.numpy(), getattr(dsc, op)(x).numpy()), op
    out = dsc.empty(1000, dsc.Dtype.F32)
    y = dsc.clip(x, 0.5, 1.5, out=out)
    assert _data_ptr(y) == _data_ptr(out) and out.numpy().max() == np.float32(1.5)
    out = dsc.empty(1000, dsc.Dtype.F32)
    y = dsc.power(x, 2.0, out=out)
    assert _data_ptr(y) == _data_ptr(out)
    assert np.allclose(out.numpy(), np.linspace(0.1, 3, 1000).astype(np.float32) ** 2, rtol=1e-6)
    del y
    assert out.numpy().shape == (1000,)


def test_reshape_shares_the_buffer_and_frees_in_either_order(dsc):
    base = np.arange(120, dtype=np.float64).reshape(10, 12)
    for first in ('view', 'base'):
        x = dsc.from_numpy(base)
        v = x.reshape(3, -1, 5)
        w = dsc.reshape(x, [120])
        assert v.shape == (3, 8, 5) and w.shape == (120,)
        assert _data_ptr(v) == _data_ptr(x) == _data_ptr(w)
        used = dsc.used_mem()
        if first == 'view':
            del v, w
            dsc.synchronize()
            assert np.array_equal(x.numpy(), base)
        else:
            del x
            dsc.synchronize()
            assert dsc.used_mem() == used                    # the buffer lives while a view references it
            assert np.array_equal(v.numpy(), base.reshape(3, 8, 5)) and np.array_equal(w.numpy(), base.reshape(-1))
            x2 = dsc.from_numpy(np.zeros(120))
            assert np.array_equal(v.numpy(), base.reshape(3, 8, 5))   # not overwritten by a new allocation
            del x2
        v2 = dsc.reshape(x if first == 'view' else v, (2, 60))
        assert v2.shape == (2, 60) and np.array_equal(v2.numpy(), base.reshape(2, 60))


def test_reductions_into_out_and_along_a_padding_axis(dsc):
    """sum and max of f32 (2, 64) into a caller's out, the axis kept and dropped; the same along axis -3, which for a tensor of two
    dimensions is a leading padding slot of extent 1 that the reductions accept, as the reference does: the result is x.  A
    wrong-shaped out ends a child process with status 1.

    Not run: axis -3 with the axis dropped.  The reference's shape rule then writes a fifth slot of its four-slot shape and asks for an
    out of 2 elements that the 128 outputs of the launch would overrun; reduce.cpp refuses the call."""
    x = _random((2, 64), np.float32, np.random.default_rng(23))
    X = dsc.from_numpy(x)
    for keep in (True, False):
        shape = (2, 1) if keep else (2,)
        out = dsc.empty(shape, dsc.Dtype.F32)
        y = dsc.sum(X, out=out, axis=-1, keepdims=keep)
        assert _data_ptr(y) == _data_ptr(out) and y.shape == shape
        assert_matches(out.numpy(), x.astype(np.float64).sum(-1, keepdims=keep).astype(np.float32), *tolerance('sum', np.float32), what=f'sum keepdims={keep}')
        out = dsc.empty(shape, dsc.Dtype.F32)
        y = dsc.max(X, out=out, axis=-1, keepdims=keep)
        assert _data_ptr(y) == _data_ptr(out) and np.array_equal(out.numpy(), x.max(-1, keepdims=keep))
    for f in (dsc.sum, dsc.max):
        out = dsc.empty((2, 64), dsc.Dtype.F32)
        y = f(X, out=out, axis=-3, keepdims=True)
        assert _data_ptr(y) == _data_ptr(out) and np.array_equal(out.numpy(), x), f.__name__
        assert np.array_equal(f(X, axis=-3, keepdims=True).numpy(), x), f.__name__
    assert_ends_the_process("dsc.sum(dsc.from_numpy(np.ones((2, 64), np.float32)), out=dsc.empty((2, 2), dsc.Dtype.F32), axis=-1)", 'shape')


# ---- counterparts of the reference's python/tests/test_ops.py (test_binary 'power', test_unary, test_clip, test_arange,
# test_random, test_reshape, test_concat), against numpy as there

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)


def _random(shape, dtype, rng, lo=0.1, hi=2.0):
    x = rng.uniform(lo, hi, shape)
    if np.dtype(dtype).kind == 'c':
        x = x + 1j * rng.uniform(lo, hi, shape)
    return x.astype(dtype)


def _close(a, b):
    return np.allclose(a, b, rtol=1e-4 if a.dtype in (np.float32, np.complex64) else 1e-9, atol=1e-6, equal_nan=True)


def test_ref_ops_power(dsc):
    rng = np.random.default_rng(11)
    for dtype in DTYPES:
        shape = [int(v) for v in rng.integers(2, 10, 4)]
        x, y = _random(shape, dtype, rng), _random(shape, dtype, rng)
        xd, yd = dsc.from_numpy(x), dsc.from_numpy(y)
        assert _close(dsc.power(xd, yd).numpy(), np.power(x, y)) and _close((yd ** xd).numpy(), y ** x)
        shape[int(rng.integers(0, 4))] = 1
        yb = _random(shape, dtype, rng)
        ybd = dsc.from_numpy(yb)
        assert _close(dsc.power(xd, ybd).numpy(), np.power(x, yb)) and _close((ybd ** xd).numpy(), yb ** x)
        s = complex(rng.random(), rng.random()) if np.dtype(dtype).kind == 'c' else float(rng.random())
        assert _close(dsc.power(xd, s).numpy(), np.power(x, s).astype(dtype)) and _close((s ** xd).numpy(), (s ** x).astype(dtype))


# ---- pow on every route of the binary launcher (the route tests of the other files run add, sub, mul and div)

# (shape of a, shape of b): one pair per branch of dsc_launch_binary; unequal pairs run in both operand orders
BINARY_ROUTES = (
    ((6, 1000), (6, 1000)),              # equal shapes, 16 bytes per lane
    ((5, 1001), (5, 1001)),              # equal shapes, odd count: one element per thread
    ((8, 512), (512,)),                  # trailing operand, packed
    ((3, 5), (5,)),                      # trailing operand, one element per thread
    ((4, 1024), (1,)),                   # scalar, packed
    ((3, 5), (1,)),                      # scalar, general kernel
    ((12, 512), (12, 1)),                # leading (column) operand, packed
    ((9, 2), (9, 1)),                    # a column too short for a pack
    ((4, 3, 8, 64), (4, 1, 8, 1)),       # general broadcast, packed
    ((4, 3, 8, 65), (4, 1, 8, 1)),       # general broadcast, one block per piece of a row
    ((2, 3, 4, 6), (3, 1, 6)),           # general broadcast, flat
)
# the other operand of the two mixed-dtype cases, chosen so that the promotion (dsc_dtype.h:73-78) widens without rounding
MIXED_WITH = {np.float32: np.complex64, np.float64: np.float32, np.complex64: np.complex128, np.complex128: np.float64}


def _pow_operands(shape_a, shape_b, dtype_a, dtype_b, rng):
    def draw(shape, dtype, re, im):
        x = rng.uniform(*re, shape)
        if np.dtype(dtype).kind == 'c':
            x = x + 1j * rng.uniform(*im, shape)
        return x.astype(dtype)
    return draw(shape_a, dtype_a, (0.1, 4), (-2, 2)), draw(shape_b, dtype_b, (-3, 3), (-1, 1))


@pytest.mark.parametrize('dtype', DTYPES)
def test_pow_on_every_binary_route(dsc, dtype):
    rng = np.random.default_rng(16)
    cases = [(sa, sb, dtype, dtype) for sa, sb in BINARY_ROUTES]
    cases += [(sb, sa, dtype, dtype) for sa, sb in BINARY_ROUTES if sa != sb]
    for shape in ((6, 1000), (5, 1001)):                     # promoted in registers; through the cast kernels
        cases += [(shape, shape, dtype, MIXED_WITH[dtype]), (shape, shape, MIXED_WITH[dtype], dtype)]
    for sa, sb, da, db in cases:
        a, b = _pow_operands(sa, sb, da, db, rng)
        out = np.result_type(da, db)
        wide = np.complex128 if np.dtype(out).kind == 'c' else np.float64
        want = np.power(a.astype(wide), b.astype(wide)).astype(out)
        got = dsc.power(dsc.from_numpy(a), dsc.from_numpy(b)).numpy()
        assert_matches(got, want, *tolerance('pow', out), what=f'pow {np.dtype(da)}{sa} ** {np.dtype(db)}{sb}')


def test_ref_ops_unary(dsc):
    rng = np.random.default_rng(12)
    for dtype in DTYPES:
        x = _random([int(v) for v in rng.integers(1, 10, 4)], dtype, rng)
        xd = dsc.from_numpy(x)
        for op in UNARY:
            assert _close(getattr(dsc, op)(xd).numpy(), NP_UNARY[op](x)), (op, dtype)
        if np.dtype(dtype).kind == 'f':
            assert _close(dsc.i0(xd).numpy(), np.i0(x).astype(dtype))
    assert abs(dsc.i0(1.0).numpy()[0] - np.i0(1.0)) < 1e-6 and dsc.i0(2, dsc.Dtype.F64).dtype == dsc.Dtype.F64


def test_ref_ops_clip(dsc):
    for dtype in DTYPES:
        x = np.arange(10).astype(dtype) - 5
        xd = dsc.from_numpy(x)
        assert _close(dsc.clip(xd, -2, 2).numpy(), np.clip(x.real, -2, 2).astype(dtype))
        assert _close(dsc.clip(xd, -3).numpy(), np.clip(x.real, -3, None).astype(dtype))
        assert _close(dsc.clip(xd, None, 2).numpy(), np.clip(x.real, None, 2).astype(dtype))


def test_ref_ops_arange_and_randn(dsc):
    rng = np.random.default_rng(13)
    for _ in range(5):
        n = int(rng.integers(1, 10_000))
        for dtype in DTYPES:
            got = dsc.arange(n, dsc.dtype.NP_TO_DTYPE[np.dtype(dtype)]).numpy()
            assert np.array_equal(got, np.arange(n, dtype=dtype))
    for _ in range(5):
        shape = tuple(int(v) for v in rng.integers(1, 10, 4))
        for dtype, dt in ((np.float32, dsc.Dtype.F32), (np.float64, dsc.Dtype.F64)):
            r = dsc.randn(*shape, dtype=dt).numpy()
            assert r.dtype == dtype and r.shape == shape and np.isfinite(r).all()


def test_ref_ops_reshape_and_concat(dsc):
    x = np.ones((10, 10))
    xd = dsc.from_numpy(x)
    for s in ((4, 5, 5), [4, 5, 5], (-1, 5), [-1, 5]):
        got = xd.reshape(*s) if isinstance(s, tuple) and len(s) == 3 else xd.reshape(s)
        assert np.array_equal(got.numpy(), x.reshape(s))
    rng = np.random.default_rng(14)
    for n_dim in range(1, 5):
        for dtype in DTYPES:
            shape = [int(v) for v in rng.integers(2, 10, n_dim)]
            for axis in range(n_dim):
                s1, s2 = list(shape), list(shape)
                s1[axis], s2[axis] = int(rng.integers(2, 10)), int(rng.integers(2, 10))
                x1, x2 = _random(s1, dtype, rng), _random(s2, dtype, rng)
                d1, d2 = dsc.from_numpy(x1), dsc.from_numpy(x2)
                assert np.array_equal(dsc.concat((d1, d2), axis).numpy(), np.concatenate((x1, x2), axis))
                assert np.array_equal(dsc.concat([d1, d2], None).numpy(), np.concatenate((x1, x2), None))


# ---- end to end: a 537-tap Kaiser-windowed sinc low-pass designed on the device, applied through rfft -> * -> irfft

def test_kaiser_fir_designed_and_applied_on_device(dsc):
    taps, fc, beta, n, rows = 537, 0.1, 8.6, 65536, 64
    m = (taps - 1) / 2
    k = dsc.arange(taps, dsc.Dtype.F32) - m                         # -268 .. 268
    r2 = (k / m) ** 2
    w = dsc.i0(beta * dsc.sqrt(dsc.clip(1 - r2, 0.0))) / dsc.i0(beta)
    h = fc * dsc.sinc(fc * k) * w
    assert h.shape == (taps,) and h.dtype == dsc.Dtype.F32
    H = dsc.rfft(h, n=n)
    rng = np.random.default_rng(15)
    x = rng.standard_normal((rows, n)).astype(np.float32)
    y = dsc.irfft(dsc.rfft(dsc.from_numpy(x)) * H).numpy()

    kk = np.arange(taps) - m
    h64 = fc * np.sinc(fc * kk) * np.i0(beta * np.sqrt(np.clip(1 - (kk / m) ** 2, 0, None))) / np.i0(beta)
    assert rel_l2(h.numpy(), h64) <= 1e-5
    want = np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * np.fft.rfft(h64, n), n, axis=-1)
    assert rel_l2(y, want) <= 1e-5


# ---- the C++ templates of dsc_amd/api/dsc_api.h on the device (tests/cpp_math_smoke.cpp)

def test_cpp_math_templates_on_gpu(tmp_path):
    import subprocess
    exe = build_cpp_smoke(tmp_path, 'cpp_math_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'math templates ok' in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
