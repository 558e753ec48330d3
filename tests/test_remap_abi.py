"""CPU tests of dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift / dsc_pad (include/dsc_mi355x.h, Section J): the prototypes are declared
with their exact signatures, exported, bound and wrapped; a C++ translation unit that names the five wrappers of dsc_api.h compiles and
links; and the plan — one piecewise-affine map per axis, dsc_amd/csrc/remap_plan.h — is numpy's roll, flip, fft.fftshift, fft.ifftshift
and pad.

The plan is stated twice and both statements are compared with numpy:
  * in numpy here (map_roll / map_flip / map_pad, map_indices, gather: one map per axis, applied with numpy.take), which
    tests/test_gpu_remap.py imports as its reference and whose merge / route are what it expects dsc.last_fft_path() to say;
  * in the library's own header, through the stand-alone host program tests/cpp_remap_plan.cpp, built with -fsanitize=address,undefined:
    the functions the host side plans with and the kernels index with.
The closed forms of numpy.pad's modes, with n the extent and t = j - before (mod with a result >= 0):
    wrap t mod n;   edge t clamped to [0, n - 1];   reflect u = t mod 2 (n - 1), u if u < n else 2 (n - 1) - u, 0 when n == 1;
    symmetric u = t mod 2 n, u if u < n else 2 n - 1 - u
are checked against numpy.pad's iterated padding on n = 1 .. 11, before = 0 .. 39, after in {0, 1, 3 n + 2, 17}: 7040 cases, no difference.
Nothing here is a tolerance: indices are integers and elements move as opaque words."""
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
NAMES = ('dsc_roll', 'dsc_flip', 'dsc_fftshift', 'dsc_ifftshift', 'dsc_pad')
PROTOTYPES = (
    'dsc_tensor *dsc_roll (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *shifts, const int *axes);',
    'dsc_tensor *dsc_flip (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes);',
    'dsc_tensor *dsc_fftshift (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes);',
    'dsc_tensor *dsc_ifftshift(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes);',
    'dsc_tensor *dsc_pad (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, const int *pad_width, int mode, double value_re, double value_im);',
)
PAD_MODES = ('constant', 'edge', 'reflect', 'symmetric', 'wrap')                # the codes 0 .. 4 of dsc_pad
AFFINE_MOD, REVERSED, CLAMP, REFLECT, SYMMETRIC, CONSTANT = range(6)            # the kinds of dsc_axis_map
ROWS, PACKS, ELEMS = 'remap_rows', 'remap_packs', 'remap_elems'
MIN_PACKS = 16                                                                   # DSC_REMAP_MIN_PACKS


# ---- the plan in numpy: a map is (n_in, n_out, kind, a, b), dsc_axis_map -------------------------------------------------------------
def map_identity(n):
    return (n, n, AFFINE_MOD, 1, 0)


def map_roll(n, shift):
    return (n, n, AFFINE_MOD, 1, (-int(shift)) % n)


def map_flip(n):
    return map_identity(n) if n <= 1 else (n, n, REVERSED, -1, n - 1)


def map_pad(n, before, after, mode):
    n_out = n + before + after
    if before == 0 and after == 0:
        return map_identity(n)
    if mode == 'edge' or (mode == 'reflect' and n == 1):
        return (n, n_out, CLAMP, 1, -before)
    if mode == 'reflect':
        return (n, n_out, REFLECT, 2 * (n - 1), (-before) % (2 * (n - 1)))
    if mode == 'symmetric':
        return (n, n_out, SYMMETRIC, 2 * n, (-before) % (2 * n))
    if mode == 'wrap':
        return (n, n_out, AFFINE_MOD, 1, (-before) % n)
    assert mode == 'constant', mode
    return (n, n_out, CONSTANT, 1, -before)


def map_indices(m):
    """source index per output index, int64; -1: the constant"""
    n, n_out, kind, a, b = m
    j = np.arange(n_out, dtype=np.int64)
    if kind == AFFINE_MOD:
        return (j + b) % n
    if kind == REVERSED:
        return n - 1 - j
    if kind == CLAMP:
        return np.clip(j + b, 0, n - 1)
    if kind == REFLECT:
        u = (j + b) % a
        return np.where(u < n, u, a - u)
    if kind == SYMMETRIC:
        u = (j + b) % a
        return np.where(u < n, u, a - 1 - u)
    t = j + b
    return np.where((t < 0) | (t >= n), -1, t)


def gather(x, maps, value=0):
    """out[j0, j1, ..] = x[m0(j0), m1(j1), ..] or the constant: one numpy.take per axis"""
    assert len(maps) == x.ndim and all(m[0] == s for m, s in zip(maps, x.shape)), (maps, x.shape)
    out = x
    outside = np.zeros([m[1] for m in maps], bool)
    for axis, m in enumerate(maps):
        idx = map_indices(m)
        assert idx.shape == (m[1],) and idx.min() >= -1 and idx.max() < m[0]
        out = np.take(out, np.maximum(idx, 0), axis=axis)
        shape = [1] * x.ndim
        shape[axis] = m[1]
        outside |= (idx < 0).reshape(shape)
    out = np.ascontiguousarray(out)
    if outside.any():
        out[outside] = np.asarray(value).astype(x.dtype)
    return out


def _axes(axis, ndim):
    axes = tuple(axis) if isinstance(axis, (tuple, list)) else (axis,)
    assert all(-ndim <= a < ndim for a in axes), axes
    return [a % ndim for a in axes]


def ref_roll(x, shift, axis=None):
    if axis is None:
        return gather(x.reshape(-1), [map_roll(x.size, shift)]).reshape(x.shape)
    shifts = tuple(shift) if isinstance(shift, (tuple, list)) else (shift,)
    axes = _axes(axis, x.ndim)
    if len(shifts) != len(axes):
        shifts, axes = shifts * (len(axes) if len(shifts) == 1 else 1), axes * (len(shifts) if len(axes) == 1 else 1)
    total = [0] * x.ndim
    for s, a in zip(shifts, axes):
        total[a] += s
    return gather(x, [map_roll(n, s) for n, s in zip(x.shape, total)])


def ref_flip(x, axis=None):
    axes = range(x.ndim) if axis is None else _axes(axis, x.ndim)
    return gather(x, [map_flip(n) if a in axes else map_identity(n) for a, n in enumerate(x.shape)])


def _ref_shift(x, axes, sign):
    total = [0] * x.ndim
    for a in (range(x.ndim) if axes is None else _axes(axes, x.ndim)):
        total[a] += sign * (x.shape[a] // 2)
    return gather(x, [map_roll(n, s) for n, s in zip(x.shape, total)])


def ref_fftshift(x, axes=None):
    return _ref_shift(x, axes, 1)


def ref_ifftshift(x, axes=None):
    return _ref_shift(x, axes, -1)


def pad_maps(shape, pad_width, mode):
    widths = np.broadcast_to(np.asarray(pad_width), (len(shape), 2))
    return [map_pad(n, int(b), int(a), mode) for n, (b, a) in zip(shape, widths)]


def ref_pad(x, pad_width, mode='constant', constant_values=0):
    return gather(x, pad_maps(x.shape, pad_width, mode), constant_values)


def merge(maps):
    """dsc_remap_merge: the maps in four slots, neighbouring identities as one, axes of one element dropped"""
    def identity(m):
        return m[0] == m[1] and (m[0] == 1 or (m[2] == AFFINE_MOD and m[4] == 0))
    kept = []
    for m in maps:
        if m[0] == 1 and m[1] == 1:
            continue
        if kept and identity(m) and identity(kept[-1]):
            kept[-1] = map_identity(kept[-1][0] * m[0])
        else:
            kept.append(map_identity(m[0]) if identity(m) else tuple(m))
    return [map_identity(1)] * (4 - len(kept)) + kept


def route(maps, itemsize, aligned=True):
    """dsc_remap_route on the merged plan: what dsc.last_fft_path() says"""
    merged = merge(maps)
    last = merged[-1]
    ne = int(np.prod([m[1] for m in merged], dtype=np.int64))
    row_bytes = last[1] * itemsize
    if not aligned or row_bytes % 16 or row_bytes // 16 < MIN_PACKS:
        return ELEMS
    if ne // last[1] * ((row_bytes // 16 + 255) // 256) >= 2 ** 31:
        return ELEMS
    if last == map_identity(last[0]):
        return ROWS
    return PACKS if itemsize < 16 else ELEMS


def bits(a):
    """the raw words of an array: NaN payloads and -0 count"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def random_bits(rng, shape, dt):
    """random bit patterns, not random floats: NaNs with payloads, infinities, denormals and -0 all occur"""
    dt = np.dtype(dt)
    words = rng.integers(0, 2 ** 32, size=int(np.prod(shape)) * dt.itemsize // 4, dtype=np.uint32)
    return words.view(dt).reshape(shape)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared_exported_bound_and_wrapped():
    text = open(HEADER).read()
    assert 'Section J' in text and 'no reference counterpart' in text[text.index('Section J'):text.index('Section J') + 200]
    for word in (ROWS, PACKS, ELEMS, 'DSC_REMAP_ROUTE'):
        assert word in text, word
    squeezed = re.sub(r' +', ' ', text)
    for proto in PROTOTYPES:
        assert re.sub(r' +', ' ', proto) in squeezed, proto
    lib = ctypes.CDLL(LIB)
    from dsc_amd import _bindings as B
    ints = ctypes.POINTER(ctypes.c_int)
    head = [B._DscCtx, B._DscTensor_p, B._DscTensor_p]
    argtypes = {'dsc_roll': head + [ctypes.c_int, ints, ints], 'dsc_flip': head + [ctypes.c_int, ints], 'dsc_fftshift': head + [ctypes.c_int, ints],
                'dsc_ifftshift': head + [ctypes.c_int, ints], 'dsc_pad': head + [ints, ctypes.c_int, ctypes.c_double, ctypes.c_double]}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in B.EXPORTS
        f = getattr(B, name)
        assert f.argtypes == argtypes[name], name
        assert f.restype is B._DscTensor_p
    import dsc_amd
    for name in ('roll', 'flip', 'fftshift', 'ifftshift', 'pad'):
        assert callable(getattr(dsc_amd, name)) and name in dsc_amd.__all__, name


def test_cpp_wrappers_and_documents():
    api = open(os.path.join(ROOT, 'dsc_amd', 'api', 'dsc_api.h')).read()
    for name in ('roll', 'flip', 'fftshift', 'ifftshift', 'pad'):
        assert re.search(r'tensor<T> %s\(const tensor<T> &x' % name, api), name
        assert 'dsc_%s(ctx, x.x_, nullptr' % name in api, name
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in ('roll', 'flip', 'fftshift', 'ifftshift', 'pad'):
            assert name in text, (doc, name)
    assert '4.11' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'bench_remap' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    makefile = open(os.path.join(ROOT, 'dsc_amd', 'csrc', 'Makefile')).read()
    assert 'remap.hip' in makefile and 'remap.cpp' in makefile


def test_cpp_remap_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_remap_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout


# ---- the numpy statement of the plan is numpy ------------------------------------------------------------------------------------------
SHAPES = ((1,), (2,), (7,), (8,), (3, 5), (4, 1, 6), (3, 5, 7), (2, 3, 4, 5), (5, 6, 7, 8))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize('dt', [F32, F64, C32, C64], ids=str)
def test_roll_flip_and_shifts_are_numpy(dt):
    rng = np.random.default_rng([dt.itemsize, 1])
    for shape in SHAPES:
        x = random_bits(rng, shape, dt)
        nd = len(shape)
        for s in (0, 1, -1, 3, x.size, -5 * x.size - 2, 2 ** 40 + 3):
            assert same(ref_roll(x, s), np.roll(x, s)), (shape, s)
        for axis in range(-nd, nd):
            n = shape[axis]
            for s in (0, 1, -1, n - 1, n, n + 3, -5 * n - 2, n // 2, -2 ** 33 - 1):
                assert same(ref_roll(x, s, axis), np.roll(x, s, axis)), (shape, s, axis)
            assert same(ref_flip(x, axis), np.flip(x, axis))
            assert same(ref_fftshift(x, axis), np.fft.fftshift(x, axis)) and same(ref_ifftshift(x, axis), np.fft.ifftshift(x, axis))
            if n > 1 and n % 2:
                assert not np.array_equal(bits(ref_fftshift(x, axis)), bits(ref_ifftshift(x, axis)))
        assert same(ref_flip(x), np.flip(x)) and same(ref_fftshift(x), np.fft.fftshift(x)) and same(ref_ifftshift(x), np.fft.ifftshift(x))
        assert same(ref_ifftshift(ref_fftshift(x)), x)
        if nd >= 2:
            assert same(ref_roll(x, (2, -1), (0, -1)), np.roll(x, (2, -1), (0, -1)))
            assert same(ref_roll(x, (2, 5), (-1, -1)), np.roll(x, (2, 5), (-1, -1)))          # a repeated axis adds its shifts
            assert same(ref_roll(x, 3, (0, 1)), np.roll(x, 3, (0, 1)))
            assert same(ref_flip(x, (0, -1)), np.flip(x, (0, -1)))
            assert same(ref_fftshift(x, (-2, -1)), np.fft.fftshift(x, (-2, -1))) and same(ref_ifftshift(x, (-2, -1)), np.fft.ifftshift(x, (-2, -1)))


@pytest.mark.parametrize('mode', PAD_MODES)
def test_pad_closed_forms_are_numpy_pad(mode):
    """n = 1 .. 11, before = 0 .. 39, after in {0, 1, 3 n + 2, 17}: numpy.pad of arange(n) gives the source indices themselves"""
    cases = 0
    for n in range(1, 12):
        x = np.arange(n, dtype=np.int64)
        for before in range(40):
            for after in (0, 1, 3 * n + 2, 17):
                idx = map_indices(map_pad(n, before, after, mode))
                want = np.pad(x, (before, after), mode=mode, **({'constant_values': -1} if mode == 'constant' else {}))
                assert np.array_equal(idx, want), (mode, n, before, after)
                cases += 1
    assert cases == 1760                                                # times the four modes with a closed form: 7040


@pytest.mark.parametrize('dt', [F32, C64], ids=str)
def test_pad_on_tensors_is_numpy_pad(dt):
    rng = np.random.default_rng([dt.itemsize, 2])
    value = 2.5 - 1.25j if dt.kind == 'c' else -3.75
    for shape in SHAPES:
        x = random_bits(rng, shape, dt)
        nd = len(shape)
        widths = [3, (2, 5), [(k + 1, 2 * k) for k in range(nd)], [(0, 0)] * (nd - 1) + [(shape[-1] * 2 + 3, 1)]]
        for mode in PAD_MODES:
            for w in widths:
                kw = {'constant_values': value} if mode == 'constant' else {}
                assert same(ref_pad(x, w, mode, value), np.pad(x, w, mode=mode, **kw)), (shape, mode, w)
    nan = ref_pad(np.ones(3, F32), 2, 'constant', np.nan)
    assert np.isnan(nan[[0, 1, 5, 6]]).all() and same(nan, np.pad(np.ones(3, F32), 2, constant_values=np.nan))


def test_merge_and_route():
    ident = map_identity
    assert merge([ident(4096), ident(64), ident(256)]) == [ident(1)] * 3 + [ident(4096 * 64 * 256)]
    assert merge([map_roll(4096, 5), ident(64), ident(256)]) == [ident(1)] * 2 + [map_roll(4096, 5), ident(64 * 256)]
    assert merge([ident(3), map_roll(5, 0), map_flip(1), map_flip(7)]) == [ident(1)] * 2 + [ident(15), map_flip(7)]
    assert route([ident(4), map_roll(8, 3), ident(1024)], 4) == ROWS
    assert route([ident(3), map_roll(1024, 1)], 4) == PACKS
    assert route([ident(3), map_roll(1023, 1)], 4) == ELEMS
    assert route([ident(3), map_roll(1024, 1)], 16) == ELEMS and route([map_roll(3, 1), ident(1024)], 16) == ROWS
    assert route([ident(3), map_roll(1024, 1)], 4, aligned=False) == ELEMS
    assert route([ident(3), map_roll(60, 1)], 4) == ELEMS and route([ident(3), map_roll(64, 1)], 4) == PACKS      # 15 and 16 packs
    assert route(pad_maps((3, 1023), ((0, 0), (1, 0)), 'reflect'), 4) == PACKS                                     # the OUTPUT row counts


# ---- the library's own header, stand-alone and under the sanitizers -------------------------------------------------------------------
@pytest.fixture(scope='module')
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('remap_plan') / 'cpp_remap_plan')
    # the sanitizers' runtimes are linked statically: the program stands alone, whatever the environment preloads into its processes
    cmd = ['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-I' + os.path.join(ROOT, 'dsc_amd', 'csrc'), os.path.join(ROOT, 'tests', 'cpp_remap_plan.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(lines):
        r = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])                  # a sanitizer report ends the program (-fno-sanitize-recover)
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [np.array(ln.split(), dtype=np.int64) for ln in out]
    return ask


def test_header_maps_are_numpy(plan_program):
    """every map of the pad grid, and rolls with shifts beyond 32 bits, from dsc_map_index itself"""
    requests, want = [], []
    for code, mode in enumerate(PAD_MODES):
        for n in range(1, 12):
            x = np.arange(n, dtype=np.int64)
            for before in range(40):
                for after in (0, 1, 3 * n + 2, 17):
                    requests.append(f'map pad {n} {before} {after} {code}')
                    want.append(np.pad(x, (before, after), mode=mode, **({'constant_values': -1} if mode == 'constant' else {})))
    for n in (1, 2, 3, 8, 17, 1000):
        x = np.arange(n, dtype=np.int64)
        for s in (0, 1, -1, n - 1, n, n + 3, -5 * n - 2, n // 2, 2 ** 40 + 3, -2 ** 62, 2 ** 31 - 1, -2 ** 31):
            requests.append(f'map roll {n} {s}')
            want.append(np.roll(x, s))
        requests.append(f'map flip {n}')
        want.append(x[::-1])
    got = plan_program(requests)
    assert len(requests) == 8800 + 6 * 13
    for req, g, w in zip(requests, got, want):
        assert np.array_equal(g, w), req


def test_header_index_arithmetic_at_the_int_limits(plan_program):
    """extents and widths near 2^31: the sums are formed in 64 bits (the sanitizers would end the program on an overflow); single
    indices are checked through a plan's merged maps, not by printing two thousand million of them"""
    big = 2 ** 31 - 1
    got = plan_program([f'plan 4 1 id:1 id:1 id:1 roll:{big}:{-2 ** 62}', f'plan 4 1 id:1 id:1 id:1 pad:{big - 7}:3:4:2',
                        f'plan 4 1 id:1 id:1 id:1 pad:{big - 7}:3:4:3', f'plan 8 1 id:1 id:1 id:1 pad:1:{big - 2}:1:4'])
    assert list(got[0][15:20]) == [big, big, AFFINE_MOD, 1, 2 ** 62 % big]
    assert list(got[1][15:20]) == [big - 7, big, REFLECT, 2 * (big - 8), 2 * (big - 8) - 3]
    assert list(got[2][15:20]) == [big - 7, big, SYMMETRIC, 2 * (big - 7), 2 * (big - 7) - 3]
    assert list(got[3][15:20]) == [1, big, AFFINE_MOD, 1, 0]


def test_header_merge_and_route_match_the_numpy_statement(plan_program):
    rng = np.random.default_rng(3)
    requests, want = [], []
    lengths = (1, 2, 3, 4, 5, 8, 16, 60, 64, 255, 256, 1024)
    for _ in range(400):
        specs, maps = [], []
        for _ in range(4):
            n = int(rng.choice(lengths))
            kind = int(rng.integers(0, 4))
            if kind == 0:
                specs.append(f'id:{n}')
                maps.append(map_identity(n))
            elif kind == 1:
                s = int(rng.integers(-3 * n, 3 * n + 1))
                specs.append(f'roll:{n}:{s}')
                maps.append(map_roll(n, s))
            elif kind == 2:
                specs.append(f'flip:{n}')
                maps.append(map_flip(n))
            else:
                b, a, mode = int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(rng.integers(0, 5))
                specs.append(f'pad:{n}:{b}:{a}:{mode}')
                maps.append(map_pad(n, b, a, PAD_MODES[mode]))
        eb, aligned = int(rng.choice((4, 8, 16))), int(rng.integers(0, 4) > 0)
        requests.append(f'plan {eb} {aligned} ' + ' '.join(specs))
        merged = merge(maps)
        flat = [v for m in merged for v in m]
        ne = int(np.prod([m[1] for m in merged], dtype=np.int64))
        want.append(flat + [ne, (ROWS, PACKS, ELEMS).index(route(maps, eb, bool(aligned)))])
    got = plan_program(requests)
    seen = set()
    for req, g, w in zip(requests, got, want):
        assert list(g) == w, (req, list(g), w)
        seen.add(w[-1])
    assert seen == {0, 1, 2}
