"""GPU tests of dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift / dsc_pad (remap.hip, remap.cpp).  Every comparison is numpy.array_equal
on the raw words of the result (NaN payloads and -0 count) against the numpy statement of the plan in tests/test_remap_abi.py, which
that file shows to be numpy.roll / flip / fft.fftshift / fft.ifftshift / pad; the inputs are random bit patterns, not random floats.

Every case asserts dsc.last_fft_path() against the route the plan's statement expects, checks that the input is left bit for bit
unchanged, repeats the call with out= the head of a larger sentinel-filled buffer (bit-identical, nothing past it touched) and, on
the pack routes, repeats it under DSC_REMAP_ROUTE=elems and compares bit for bit.  Argument errors end the process and run in child
processes."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import assert_ends_the_process, build_cpp_smoke, device_view, dsc, sync_fixture  # noqa: F401
from tests.test_remap_abi import (C32, C64, ELEMS, F32, F64, PACKS, PAD_MODES, ROWS, bits, map_flip, map_identity, map_roll, pad_maps,
                                  random_bits, ref_fftshift, ref_flip, ref_ifftshift, ref_pad, ref_roll, route)

pytestmark = pytest.mark.gpu

DTYPES = [F32, F64, C32, C64]
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097)
SENTINEL = -7.25
EXTRA = 1031
_sync = sync_fixture('DSC_REMAP_ROUTE')


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check(dsc, call, X, x, want, path):
    """call(out) on the GPU: the route, the bits, the input left alone, a second call into the head of a sentinel-filled buffer, and on
    the pack routes a third on remap_elems"""
    y = call(None)
    assert dsc.last_fft_path() == path, (dsc.last_fft_path(), path, x.shape, x.dtype)
    yh = y.numpy()
    assert same(yh, want), (path, x.shape, x.dtype)
    del y
    big = dsc.from_numpy(np.full(want.size + EXTRA, SENTINEL, dtype=x.dtype))
    out = device_view(dsc,big, want.shape, x.dtype)
    call(out)
    assert dsc.last_fft_path() == path
    whole = big.numpy()
    assert np.array_equal(bits(whole[:want.size]), bits(want).reshape(-1)), 'out= differs'
    assert np.all(whole[want.size:] == SENTINEL), 'bytes past the output changed'
    del out, big
    if path != ELEMS:
        os.environ['DSC_REMAP_ROUTE'] = 'elems'
        z = call(None)
        os.environ.pop('DSC_REMAP_ROUTE', None)
        assert dsc.last_fft_path() == ELEMS
        assert same(z.numpy(), yh), ('the fallback differs', path, x.shape, x.dtype)
    assert X.numpy().tobytes() == x.tobytes(), 'the input changed'


def roll_maps(shape, shift, axis):
    maps = [map_identity(n) for n in shape]
    maps[axis] = map_roll(shape[axis], shift)
    return maps


# ---------------------------------------------------------------------------------------------------- the last axis, every length

@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_roll_last_axis(dsc, dt):
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 1])
    V = 16 // dt.itemsize
    seen = set()
    for n in LENGTHS:
        x = random_bits(rng, (3, n), dt)
        X = dsc.from_numpy(x)
        for s in (0, 1, -1, V - 1, V, V + 1, n - 1, n, n + 3, -5 * n - 2, n // 2):
            path = route(roll_maps(x.shape, s, 1), dt.itemsize)
            seen.add(path)
            check(dsc, lambda out: dsc.roll(X, s, axis=-1, out=out), X, x, ref_roll(x, s, -1), path)
    assert seen == ({ROWS, PACKS, ELEMS} if V > 1 else {ROWS, ELEMS}), seen


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_flip_and_shifts_last_axis(dsc, dt):
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', 2])
    for n in LENGTHS:
        x = random_bits(rng, (3, n), dt)
        X = dsc.from_numpy(x)
        check(dsc, lambda out: dsc.flip(X, axis=-1, out=out), X, x, ref_flip(x, -1), route([map_identity(3), map_flip(n)], dt.itemsize))
        fwd, inv = ref_fftshift(x, -1), ref_ifftshift(x, -1)
        check(dsc, lambda out: dsc.fftshift(X, axes=-1, out=out), X, x, fwd, route(roll_maps(x.shape, n // 2, 1), dt.itemsize))
        check(dsc, lambda out: dsc.ifftshift(X, axes=-1, out=out), X, x, inv, route(roll_maps(x.shape, -(n // 2), 1), dt.itemsize))
        a, b = dsc.fftshift(X, axes=-1), dsc.ifftshift(X, axes=-1)
        if n > 1 and n % 2:
            assert not np.array_equal(bits(a.numpy()), bits(b.numpy())), n
        else:
            assert same(a.numpy(), b.numpy())
        assert same(dsc.ifftshift(a, axes=-1).numpy(), x) and same(dsc.fftshift(b, axes=-1).numpy(), x)


# ---------------------------------------------------------------------------------------------------- pad

@pytest.mark.parametrize('mode', PAD_MODES)
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_pad_last_axis(dsc, dt, mode):
    rng = np.random.default_rng([dt.itemsize, dt.kind == 'c', len(mode), 3])
    V = 16 // dt.itemsize
    value = (2.5 - 1.25j) if dt.kind == 'c' else -3.75
    for n in LENGTHS:
        x = random_bits(rng, (3, n), dt)
        X = dsc.from_numpy(x)
        for w in ((0, 0), (1, 0), (0, 1), (V, V), (3, 2), (n - 1, n - 1), (n, n + 1), (2 * n + 3, 5)):
            width = ((0, 0), w)
            path = route(pad_maps(x.shape, width, mode), dt.itemsize)
            check(dsc, lambda out: dsc.pad(X, width, mode=mode, constant_values=value, out=out), X, x, ref_pad(x, width, mode, value), path)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_pad_constants_and_one_element_rows(dsc, dt):
    rng = np.random.default_rng([dt.itemsize, 4])
    x = random_bits(rng, (3, 64), dt)
    X = dsc.from_numpy(x)
    for value in (np.nan, 0.0, -0.0) + ((complex(np.nan, 1.5), 1e30 + 2j) if dt.kind == 'c' else (1e30,)):
        want = ref_pad(x, ((1, 2), (4, 8)), 'constant', value)
        check(dsc, lambda out: dsc.pad(X, ((1, 2), (4, 8)), constant_values=value, out=out), X, x, want, PACKS if dt.itemsize < 16 else ELEMS)
    one = random_bits(rng, (3, 1), dt)
    ONE = dsc.from_numpy(one)
    for w in ((2, 3), (0, 70), (64, 64)):
        width = ((0, 0), w)
        want = ref_pad(one, width, 'reflect')
        assert same(want, np.pad(one, width, mode='reflect'))
        check(dsc, lambda out: dsc.pad(ONE, width, mode='reflect', out=out), ONE, one, want, route(pad_maps(one.shape, width, 'reflect'), dt.itemsize))
    assert same(dsc.pad(X, 2).numpy(), np.pad(x, 2)) and same(dsc.pad(X, (1, 3), mode='wrap').numpy(), np.pad(x, (1, 3), mode='wrap'))


# ---------------------------------------------------------------------------------------------------- other axes, several at once

@pytest.mark.parametrize('shape', [(5, 6, 7, 8), (3, 4, 16, 32)], ids=str)
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_every_axis_pairs_and_all(dsc, dt, shape):
    rng = np.random.default_rng([dt.itemsize, shape[0], 5])
    x = random_bits(rng, shape, dt)
    X = dsc.from_numpy(x)
    ident = [map_identity(n) for n in shape]
    for axes in (0, 1, 2, 3, -4, (-2, -1), (0, 1, 2, 3)):
        ax = [a % 4 for a in (axes if isinstance(axes, tuple) else (axes,))]
        rolled = [map_roll(n, n // 2) if i in ax else ident[i] for i, n in enumerate(shape)]
        unrolled = [map_roll(n, -(n // 2)) if i in ax else ident[i] for i, n in enumerate(shape)]
        flipped = [map_flip(n) if i in ax else ident[i] for i, n in enumerate(shape)]
        check(dsc, lambda out: dsc.fftshift(X, axes=axes, out=out), X, x, ref_fftshift(x, axes), route(rolled, dt.itemsize))
        check(dsc, lambda out: dsc.ifftshift(X, axes=axes, out=out), X, x, ref_ifftshift(x, axes), route(unrolled, dt.itemsize))
        check(dsc, lambda out: dsc.flip(X, axis=axes, out=out), X, x, ref_flip(x, axes), route(flipped, dt.itemsize))
        shifts = tuple(3 * k - 4 for k in range(len(ax)))
        moved = [map_roll(n, shifts[ax.index(i)]) if i in ax else ident[i] for i, n in enumerate(shape)]
        check(dsc, lambda out: dsc.roll(X, shifts, axis=axes, out=out), X, x, ref_roll(x, shifts, axes), route(moved, dt.itemsize))
    check(dsc, lambda out: dsc.fftshift(X, out=out), X, x, ref_fftshift(x), route([map_roll(n, n // 2) for n in shape], dt.itemsize))
    check(dsc, lambda out: dsc.flip(X, out=out), X, x, ref_flip(x), route([map_flip(n) for n in shape], dt.itemsize))
    assert same(dsc.flip(X, axis=()).numpy(), x) and same(dsc.fftshift(X, axes=()).numpy(), x)          # numpy: an empty tuple names no axis
    widths = ((1, 0), (2, 3), (0, 9), (5, 4))
    for mode in PAD_MODES:
        check(dsc, lambda out: dsc.pad(X, widths, mode=mode, constant_values=1.5, out=out), X, x, ref_pad(x, widths, mode, 1.5),
              route(pad_maps(shape, widths, mode), dt.itemsize))
    twice = [ident[0], map_roll(shape[1], 7), ident[2], map_roll(shape[3], -3)]
    check(dsc, lambda out: dsc.roll(X, (2, 5, -3), axis=(1, 1, -1), out=out), X, x, ref_roll(x, (2, 5, -3), (1, 1, -1)), route(twice, dt.itemsize))


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_flattened_roll_and_one_dimension(dsc, dt):
    rng = np.random.default_rng([dt.itemsize, 6])
    x = random_bits(rng, (3, 5, 7), dt)
    X = dsc.from_numpy(x)
    for s in (0, 1, -1, 52, 105, -1000, 2 ** 40 + 3):
        check(dsc, lambda out: dsc.roll(X, s, out=out), X, x, ref_roll(x, s), route([map_roll(105, s)], dt.itemsize))
    for n in (1, 5, 64, 1000, 4099):
        v = random_bits(rng, (n,), dt)
        Vt = dsc.from_numpy(v)
        check(dsc, lambda out: dsc.roll(Vt, 3, axis=0, out=out), Vt, v, ref_roll(v, 3, 0), route([map_roll(n, 3)], dt.itemsize))
        check(dsc, lambda out: dsc.roll(Vt, -7, out=out), Vt, v, ref_roll(v, -7), route([map_roll(n, -7)], dt.itemsize))
        check(dsc, lambda out: dsc.flip(Vt, out=out), Vt, v, ref_flip(v), route([map_flip(n)], dt.itemsize))
        check(dsc, lambda out: dsc.fftshift(Vt, out=out), Vt, v, ref_fftshift(v), route([map_roll(n, n // 2)], dt.itemsize))
        check(dsc, lambda out: dsc.pad(Vt, (n + 2, 3), mode='symmetric', out=out), Vt, v, ref_pad(v, (n + 2, 3), 'symmetric'),
              route(pad_maps((n,), (n + 2, 3), 'symmetric'), dt.itemsize))


# ---------------------------------------------------------------------------------------------------- routes

def test_route_coverage(dsc):
    rng = np.random.default_rng(7)
    x = random_bits(rng, (4, 8, 1024), F32)
    X = dsc.from_numpy(x)
    check(dsc, lambda out: dsc.roll(X, 3, axis=1, out=out), X, x, ref_roll(x, 3, 1), ROWS)
    for dt, path in ((F32, PACKS), (F64, PACKS), (C32, PACKS), (C64, ELEMS)):          # 16-byte elements: a mapped last axis is remap_elems
        x = random_bits(rng, (3, 1024), dt)
        X = dsc.from_numpy(x)
        check(dsc, lambda out: dsc.roll(X, 1, axis=-1, out=out), X, x, ref_roll(x, 1, -1), path)
        check(dsc, lambda out: dsc.roll(X, 1, axis=0, out=out), X, x, ref_roll(x, 1, 0), ROWS)
    x = random_bits(rng, (3, 1023), F32)
    X = dsc.from_numpy(x)
    check(dsc, lambda out: dsc.roll(X, 1, axis=-1, out=out), X, x, ref_roll(x, 1, -1), ELEMS)
    check(dsc, lambda out: dsc.roll(X, 1, axis=0, out=out), X, x, ref_roll(x, 1, 0), ELEMS)
    x = random_bits(rng, (300, 2048), F32)                                          # more than one workgroup per row, many rows
    X = dsc.from_numpy(x)
    check(dsc, lambda out: dsc.roll(X, (7, 1001), axis=(0, 1), out=out), X, x, ref_roll(x, (7, 1001), (0, 1)), PACKS)
    check(dsc, lambda out: dsc.pad(X, ((3, 2), (100, 156)), mode='reflect', out=out), X, x, ref_pad(x, ((3, 2), (100, 156)), 'reflect'), PACKS)
    check(dsc, lambda out: dsc.flip(X, axis=0, out=out), X, x, ref_flip(x, 0), ROWS)
    check(dsc, lambda out: dsc.pad(X, ((3, 2), (0, 0)), constant_values=np.nan, out=out), X, x, ref_pad(x, ((3, 2), (0, 0)), 'constant', np.nan), ROWS)


def test_a_base_off_the_pack_boundary_leaves_the_pack_routes(dsc):
    """the same [3, 1024] f32 tensors over device pointers 8 bytes past a 16-byte boundary, as the input and as out=.  8 bytes is the
    smallest offset there is: dsc_tensor_from_device_ptr refuses a pointer that is not 8-byte aligned, for every dtype."""
    rng = np.random.default_rng(8)
    x = random_bits(rng, (3, 1024), F32)
    flat = np.concatenate([np.zeros(2, F32), x.reshape(-1), np.zeros(2, F32)])
    big = dsc.from_numpy(flat)
    assert big._c_ptr.contents.data % 16 == 0
    Xo = device_view(dsc,big, x.shape, F32, byte_offset=8)
    assert same(Xo.numpy(), x)
    for f, want in ((lambda out: dsc.roll(Xo, 1, axis=-1, out=out), ref_roll(x, 1, -1)), (lambda out: dsc.roll(Xo, 1, axis=0, out=out), ref_roll(x, 1, 0)),
                    (lambda out: dsc.pad(Xo, ((0, 0), (4, 4)), mode='reflect', out=out), ref_pad(x, ((0, 0), (4, 4)), 'reflect'))):
        assert same(f(None).numpy(), want)
        assert dsc.last_fft_path() == ELEMS
    X = dsc.from_numpy(x)
    dest = dsc.from_numpy(np.full(x.size + 8, SENTINEL, F32))
    out = device_view(dsc,dest, x.shape, F32, byte_offset=8)
    for f, want in ((lambda: dsc.roll(X, 1, axis=-1, out=out), ref_roll(x, 1, -1)), (lambda: dsc.roll(X, 1, axis=0, out=out), ref_roll(x, 1, 0))):
        f()
        assert dsc.last_fft_path() == ELEMS
        whole = dest.numpy()
        assert np.array_equal(bits(whole[2:2 + x.size]), bits(want).reshape(-1))
        assert np.all(whole[:2] == SENTINEL) and np.all(whole[2 + x.size:] == SENTINEL)
    assert same(big.numpy(), flat)


def test_fftshift_of_fft2(dsc):
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((2, 16, 16)) + 1j * rng.standard_normal((2, 16, 16))).astype(C32)
    S = dsc.fft2(dsc.from_numpy(x))
    spectrum = S.numpy()
    got = dsc.fftshift(S, axes=(-2, -1)).numpy()
    assert same(got, np.fft.fftshift(spectrum, axes=(-2, -1)))
    assert np.allclose(got, np.fft.fftshift(np.fft.fft2(x.astype(C64)), axes=(-2, -1)), rtol=0, atol=1e-3)


# ---------------------------------------------------------------------------------------------------- child processes

ERRORS = {
    'axis_too_large': ("dsc.roll(X, 1, axis=2)", 'out of range'),
    'axis_too_small': ("dsc.fftshift(X, axes=-3)", 'out of range'),
    'flip_axis_out_of_range': ("dsc.flip(X, axis=(0, 5))", 'out of range'),
    'flip_repeated_axis': ("dsc.flip(X, axis=(1, -1))", 'repeated axis'),
    'negative_pad_width': ("dsc.pad(X, ((0, 0), (1, -1)))", 'negative pad width'),
    'out_shape': ("dsc.pad(X, 1, out=dsc.from_numpy(np.ones((4, 65), np.float32)))", 'out must have'),
    'out_dtype': ("dsc.roll(X, 1, axis=0, out=dsc.from_numpy(np.ones((2, 64), np.float64)))", 'out must have'),
    'out_overlaps_x': ("dsc.roll(X, 1, axis=-1, out=X)", 'out must not share memory'),
    'unknown_mode': ("from dsc_amd import _bindings as B\nfrom dsc_amd.context import _get_ctx\n"
                     "B.dsc_pad(_get_ctx(), X._c_ptr, None, (B.c_int * 4)(1, 1, 1, 1), 7, 0.0, 0.0)", 'unknown mode'),
    'too_many_elements': ("dsc.pad(X, ((2 ** 30, 0), (0, 0)))", 'more than 2^31 - 1 elements'),
    'bad_route': ("import os\nos.environ['DSC_REMAP_ROUTE'] = 'fast'\ndsc.flip(X)", 'DSC_REMAP_ROUTE must be'),
}


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_argument_errors_end_the_process(name):
    """like every operator: a message on stderr and exit status 1; nothing runs on the GPU after it"""
    stmt, message = ERRORS[name]
    assert_ends_the_process("X = dsc.from_numpy(np.ones((2, 64), np.float32))\n" + stmt, message, without_env='DSC_REMAP_ROUTE')


def test_an_unknown_mode_name_is_a_python_error(dsc):
    with pytest.raises(ValueError):
        dsc.pad(dsc.from_numpy(np.ones(4, np.float32)), 1, mode='mean')


def test_cpp_remap_smoke_on_the_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_remap_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'remap templates ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
