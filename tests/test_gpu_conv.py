"""GPU tests of dsc.convolve / dsc.correlate against the numpy FFT oracle of tests/test_conv_abi.py (f64 on the host): every mode,
f32 and f64, filter lengths 1 .. 16383 (conv_regs) and 40000 (conv_composed), rows shorter than one block, odd, 2^k + 1 and ~300 000
samples long, [T] / [B, T] / [2, 3, T] inputs; impulses at the block edges for every store alignment; the DSC_NO_CONV_FUSED switch, a
tightly sized context, no writes past the output or into the next row, determinism, argument errors, one full-size [64, 2^20] case and the C++ API."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke, device_view, dsc, run_child, sync_fixture  # noqa: F401
from tests.test_conv_abi import conv_plan, conv_span, np_convolve_fft

pytestmark = pytest.mark.gpu

TOL = {np.float32: 1e-5, np.float64: 1e-12}
MS = (1, 2, 3, 16, 63, 255, 256, 1000, 4097, 16383)
TS = (300, 1001, 4097, 300007)          # below one block, odd, 2^k + 1, ~300 000
_sync = sync_fixture()


def row_rel(got, want):
    """largest per-row rel-L2 error"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    num = np.linalg.norm(got - want, axis=-1)
    den = np.maximum(np.linalg.norm(want, axis=-1), 1e-300)
    return float(np.max(num / den))


def _run(dsc, fn_name, x, h, mode, out=None):
    fn = getattr(dsc, fn_name)
    return fn(dsc.from_numpy(x), dsc.from_numpy(h), mode, out=out)


def _cases():
    out = []
    for M in MS:
        for T in TS:
            for fn in ('convolve', 'correlate'):
                for d, dtype in enumerate((np.float32, np.float64)):
                    for mode in ('full', 'same', 'valid'):
                        if mode == 'valid' and M > T:
                            continue
                        i = len(out)
                        shape = [(T,), (3, T), (2, 3, T)][i % 3] if T < 100000 else [(T,), (2, T)][i % 2]
                        out.append((fn, dtype, mode, M, shape))
    return out


@pytest.mark.parametrize('fn,dtype,mode,M,shape', _cases(), ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_matches_oracle(dsc, fn, dtype, mode, M, shape):
    rng = np.random.default_rng([M, shape[-1], len(shape)])
    x = rng.standard_normal(shape).astype(dtype)
    h = rng.standard_normal(M).astype(dtype)
    y = _run(dsc, fn, x, h, mode)
    assert dsc.last_fft_path() == 'conv_regs'
    got = y.numpy()
    want = np_convolve_fft(x, h, mode, correlate=fn == 'correlate')
    assert got.shape == want.shape and got.dtype == dtype
    assert row_rel(got, want) <= TOL[dtype]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('M,mode,T', [
    (256, 'same', 15391),                # even M: odd n0 = 127, so odd frame starts; odd rows
    (255, 'full', 15400),                # even rows, even T_out: every pair aligned
    (255, 'full', 15401),                # odd T_out: rows after the first start on odd elements
    (63, 'valid', 16139),                # n0 = M - 1, odd T_out
    (4, 'same', 12283),                  # odd n0 = 1
    (1000, 'same', 95309)])              # 32768-point blocks in f32, 8192 in f64
def test_block_edges(dsc, dtype, M, mode, T):
    """One impulse per row, at n0 + b hop + {-1, 0, 1} and at the frame starts n0 + b hop - D + {-1, 0, 1} of the first four blocks:
    every row must be h, shifted (and cropped to the row)."""
    p = conv_plan(T, M, mode, dtype)
    hop, D, n0 = p['hop'], p['D'], p['n0']
    pos = sorted({q for b in range(4) for base in (n0 + b * hop, n0 + b * hop - D) for q in (base - 1, base, base + 1) if 0 <= q < T})
    assert p['n_blocks'] >= 3 and len(pos) >= 12
    x = np.zeros((len(pos), T), dtype=dtype)
    x[np.arange(len(pos)), pos] = 1
    h = np.random.default_rng(M).uniform(0.5, 1.5, M).astype(dtype)
    got = _run(dsc, 'convolve', x, h, mode).numpy()
    assert dsc.last_fft_path() == 'conv_regs'
    n0, T_out = conv_span(T, M, mode)
    for r, q in enumerate(pos):
        want = np.zeros(T_out)
        o = np.arange(M) + q - n0                                # out index of h[k]
        keep = (o >= 0) & (o < T_out)
        want[o[keep]] = h[keep]
        assert np.max(np.abs(got[r] - want)) <= (1e-5 if dtype == np.float32 else 1e-12), (r, q)


@pytest.mark.parametrize('fn', ['convolve', 'correlate'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_long_filter_takes_composed(dsc, fn, dtype):
    rng = np.random.default_rng(40000)
    x = rng.standard_normal((2, 100003)).astype(dtype)
    h = rng.standard_normal(40000).astype(dtype)
    for mode in ('full', 'same', 'valid'):
        got = _run(dsc, fn, x, h, mode).numpy()
        assert dsc.last_fft_path() == 'conv_composed'
        assert row_rel(got, np_convolve_fft(x, h, mode, correlate=fn == 'correlate')) <= TOL[dtype]


SWITCH = '''
import json, sys, numpy as np, dsc_amd as dsc
dsc.init(4 << 30, 2 << 30)
res = {}
for i, (M, T, mode, dt) in enumerate(((1, 5000, 'full', np.float32), (63, 100001, 'same', np.float32), (255, 30000, 'valid', np.float64),
                                      (4097, 70001, 'full', np.float32), (16383, 40000, 'same', np.float64))):
    rng = np.random.default_rng(M)
    x, h = rng.standard_normal((3, T)).astype(dt), rng.standard_normal(M).astype(dt)
    y = dsc.correlate(dsc.from_numpy(x), dsc.from_numpy(h), mode) if i % 2 else dsc.convolve(dsc.from_numpy(x), dsc.from_numpy(h), mode)
    np.save(sys.argv[1] + '/%d.npy' % i, y.numpy())
    res[i] = dsc.last_fft_path()
print(json.dumps(res))
'''


def test_switch_selects_composed_and_agrees_with_fused(tmp_path):
    (tmp_path / 'f').mkdir()
    (tmp_path / 'c').mkdir()
    fused = run_child(SWITCH, timeout=600, check=True, args=(str(tmp_path / 'f'),))
    composed = run_child(SWITCH, {'DSC_NO_CONV_FUSED': '1'}, timeout=600, check=True, args=(str(tmp_path / 'c'),))
    fused, composed = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (fused, composed))
    assert set(fused.values()) == {'conv_regs'} and set(composed.values()) == {'conv_composed'}
    for i in fused:
        a, b = np.load(tmp_path / 'f' / f'{i}.npy'), np.load(tmp_path / 'c' / f'{i}.npy')
        assert row_rel(a, b.astype(np.float64)) <= (1e-5 if a.dtype == np.float32 else 1e-12), i


TIGHT = '''
import numpy as np, dsc_amd as dsc
from tests.test_conv_abi import np_convolve_fft
rows, T, M = 4, 1000003, 40000
x_b, out_b = rows * T * 4, rows * (T + M - 1) * 4
dsc.init(x_b + out_b + M * 4 + (96 << 20), 48 << 20)     # x, out, h, plan tables, the inner filter's spectra; scratch: a few blocks
x = np.random.default_rng(3).standard_normal((rows, T)).astype(np.float32)
h = np.random.default_rng(4).standard_normal(M).astype(np.float32)
y = dsc.convolve(dsc.from_numpy(x), dsc.from_numpy(h)).numpy()
assert dsc.last_fft_path() == 'conv_composed'
want = np_convolve_fft(x, h)
e = float(np.max(np.linalg.norm(y - want, axis=-1) / np.linalg.norm(want, axis=-1)))
assert e < 1e-5, e
print('TIGHT OK', e)
'''


def test_tight_context_chunks():
    assert 'TIGHT OK' in run_child(TIGHT, timeout=600, check=True).stdout


@pytest.mark.parametrize('dtype,T,M,mode', [(np.float32, 10001, 255, 'full'), (np.float64, 4097, 16383, 'same'),
                                             (np.float32, 30001, 40000, 'full'), (np.float64, 777, 3, 'valid')])
def test_no_stray_writes(dsc, dtype, T, M, mode):
    rows = 3
    n0, T_out = conv_span(T, M, mode)
    extra = 70000
    sentinel = np.full(rows * T_out + extra, -7.25, dtype=dtype)
    big = dsc.from_numpy(sentinel)
    out = device_view(dsc, big, (rows, T_out), dtype)
    rng = np.random.default_rng(T)
    x, h = rng.standard_normal((rows, T)).astype(dtype), rng.standard_normal(M).astype(dtype)
    _run(dsc, 'convolve', x, h, mode, out=out)
    whole = big.numpy()
    assert np.all(whole[rows * T_out:] == np.asarray(-7.25, dtype=dtype)), 'bytes past the output changed'
    assert row_rel(whole[:rows * T_out].reshape(rows, T_out), np_convolve_fft(x, h, mode)) <= TOL[dtype]
    del out


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('M,mode,T', [(256, 'same', 4001), (63, 'valid', 9001), (4, 'same', 3000), (1000, 'valid', 40003),
                                      (255, 'same', 700), (16383, 'same', 20001)])
def test_last_block_stays_in_its_row(dsc, dtype, M, mode, T):
    """Every other row is zero.  The last block of a row reaches past T_out; without the row-end store predicate its extra samples
    land on the first samples of the next row, which must stay exactly zero.  Those samples are stored by the next row's first block
    too, and in the same group its stores come earlier in program order than the stray ones, so a missing predicate shows."""
    rows = 24
    x = np.random.default_rng(M + T).standard_normal((rows, T)).astype(dtype)
    x[1::2] = 0
    h = np.random.default_rng(M).uniform(0.5, 1.5, M).astype(dtype)
    got = _run(dsc, 'convolve', x, h, mode).numpy()
    assert dsc.last_fft_path() == 'conv_regs'
    assert p_overhang(T, M, mode, dtype) > 0
    assert not np.any(got[1::2]), 'a block wrote into the next row'
    assert row_rel(got[0::2], np_convolve_fft(x[0::2], h, mode)) <= TOL[dtype]


def p_overhang(T, M, mode, dtype):
    p = conv_plan(T, M, mode, dtype)
    return p['n_blocks'] * p['hop'] - p['T_out']


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_deterministic(dsc, dtype):
    rng = np.random.default_rng(9)
    x, h = dsc.from_numpy(rng.standard_normal((4, 200001)).astype(dtype)), dsc.from_numpy(rng.standard_normal(1000).astype(dtype))
    a, b = dsc.convolve(x, h, 'same').numpy(), dsc.convolve(x, h, 'same').numpy()
    assert a.tobytes() == b.tobytes()
    os.environ['DSC_NO_CONV_FUSED'] = '1'
    try:
        c, d = dsc.correlate(x, h).numpy(), dsc.correlate(x, h).numpy()
    finally:
        del os.environ['DSC_NO_CONV_FUSED']
    assert c.tobytes() == d.tobytes()


def test_argument_errors_raise(dsc):
    f32 = lambda *s: dsc.from_numpy(np.ones(s, dtype=np.float32))      # noqa: E731
    x, h = f32(100), f32(5)
    for fn in (dsc.convolve, dsc.correlate):
        with pytest.raises(ValueError):
            fn(dsc.from_numpy(np.ones(100, dtype=np.float64)), h)                 # dtypes differ
        with pytest.raises(ValueError):
            fn(dsc.from_numpy(np.ones(100, dtype=np.complex64)), h)               # complex input
        with pytest.raises(ValueError):
            fn(x, dsc.from_numpy(np.ones(5, dtype=np.complex64)))
        with pytest.raises(ValueError):
            fn(f32(2, 2, 2, 100), h)                                              # 4 dims
        with pytest.raises(ValueError):
            fn(x, f32(2, 5))                                                      # h not 1-D
        with pytest.raises(ValueError):
            fn(f32(4), h, 'valid')                                                # valid with M > T
        with pytest.raises(ValueError):
            fn(x, h, 'middle')
        with pytest.raises(ValueError, match='out must be'):
            fn(x, h, 'full', out=f32(100))                                        # wrong shape
        with pytest.raises(ValueError, match='out must be'):
            fn(x, h, 'same', out=dsc.from_numpy(np.ones(100, dtype=np.float64)))  # wrong dtype
        with pytest.raises(ValueError, match='share memory'):
            fn(x, h, 'same', out=x)                                               # out aliases x
    with pytest.raises(ValueError):
        dsc.convolve(x, f32(1, 1, 5))                                             # h 3-D


def test_full_size_against_oracle(dsc):
    rows, T, M = 64, 1 << 20, 255
    rng = np.random.default_rng(11)
    x = rng.standard_normal((rows, T)).astype(np.float32)
    h = rng.standard_normal(M).astype(np.float32)
    y = dsc.convolve(dsc.from_numpy(x), dsc.from_numpy(h))
    assert dsc.last_fft_path() == 'conv_regs'
    assert y.shape == (rows, T + M - 1)
    for r in (0, 1, 31, 62, 63):
        r = int(r)
        got = y[r:r + 1].numpy()[0]
        assert row_rel(got[None], np_convolve_fft(x[r], h)[None]) <= 1e-5, r


def test_cpp_conv_templates_on_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_conv_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'conv templates ok' in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
