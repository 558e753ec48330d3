"""GPU tests of dsc.stft / dsc.istft and the window helpers against the numpy restatement of tests/test_stft_abi.py (f64 on the
host), whole-array rel-L2: five of the fused (stft_regs) lengths — 64, 256, 1024, 4096, 32768 — and four composed (stft_composed)
ones with the hop families n/4, n/2, n, 2n and odd; per (n_fft, hop, dtype) ONE draw of center, padding, shape ([T] / [B, T] /
[2, 3, T]) and window (none / Hann / Kaiser / random asymmetric), the full product of those options at 256, 4096 and 32 only; the
DSC_NO_STFT_FUSED switch, a tightly sized context, istft against torch.istft, round trips, NOLA, and one full-size [64, 2^20] case.
Every fused length, every option at every length, the edges of the signal, workgroup geometry, the istft chunking branches and the
out= / stray-write checks, per frame and per sample against a long-double reference, are in tests/test_gpu_stft_routes.py."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke, dsc, run_child, sync_fixture  # noqa: F401
from tests.test_stft_abi import np_istft, np_stft

pytestmark = pytest.mark.gpu

FUSED = (64, 256, 1024, 4096, 32768)
COMPOSED = (4, 32, 65536, 262144)
TOL = {np.float32: 1e-5, np.float64: 1e-12}
_sync = sync_fixture()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


def make_window(kind, n, dtype, seed=0):
    import torch
    if kind is None:
        return None
    if kind == 'hann':
        return torch.hann_window(n, dtype=torch.float64).numpy().astype(dtype)
    if kind == 'kaiser':
        return torch.kaiser_window(n, dtype=torch.float64).numpy().astype(dtype)
    return np.random.default_rng(seed + n).uniform(0.2, 1.8, n).astype(dtype)     # asymmetric


def _hops(n):
    odd = [3, 125] if n <= 1024 else [125] if n <= 65536 else [4097]
    big = [n // 4, n] if n >= 262144 else [n // 4, n // 2, n, 2 * n]
    return [h for h in big if h >= 1] + odd


def _signal_length(n, hop, center, t_kind):
    """t_kind 0: just above n/2 (center only; n without), 1: exactly n, 2: not a multiple of hop"""
    if n >= 65536 and hop < 4096:
        return n + 3                                                             # keep the odd-hop spectra of the long frames small
    if t_kind == 0:
        return n // 2 + 1 if center else n
    return n if t_kind == 1 else n + n // 2 + 7 + (hop if hop < n else 0)


def _cases():
    """Every size x hop family x dtype; the other options drawn independently (own seed per case)."""
    out = []
    for n in FUSED + COMPOSED:
        for hop in _hops(n):
            for d, dtype in enumerate((np.float32, np.float64)):
                rng = np.random.default_rng([n, hop, d])
                center = bool(rng.integers(2))
                pad_mode = ('reflect', 'constant')[rng.integers(2)]
                T = _signal_length(n, hop, center, int(rng.integers(3)))
                shape = [(T,), (3, T), (2, 3, T)][rng.integers(3)] if n <= 32768 else [(T,), (2, T)][rng.integers(2)]
                win = (None, 'hann', 'kaiser', 'rand')[rng.integers(4)]
                out.append((n, hop, dtype, center, pad_mode, shape, win))
    return out


def _product_cases():
    """dtype x padding x window x center, all combinations, for the LDS-staged kernel (256), the mid kernel (4096) and a composed
    size (32); odd hops, T not a multiple of hop; shapes in turn (all three for every combination at 256)."""
    out = []
    for n, hop in ((256, 125), (4096, 125), (32, 3)):
        for i, (dtype, pad_mode, win, center) in enumerate(itertools.product((np.float32, np.float64), ('reflect', 'constant'),
                                                                               (None, 'hann', 'kaiser', 'rand'), (True, False))):
            T = 3 * n + 7
            shapes = [(T,), (3, T), (2, 3, T)] if n == 256 else [[(T,), (3, T), (2, 3, T)][i % 3]]
            out += [(n, hop, dtype, center, pad_mode, shape, win) for shape in shapes]
    return out


@pytest.mark.parametrize('n_fft,hop,dtype,center,pad_mode,shape,win', _cases() + _product_cases(),
                         ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_stft_matches_numpy(dsc, n_fft, hop, dtype, center, pad_mode, shape, win):
    rng = np.random.default_rng(n_fft * 7 + hop)
    x = rng.standard_normal(shape).astype(dtype)
    w = make_window(win, n_fft, dtype)
    X = dsc.stft(dsc.from_numpy(x), n_fft, hop, None if w is None else dsc.from_numpy(w), center, pad_mode)
    path = dsc.last_fft_path()
    assert path == ('stft_regs' if n_fft in FUSED else 'stft_composed')
    want = np_stft(x, n_fft, hop, w, center, pad_mode)
    got = X.numpy()
    assert got.shape == want.shape and got.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    assert rel(got, want) <= TOL[dtype], (path, rel(got, want))


SWITCH = '''
import json, sys, numpy as np, dsc_amd as dsc
dsc.init(4 << 30, 2 << 30)
res = {}
for n, hop, dt in ((64, 3, np.float32), (1024, 256, np.float32), (4096, 125, np.float64), (32768, 8192, np.float32)):
    x = np.random.default_rng(n).standard_normal((2, 3 * n + 11)).astype(dt)
    w = np.random.default_rng(1).uniform(0.2, 1.8, n).astype(dt)
    X = dsc.stft(dsc.from_numpy(x), n, hop, dsc.from_numpy(w))
    np.save(sys.argv[1] + '/%d.npy' % n, X.numpy())
    res[n] = dsc.last_fft_path()
print(json.dumps(res))
'''


def test_switch_selects_composed_and_agrees_with_fused(tmp_path):
    (tmp_path / 'f').mkdir()
    (tmp_path / 'c').mkdir()
    fused = run_child(SWITCH, timeout=600, check=True, args=(str(tmp_path / 'f'),))
    composed = run_child(SWITCH, {'DSC_NO_STFT_FUSED': '1'}, timeout=600, check=True, args=(str(tmp_path / 'c'),))
    fused, composed = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (fused, composed))
    assert set(fused.values()) == {'stft_regs'} and set(composed.values()) == {'stft_composed'}
    for n in fused:
        a, b = np.load(tmp_path / 'f' / f'{n}.npy'), np.load(tmp_path / 'c' / f'{n}.npy')
        tol = 1e-5 if a.dtype == np.complex64 else 1e-12
        assert rel(a, b) <= tol, (n, rel(a, b))


TIGHT = '''
import numpy as np, dsc_amd as dsc
from tests.test_stft_abi import np_stft, np_istft
n, hop, rows, T = 65536, 16384, 2, 65536 * 5 + 3
frames = 1 + T // hop
x_b, out_b = rows * T * 8, rows * frames * (n // 2 + 1) * 16
dsc.init(x_b + out_b + rows * T * 8 + (24 << 20), 16 * n * 8)     # x, X, istft's y, plan tables; scratch: a chunk of 8 frames
x = np.random.default_rng(3).standard_normal((rows, T))
w = np.hanning(n + 1)[:n]
wt = dsc.from_numpy(w)
X = dsc.stft(dsc.from_numpy(x), n, hop, wt)
assert dsc.last_fft_path() == 'stft_composed'
Xh = X.numpy()
e1 = np.linalg.norm(Xh - np_stft(x, n, hop, w)) / np.linalg.norm(np_stft(x, n, hop, w))
y = dsc.istft(X, n, hop, wt, length=T).numpy()
e2 = np.linalg.norm(y - x) / np.linalg.norm(x)
assert e1 < 1e-12 and e2 < 1e-12, (e1, e2)
print('TIGHT OK', e1, e2)
'''


def test_tight_context_chunks():
    assert 'TIGHT OK' in run_child(TIGHT, timeout=600, check=True).stdout


@pytest.mark.parametrize('n_fft,hop,center,win,length', [
    (256, 64, True, 'hann', None), (256, 64, True, 'hann', 3000), (1024, 125, False, 'rand', None), (64, 16, True, 'kaiser', 500),
    (4096, 1024, False, 'rand', 4096 * 3 + 1000), (32, 8, True, None, 77)])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_istft_matches_torch(dsc, n_fft, hop, center, win, length, dtype):
    import torch
    rng = np.random.default_rng(n_fft + hop)
    T = 5 * n_fft + 13
    x = rng.standard_normal((2, T))
    w = make_window(win, n_fft, np.float64)
    wt = torch.ones(n_fft, dtype=torch.float64) if w is None else torch.from_numpy(w)
    spec = torch.stft(torch.from_numpy(x), n_fft, hop, window=wt, center=center, return_complex=True)
    want = torch.istft(spec, n_fft, hop, window=wt, center=center, length=length).numpy()
    assert np.allclose(np_istft(spec.transpose(-2, -1).numpy(), n_fft, hop, w, center, length), want, atol=1e-10)
    cd = np.complex64 if dtype == np.float32 else np.complex128
    X = dsc.from_numpy(np.ascontiguousarray(spec.transpose(-2, -1).numpy().astype(cd)))
    y = dsc.istft(X, n_fft, hop, None if w is None else dsc.from_numpy(w.astype(dtype)), center, length)
    assert dsc.last_fft_path() == 'istft_ola'
    got = y.numpy()
    assert got.shape == want.shape
    assert rel(got, want) <= TOL[dtype]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n_fft', [64, 1024, 65536])
def test_round_trip(dsc, n_fft, dtype):
    x = np.random.default_rng(n_fft).standard_normal((2, 3 * n_fft + 17)).astype(dtype)
    xt = dsc.from_numpy(x)
    hann = dsc.hann_window(n_fft, dtype=dsc.Dtype.F32 if dtype == np.float32 else dsc.Dtype.F64)
    y = dsc.istft(dsc.stft(xt, n_fft, n_fft // 4, hann), n_fft, n_fft // 4, hann, length=x.shape[-1]).numpy()
    assert rel(y, x) <= TOL[dtype]
    xr = x[:, :3 * n_fft]
    y = dsc.istft(dsc.stft(dsc.from_numpy(xr), n_fft, n_fft, center=False), n_fft, n_fft, center=False).numpy()
    assert rel(y, xr) <= TOL[dtype]


def test_nola_violation_raises(dsc):
    n = 256
    x = dsc.from_numpy(np.random.default_rng(0).standard_normal(4 * n).astype(np.float32))
    hann = dsc.hann_window(n)
    X = dsc.stft(x, n, n, hann, center=False)
    with pytest.raises(ValueError, match='NOLA'):
        dsc.istft(X, n, n, hann, center=False)
    with pytest.raises(ValueError):
        dsc.stft(x, 100, 25)                        # not a power of two
    with pytest.raises(ValueError):
        dsc.stft(x, 2048, 512)                      # T <= n_fft / 2 with reflect padding
    with pytest.raises(ValueError, match='out must be'):
        dsc.stft(x, n, 64, hann, out=dsc.empty((16, n // 2 + 1), dsc.Dtype.C32))   # 17 frames
    with pytest.raises(ValueError, match='out must be'):
        dsc.istft(X, n, n, center=False, out=dsc.empty(4 * n, dsc.Dtype.F64))
    with pytest.raises(ValueError, match='2\\^31'):
        dsc.istft(X, n, n, center=False, length=1 << 31)


def test_windows_equal_torch(dsc):
    import torch
    for n in (1, 8, 255, 1024):
        for periodic in (True, False):
            for name in ('hann', 'hamming', 'blackman'):
                got = getattr(dsc, name + '_window')(n, periodic, dtype=dsc.Dtype.F64).numpy()
                want = getattr(torch, name + '_window')(n, periodic, dtype=torch.float64).numpy()
                assert np.allclose(got, want, rtol=0, atol=1e-14), (name, n, periodic)
            got = dsc.kaiser_window(n, periodic, beta=8.0, dtype=dsc.Dtype.F64).numpy()
            want = torch.kaiser_window(n, periodic, beta=8.0, dtype=torch.float64).numpy()
            assert np.allclose(got, want, rtol=1e-10, atol=1e-14), ('kaiser', n, periodic)
    assert dsc.hann_window(16).numpy().dtype == np.float32


def test_full_size_against_numpy_and_composed(dsc):
    n, hop, rows, T = 1024, 256, 64, 1 << 20
    x = np.random.default_rng(11).standard_normal((rows, T)).astype(np.float32)
    w = make_window('hann', n, np.float32)
    xt, wt = dsc.from_numpy(x), dsc.from_numpy(w)
    X = dsc.stft(xt, n, hop, wt)
    assert dsc.last_fft_path() == 'stft_regs'
    pick = np.random.default_rng(5).choice(rows, 4, replace=False)
    for r in pick:                                  # one row at a time: the slice is a device-side copy of that row
        r = int(r)
        assert rel(X[r:r + 1].numpy()[0], np_stft(x[r], n, hop, w)) <= 1e-5
    os.environ['DSC_NO_STFT_FUSED'] = '1'
    try:
        Xc = dsc.stft(xt, n, hop, wt)
        assert dsc.last_fft_path() == 'stft_composed'
    finally:
        del os.environ['DSC_NO_STFT_FUSED']
    d = dsc.sum(dsc.sum(dsc.absolute(dsc.sub(X, Xc)), axis=-1), axis=-2).numpy()
    s = dsc.sum(dsc.sum(dsc.absolute(X), axis=-1), axis=-2).numpy()
    assert float(np.max(d / s)) <= 1e-5


def test_cpp_stft_templates_on_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_stft_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'stft templates ok' in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
