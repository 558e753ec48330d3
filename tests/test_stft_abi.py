"""CPU tests of dsc_stft / dsc_istft (include/dsc_mi355x.h, Section D): the prototypes are declared, exported and bound, the frame
count and output shapes match torch.stft, and this file's numpy restatement of STFT / ISTFT — the oracle of tests/test_gpu_stft.py —
matches torch.stft / torch.istft in f64."""
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


# ---- the oracle: framing, window, np.fft.rfft; irfft, window, overlap-add, envelope ---------------------------------------------
def np_stft(x, n_fft, hop, window=None, center=True, pad_mode='reflect'):
    """[.., T] -> [.., n_frames, n_fft // 2 + 1] complex128 (frames-major)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    if center:
        pad = n_fft // 2
        x = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode='reflect' if pad_mode == 'reflect' else 'constant')
    n_frames = 1 + (x.shape[-1] - n_fft) // hop
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(x[..., idx] * w, axis=-1)


def np_istft(X, n_fft, hop, window=None, center=True, length=None):
    """[.., n_frames, n_fft // 2 + 1] -> [.., length] float64 (torch.istft semantics)."""
    X = np.asarray(X, dtype=np.complex128)
    w = np.ones(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    n_frames = X.shape[-2]
    frames = np.fft.irfft(X, n=n_fft, axis=-1) * w
    expected = n_fft + hop * (n_frames - 1)
    y = np.zeros(X.shape[:-2] + (expected,))
    env = np.zeros(expected)
    for f in range(n_frames):
        y[..., f * hop:f * hop + n_fft] += frames[..., f, :]
        env[f * hop:f * hop + n_fft] += w * w
    start = n_fft // 2 if center else 0
    end = start + length if length is not None else (expected - n_fft // 2 if center else expected)
    y, env = y[..., start:min(end, expected)], env[start:min(end, expected)]
    assert env.min() >= 1e-11, 'NOLA'
    y = y / env
    if end > expected:
        y = np.concatenate([y, np.zeros(y.shape[:-1] + (end - expected,))], axis=-1)
    return y


def stft_frames(T, n_fft, hop, center):
    return 1 + T // hop if center else 1 + (T - n_fft) // hop


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r'dsc_tensor \*dsc_stft\(dsc_ctx \*ctx, const dsc_tensor \*x, int n_fft, int hop, const dsc_tensor \*window,\s*'
                     r'bool center, int pad_mode, dsc_tensor \*out\);', text)
    assert re.search(r'dsc_tensor \*dsc_istft\(dsc_ctx \*ctx, const dsc_tensor \*X, int n_fft, int hop, const dsc_tensor \*window,\s*'
                     r'bool center, int length, dsc_tensor \*out\);', text)
    lib = ctypes.CDLL(LIB)
    assert lib.dsc_stft and lib.dsc_istft
    from dsc_amd import _bindings
    assert 'dsc_stft' in _bindings.EXPORTS and 'dsc_istft' in _bindings.EXPORTS
    import dsc_amd
    for name in ('stft', 'istft', 'hann_window', 'hamming_window', 'blackman_window', 'kaiser_window'):
        assert callable(getattr(dsc_amd, name))


@pytest.mark.parametrize('T', [3, 33, 64, 65, 100, 257, 1000])
@pytest.mark.parametrize('n_fft', [4, 32, 64])
@pytest.mark.parametrize('hop', [1, 3, 16, 64, 125])
@pytest.mark.parametrize('center', [True, False])
def test_frame_count_and_shape_match_torch(T, n_fft, hop, center):
    torch = pytest.importorskip('torch')
    from dsc_amd import stft_n_frames
    if center and T <= n_fft // 2:
        return
    if not center and T < n_fft:
        return
    x = torch.zeros(2, T, dtype=torch.float64)
    ref = torch.stft(x, n_fft, hop, window=torch.ones(n_fft, dtype=torch.float64), center=center, return_complex=True)
    assert stft_n_frames(T, n_fft, hop, center) == stft_frames(T, n_fft, hop, center) == ref.shape[-1]
    assert np_stft(x.numpy(), n_fft, hop, center=center).shape == tuple(ref.transpose(-2, -1).shape)


@pytest.mark.parametrize('n_fft,hop,center,pad_mode,win', [
    (64, 16, True, 'reflect', 'hann'), (64, 16, True, 'constant', 'rand'), (256, 3, False, 'reflect', 'rand'),
    (32, 64, True, 'reflect', None), (128, 125, True, 'constant', 'kaiser'), (4, 1, True, 'reflect', 'rand')])
def test_numpy_restatement_matches_torch(n_fft, hop, center, pad_mode, win):
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(n_fft + hop)
    w = {None: np.ones(n_fft), 'hann': torch.hann_window(n_fft, dtype=torch.float64).numpy(),
         'kaiser': torch.kaiser_window(n_fft, dtype=torch.float64).numpy(), 'rand': rng.uniform(0.5, 1.5, n_fft)}[win]
    x = rng.standard_normal((3, 3 * n_fft + 5))
    ref = torch.stft(torch.from_numpy(x), n_fft, hop, window=torch.from_numpy(w), center=center, pad_mode=pad_mode,
                     return_complex=True).transpose(-2, -1).numpy()
    got = np_stft(x, n_fft, hop, w, center, pad_mode)
    assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)
    if hop <= n_fft:                                          # NOLA holds
        for length in (None, x.shape[-1], x.shape[-1] + 2 * hop + 1):
            ref_i = torch.istft(torch.from_numpy(ref).transpose(-2, -1), n_fft, hop, window=torch.from_numpy(w), center=center,
                                length=length).numpy()
            got_i = np_istft(ref, n_fft, hop, w, center, length)
            assert got_i.shape == ref_i.shape
            assert np.linalg.norm(got_i - ref_i) <= 1e-12 * np.linalg.norm(ref_i)


def test_nola_envelope_minimum_matches_the_direct_sum():
    """dsc.istft's host-side NOLA check (O(n_fft + hop), periodic middle) against the envelope summed frame by frame."""
    from dsc_amd.tensor import _nola_min
    rng = np.random.default_rng(0)
    for _ in range(1500):
        n = int(2 ** rng.integers(2, 8))
        hop, n_frames = int(rng.integers(1, 3 * n)), int(rng.integers(1, 40))
        w2 = rng.uniform(0, 1, n) ** 2
        if rng.random() < 0.3:
            w2[rng.integers(0, n)] = 0.0
        expected = n + hop * (n_frames - 1)
        start = int(rng.integers(0, expected))
        end = int(rng.integers(start, expected + 50))
        env = np.zeros(expected)
        for f in range(n_frames):
            env[f * hop:f * hop + n] += w2
        want = env[start:min(end, expected)].min() if min(end, expected) > start else np.inf
        got = _nola_min(w2, n, hop, n_frames, start, end)
        assert got == want or abs(got - want) <= 1e-12 * max(1.0, want), (n, hop, n_frames, start, end)


def test_windows_match_torch_on_the_host():
    torch = pytest.importorskip('torch')
    from dsc_amd import tensor as T
    for n in (1, 2, 7, 64):
        for periodic in (True, False):
            assert np.allclose(T._cosine_sum(n, periodic, (0.5, 0.5)), torch.hann_window(n, periodic, dtype=torch.float64).numpy(), atol=1e-15)
            assert np.allclose(T._cosine_sum(n, periodic, (0.42, 0.5, 0.08)),
                               torch.blackman_window(n, periodic, dtype=torch.float64).numpy(), atol=1e-15)


def test_cpp_stft_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_stft_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout
