"""CPU tests of dsc_convolve / dsc_correlate (include/dsc_mi355x.h, Section E): the prototypes are declared, exported and bound, this
file's numpy FFT restatement — the oracle of tests/test_gpu_conv.py — matches np.convolve / np.correlate, and a restatement of the
overlap-save block plan of dsc_amd/csrc/conv.cpp covers every output sample exactly once."""
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
MODES = ('full', 'same', 'valid')


# ---- the oracle: one f64 FFT per row, long enough for the whole linear convolution --------------------------------------------
def conv_span(T, M, mode):
    """(n0, T_out): the result is np.convolve(x, h, 'full')[n0 : n0 + T_out]."""
    return {'full': (0, T + M - 1), 'same': ((M - 1) // 2, T), 'valid': (M - 1, T - M + 1)}[mode]


def np_convolve_fft(x, h, mode='full', correlate=False):
    """[.., T] x [M] -> [.., T_out] float64."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if correlate:
        h = h[::-1]
    T, M = x.shape[-1], h.shape[0]
    n = 1 << int(np.ceil(np.log2(T + M - 1)))
    y = np.fft.irfft(np.fft.rfft(x, n, axis=-1) * np.fft.rfft(h, n), n, axis=-1)
    n0, T_out = conv_span(T, M, mode)
    return y[..., n0:n0 + T_out]


# ---- the block plan of conv.cpp ------------------------------------------------------------------------------------------------
SAMPLE_COST = {np.float32: (3.71, 2.97, 2.24, 2.19, 2.43, 2.94, 2.66),      # kSampleCost of conv.cpp, n = 512 .. 32768
               np.float64: (6.12, 4.61, 4.00, 4.42, 4.84, 6.80, 6.16)}
F64_NO_SPILL_MAX_N = 8192


def conv_block_n(D, T_out, n_max=32768, dtype=np.float32):
    n_min = 512
    while n_min < 2 * D:
        n_min *= 2
    n_max = max(n_max, n_min)
    if dtype == np.float64 and n_min <= F64_NO_SPILL_MAX_N < n_max:
        n_max = F64_NO_SPILL_MAX_N
    best, best_cost, n = n_min, None, n_min
    while n <= n_max:
        c = SAMPLE_COST[dtype][n.bit_length() - 10] if n <= 32768 else n.bit_length() - 1
        cost = c * n / (n - D)
        if best_cost is None or cost < best_cost:
            best, best_cost = n, cost
        n *= 2
    if T_out + D <= best:
        best = n_min
        while best < T_out + D:
            best *= 2
    return best


def conv_plan(T, M, mode, dtype=np.float32):
    """n (block), D (discard), hop, blocks per row, n0, T_out of dsc_convolve; block b reads x[n0 + b hop - D + i], i < n, and keeps
    samples [D, n) as out[b hop + j - D]."""
    n0, T_out = conv_span(T, M, mode)
    D = (M - 1) + ((M - 1) & 1)
    n = conv_block_n(D, T_out, 32768 if D <= 16384 else 1 << 20, dtype)
    hop = n - D
    return dict(n=n, D=D, hop=hop, n_blocks=-(-T_out // hop), n0=n0, T_out=T_out)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared_exported_and_bound():
    text = open(HEADER).read()
    for name in ('dsc_convolve', 'dsc_correlate'):
        assert re.search(name + r'\(dsc_ctx \*ctx, const dsc_tensor \*x, const dsc_tensor \*h, int mode, dsc_tensor \*out\);', text)
    lib = ctypes.CDLL(LIB)
    assert lib.dsc_convolve and lib.dsc_correlate
    from dsc_amd import _bindings
    assert 'dsc_convolve' in _bindings.EXPORTS and 'dsc_correlate' in _bindings.EXPORTS
    import dsc_amd
    assert callable(dsc_amd.convolve) and callable(dsc_amd.correlate)
    assert 'convolve' in dsc_amd.__all__ and 'correlate' in dsc_amd.__all__


@pytest.mark.parametrize('M', [1, 2, 3, 4, 16, 63])
@pytest.mark.parametrize('T', [1, 5, 64, 101])
@pytest.mark.parametrize('mode', MODES)
def test_fft_oracle_matches_numpy(T, M, mode):
    rng = np.random.default_rng(T * 100 + M)
    x, h = rng.standard_normal((3, T)), rng.standard_normal(M)
    got, got_c = np_convolve_fft(x, h, mode), np_convolve_fft(x, h, mode, correlate=True)
    if mode == 'valid' and M > T:
        return
    for r in range(3):
        full = np.convolve(x[r], h, 'full')
        n0, T_out = conv_span(T, M, mode)
        assert np.allclose(got[r], full[n0:n0 + T_out], rtol=0, atol=1e-12)
        full_c = np.correlate(x[r], h, 'full')
        assert np.allclose(got_c[r], full_c[n0:n0 + T_out], rtol=0, atol=1e-12)
        if M <= T:                                     # numpy's own mode semantics
            assert np.allclose(got[r], np.convolve(x[r], h, mode), rtol=0, atol=1e-12)
            assert np.allclose(got_c[r], np.correlate(x[r], h, mode), rtol=0, atol=1e-12)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('mode', MODES)
def test_block_plan_covers_the_output_once(mode, dtype):
    for T in (1, 2, 7, 300, 511, 4097, 65537, 300007, 1 << 20):
        for M in (1, 2, 3, 16, 63, 255, 256, 1000, 4095, 4097, 8193, 16383, 16385, 40000):
            if mode == 'valid' and M > T:
                continue
            p = conv_plan(T, M, mode, dtype)
            n, D, hop, nb, n0, T_out = (p[k] for k in ('n', 'D', 'hop', 'n_blocks', 'n0', 'T_out'))
            assert D % 2 == 0 and hop % 2 == 0 and D >= M - 1 and 2 * D <= n and n & (n - 1) == 0 and n >= 512
            assert (n <= 32768) == (D <= 16384)
            kept = [(b * hop, min(b * hop + hop, T_out)) for b in range(nb)]
            assert kept[0][0] == 0 and kept[-1][1] == T_out                  # union [0, T_out) ...
            assert all(a[1] == b[0] for a, b in zip(kept, kept[1:]))         # ... without gaps or overlaps
            assert all(a < b for a, b in kept)                               # no empty block
            if T_out + D <= n:
                assert nb == 1
            if dtype == np.float64 and D <= 4096:                      # no spilling f64 block size where a smaller one holds D
                assert n <= 8192


def test_block_plan_sample_by_sample():
    """Running the plan with numpy (circular convolution per block, keep [D, n)) reproduces the linear convolution."""
    rng = np.random.default_rng(1)
    for T, M, mode in ((3000, 255, 'full'), (2049, 256, 'same'), (5000, 63, 'valid'), (700, 1000, 'full'), (9000, 1, 'same')):
        x, h = rng.standard_normal(T), rng.standard_normal(M)
        p = conv_plan(T, M, mode)
        n, D, hop = p['n'], p['D'], p['hop']
        H = np.fft.rfft(h, n)
        out = np.full(p['T_out'], np.nan)
        for b in range(p['n_blocks']):
            s = p['n0'] + b * hop - D
            idx = np.arange(s, s + n)
            frame = np.where((idx >= 0) & (idx < T), x[np.clip(idx, 0, T - 1)], 0.0)
            y = np.fft.irfft(np.fft.rfft(frame) * H, n)
            o = b * hop + np.arange(D, n) - D
            keep = o < p['T_out']
            assert np.all(np.isnan(out[o[keep]]))
            out[o[keep]] = y[D:][keep]
        assert np.allclose(out, np_convolve_fft(x, h, mode), rtol=0, atol=1e-10)


def test_cpp_conv_smoke_compiles_and_links(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_conv_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout
