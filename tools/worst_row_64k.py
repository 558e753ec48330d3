#!/usr/bin/env python3
# usage: [DSC_MI355X_LIB=<build>.so] tools/worst_row_64k.py [--save DIR]
# The worst row (rel-L2 against float64 numpy) of the five operators that share
# three_passes() of fft_64k_common.h, on 300 seeded rows; DSC_MI355X_LIB selects the build.  --save writes the raw outputs to
# DIR/<op>.npy (to compare two builds bit by bit).
import os
import sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
fd = os.dup(1); os.dup2(2, 1)
import dsc_amd as dsc
dsc.init(6 << 30, 1 << 30)
os.dup2(fd, 1)
save = sys.argv[sys.argv.index('--save') + 1] if '--save' in sys.argv else None
N, M, R = 65536, 32768, 300
rng = np.random.default_rng(300)
x = rng.standard_normal((R, N)).astype(np.float32)
Y = (rng.standard_normal((R, M + 1)) + 1j * rng.standard_normal((R, M + 1))).astype(np.complex64)
H = (rng.standard_normal(M + 1) + 1j * rng.standard_normal(M + 1)).astype(np.complex64)
z = (rng.standard_normal((R, M)) + 1j * rng.standard_normal((R, M))).astype(np.complex64)


def real_ends(S):
    S = S.astype(np.complex128)
    S[..., 0] = S[..., 0].real
    S[..., -1] = S[..., -1].real
    return S


cases = {
    'rfft': (lambda: dsc.rfft(dsc.from_numpy(x)), lambda: np.fft.rfft(x.astype(np.float64), axis=-1)),
    'irfft': (lambda: dsc.irfft(dsc.from_numpy(Y)), lambda: np.fft.irfft(real_ends(Y), n=N, axis=-1)),
    'filter': (lambda: dsc.filter_fft(dsc.from_numpy(x), dsc.from_numpy(H)),
               lambda: np.fft.irfft(real_ends(np.fft.rfft(x.astype(np.float64), axis=-1) * H.astype(np.complex128)), n=N, axis=-1)),
    'fft': (lambda: dsc.fft(dsc.from_numpy(z)), lambda: np.fft.fft(z.astype(np.complex128), axis=-1)),
    'ifft': (lambda: dsc.ifft(dsc.from_numpy(z)), lambda: np.fft.ifft(z.astype(np.complex128), axis=-1)),
}
for name, (run, ref) in cases.items():
    got = run().numpy()
    path = dsc.last_fft_path()
    want = ref()
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f'{name} ({path}): worst row {int(err.argmax())} of {R}: rel-L2 {err.max():.4e}, mean over rows {err.mean():.4e}', flush=True)
    if save:
        os.makedirs(save, exist_ok=True)
        np.save(os.path.join(save, name + '.npy'), got)
