#!/usr/bin/env python3
"""tools/bench_stft.py — HIP-event timings of dsc.stft / dsc.istft on [64, 2^20] f32 with a Hann window, hop = n_fft / 4, n_fft in
{256, 1024, 4096}.  The forward routes stft_regs (fused) and stft_composed (DSC_NO_STFT_FUSED) are timed interleaved, round by round,
in one process.  Roofline share on algorithmic bytes against 8 TB/s: forward = input read once + bins written once, inverse = bins
read once + samples written once."""
import argparse
import os
import sys

sys.path.insert(0, '.')
import numpy as np                         # noqa: E402

import dsc_amd as dsc                      # noqa: E402
from dsc_amd import _bindings as B         # noqa: E402
from dsc_amd.context import _get_ctx       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--log2t', type=int, default=20)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--rounds', type=int, default=3)
args = ap.parse_args()

dsc.init(24 << 30, 4 << 30)
ctx = _get_ctx()
rows, T = args.rows, 1 << args.log2t


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def set_route(fused):
    if fused:
        os.environ.pop('DSC_NO_STFT_FUSED', None)
    else:
        os.environ['DSC_NO_STFT_FUSED'] = '1'


def report(name, ms, nbytes):
    gbs = nbytes / ms / 1e6
    print(f'{name:40s} {ms:9.3f} ms  {gbs:8.1f} GB/s  {gbs / 80:5.1f} % of 8 TB/s', flush=True)


x = dsc.from_numpy(np.random.default_rng(0).standard_normal((rows, T)).astype(np.float32))
print(f'x = [{rows}, 2^{args.log2t}] f32, Hann window, hop = n_fft / 4; best of {args.rounds} interleaved rounds of {args.reps} calls', flush=True)
for n_fft in (256, 1024, 4096):
    hop = n_fft // 4
    w = dsc.hann_window(n_fft)
    frames = 1 + T // hop
    X = dsc.stft(x, n_fft, hop, w)
    fwd_bytes = rows * T * 4 + rows * frames * (n_fft // 2 + 1) * 8
    inv_bytes = rows * frames * (n_fft // 2 + 1) * 8 + rows * T * 4
    y = dsc.empty((rows, T), dsc.Dtype.F32)
    runs = {'stft_regs': lambda: dsc.stft(x, n_fft, hop, w, out=X), 'stft_composed': lambda: dsc.stft(x, n_fft, hop, w, out=X),
            'istft_ola': lambda: dsc.istft(X, n_fft, hop, w, length=T, out=y)}
    best = {k: 1e30 for k in runs}
    for name, f in runs.items():                           # warm-up: plans, clocks
        set_route(name != 'stft_composed')
        for _ in range(3):
            f()
        dsc.synchronize()
    for _ in range(args.rounds):
        for name, f in runs.items():
            set_route(name != 'stft_composed')
            best[name] = min(best[name], events(f, args.reps))
            assert dsc.last_fft_path() == name, dsc.last_fft_path()
    set_route(True)
    report(f'stft  n_fft {n_fft:5d} stft_regs', best['stft_regs'], fwd_bytes)
    report(f'stft  n_fft {n_fft:5d} stft_composed', best['stft_composed'], fwd_bytes)
    print(f'{"":40s} fused / composed = {best["stft_regs"] / best["stft_composed"]:.3f}', flush=True)
    report(f'istft n_fft {n_fft:5d} istft_ola', best['istft_ola'], inv_bytes)
    del X, y
