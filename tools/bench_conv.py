#!/usr/bin/env python3
"""tools/bench_conv.py — HIP-event timings of dsc.convolve (full mode) on [64, 2^20] f32 and f64, M in {15, 63, 255, 1023, 4095, 16383}:
(a) conv_regs, (b) conv_composed (DSC_NO_CONV_FUSED, read at every call), (c) what a user writes today: rfft(x, 2^21), mul by H,
irfft, crop.  The three are timed interleaved, round by round, in one process.  Roofline share on algorithmic bytes against 8 TB/s:
x read once + out written once + h.  --sweep: conv_regs at every block size n (DSC_CONV_N) for a few M, which backs the block rule
of dsc_amd/csrc/conv.cpp (--dtype f32 / f64).  After the full-mode table, two cases whose blocks load sample by sample: valid
mode with even M (every block starts on an odd element) and odd T (every other row does)."""
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
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--sweep', action='store_true')
ap.add_argument('--dtype', choices=('f32', 'f64'), default='f32', help='--sweep only')
args = ap.parse_args()

dsc.init(24 << 30, 4 << 30)
ctx = _get_ctx()
rows, T = args.rows, 1 << args.log2t


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def set_env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def report(name, ms, nbytes):
    gbs = nbytes / ms / 1e6
    print(f'{name:44s} {ms:9.3f} ms  {gbs:8.1f} GB/s  {gbs / 80:5.1f} % of 8 TB/s', flush=True)


def best_of(runs, route_env):
    """runs: name -> callable; route_env: name -> (env var, value).  Best per-call time of each over interleaved rounds."""
    best = {k: 1e30 for k in runs}
    for name, f in runs.items():                           # warm-up: plans, clocks
        set_env(*route_env[name])
        for _ in range(2):
            f()
        dsc.synchronize()
    for _ in range(args.rounds):
        for name, f in runs.items():
            set_env(*route_env[name])
            best[name] = min(best[name], events(f, args.reps))
    for var, _ in route_env.values():
        set_env(var, None)
    return best


if args.sweep:
    sdt, snp, srb = (dsc.Dtype.F32, np.float32, 4) if args.dtype == 'f32' else (dsc.Dtype.F64, np.float64, 8)
    print(f'x = [{rows}, 2^{args.log2t}] {args.dtype}, full mode, conv_regs at every block size n; best of {args.rounds} interleaved rounds '
          f'of {args.reps} calls', flush=True)
    x = dsc.from_numpy(np.random.default_rng(0).standard_normal((rows, T)).astype(snp))
    for M in (63, 1023, 4095):
        h = dsc.from_numpy(np.random.default_rng(M).standard_normal(M).astype(snp))
        y = dsc.empty((rows, T + M - 1), sdt)
        D = (M - 1) + ((M - 1) & 1)
        ns = [n for n in (512, 1024, 2048, 4096, 8192, 16384, 32768) if n >= 2 * D]
        runs = {n: (lambda: dsc.convolve(x, h, out=y)) for n in ns}
        best = best_of(runs, {n: ('DSC_CONV_N', str(n)) for n in ns})
        nbytes = (rows * T + rows * (T + M - 1) + M) * srb
        for n in ns:
            import math
            rule = n * math.log2(n) / (n - D)
            report(f'M {M:5d} n {n:5d} (n log2 n / hop = {rule:5.2f})', best[n], nbytes)
        del y
    sys.exit(0)

for dt, npdt, rb in ((dsc.Dtype.F32, np.float32, 4), (dsc.Dtype.F64, np.float64, 8)):
    print(f'x = [{rows}, 2^{args.log2t}] {npdt.__name__}, full mode; best of {args.rounds} interleaved rounds of {args.reps} calls', flush=True)
    x = dsc.from_numpy(np.random.default_rng(0).standard_normal((rows, T)).astype(npdt))
    n_user = 1 << (args.log2t + 1)
    for M in (15, 63, 255, 1023, 4095, 16383):
        h = dsc.from_numpy(np.random.default_rng(M).standard_normal(M).astype(npdt))
        T_out = T + M - 1
        y = dsc.empty((rows, T_out), dt)
        H = dsc.rfft(h, n=n_user)

        def user():
            Y = dsc.irfft(dsc.mul(dsc.rfft(x, n=n_user), H))
            return Y[:, :T_out]

        runs = {'conv_regs': lambda: dsc.convolve(x, h, out=y), 'conv_composed': lambda: dsc.convolve(x, h, out=y), 'user_rfft_mul_irfft': user}
        route = {'conv_regs': ('DSC_NO_CONV_FUSED', None), 'conv_composed': ('DSC_NO_CONV_FUSED', '1'), 'user_rfft_mul_irfft': ('DSC_NO_CONV_FUSED', None)}
        best = best_of(runs, route)
        nbytes = rows * T * rb + rows * T_out * rb + M * rb
        for name in runs:
            report(f'{npdt.__name__} M {M:5d} {name}', best[name], nbytes)
        print(f'{"":44s} regs / composed = {best["conv_regs"] / best["conv_composed"]:.3f}, regs / user = '
              f'{best["conv_regs"] / best["user_rfft_mul_irfft"]:.3f}', flush=True)
        del y, H
    # the sample-by-sample load: valid mode with even M (every block starts on an odd element), and odd rows (every other row does)
    for M, mode, Tm in ((256, 'valid', T), (255, 'full', T + 1)):
        xm = dsc.from_numpy(np.random.default_rng(1).standard_normal((rows, Tm)).astype(npdt))
        h = dsc.from_numpy(np.random.default_rng(M).standard_normal(M).astype(npdt))
        T_out = Tm + M - 1 if mode == 'full' else Tm - M + 1
        y = dsc.empty((rows, T_out), dt)
        best = best_of({'conv_regs': lambda: dsc.convolve(xm, h, mode, out=y)}, {'conv_regs': ('DSC_NO_CONV_FUSED', None)})
        report(f'{npdt.__name__} M {M:5d} {mode} T {Tm} conv_regs', best['conv_regs'], (rows * Tm + rows * T_out + M) * rb)
        del xm, y
    del x
