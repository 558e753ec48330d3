#!/usr/bin/env python3
"""tools/bench_fft2.py — HIP-event timings of dsc.fft2 (complex input) and dsc.rfft2 (real input) on [batch, N0, N1] tensors of about
1 GiB of input, f32 and f64: every size of the fused windows (N0, N1 in 32 / 64 / 128; rfft2: N1 in 64 / 128 / 256) plus 256 x 256 and
512 x 512 (composed).  Per case three routes, timed interleaved round by round in one process after a warm-up, each window at least
0.2 s of launches:
  (a) the call                                   fft2_regs / rfft2_regs where fused
  (b) the call with DSC_NO_FFT2_FUSED=1          fft2_composed / rfft2_composed (the switch is read at every call)
  (c) the hand composition fft(fft(x, axis=-1), axis=-2) (rfft2: fft(rfft(x, axis=-1), axis=-2)): what a user wrote before
Reported: best ms per call, GB/s of algorithmic bytes (input once + output once), share of the 8 TB/s roofline, and the spread
(max / min - 1) of (c) over the rounds — the noise a difference between routes has to exceed.
--hand-only times (c) alone and uses nothing newer than dsc.fft / dsc.rfft: run that on the parent commit's build for the yardstick."""
import argparse
import os
import sys

sys.path.insert(0, '.')
import numpy as np                         # noqa: E402

import dsc_amd as dsc                      # noqa: E402
from dsc_amd import _bindings as B         # noqa: E402
from dsc_amd.context import _get_ctx       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--gib', type=float, default=1.0, help='input size per case')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--window', type=float, default=0.2, help='seconds of launches per timing')
ap.add_argument('--hand-only', action='store_true')
ap.add_argument('--dtype', choices=('f32', 'f64', 'both'), default='both')
ap.add_argument('--kind', choices=('fft2', 'rfft2', 'both'), default='both')
args = ap.parse_args()

dsc.init(24 << 30, 4 << 30)
ctx = _get_ctx()


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def set_fused(on):
    if on:
        os.environ.pop('DSC_NO_FFT2_FUSED', None)
    else:
        os.environ['DSC_NO_FFT2_FUSED'] = '1'


def measure(runs):
    """runs: name -> (callable, fused switch).  Per-call ms of every round, routes alternating."""
    reps, times = {}, {k: [] for k in runs}
    for name, (f, fused) in runs.items():                 # warm-up: code objects, plans, clocks; then size the window
        set_fused(fused)
        for _ in range(3):
            f()
        dsc.synchronize()
        reps[name] = max(3, int(args.window * 1e3 / events(f, 3)) + 1)
    for _ in range(args.rounds):
        for name, (f, fused) in runs.items():
            set_fused(fused)
            times[name].append(events(f, reps[name]))
    set_fused(True)
    return times


def report(label, name, path, ms, nbytes):
    gbs = nbytes / ms / 1e6
    print(f'{label:24s} {name:12s} {path:15s} {ms:8.3f} ms  {gbs:7.1f} GB/s  {gbs / 80:5.1f} % of 8 TB/s', flush=True)


print(f'about {args.gib} GiB of input per case; best of {args.rounds} interleaved rounds, each at least {args.window} s of launches', flush=True)
sizes = {'fft2': [(a, b) for a in (32, 64, 128) for b in (32, 64, 128)] + [(256, 256), (512, 512)],
         'rfft2': [(a, b) for a in (32, 64, 128) for b in (64, 128, 256)] + [(256, 256), (512, 512)]}
for dname, rdt, rb in (('f32', dsc.Dtype.F32, 4), ('f64', dsc.Dtype.F64, 8)):
    if args.dtype not in (dname, 'both'):
        continue
    n_real = int(args.gib * (1 << 30)) // rb
    noise = np.random.default_rng(0).standard_normal(n_real, dtype=np.float32 if rb == 4 else np.float64)
    flat = {'rfft2': dsc.from_numpy(noise), 'fft2': dsc.from_numpy(noise.view(np.complex64 if rb == 4 else np.complex128))}
    del noise
    for kind in ('fft2', 'rfft2'):
        if args.kind not in (kind, 'both'):
            continue
        eb = rb if kind == 'rfft2' else 2 * rb
        for N0, N1 in sizes[kind]:
            batch = max(1, int(args.gib * (1 << 30)) // (N0 * N1 * eb))
            x = dsc.reshape(flat[kind], batch, N0, N1)    # a view of the one block of noise: every case reads the same bytes
            out_cols = N1 // 2 + 1 if kind == 'rfft2' else N1
            nbytes = batch * N0 * N1 * eb + batch * N0 * out_cols * 2 * rb
            first = dsc.rfft if kind == 'rfft2' else dsc.fft
            runs = {'hand': ((lambda: dsc.fft(first(x, axis=-1), axis=-2)), True)}
            if not args.hand_only:
                call = dsc.rfft2 if kind == 'rfft2' else dsc.fft2
                runs = {'call': ((lambda: call(x)), True), 'call_nofused': ((lambda: call(x)), False), **runs}
            paths = {}
            for name, (f, fused) in runs.items():
                set_fused(fused)
                f()
                paths[name] = dsc.last_fft_path()
            times = measure(runs)
            label = f'{dname} {kind} {batch}x{N0}x{N1}'
            for name in runs:
                report(label, name, paths[name], min(times[name]), nbytes)
            h = times['hand']
            line = f'{"":24s} spread of hand over the rounds {100 * (max(h) / min(h) - 1):.1f} %'
            if not args.hand_only:
                line += f'; call / hand = {min(times["call"]) / min(h):.3f}, call / call_nofused = {min(times["call"]) / min(times["call_nofused"]):.3f}'
            print(line, flush=True)
            del x
    del flat
