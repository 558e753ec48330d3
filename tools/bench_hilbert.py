#!/usr/bin/env python3
"""tools/bench_hilbert.py — HIP-event timings of dsc.hilbert and dsc.envelope on 2^26 samples ([2^26 / N, N]) for N = 512 .. 32768, f32 and
f64.  Per case three routes, timed interleaved round by round in one process after a warm-up, each window at least 0.2 s of launches:
  (hand)          the composition a user wrote before: ifft(fft(x) * h), h = 1, 2, .., 2, 1, 0, .., 0 (envelope: absolute of it)
  (call_nofused)  the call with DSC_NO_HILBERT_FUSED=1    hilbert_composed / envelope_composed (the switch is read at every call)
  (call)          the call                                hilbert_regs / envelope_regs
Reported: best ms per call, GB/s of algorithmic bytes (hilbert 3 x, envelope 2 x the input bytes), share of the 8 TB/s roofline, and
the spread (max / min - 1) of every route over the rounds — the noise a difference between routes has to exceed.
--hand-only times (hand) alone and uses nothing newer than dsc.fft / dsc.ifft / dsc.mul / dsc.absolute: it runs on an older build.
--once N: three calls each of hilbert, envelope and the plain fused filter with the same response at that length (f32) and nothing
else, for a profiler: the filter reads x once, so its FETCH_SIZE is the yardstick for the second read of x."""
import argparse
import os
import sys

sys.path.insert(0, '.')
import numpy as np                         # noqa: E402

import dsc_amd as dsc                      # noqa: E402
from dsc_amd import _bindings as B         # noqa: E402
from dsc_amd.context import _get_ctx       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2-samples', type=int, default=26)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--window', type=float, default=0.2, help='seconds of launches per timing')
ap.add_argument('--hand-only', action='store_true')
ap.add_argument('--dtype', choices=('f32', 'f64', 'both'), default='both')
ap.add_argument('--kind', choices=('hilbert', 'envelope', 'both'), default='both')
ap.add_argument('--once', type=int, default=0)
args = ap.parse_args()

dsc.init(8 << 30, 1 << 30)
ctx = _get_ctx()
SWITCH = 'DSC_NO_HILBERT_FUSED'
samples = 1 << args.log2_samples

if args.once:                                             # f32: three calls each of hilbert, envelope and their sibling, the plain fused filter
    N = args.once
    x = dsc.from_numpy(np.random.default_rng(0).standard_normal((samples // N, N), dtype=np.float32))
    hr = np.full(N // 2 + 1, -1j, np.complex64)
    hr[0] = hr[-1] = 0
    H = dsc.from_numpy(hr)
    for _ in range(3):
        y = dsc.hilbert(x)
    p1 = dsc.last_fft_path()
    for _ in range(3):
        y = dsc.envelope(x)
    p2 = dsc.last_fft_path()
    for _ in range(3):
        y = dsc.filter_fft(x, H)
    p3 = dsc.last_fft_path()
    dsc.synchronize()
    print(f'f32 N = {N}, {samples // N} rows: {p1}, {p2}, {p3}; input {samples * 4} bytes, output {samples * 8} / {samples * 4} / {samples * 4} bytes')
    sys.exit(0)


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def set_fused(on):
    if on:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = '1'


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


print(f'2^{args.log2_samples} samples per case; best of {args.rounds} interleaved rounds, each at least {args.window} s of launches', flush=True)
for dname, rb in (('f32', 4), ('f64', 8)):
    if args.dtype not in (dname, 'both'):
        continue
    rdt, cdt = (np.float32, np.complex64) if rb == 4 else (np.float64, np.complex128)
    flat = dsc.from_numpy(np.random.default_rng(0).standard_normal(samples, dtype=rdt))
    for N in (512, 1024, 2048, 4096, 8192, 16384, 32768):
        x = dsc.reshape(flat, samples // N, N)            # a view of the one block of noise: every case reads the same bytes
        hh = np.zeros(N, cdt)
        hh[0] = hh[N // 2] = 1
        hh[1:N // 2] = 2
        h = dsc.from_numpy(hh)
        for kind in ('hilbert', 'envelope'):
            if args.kind not in (kind, 'both'):
                continue
            nbytes = samples * rb * (3 if kind == 'hilbert' else 2)
            if kind == 'hilbert':
                runs = {'hand': ((lambda: dsc.ifft(dsc.mul(dsc.fft(x), h))), True)}
            else:
                runs = {'hand': ((lambda: dsc.absolute(dsc.ifft(dsc.mul(dsc.fft(x), h)))), True)}
            if not args.hand_only:
                call = getattr(dsc, kind)
                runs = {**runs, 'call_nofused': ((lambda: call(x)), False), 'call': ((lambda: call(x)), True)}
            paths = {}
            for name, (f, fused) in runs.items():
                set_fused(fused)
                f()
                paths[name] = 'fft, mul, ifft' + (', abs' if kind == 'envelope' else '') if name == 'hand' else dsc.last_fft_path()
            times = measure(runs)
            label = f'{dname} {kind} {samples // N}x{N}'
            for name in runs:
                ms = min(times[name])
                gbs = nbytes / ms / 1e6
                spread = 100 * (max(times[name]) / ms - 1)
                print(f'{label:28s} {name:13s} {paths[name]:20s} {ms:8.3f} ms  {gbs:7.1f} GB/s  {gbs / 80:5.1f} % of 8 TB/s  spread {spread:4.1f} %', flush=True)
            if not args.hand_only:
                c = min(times['call'])
                print(f'{"":28s} call / hand = {c / min(times["hand"]):.3f}, call / call_nofused = {c / min(times["call_nofused"]):.3f}', flush=True)
        del x, h
    del flat
