#!/usr/bin/env python3
"""tools/bench_resample.py — HIP-event timings of dsc.decimate, dsc.resample_poly and dsc.upfirdn (the direct polyphase kernel,
polyphase.hip) on [64, 2^20], f32 and f64, written to profiles/resample_bench.txt.  Per case two routes, timed interleaved round by round
in one process after a warm-up, each window at least 0.2 s of launches:
  (call)  the operator                                   polyphase_direct
  (hand)  the composition a user writes without it, with nothing newer than convolve, slicing and set_slice:
            up == 1   convolve(x, h, 'same')[:, ::down]
            up  > 1   z[:, ::up] = x into a zero-filled [64, 2^20 up] buffer (zeroed once, outside the timing), then
                      convolve(z, h up, 'same')[:, ::down]
          160 / 147 and 147 / 160 have no (hand) row: the zero-stuffed buffer would hold 64 x 2^20 x 160 (147) samples, more than a
          tensor can (2^31 - 1 elements).
  upfirdn at 1 / 1 (M = 15, 63, 255) is the "direct route for short filters" question of DESIGN 4.6: its (hand) row is
  convolve(x, h, 'full'), the fused overlap-save route conv_regs.
Reported: best ms per call, share of the 8 TB/s roofline on algorithmic bytes (x read once, y written once, the taps), FMAs per output
(K = ceil(M / up)), the spread (max / min - 1) over the rounds, and call / hand."""
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
ap.add_argument('--log2-t', type=int, default=20)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--window', type=float, default=0.2, help='seconds of launches per timing')
ap.add_argument('--dtype', choices=('f32', 'f64', 'both'), default='both')
ap.add_argument('--out', default=os.path.join('profiles', 'resample_bench.txt'))
args = ap.parse_args()

dsc.init(20 << 30, 1 << 30)
ctx = _get_ctx()
rows, T = args.rows, 1 << args.log2_t
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def measure(runs):
    reps, times = {}, {k: [] for k in runs}
    for name, f in runs.items():                          # warm-up: code objects, plans, clocks; then size the window
        for _ in range(3):
            f()
        dsc.synchronize()
        reps[name] = max(3, int(args.window * 1e3 / events(f, 3)) + 1)
    for _ in range(args.rounds):
        for name, f in runs.items():
            times[name].append(events(f, reps[name]))
    return times


def report(label, runs, paths, nbytes, K):
    times = measure(runs)
    for name in runs:
        ms = min(times[name])
        gbs = nbytes / ms / 1e6
        spread = 100 * (max(times[name]) / ms - 1)
        say(f'{label:34s} {name:5s} {paths[name]:28s} {ms:8.3f} ms  {gbs / 80:5.1f} % of 8 TB/s  {K:4d} FMA / output  spread {spread:4.1f} %')
    if 'hand' in runs:
        say(f'{"":34s} call / hand = {min(times["call"]) / min(times["hand"]):.3f}')


say(f'[{rows}, 2^{args.log2_t}] per case; best of {args.rounds} interleaved rounds, each at least {args.window} s of launches')
for dname, rb in (('f32', 4), ('f64', 8)):
    if args.dtype not in (dname, 'both'):
        continue
    rdt = np.float32 if rb == 4 else np.float64
    ddt = dsc.Dtype.F32 if rb == 4 else dsc.Dtype.F64
    x = dsc.from_numpy(np.random.default_rng(0).standard_normal((rows, T), dtype=rdt))

    def rate_case(label, up, down, h, call):
        """h: the taps the operator designs (a Tensor); call: the operator"""
        M = h.shape[0]
        T_out = -(-T * up // down)
        nbytes = (rows * T + rows * T_out + M) * rb
        runs, paths = {'call': call}, {}
        call()
        paths['call'] = dsc.last_fft_path()
        z = None
        if rows * T * up <= 0x7fffffff:
            if up == 1:
                runs['hand'] = lambda: dsc.convolve(x, h, 'same')[:, ::down]
                paths['hand'] = 'convolve, slice'
            else:
                z = dsc.from_numpy(np.zeros((rows, T * up), dtype=rdt))
                hg = dsc.from_numpy(h.numpy() * rdt(up))

                def hand():
                    z[:, ::up] = x
                    return dsc.convolve(z, hg, 'same')[:, ::down]
                runs['hand'] = hand
                paths['hand'] = 'set_slice, convolve, slice'
            got, want = call().numpy()[:2], runs['hand']().numpy()[:2]
            err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            assert got.shape == want.shape and err < (1e-4 if rb == 4 else 1e-11), (label, got.shape, want.shape, err)
        report(f'{dname} {label}', runs, paths, nbytes, -(-M // up))
        del z

    for q in (2, 4, 8):
        rate_case(f'decimate q={q}', 1, q, dsc.firwin(20 * q + 1, 1.0 / q, 'hamming', dtype=ddt), lambda q=q: dsc.decimate(x, q))
    for up, down in ((2, 1), (4, 1), (3, 2), (2, 3), (160, 147), (147, 160)):
        r = max(up, down)
        rate_case(f'resample_poly {up}/{down}', up, down, dsc.firwin(20 * r + 1, 1.0 / r, 'kaiser', 5.0, ddt),
                  lambda up=up, down=down: dsc.resample_poly(x, up, down))
    for M in (15, 63, 255):
        h = dsc.from_numpy(np.random.default_rng(M).standard_normal(M).astype(rdt))
        runs = {'call': lambda h=h: dsc.upfirdn(h, x, 1, 1), 'hand': lambda h=h: dsc.convolve(x, h, 'full')}
        paths = {}
        for name, f in runs.items():
            f()
            paths[name] = dsc.last_fft_path()
        report(f'{dname} upfirdn 1/1 M={M}', runs, paths, (rows * T + rows * (T + M - 1) + M) * rb, M)
    del x

if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
