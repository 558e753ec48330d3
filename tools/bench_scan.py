#!/usr/bin/env python3
"""tools/bench_scan.py — HIP-event timings of dsc.cumsum, dsc.diff, dsc.unwrap and dsc.phase (scan.hip), written to
profiles/scan_bench.txt.  2^26 elements per case, viewed as [8192, 8192], [64, 2^20], [1, 2^26] (last axis) and [4096, 64, 256] (axis 1),
f32 and f64 (phase: c32 and c64 in).  Per case the routes are timed interleaved round by round in one process after a warm-up, each
window at least --window seconds of launches:
  (call)   the operator on the route the library picks
  (rows)   inner == 1 with fewer rows than the crossover: DSC_SCAN_ROUTE=rows, the one-launch route forced onto the few rows
  (tiles)  inner == 1 where the library picks scan_rows: DSC_SCAN_ROUTE=tiles
  (angle)  dsc.angle on the same input: the project's measured streaming rate for one read and one write of the same bytes
  (comp)   phase only: the two-operator composition dsc.unwrap(dsc.angle(z))
Then the crossover sweep: cumsum and unwrap f32 on [rows, 2^26 / rows] for rows = 16 .. 512, both routes forced.
Reported: best ms per call, share of the 8 TB/s roofline on algorithmic bytes (one read and one write; the read is complex for phase),
the spread (max / min - 1) over the rounds."""
import argparse
import os
import sys

sys.path.insert(0, '.')
import numpy as np                         # noqa: E402

import dsc_amd as dsc                      # noqa: E402
from dsc_amd import _bindings as B         # noqa: E402
from dsc_amd.context import _get_ctx       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2-n', type=int, default=26)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--window', type=float, default=0.1, help='seconds of launches per timing')
ap.add_argument('--dtype', choices=('f32', 'f64', 'both'), default='both')
ap.add_argument('--out', default=os.path.join('profiles', 'scan_bench.txt'))
args = ap.parse_args()

dsc.init(12 << 30, 1 << 28)
ctx = _get_ctx()
N = 1 << args.log2_n
side = 1 << (args.log2_n // 2)
SHAPES = [((side, N // side), -1), ((64, N // 64), -1), ((1, N), -1), ((N // (64 * 256), 64, 256), 1)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def forced(route, f):
    def g():
        if route is None:
            os.environ.pop('DSC_SCAN_ROUTE', None)
        else:
            os.environ['DSC_SCAN_ROUTE'] = route
        r = f()
        os.environ.pop('DSC_SCAN_ROUTE', None)
        return r
    return g


def measure(runs):
    reps, times, paths = {}, {k: [] for k in runs}, {}
    for name, f in runs.items():                          # warm-up: code objects, clocks; then size the window
        for _ in range(3):
            f()
        paths[name] = dsc.last_fft_path() if name != 'angle' else 'unary_kernel'
        dsc.synchronize()
        reps[name] = max(3, int(args.window * 1e3 / events(f, 3)) + 1)
    for _ in range(args.rounds):
        for name, f in runs.items():
            times[name].append(events(f, reps[name]))
    return times, paths


def report(label, runs, nbytes):
    times, paths = measure(runs)
    for name in runs:
        ms = min(times[name])
        spread = 100 * (max(times[name]) / ms - 1)
        say(f'{label:36s} {name:6s} {paths[name]:12s} {ms:8.3f} ms  {nbytes[name] / ms / 1e6 / 80:5.1f} % of 8 TB/s  spread {spread:4.1f} %')
    return {name: min(t) for name, t in times.items()}


say(f'2^{args.log2_n} elements per case; best of {args.rounds} interleaved rounds, each at least {args.window} s of launches')
rng = np.random.default_rng(0)
steps = rng.uniform(0.0, 2.5, N)
true_phase = np.cumsum(steps)
del steps
wrapped64 = np.mod(true_phase + np.pi, 2 * np.pi) - np.pi
for dname, rb in (('f32', 4), ('f64', 8)):
    if args.dtype not in (dname, 'both'):
        continue
    rdt, cdt = (np.float32, np.complex64) if rb == 4 else (np.float64, np.complex128)
    data = {'cumsum': dsc.from_numpy(rng.standard_normal(N).astype(rdt)), 'unwrap': dsc.from_numpy(wrapped64.astype(rdt))}
    data['diff'] = data['cumsum']
    z = np.empty(N, cdt)
    z.real, z.imag = np.cos(wrapped64), np.sin(wrapped64)
    data['phase'] = dsc.from_numpy(z)
    del z
    for shape, axis in SHAPES:
        outer = int(np.prod(shape[:axis % len(shape)]))
        inner = int(np.prod(shape[axis % len(shape) + 1:]))
        for op in ('cumsum', 'diff', 'unwrap', 'phase'):
            x = dsc.reshape(data[op], *shape)
            f = getattr(dsc, op)
            n_out = N - outer * inner if op == 'diff' else N
            in_b = 2 * rb if op == 'phase' else rb
            nb = N * in_b + n_out * rb
            runs = {'call': forced(None, lambda: f(x, axis=axis))}
            nbytes = {'call': nb, 'rows': nb, 'tiles': nb, 'comp': nb, 'angle': N * in_b + N * rb}
            if op != 'diff' and inner == 1:
                runs['call']()
                other = 'rows' if dsc.last_fft_path() == 'scan_tiles' else 'tiles'
                runs[other] = forced(other, lambda: f(x, axis=axis))
            if op == 'phase':
                runs['comp'] = forced(None, lambda: dsc.unwrap(dsc.angle(x), axis=axis))
            runs['angle'] = lambda: dsc.angle(x)
            report(f'{dname} {op} {list(shape)} axis {axis}', runs, nbytes)
            del x
    if rb == 4:
        say('crossover: [rows, 2^%d / rows], last axis, both routes forced; tiles / rows below 1 = scan_tiles is faster' % args.log2_n)
        for op in ('cumsum', 'unwrap'):
            for rows in (16, 64, 128, 192, 256, 384, 512):
                n = N // rows // 4 * 4
                flat = dsc.reshape(data[op], N)
                x = dsc.reshape(flat[:rows * n], rows, n)
                f = getattr(dsc, op)
                runs = {'rows': forced('rows', lambda: f(x)), 'tiles': forced('tiles', lambda: f(x))}
                nb = 2 * rows * n * rb
                best = report(f'{dname} {op} [{rows}, {n}]', runs, {'rows': nb, 'tiles': nb})
                say(f'{"":36s} tiles / rows = {best["tiles"] / best["rows"]:.3f}')
                del x, flat
    del data

if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
