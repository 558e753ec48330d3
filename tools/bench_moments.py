#!/usr/bin/env python3
"""tools/bench_moments.py — HIP-event timings of dsc.sumsq, dsc.var, dsc.vdot and dsc.detrend (moments.hip), written to
profiles/moments_bench.txt.  2^26 elements per case, viewed as [8192, 8192], [64, 2^20], [1, 2^26] (last axis) and [4096, 64, 256] (axis 1),
f32, f64 and c32.  Per case the runs are timed interleaved round by round in one process after a warm-up, each window at least --window
seconds of launches:
  (call)   the operator on the route the library picks
  (rows)   inner == 1 with fewer rows than the crossover: DSC_MOMENT_ROUTE=rows, the one-launch route forced onto the few rows
  (tiles)  inner == 1 where the library picks the rows route: DSC_MOMENT_ROUTE=tiles
  (sum)    dsc.sum on the same tensor: the project's measured rate for one read of the same bytes
  (comp)   the composition a user writes without the operator: sum(mul(x, conj(x))), mean(abs(sub(x, mean(x))) ** 2), sub(x, mean(x))
Then the crossover sweep: sumsq, var and detrend f32 on [rows, 2^26 / rows] for rows = 16 .. 4096, both routes forced.
Reported: best ms per call, share of the 8 TB/s roofline on algorithmic bytes (one read of x — two operands for vdot — plus one write
for detrend), the spread (max / min - 1) over the rounds."""
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
ap.add_argument('--dtype', choices=('f32', 'f64', 'c32', 'all'), default='all')
ap.add_argument('--crossover-only', action='store_true', help='skip the cases, run the sweep')
ap.add_argument('--out', default=os.path.join('profiles', 'moments_bench.txt'))
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
            os.environ.pop('DSC_MOMENT_ROUTE', None)
        else:
            os.environ['DSC_MOMENT_ROUTE'] = route
        r = f()
        os.environ.pop('DSC_MOMENT_ROUTE', None)
        return r
    return g


def measure(runs):
    reps, times, paths = {}, {k: [] for k in runs}, {}
    for name, f in runs.items():                          # warm-up: code objects, clocks; then size the window
        for _ in range(3):
            f()
        paths[name] = dsc.last_fft_path() if name in ('call', 'rows', 'tiles') else '-'
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
        say(f'{label:38s} {name:6s} {paths[name]:13s} {ms:8.3f} ms  {nbytes / ms / 1e6 / 80:5.1f} % of 8 TB/s  spread {spread:4.1f} %')
    return {name: min(t) for name, t in times.items()}


def composition(op, x, axis):
    if op == 'sumsq':
        return lambda: dsc.sum(dsc.mul(x, dsc.conj(x)), axis=axis)
    if op == 'var':
        def var():
            d = dsc.absolute(dsc.sub(x, dsc.mean(x, axis=axis)))
            return dsc.mean(dsc.mul(d, d), axis=axis)
        return var
    return lambda: dsc.sub(x, dsc.mean(x, axis=axis))


OPS = {'sumsq': lambda x, y, axis: dsc.sumsq(x, axis=axis), 'var': lambda x, y, axis: dsc.var(x, axis=axis),
       'vdot': lambda x, y, axis: dsc.vdot(x, y, axis=axis), 'detrend': lambda x, y, axis: dsc.detrend(x, axis=axis)}

say(f'2^{args.log2_n} elements per case; best of {args.rounds} interleaved rounds, each at least {args.window} s of launches')
rng = np.random.default_rng(0)
noise = rng.standard_normal(N)
for dname, ndt in (('f32', np.float32), ('f64', np.float64), ('c32', np.complex64)):
    if args.dtype not in (dname, 'all'):
        continue
    eb = np.dtype(ndt).itemsize
    host = (noise + 1j * np.roll(noise, 1)).astype(ndt) if dname == 'c32' else noise.astype(ndt)
    flat, flat_y = dsc.from_numpy(host), dsc.from_numpy(np.roll(host, 7))
    del host
    for shape, axis in ([] if args.crossover_only else SHAPES):
        inner = int(np.prod(shape[axis % len(shape) + 1:]))
        x, y = dsc.reshape(flat, *shape), dsc.reshape(flat_y, *shape)
        for op, f in OPS.items():
            nb = N * eb * {'sumsq': 1, 'var': 1, 'vdot': 2, 'detrend': 2}[op]
            runs = {'call': forced(None, lambda: f(x, y, axis))}
            if inner == 1:
                runs['call']()
                other = 'rows' if dsc.last_fft_path().endswith('tiles') else 'tiles'
                runs[other] = forced(other, lambda: f(x, y, axis))
            if op != 'vdot':
                runs['sum'] = lambda: dsc.sum(x, axis=axis)
                runs['comp'] = composition(op, x, axis)
            best = report(f'{dname} {op} {list(shape)} axis {axis}', runs, nb)
            if op == 'sumsq':
                say(f'{"":38s} sumsq / sum = {best["call"] / best["sum"]:.3f} (time; above 1 = slower than dsc.sum)')
        del x, y
    if dname == 'f32':
        say('crossover: [rows, 2^%d / rows], last axis, both routes forced; tiles / rows below 1 = the tiles route is faster' % args.log2_n)
        for op in ('sumsq', 'var', 'detrend'):
            for rows in (16, 64, 128, 256, 512, 1024, 2048, 4096):
                n = N // rows // 4 * 4
                whole = dsc.reshape(flat, N)
                x = dsc.reshape(whole[:rows * n], rows, n)
                f = OPS[op]
                runs = {'rows': forced('rows', lambda: f(x, None, -1)), 'tiles': forced('tiles', lambda: f(x, None, -1))}
                best = report(f'{dname} {op} [{rows}, {n}]', runs, rows * n * eb * (2 if op == 'detrend' else 1))
                say(f'{"":38s} tiles / rows = {best["tiles"] / best["rows"]:.3f}')
                del x, whole
    del flat, flat_y

if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
