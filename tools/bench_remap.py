#!/usr/bin/env python3
"""tools/bench_remap.py — HIP-event timings of dsc.roll, dsc.flip, dsc.fftshift and dsc.pad (remap.hip), written to
profiles/remap_bench.txt.  2^26 elements per case: [8192, 8192] in f32 and c32 (fftshift on axis -1, on axis -2 and on both; roll by 1
and by 4097 and flip along axis -1; pad of axis -1 by 512 on each side, reflect and constant), [64, 2^20] (fftshift along axis -1, pad
by 2048 in reflect), [4096, 128, 128] c32 (fftshift over the last two axes: the fft2 display case) and [8192, 8192] f64 (fftshift on
both axes, roll by 1).  Per case, timed interleaved round by round in one process after a warm-up, each window at least --window
seconds of launches:
  (call)   the operator on the route the library picks
  (elems)  the same call under DSC_REMAP_ROUTE=elems
  (comp)   the composition of existing operators that was the only device-side way before: dsc_tensor_get_slice pieces and
           dsc_concat for shifts and rolls, one negative-step slice for flip, negative-step slices and dsc_concat for the reflect pad,
           two constant tensors made outside the timing and dsc_concat for the constant pad; its result is compared with the call's
           bit for bit before anything is timed
  (copy1 .. copy3)  x[:, :] through dsc_tensor_get_slice, the 16-byte region_rows_kernel: a plain aligned copy of the same bytes, three
           times, to show the run-to-run spread of the baseline
Reported: best ms per call, share of the 8 TB/s roofline on algorithmic bytes (the input read once and the output written once), the
spread (max / min - 1) over the rounds; then comp / call (above 1: the composition is slower) and call / copy (best copy)."""
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
ap.add_argument('--only', default='', help='comma-separated substrings of the case labels to run')
ap.add_argument('--call-only', action='store_true', help='time the call and the copies only (A/B runs of two builds of the library)')
ap.add_argument('--no-verify', action='store_true', help='skip the bitwise comparison of call and composition')
ap.add_argument('--out', default=os.path.join('profiles', 'remap_bench.txt'))
args = ap.parse_args()

dsc.init(14 << 30, 1 << 28)
ctx = _get_ctx()
N = 1 << args.log2_n
side = 1 << (args.log2_n // 2)
lines = []
DTYPES = {'f32': np.float32, 'f64': np.float64, 'c32': np.complex64}


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(f, reps):
    B.dsc_timer_start(ctx)
    for _ in range(reps):
        f()
    return B.dsc_timer_stop(ctx) / reps


def forced(f):
    def g():
        os.environ['DSC_REMAP_ROUTE'] = 'elems'
        r = f()
        os.environ.pop('DSC_REMAP_ROUTE', None)
        return r
    return g


def measure(runs):
    reps, times, paths = {}, {k: [] for k in runs}, {}
    for name, f in runs.items():                          # warm-up: code objects, clocks; then size the window
        for _ in range(3):
            f()
        paths[name] = dsc.last_fft_path() if name in ('call', 'elems') else '-'
        dsc.synchronize()
        reps[name] = max(3, int(args.window * 1e3 / events(f, 3)) + 1)
    for _ in range(args.rounds):
        for name, f in runs.items():
            times[name].append(events(f, reps[name]))
    return times, paths


def halves(x, axis, at):
    """concat([x[at:], x[:at]]) along the axis: numpy.roll(x, -at, axis)"""
    lead = (slice(None),) * (axis % x.n_dim)
    return dsc.concat([x[lead + (slice(at, None),)], x[lead + (slice(None, at),)]], axis=axis % x.n_dim)


def case(label, x, call, comp, out_ne):
    if args.only and not any(part in label for part in args.only.split(',')):
        return
    if not args.no_verify and not args.call_only:
        a, b = call(), comp()
        assert a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), f'{label}: the composition and the call differ'
        del a, b
    full = (slice(None),) * x.n_dim
    runs = {'call': call} if args.call_only else {'call': call, 'elems': forced(call), 'comp': comp}
    for k in (1, 2, 3):
        runs[f'copy{k}'] = lambda: x[full]
    es = {dsc.Dtype.F32: 4, dsc.Dtype.F64: 8, dsc.Dtype.C32: 8, dsc.Dtype.C64: 16}[x.dtype]
    nb = (x.ne + out_ne) * es
    times, paths = measure(runs)
    best = {}
    for name in runs:
        ms = best[name] = min(times[name])
        spread = 100 * (max(times[name]) / ms - 1)
        share = (2 * x.ne * es if name.startswith('copy') else nb) / ms / 1e6 / 80
        say(f'{label:52s} {name:6s} {paths[name]:12s} {ms:8.3f} ms  {share:5.1f} % of 8 TB/s  spread {spread:4.1f} %')
    copy = min(best[f'copy{k}'] for k in (1, 2, 3))
    copy_spread = 100 * (max(best[f'copy{k}'] for k in (1, 2, 3)) / copy - 1)
    # the copy moves 2 ne elements, a pad ne + out_ne: compare per byte
    per_byte = (best['call'] / nb) / (copy / (2 * x.ne * es))
    ratios = '' if args.call_only else f'comp / call = {best["comp"] / best["call"]:.2f}   elems / call = {best["elems"] / best["call"]:.2f}   '
    say(f'{"":52s} {ratios}call / copy = {per_byte:.3f} per byte (copies within {copy_spread:.1f} %)')


say(f'2^{args.log2_n} elements per case; best of {args.rounds} interleaved rounds, each at least {args.window} s of launches')
rng = np.random.default_rng(0)
for dname in ('f32', 'c32', 'f64'):
    npdt = DTYPES[dname]
    host = rng.standard_normal(N).astype(npdt) if dname != 'c32' else (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(npdt)
    flat = dsc.from_numpy(host)
    del host
    x = dsc.reshape(flat, side, N // side)
    n0, n1 = side, N // side
    tag = f'{dname} [{n0}, {n1}]'
    if dname != 'f64':
        case(f'{tag} fftshift axis -1', x, lambda: dsc.fftshift(x, axes=-1), lambda: halves(x, 1, n1 - n1 // 2), N)
        case(f'{tag} fftshift axis -2', x, lambda: dsc.fftshift(x, axes=-2), lambda: halves(x, 0, n0 - n0 // 2), N)
    case(f'{tag} fftshift both', x, lambda: dsc.fftshift(x), lambda: halves(halves(x, 0, n0 - n0 // 2), 1, n1 - n1 // 2), N)
    case(f'{tag} roll 1 axis -1', x, lambda: dsc.roll(x, 1, axis=-1), lambda: halves(x, 1, n1 - 1), N)
    if dname != 'f64':
        case(f'{tag} roll 4097 axis -1', x, lambda: dsc.roll(x, 4097, axis=-1), lambda: halves(x, 1, n1 - 4097), N)
        case(f'{tag} flip axis -1', x, lambda: dsc.flip(x, axis=-1), lambda: x[:, ::-1], N)
        w = 512
        case(f'{tag} pad {w} reflect axis -1', x, lambda: dsc.pad(x, ((0, 0), (w, w)), mode='reflect'),
             lambda: dsc.concat([x[:, w:0:-1], x, x[:, n1 - 2:n1 - 2 - w:-1]], axis=1), n0 * (n1 + 2 * w))
        zeros = dsc.from_numpy(np.zeros((n0, w), npdt))
        case(f'{tag} pad {w} constant axis -1', x, lambda: dsc.pad(x, ((0, 0), (w, w))), lambda: dsc.concat([zeros, x, zeros], axis=1), n0 * (n1 + 2 * w))
        del zeros
        rows, n = 64, N // 64
        xl = dsc.reshape(flat, rows, n)
        tag = f'{dname} [{rows}, {n}]'
        case(f'{tag} fftshift axis -1', xl, lambda: dsc.fftshift(xl, axes=-1), lambda: halves(xl, 1, n - n // 2), N)
        w = 2048
        case(f'{tag} pad {w} reflect axis -1', xl, lambda: dsc.pad(xl, ((0, 0), (w, w)), mode='reflect'),
             lambda: dsc.concat([xl[:, w:0:-1], xl, xl[:, n - 2:n - 2 - w:-1]], axis=1), rows * (n + 2 * w))
        del xl
    if dname == 'c32':
        img = dsc.reshape(flat, N // (128 * 128), 128, 128)
        case(f'{dname} [{N // (128 * 128)}, 128, 128] fftshift axes (-2, -1)', img, lambda: dsc.fftshift(img, axes=(-2, -1)),
             lambda: halves(halves(img, 1, 64), 2, 64), N)
        del img
    del x, flat

if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
