#!/usr/bin/env python3
"""tools/bench_math_ops.py — HIP-event timings of the math, creation and clip operators on 2^28-element tensors of every dtype,
with algorithmic bytes (every input read once, the output written once) against the 8 TB/s HBM roofline.  One line per operator
and dtype; `--log2n 24` for a quicker pass (e.g. under rocprofv3).  An operator well below the unary family's 76-79 % with
algorithmic bytes this simple is ALU-bound, not memory-bound: the last column says which."""
import argparse
import sys

sys.path.insert(0, '.')
import dsc_amd as dsc                      # noqa: E402
from dsc_amd import _bindings as B         # noqa: E402
from dsc_amd.context import _get_ctx       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--log2n', type=int, default=28)
ap.add_argument('--reps', type=int, default=10)
args = ap.parse_args()
N = 1 << args.log2n

dsc.init(40 << 30, 4 << 30)
ctx = _get_ctx()


def timeit(f, reps=args.reps, warm=2):
    """best of three rounds after a clock ramp (tools/bench_ops.py)"""
    import time
    f()
    dsc.synchronize()
    t0 = time.perf_counter()
    f()
    dsc.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    for _ in range(max(warm, int(0.05 / one))):
        f()
    dsc.synchronize()
    best = 1e30
    for _ in range(3):
        B.dsc_timer_start(ctx)
        for _ in range(reps):
            f()
        best = min(best, B.dsc_timer_stop(ctx) / reps)
    return best


def report(name, ms, nbytes):
    gbs = nbytes / ms / 1e6
    pct = gbs / 80
    bound = 'HBM' if pct >= 60 else 'ALU'
    print(f'{name:34s} {ms:9.3f} ms  {gbs:8.1f} GB/s  {pct:5.1f} % of 8 TB/s  {bound}', flush=True)


# inputs: uniform in (0.1, 3) made on the device (arange f64, scaled), complex ones rotated by (0.6 + 0.8i)
base = dsc.arange(N, dsc.Dtype.F64) * (2.9 / N) + 0.1
xs = {dsc.Dtype.F32: base.cast(dsc.Dtype.F32), dsc.Dtype.F64: base,
      dsc.Dtype.C32: base.cast(dsc.Dtype.C32) * complex(0.6, 0.8), dsc.Dtype.C64: base.cast(dsc.Dtype.C64) * complex(0.6, 0.8)}
esz = {dsc.Dtype.F32: 4, dsc.Dtype.F64: 8, dsc.Dtype.C32: 8, dsc.Dtype.C64: 16}
print(f'N = 2^{args.log2n} elements per tensor; bytes = inputs read + output written once', flush=True)
for dt in (dsc.Dtype.F32, dsc.Dtype.F64, dsc.Dtype.C32, dsc.Dtype.C64):
    x = xs[dt]
    out = dsc.empty(N, dt)
    nb = N * esz[dt]
    for op in ('cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt'):
        f = getattr(B, 'dsc_' + op)
        report(f'{op} {dt}', timeit(lambda: f(ctx, x._c_ptr, out._c_ptr)), 2 * nb)
    y = x * 0.5                            # an exponent tensor of its own: three distinct streams
    report(f'pow {dt} (same shape)', timeit(lambda: B.dsc_pow(ctx, x._c_ptr, y._c_ptr, out._c_ptr)), 3 * nb)
    row = dsc.reshape(x, -1, 4096)
    e = x[0:4096]                          # a contiguous copy: the broadcast row
    out2 = dsc.reshape(out, -1, 4096)
    report(f'pow {dt} [N/4096, 4096] x [4096]', timeit(lambda: B.dsc_pow(ctx, row._c_ptr, e._c_ptr, out2._c_ptr)), 2 * nb)
    report(f'clip {dt}', timeit(lambda: B.dsc_clip(ctx, x._c_ptr, out._c_ptr, 0.5, 2.0)), 2 * nb)
    if dt in (dsc.Dtype.F32, dsc.Dtype.F64):
        report(f'i0 {dt}', timeit(lambda: B.dsc_tensor_free(ctx, B.dsc_i0(ctx, x._c_ptr))), 2 * nb)      # i0 has no out=

    def arange():
        B.dsc_tensor_free(ctx, B.dsc_arange(ctx, N, dt.value))
    report(f'arange {dt}', timeit(arange), nb)
    del out, row, out2, e, y
