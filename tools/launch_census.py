#!/usr/bin/env python3
"""One small call per entry of the kernel files' dispatch tables, and the comparison of two builds' kernel traces of it.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/launch_census.py --run > DIR/paths.txt     (once per build, DSC_MI355X_LIB)
  python3 tools/launch_census.py --compare DIR_A DIR_B

--run     every complex length 1 .. 2^21 x rfft / irfft / fft / ifft (real and complex input) x f32 / f64 x full / zero-padded lines, on the
          last axis (2 rows from 65536 points up) and, up to 2^16, on axis 0 with 70 columns; long axis-0 lines in 16 real / 8 complex
          columns (the four-step passes at every length of the column table); every fft2 / rfft2 window; decimate / resample_poly shapes
          for each polyphase tile form.  DSC_NO_FUSED_L2=1: rows of 65536 and 131072 points reach the two-pass launcher.  Then the
          operators (stft, istft, convolve, correlate, hilbert, envelope, fft2, cumsum, unwrap, diff, resample_poly): one small call per
          route, the composed routes with their DSC_NO_..._FUSED switch set around the call, scan_rows / scan_tiles through
          DSC_SCAN_ROUTE, hilbert / envelope also on f32 rows long enough to be filtered in f64 and from rows off the 16-byte alignment
          (every instantiation of the composed route's store), and the chunked branches of stft, istft, convolve, correlate, hilbert and envelope at n = 1024 in a second
          context with 64 KiB of scratch, three chunks each.  Then the streaming files (elementwise, layout, reduce): one small call per
          branch of every launcher in them x the four dtypes — the five binary operators on every broadcast route and with operands of
          two dtypes, the unary functions, casts and arange at aligned, odd and 8-bytes-off-alignment counts, the four reductions on
          every kernel, slices (get and set) and transposes per element size.  Then the axis operators (reduce, scan, moments, remap
          .cpp) in a context of their own, f32 and c32: one small call per route of each family, chosen by shape and forced through
          DSC_SCAN_ROUTE / DSC_MOMENT_ROUTE / DSC_REMAP_ROUTE.  Prints one line per call, 'CALL ... <dsc.last_fft_path()>'.
--run axis  the axis operators' block alone.
--compare the kernel-trace CSVs below the two directories in dispatch order: the same sequence of (Kernel_Name, Grid_Size, Workgroup_Size,
          LDS_Block_Size), and the same paths.txt.  Exits 1 on a difference.
"""
import contextlib
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(only_axis=False):
    os.environ['DSC_NO_FUSED_L2'] = '1'
    sys.path.insert(0, ROOT)
    import numpy as np
    import dsc_amd as dsc
    if only_axis:
        dsc.init(2 << 30, 256 << 20)
        axis_operators(dsc, np)
        dsc.synchronize()
        return
    dsc.init(10 << 30, 2 << 30)
    F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
    cpx = {F32: C64, F64: C128}

    def call(what, fn, shape, dt, **kw):
        x = dsc.from_numpy(np.ones(shape, dtype=dt))
        y = fn(x, **kw)
        print('CALL', what, np.dtype(dt).name, shape, kw, dsc.last_fft_path(), flush=True)
        del x, y

    def transforms(L, shape_of, axis, rdt):
        # (kind, input dtype, full input length, padded input length and its n) as tests/test_gpu_fft_routes.py::fits
        for kind, dt, full, short, n in (('rfft', rdt, 2 * L, max(1, 2 * L - 3), 2 * L), ('irfft', cpx[rdt], L + 1, max(2, L // 2 + 1), L + 1),
                                         ('fft', cpx[rdt], L, max(1, L - 3), L), ('fft', rdt, L, max(1, L - 3), L),
                                         ('ifft', cpx[rdt], L, max(1, L - 3), L), ('ifft', rdt, L, max(1, L - 3), L)):
            call(kind, getattr(dsc, kind), shape_of(full), dt, axis=axis)
            call(kind, getattr(dsc, kind), shape_of(short), dt, n=n, axis=axis)

    for rdt in (F32, F64):
        for lg in range(0, 22):                                     # 1 and 2^21: the generic LDS and four-step kernels
            L = 1 << lg
            transforms(L, lambda m: (2 if L >= 32768 else 3, m), -1, rdt)
            if lg <= 16:
                transforms(L, lambda m: (m, 70), 0, rdt)
        for lg in range(12, 22):                                    # real four-step: n = 2^(lg + 1) = n1 n2, split at n1, merge at n2
            call('rfft', dsc.rfft, (2 << lg, 16), rdt, axis=0)
            call('irfft', dsc.irfft, ((1 << lg) + 1, 16), cpx[rdt], axis=0)
        for lg in range(17, 22):                                    # complex four-step, eight columns: the widened split
            call('fft', dsc.fft, (1 << lg, 8), cpx[rdt], axis=0)
            call('ifft', dsc.ifft, (1 << lg, 8), cpx[rdt], axis=0)
        for n0 in (32, 64, 128):
            for n1 in (32, 64, 128):
                for dt in (cpx[rdt], rdt):
                    call('fft2', dsc.fft2, (2, n0, n1), dt)
                    call('ifft2', dsc.ifft2, (2, n0 - 3, n1 - 1), dt, s=(n0, n1))
                call('rfft2', dsc.rfft2, (2, n0, 2 * n1), rdt)
        for T in (300, 900, 4096):                                  # 1, 2 and 4 outputs per thread
            call('decimate', lambda x: dsc.decimate(x, 2), (2, T), rdt)
        for T in (100, 260, 4096):
            call('resample_poly', lambda x: dsc.resample_poly(x, 3, 2), (2, T), rdt)
    operators(dsc, np, call)
    dsc.synchronize()
    dsc.shutdown()
    dsc.init(2 << 30, 256 << 20)
    streaming(dsc, np)
    dsc.synchronize()
    dsc.shutdown()
    dsc.init(2 << 30, 256 << 20)
    axis_operators(dsc, np)
    dsc.synchronize()


@contextlib.contextmanager
def switch(name, value='1'):
    os.environ[name] = value
    try:
        yield
    finally:
        del os.environ[name]


@contextlib.contextmanager
def offset_ones(dsc, np, shape, dt):
    """ones in a view 8 bytes off the 16-byte alignment of the packed kernels, as tests/test_gpu_math_ops.py::_Offset"""
    import ctypes
    from dsc_amd import _bindings as B
    from dsc_amd.context import _get_ctx
    from dsc_amd.dtype import NP_TO_DTYPE
    x = np.ones(shape, dtype=dt)
    raw = B.dsc_device_alloc(_get_ctx(), x.nbytes + 256)
    view = dsc.Tensor(B.dsc_tensor_from_device_ptr(_get_ctx(), raw + 8, x.nbytes, x.ndim, (ctypes.c_int * x.ndim)(*shape), NP_TO_DTYPE[x.dtype].value))
    B.dsc_copy_from_host(_get_ctx(), view._c_ptr, x.ctypes.data, x.nbytes)
    try:
        yield view
    finally:
        del view
        dsc.synchronize()
        B.dsc_device_free(_get_ctx(), raw)


def operators(dsc, np, call):
    F32, F64 = np.float32, np.float64
    cpx = {F32: np.complex64, F64: np.complex128}

    def ones(n, dt):
        return dsc.from_numpy(np.ones(n, dtype=dt))

    def signal_ops(dt, stft_T, spectrum, conv_T, hilbert_rows):
        """stft / istft / convolve / correlate / hilbert / envelope at n = 1024 on whichever route the switches and the context give"""
        call('stft', lambda x: dsc.stft(x, 1024, 256), (1, stft_T), dt)
        for shape in spectrum:
            call('istft', lambda x: dsc.istft(x, 1024, 256), shape, cpx[dt])
        for name in ('convolve', 'correlate'):
            call(name, lambda x: getattr(dsc, name)(x, ones(63, dt), 'full'), (1, conv_T), dt)
        for name in ('hilbert', 'envelope'):
            call(name, getattr(dsc, name), (hilbert_rows, 1024), dt)

    for dt in (F32, F64):
        signal_ops(dt, 4864, [(2, 20, 513)], 7000, 11)                                # the fused routes (istft has one route)
        with switch('DSC_NO_STFT_FUSED'), switch('DSC_NO_CONV_FUSED'), switch('DSC_NO_HILBERT_FUSED'):
            signal_ops(dt, 4864, [], 7000, 11)                                         # the composed ones, one chunk
        call('stft', lambda x: dsc.stft(x, 32, 8), (2, 300), dt)                      # lengths without a fused kernel
        call('stft', lambda x: dsc.stft(x, 65536, 16384), (1, 1 << 17), dt)
        call('convolve', lambda x: dsc.convolve(x, ones(40000, dt), 'same'), (1, 50000), dt)
        call('hilbert', dsc.hilbert, (3, 64), dt)
        call('envelope', dsc.envelope, (2, 1 << 17), dt)                              # f32: widened rows
        call('hilbert', dsc.hilbert, (2, 1 << 17), dt)                                #      ... and their complex store
        # the composed route's store from rows whose base is not 16-byte aligned (sample by sample); f32 also at the widened length
        for shape in ((3, 1024),) + (((2, 1 << 17),) if dt == F32 else ()):
            with switch('DSC_NO_HILBERT_FUSED'), offset_ones(dsc, np, shape, dt) as x:
                for name in ('hilbert', 'envelope'):
                    y = getattr(dsc, name)(x)
                    print('CALL', name, np.dtype(dt).name, shape, 'unaligned', dsc.last_fft_path(), flush=True)
                    del y
        for fused in (True, False):
            with contextlib.nullcontext() if fused else switch('DSC_NO_FFT2_FUSED'):
                call('fft2', dsc.fft2, (2, 32, 32), cpx[dt])
                call('ifft2', dsc.ifft2, (2, 32, 32), cpx[dt])
                call('rfft2', dsc.rfft2, (2, 32, 64), dt)
        call('fft2', dsc.fft2, (2, 16, 512), cpx[dt])                                 # no one-pass kernel
        call('irfft2', dsc.irfft2, (2, 32, 33), cpx[dt])
        for route in ('rows', 'tiles'):
            with switch('DSC_SCAN_ROUTE', route):
                call('cumsum', dsc.cumsum, (3, 20000), dt)
                call('unwrap', dsc.unwrap, (3, 20000), dt)
        call('cumsum', dsc.cumsum, (3, 20000), dt)                                    # the routes chosen by shape: tiles, rows, cols
        call('cumsum', dsc.cumsum, (200, 300), cpx[dt])
        call('unwrap', lambda x: dsc.unwrap(x, axis=0), (300, 70), dt)
        call('diff', dsc.diff, (3, 5000), dt)
        call('diff', lambda x: dsc.diff(x, axis=0), (300, 70), dt)
        call('resample_poly', lambda x: dsc.resample_poly(x, 3, 2), (2, 1000), dt)
        call('resample_poly', lambda x: dsc.resample_poly(x, 2, 2), (2, 1000), dt)    # a copy
        call('resample_poly', lambda x: dsc.resample_poly(x, 1, 3, taps=ones(31, dt)), (2, 1000), dt)

    # Chunked.  64 KiB of scratch and lines of n = 1024: stft / istft keep 8 frames per chunk (20 frames; 5 rows of 4 frames, two rows
    # at a time; one row of 20 frames in windows of frames), convolve / correlate in 1024-point blocks 3 blocks (8 blocks), hilbert /
    # envelope 7 rows rounded to 4 (11 rows).  f64 in a context of twice the size.
    for dt in (F32, F64):
        dsc.synchronize()
        dsc.shutdown()
        dsc.init(256 << 20, (64 << 10) * np.dtype(dt).itemsize // 4)
        with switch('DSC_NO_STFT_FUSED'), switch('DSC_NO_CONV_FUSED'), switch('DSC_NO_HILBERT_FUSED'), switch('DSC_CONV_N', '1024'):
            signal_ops(dt, 4864, [(5, 4, 513), (1, 20, 513)], 7000, 11)


def streaming(dsc, np):
    import ctypes
    from dsc_amd import _bindings as B
    from dsc_amd.context import _get_ctx
    from dsc_amd.dtype import NP_TO_DTYPE
    DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
    BINARY = ('add', 'sub', 'mul', 'true_div', 'power')
    UNARY = ('absolute', 'angle', 'conj', 'real', 'imag', 'cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt', 'i0', 'clip')

    def ones(shape, dt):
        return dsc.from_numpy(np.ones(shape, dtype=dt))

    def call(what, fn, shape, dt, *note):                           # as run()'s, with notes in place of keyword arguments
        x = ones(shape, dt)
        y = fn(x)
        print('CALL', what, np.dtype(dt).name, shape, *note, flush=True)
        del x, y

    def offset_view(shape, dt):
        return offset_ones(dsc, np, shape, dt)

    def unary_and_cast(x, dt, what):
        for name in UNARY:
            if name == 'i0' and np.dtype(dt).kind == 'c':
                continue
            y = dsc.clip(x, 0.5, 2.0) if name == 'clip' else getattr(dsc, name)(x)
            print('CALL', name, what, flush=True)
            del y
        for to in DTYPES:
            if to != dt:
                y = x.cast(NP_TO_DTYPE[np.dtype(to)])
                print('CALL cast', what, np.dtype(to).name, flush=True)
                del y

    # (shape of a, shape of b) per branch of dsc_launch_binary, the unequal ones in both operand orders
    pairs = [((6, 1000), (6, 1000)), ((5, 1001), (5, 1001)), ((8, 512), (512,)), ((3, 5), (5,)), ((4, 1024), (1,)), ((3, 5), (1,)),
             ((12, 512), (12, 1)), ((9, 2), (9, 1)), ((4, 3, 8, 64), (4, 1, 8, 1)), ((4, 3, 8, 65), (4, 1, 8, 1)), ((2, 3, 4, 6), (3, 1, 6))]
    pairs += [(sb, sa) for sa, sb in pairs if sa != sb]
    for dt in DTYPES:
        for name in BINARY:
            for sa, sb in pairs:
                call(name, lambda x: getattr(dsc, name)(x, ones(sb, dt)), sa, dt, sb)
            for other in DTYPES:                                    # two dtypes: promoted in registers (even count), through the casts (odd)
                if other != dt:
                    for shape in ((6, 1000), (5, 1001)):
                        call(name, lambda x: getattr(dsc, name)(x, ones(shape, other)), shape, dt, np.dtype(other).name)
        for n in (4096, 4099, 3):
            unary_and_cast(ones(n, dt), dt, '%s %d' % (np.dtype(dt).name, n))
        with offset_view((1001,), dt) as view:
            unary_and_cast(view, dt, '%s 1001 + 8 bytes' % np.dtype(dt).name)
        for sa, sb in (((8, 512), (512,)), ((4, 3, 8, 65), (4, 1, 8, 1)), ((2, 3, 4, 6), (3, 1, 6))):
            with offset_view(sa, dt) as view:                       # the large operand off alignment: no packs on the trailing and general routes
                for name in BINARY:
                    y, z = getattr(dsc, name)(view, ones(sb, dt)), getattr(dsc, name)(ones(sb, dt), view)
                    print('CALL', name, np.dtype(dt).name, sa, sb, '+ 8 bytes, both orders', flush=True)
                    del y, z
        for n in (1, 4099):
            y = dsc.arange(n, NP_TO_DTYPE[np.dtype(dt)])
            print('CALL arange', np.dtype(dt).name, n, flush=True)
            del y
        for name in ('sum', 'mean', 'max', 'min'):                  # row, sequential, wave, segmented, sequential in packs
            for shape, axis in (((37, 5000), 1), ((37, 5000), 0), ((2048, 1024), 1), ((3000, 700), 0), ((2, 524288), 0)):
                call(name, lambda x: getattr(dsc, name)(x, axis=axis), shape, dt, axis)
        for key in ((slice(None), slice(None, 60)), (slice(None), slice(1, 62)), (slice(None), slice(None, 600)), (slice(None), slice(None, None, 2)),
                    (slice(None), slice(None, 512))):               # flat (widened where the element allows), flat, rows, strided, widened to 16 bytes
            call('get_slice', lambda x: x[key], (8, 1024), dt, key)
            call('set_slice', lambda x: x.__setitem__(key, 2.0), (8, 1024), dt, key, 'scalar')
            call('set_slice', lambda x: x.__setitem__(key, x[key]), (8, 1024), dt, key, 'tensor')
        for shape in ((64, 128), (33, 50)):
            call('transpose', dsc.transpose, shape, dt)
        for n in (1000, 1001):                                      # scan.hip: 16-byte packs and one element per pack
            call('cumsum', dsc.cumsum, (3, n), dt)
            call('diff', lambda x: dsc.diff(x, axis=0), (30, n), dt)
            turns = ('unwrap', dsc.unwrap) if np.dtype(dt).kind == 'f' else ('phase', dsc.phase)
            call(turns[0], turns[1], (3, n), dt)
            call('cumsum', lambda x: dsc.cumsum(x, axis=0), (30, n), dt)
            call(turns[0], lambda x: turns[1](x, axis=0), (30, n), dt)
            with switch('DSC_SCAN_ROUTE', 'tiles'):                 # the totals pass (20021: no packs); 32768: the totals of a row fill whole packs
                for m in (20 * n + n % 2, 32768):
                    call('cumsum', dsc.cumsum, (3, m), dt, 'tiles')
                    call(turns[0], turns[1], (3, m), dt, 'tiles')
        for shape in ((8, 16, 32), (3, 5, 7)):
            call('transpose', lambda x: dsc.transpose(x, (2, 0, 1)), shape, dt)


def axis_operators(dsc, np):
    """reduce.cpp, scan.cpp, moments.cpp, remap.cpp: one small call per route, with the route the library reports after it (the
    reductions report none: the line carries the call before them)"""
    def call(what, fn, shape, dt, *note):
        x = dsc.from_numpy(np.ones(shape, dtype=dt))
        y = fn(x)
        print('CALL', what, np.dtype(dt).name, shape, *note, dsc.last_fft_path(), flush=True)
        del x, y

    def along(name, axis, **kw):
        return lambda x: getattr(dsc, name)(x, axis=axis, **kw)

    for dt in (np.float32, np.complex64):
        real = np.dtype(dt).kind == 'f'
        turns = 'unwrap' if real else 'phase'
        for name in ('sum', 'max'):                                 # row, row per wave, segmented, sequential, sequential in packs
            for shape, axis in (((4, 64), 1), ((1024, 64), 1), ((256, 8), 0), ((30, 300), 0), ((2, 524288), 0)):
                call(name, along(name, axis), shape, dt, axis)
        for name in ('cumsum', turns):                              # tiles, rows, cols, then either forced on the other's shape
            for shape, axis in (((3, 20000), 1), ((200, 300), 1), ((30, 300), 0)):
                call(name, along(name, axis), shape, dt, axis)
            for route, shape in (('rows', (3, 20000)), ('tiles', (200, 300))):
                with switch('DSC_SCAN_ROUTE', route):
                    call(name, along(name, 1), shape, dt, route)
        call('diff', along('diff', 1), (3, 1001), dt, 1)
        call('diff', along('diff', 0), (30, 300), dt, 0)
        moments = (('sumsq', {}), ('var', {}), ('vdot', {}), ('detrend', {'type': 'linear'}))
        for name, kw in moments:                                    # rows by workgroup and by wave, tiles, cols, cols in segments
            fn = (lambda axis: lambda x: dsc.vdot(x, x, axis=axis)) if name == 'vdot' else (lambda axis: along(name, axis, **kw))
            for shape, axis in (((4, 64), 1), ((1024, 64), 1), ((3, 20000), 1), ((30, 300), 0), ((256, 8), 0)):
                call(name, fn(axis), shape, dt, axis)
            for route, shape in (('rows', (3, 20000)), ('tiles', (1024, 64))):
                with switch('DSC_MOMENT_ROUTE', route):
                    call(name, fn(1), shape, dt, route)
        call('flip', along('flip', 0), (8, 64), dt, 0)              # rows, packs, elems, elems forced
        call('flip', along('flip', 1), (8, 64), dt, 1)
        call('flip', along('flip', 1), (3, 5), dt, 1)
        with switch('DSC_REMAP_ROUTE', 'elems'):
            call('flip', along('flip', 0), (8, 64), dt, 'elems')
        call('roll', lambda x: dsc.roll(x, 3), (8, 64), dt, 'axis=None')
        call('pad', lambda x: dsc.pad(x, ((1, 2), (3, 4))), (8, 64), dt, 'constant')


def trace(d):
    files = sorted(glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True))
    if len(files) != 1:
        sys.exit('%s: %d kernel-trace files, expected one' % (d, len(files)))
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))

    def size(r, name):
        if name in r:
            return int(r[name])
        return int(r[name + '_X']) * int(r[name + '_Y']) * int(r[name + '_Z'])
    return [(r['Kernel_Name'], size(r, 'Grid_Size'), size(r, 'Workgroup_Size'), int(r['LDS_Block_Size'])) for r in rows]


def compare(a, b):
    ta, tb = trace(a), trace(b)
    diffs = [(i, x, y) for i, (x, y) in enumerate(zip(ta, tb)) if x != y]
    for i, x, y in diffs[:20]:
        print('dispatch %d:\n  A %s\n  B %s' % (i, x, y))
    pa, pb = ([ln for ln in open(os.path.join(d, 'paths.txt')) if ln.startswith('CALL ')] for d in (a, b))
    path_diffs = [(x, y) for x, y in zip(pa, pb) if x != y]
    for x, y in path_diffs[:20]:
        print('path:\n  A %s  B %s' % (x, y))
    print('dispatches: %d in A, %d in B, %d differing; %d distinct kernels; calls: %d in A, %d in B, %d differing' % (
        len(ta), len(tb), len(diffs), len({t[0] for t in ta}), len(pa), len(pb), len(path_diffs)))
    sys.exit(1 if diffs or path_diffs or len(ta) != len(tb) or len(pa) != len(pb) else 0)


if __name__ == '__main__':
    if sys.argv[1:] in (['--run'], ['--run', 'axis']):
        run(only_axis=len(sys.argv) == 3)
    elif len(sys.argv) == 4 and sys.argv[1] == '--compare':
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
