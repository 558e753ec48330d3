#!/usr/bin/env python3
"""Generate tests/golden/math.npz + math_manifest.json: outputs of the reference ITSELF (oracle/_ref/libdsc_ref.so, built by
`python -c "import __graft_entry__ as g; g.build()"`) for the operators beyond the FFT path — cos .. sqrt, pow, clip, i0, arange,
randn, reshape, concat.

    python tests/golden/make_golden_math.py          (from the repository root, where oracle/_ref exists)

Only the reference's outputs (`<key>_y`) and a few arrays of special values are stored: a manifest record names the operator,
its scalar arguments and its inputs, each either a seeded draw (`draw()`, bit-reproducible from its spec) or a stored array.
`inputs()` rebuilds a record's inputs; `evaluate()` replays the record on the reference — what tests/test_math_ops_abi.py uses to
show that the committed fixtures are the reference's output."""
import json
import os
import sys
from ctypes import POINTER, c_double, c_int, c_uint8, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NPZ = os.path.join(HERE, 'math.npz')
MANIFEST = os.path.join(HERE, 'math_manifest.json')

DT = {'f32': np.float32, 'f64': np.float64, 'c32': np.complex64, 'c64': np.complex128}
CODE = {'f32': 0, 'f64': 1, 'c32': 2, 'c64': 3}
UNARY = ('cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt')
NONE = 2 ** 31 - 1                      # DSC_VALUE_NONE


def bind(L):
    """The reference symbols beyond oracle/ref.py's set (dsc.h:212-232, 285-353)."""
    from oracle.ref import TP
    if getattr(L, '_math_bound', False):
        return
    L.dsc_pow.argtypes = [c_void_p, TP, TP, TP]
    L.dsc_pow.restype = TP
    for name in UNARY:
        f = getattr(L, 'dsc_' + name)
        f.argtypes = [c_void_p, TP, TP]
        f.restype = TP
    L.dsc_i0.argtypes = [c_void_p, TP]
    L.dsc_i0.restype = TP
    L.dsc_clip.argtypes = [c_void_p, TP, TP, c_double, c_double]
    L.dsc_clip.restype = TP
    L.dsc_arange.argtypes = [c_void_p, c_int, c_uint8]
    L.dsc_arange.restype = TP
    L.dsc_randn.argtypes = [c_void_p, c_int, POINTER(c_int), c_uint8]
    L.dsc_randn.restype = TP
    L.dsc_reshape.argtypes = [c_void_p, TP, c_int]         # variadic: the dimensions follow as c_int
    L.dsc_reshape.restype = TP
    L.dsc_concat.argtypes = [c_void_p, c_int, c_int]       # variadic: the tensors follow
    L.dsc_concat.restype = TP
    L._math_bound = True


def evaluate(R, rec, xs):
    """Run one manifest record on the reference context R (oracle.ref.Ref) with inputs xs; returns the output array."""
    L, ctx = R.L, R.ctx
    bind(L)
    op = rec['op']
    if op in UNARY:
        t = R.put(xs[0])
        y = R.take(getattr(L, 'dsc_' + op)(ctx, t, None))
        R.free(t)
    elif op == 'pow':
        ta, tb = R.put(xs[0]), R.put(xs[1])
        y = R.take(L.dsc_pow(ctx, ta, tb, None))
        R.free(ta, tb)
    elif op == 'i0':
        t = R.put(xs[0])
        y = R.take(L.dsc_i0(ctx, t))
        R.free(t)
    elif op == 'clip':
        t = R.put(xs[0])
        lo = rec['lo'] if rec['lo'] is not None else float('-inf')
        hi = rec['hi'] if rec['hi'] is not None else float('inf')
        y = R.take(L.dsc_clip(ctx, t, None, lo, hi))
        R.free(t)
    elif op == 'arange':
        y = R.take(L.dsc_arange(ctx, rec['n'], CODE[rec['dtype']]))
    elif op == 'randn':
        shape = rec['shape']
        y = R.take(L.dsc_randn(ctx, len(shape), (c_int * len(shape))(*shape), CODE[rec['dtype']]))
    elif op == 'reshape':
        t = R.put(xs[0])
        dims = rec['dims']
        y = R.take(L.dsc_reshape(ctx, t, len(dims), *[c_int(d) for d in dims]))
        R.free(t)
    elif op == 'concat':
        ts = [R.put(x) for x in xs]
        axis = rec['axis'] if rec['axis'] is not None else NONE
        y = R.take(L.dsc_concat(ctx, axis, len(ts), *ts))
        R.free(*ts)
    else:
        raise ValueError(op)
    return y


def draw(g):
    """A seeded input from its manifest spec: uniform in g['re'] (and g['im'] for the imaginary part), built from
    tests.helpers.lcg_signal — an integer recurrence and exact IEEE scaling, so the same bits on any numpy."""
    from tests.helpers import lcg_signal
    shape = tuple(g['shape'])
    lo, hi = g['re']
    re = lo + (hi - lo) * ((lcg_signal(shape, g['seed'], np.float64) + 1.0) * 0.5)
    if g.get('im') is None:
        return re.astype(DT[g['dtype']])
    lo, hi = g['im']
    x = np.empty(shape, np.complex128)
    x.real = re
    x.imag = lo + (hi - lo) * ((lcg_signal(shape, g['seed'] + 7919, np.float64) + 1.0) * 0.5)
    return x.astype(DT[g['dtype']])


def inputs(rec, z):
    """The input arrays of a manifest record: drawn from their spec (plus a stored tail of special values), or stored whole
    in math.npz (the special-value cases); z = the opened math.npz."""
    xs = []
    for spec in rec['inputs']:
        if 'stored' in spec:
            xs.append(z[spec['stored']])
            continue
        x = draw(spec['gen'])
        if spec.get('tail'):
            x = np.concatenate([x.reshape(-1), z[spec['tail']]]).astype(x.dtype)
        xs.append(x)
    return xs


def cases():
    """(record, stored arrays) of every fixture, deterministic.  Records name their inputs (`inputs`); only the special values
    and the reference's outputs are stored."""
    rng = np.random.default_rng(20261015)          # shapes of the concat cases only (they are written into the manifest)
    out = []
    stored = {}
    seed = [1000]

    def gen(shape, dt, re, im=None, tail=None):
        seed[0] += 1
        spec = {'gen': {'shape': [int(v) for v in shape], 'seed': seed[0], 'dtype': dt, 're': list(re),
                        'im': list(im) if im is not None and dt[0] == 'c' else None}}
        if tail is not None:
            spec['tail'] = tail
        return spec

    def keep(name, x):
        stored[name] = np.ascontiguousarray(x)
        return {'stored': name}

    def add(rec, *specs):
        rec['inputs'] = list(specs)
        rec['n_in'] = len(specs)
        out.append(rec)

    # ---- unary x 4 dtypes on seeded inputs in sane ranges (odd length: the scalar tail runs too)
    n = 257
    real_range = {'cos': (-100, 100), 'sin': (-100, 100), 'sinc': (-10, 10), 'logn': (1e-3, 1e3), 'log2': (1e-3, 1e3),
                  'log10': (1e-3, 1e3), 'exp': (-20, 20), 'sqrt': (0, 1e3)}
    cplx_range = {'cos': (100, 10), 'sin': (100, 10), 'sinc': (10, 3), 'logn': (100, 100), 'log2': (100, 100),
                  'log10': (100, 100), 'exp': (20, 100), 'sqrt': (100, 100)}
    for op in UNARY:
        for dt in ('f32', 'f64', 'c32', 'c64'):
            if dt[0] == 'f':
                spec = gen((n,), dt, real_range[op])
            else:
                r, i = cplx_range[op]
                spec = gen((n,), dt, (-r, r), (-i, i))
            add({'key': f'{op}_{dt}', 'op': op, 'dtype': dt, 'kind': 'random'}, spec)

    # ---- special values
    inf, nan = float('inf'), float('nan')
    real_special = [0.0, -0.0, -1.0, 1.0, inf, -inf, nan, 1e-30, 2.0, -2.5]
    for dt in ('f32', 'f64'):
        keep(f'special_{dt}', np.array(real_special, DT[dt]))
    for op in ('sinc', 'logn', 'log2', 'log10', 'sqrt', 'exp', 'cos', 'sin'):
        for dt in ('f32', 'f64'):
            add({'key': f'{op}_{dt}_special', 'op': op, 'dtype': dt, 'kind': 'special'}, {'stored': f'special_{dt}'})
    cplx_special = [complex(0, 0), complex(-4, 0), complex(-4, -0.0), complex(-1, 0), complex(-1, -0.0), complex(0, -0.0),
                    complex(-0.0, 0), complex(1, 0), complex(0, 1), complex(4, -0.0)]
    for dt in ('c32', 'c64'):
        keep(f'special_{dt}', np.array(cplx_special, DT[dt]))
    for op in ('sinc', 'logn', 'log2', 'log10', 'sqrt'):
        for dt in ('c32', 'c64'):
            add({'key': f'{op}_{dt}_special', 'op': op, 'dtype': dt, 'kind': 'special'}, {'stored': f'special_{dt}'})
    for dt, big in (('f32', 88.8), ('f64', 709.9)):
        add({'key': f'exp_{dt}_overflow', 'op': 'exp', 'dtype': dt, 'kind': 'special'},
            keep(f'exp_{dt}_overflow_x', np.array([big, -big, 1000, -1000, 88.7, -103.0, 709.7, -745.2, 0, 1], DT[dt])))
    for dt in ('c32', 'c64'):
        add({'key': f'exp_{dt}_overflow', 'op': 'exp', 'dtype': dt, 'kind': 'special'},
            keep(f'exp_{dt}_overflow_x', np.array([complex(1000, 0), complex(1000, 1), complex(-1000, 2), complex(88.8, 0.5), complex(0, 0)], DT[dt])))

    # ---- pow: every binary route (same shape, each broadcast axis, scalars, rows, columns, mixed dtypes)
    def base(shape, dt):                 # away from 0: complex bases in the right half plane and across the branch cut's neighbours
        return gen(shape, dt, (0.1, 3.0)) if dt[0] == 'f' else gen(shape, dt, (-2.0, 2.0), (0.1, 2.0))

    def expo(shape, dt):
        return gen(shape, dt, (-3.0, 3.0)) if dt[0] == 'f' else gen(shape, dt, (-2.0, 2.0), (-1.0, 1.0))

    for dt in ('f32', 'f64', 'c32', 'c64'):
        for shape in ((2, 3, 4, 8), (2, 3, 3, 5)):
            tag = 'x'.join(map(str, shape))
            add({'key': f'pow_{dt}_same_{tag}', 'op': 'pow', 'dtype': dt, 'kind': 'same'}, base(shape, dt), expo(shape, dt))
            for ax in range(4):
                small = list(shape)
                small[ax] = 1
                add({'key': f'pow_{dt}_bcast{ax}_{tag}', 'op': 'pow', 'dtype': dt, 'kind': 'bcast'}, base(shape, dt), expo(small, dt))
                add({'key': f'pow_{dt}_bcast{ax}_{tag}_left', 'op': 'pow', 'dtype': dt, 'kind': 'bcast'}, base(small, dt), expo(shape, dt))
        add({'key': f'pow_{dt}_scalar_right', 'op': 'pow', 'dtype': dt, 'kind': 'scalar'}, base((8, 32), dt), expo((1,), dt))
        add({'key': f'pow_{dt}_scalar_left', 'op': 'pow', 'dtype': dt, 'kind': 'scalar'}, base((1,), dt), expo((8, 32), dt))
        add({'key': f'pow_{dt}_column', 'op': 'pow', 'dtype': dt, 'kind': 'bcast'}, base((8, 32), dt), expo((8, 1), dt))
        add({'key': f'pow_{dt}_row', 'op': 'pow', 'dtype': dt, 'kind': 'bcast'}, base((8, 32), dt), expo((32,), dt))
    for da, db in (('f64', 'c32'), ('f32', 'c64'), ('c32', 'f32'), ('f32', 'f64'), ('c64', 'f32'), ('c32', 'c64')):
        add({'key': f'pow_mixed_{da}_{db}', 'op': 'pow', 'dtype': da + db, 'kind': 'mixed'}, base((8, 32), da), expo((8, 32), db))
        add({'key': f'pow_mixed_{da}_{db}_bcast', 'op': 'pow', 'dtype': da + db, 'kind': 'mixed'}, base((8, 32), da), expo((32,), db))
    for dt in ('f32', 'f64'):                          # negative bases with non-integer exponents, 0 ** 0
        a = np.array([-2.0, -2.0, -0.5, 0.0, 0.0, 0.0, -0.0, 2.0, -3.0, inf, -inf, nan], DT[dt])
        b = np.array([0.5, 3.0, 2.5, 0.0, -1.0, 2.0, 0.0, -0.5, 2.0, -1.0, 3.0, 0.0], DT[dt])
        add({'key': f'pow_{dt}_special', 'op': 'pow', 'dtype': dt, 'kind': 'special'}, keep(f'pow_{dt}_special_a', a), keep(f'pow_{dt}_special_b', b))
    for dt in ('c32', 'c64'):
        a = np.array([complex(0, 0), complex(-2, 0), complex(-2, 0), complex(0, 1), complex(1, 1), complex(0, 0)], DT[dt])
        b = np.array([complex(0, 0), complex(0.5, 0), complex(2, 0), complex(2, 0), complex(0, 0), complex(2, 0)], DT[dt])
        add({'key': f'pow_{dt}_special', 'op': 'pow', 'dtype': dt, 'kind': 'special'}, keep(f'pow_{dt}_special_a', a), keep(f'pow_{dt}_special_b', b))

    # ---- clip: both bounds, one, none; NaN inputs (one input per dtype, shared by the five bound pairs)
    for dt in ('f32', 'f64', 'c32', 'c64'):
        if dt[0] == 'f':
            keep(f'clip_{dt}_tail', np.array([nan, -0.0, inf, -inf], DT[dt]))
        else:
            keep(f'clip_{dt}_tail', np.array([complex(nan, 1), complex(1, nan), complex(-inf, 2), complex(-0.0, 3)], DT[dt]))
        spec = gen((253,), dt, (-5, 5), (-5, 5), tail=f'clip_{dt}_tail')
        for tag, lo, hi in (('both', -2.0, 2.0), ('lo', -3.0, None), ('hi', None, 2.0), ('none', None, None), ('tight', 0.25, 0.5)):
            add({'key': f'clip_{dt}_{tag}', 'op': 'clip', 'dtype': dt, 'kind': tag, 'lo': lo, 'hi': hi}, spec)

    # ---- i0: both branches and the seam at +-3.75
    for dt in ('f32', 'f64'):
        keep(f'i0_{dt}_seam', np.array([3.75, -3.75, np.nextafter(DT[dt](3.75), DT[dt](0)), np.nextafter(DT[dt](3.75), DT[dt](10)), 0.0, -0.0, 100.0], DT[dt]))
        add({'key': f'i0_{dt}', 'op': 'i0', 'dtype': dt, 'kind': 'random'}, gen((249,), dt, (-30, 30), tail=f'i0_{dt}_seam'))

    # ---- creation
    for dt in ('f32', 'f64', 'c32', 'c64'):
        for n_ in (1, 7, 1000):
            add({'key': f'arange_{dt}_{n_}', 'op': 'arange', 'dtype': dt, 'n': n_})
    for dt in ('f32', 'f64'):
        for shape in ((1000,), (4, 5, 6, 7)):
            add({'key': f'randn_{dt}_' + 'x'.join(map(str, shape)), 'op': 'randn', 'dtype': dt, 'shape': list(shape)})

    # ---- reshape with -1
    x = gen((10, 10), 'f64', (-1, 1))
    for dims in ((4, -1, 5), (-1, 5), (100,), (2, 5, 2, -1)):
        add({'key': 'reshape_' + '_'.join(str(d).replace('-', 'm') for d in dims), 'op': 'reshape', 'dtype': 'f64', 'dims': list(dims)}, x)
    add({'key': 'reshape_c32_m1_6', 'op': 'reshape', 'dtype': 'c32', 'dims': [-1, 6]}, gen((3, 4, 5), 'c32', (-1, 1), (-1, 1)))

    # ---- concat on every axis of 1-4-D inputs, plus flatten
    dts = ('f32', 'f64', 'c32', 'c64')
    k = 0
    for nd in range(1, 5):
        shape = [int(v) for v in rng.integers(2, 5, nd)]
        for ax in range(nd):
            dt = dts[k % 4]
            k += 1
            parts = []
            for _ in range(2 if ax % 2 == 0 else 3):
                s = list(shape)
                s[ax] = int(rng.integers(2, 6))
                parts.append(gen(s, dt, (-1, 1), (-1, 1)))
            add({'key': f'concat_{nd}d_axis{ax}_{dt}', 'op': 'concat', 'dtype': dt, 'axis': ax}, *parts)
            add({'key': f'concat_{nd}d_axis{ax - nd}_{dt}', 'op': 'concat', 'dtype': dt, 'axis': ax - nd}, *parts)
        s2 = list(shape)
        s2[0] += 1
        dt = dts[nd % 4]
        add({'key': f'concat_{nd}d_flat_{dt}', 'op': 'concat', 'dtype': dt, 'axis': None}, gen(shape, dt, (-1, 1), (-1, 1)), gen(s2, dt, (-1, 1), (-1, 1)))
    return out, stored


def main():
    from oracle import ref
    R = ref.Ref.get()
    manifest, arrays = cases()
    for rec in manifest:
        arrays[f"{rec['key']}_y"] = evaluate(R, rec, inputs(rec, arrays))
    assert len({r['key'] for r in manifest}) == len(manifest)
    np.savez_compressed(NPZ, **arrays)
    with open(MANIFEST, 'w') as f:
        json.dump(manifest, f, indent=0)
        f.write('\n')
    print(f'wrote {len(manifest)} cases to {os.path.relpath(NPZ, ROOT)} ({os.path.getsize(NPZ) >> 10} KiB)')


if __name__ == '__main__':
    main()
