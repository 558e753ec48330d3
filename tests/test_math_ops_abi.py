"""CPU-only checks of the math / creation / shape operators' boundary: every name the reference's ctypes bindings look up now
resolves in libdsc_mi355x.so, the new prototypes of include/dsc_mi355x.h are exported and bound, and — where the reference build
exists (oracle/_ref) — replaying fixtures of tests/golden/math.npz on it reproduces them bit for bit.  No GPU call is made."""
import ctypes
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import build_cpp_smoke

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
LIB = os.path.join(ROOT, 'dsc_amd', 'libdsc_mi355x.so')

NEW = ['dsc_arange', 'dsc_clip', 'dsc_concat', 'dsc_cos', 'dsc_exp', 'dsc_i0', 'dsc_log10', 'dsc_log2', 'dsc_logn', 'dsc_pow',
       'dsc_randn', 'dsc_reshape', 'dsc_sin', 'dsc_sinc', 'dsc_sqrt']


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'dsc_amd', 'csrc')])
    return ctypes.CDLL(LIB)


def _generator():
    spec = importlib.util.spec_from_file_location('make_golden_math', os.path.join(GOLDEN, 'make_golden_math.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_reference_binding_resolves(lib):
    """All 59 names of the reference's python/dsc/_bindings.py, 'path' and 'out' alike."""
    rows = [ln.split() for ln in open(os.path.join(GOLDEN, 'reference_binding_symbols.txt')) if ln.strip() and not ln.startswith('#')]
    assert len(rows) == 59
    missing = [n for n, _ in rows if not hasattr(lib, n)]
    assert not missing, missing


def test_new_prototypes_are_declared_exported_and_bound(lib):
    from dsc_amd import _bindings as B
    src = open(os.path.join(ROOT, 'include', 'dsc_mi355x.h')).read()
    for name in NEW:
        assert f'{name}(' in src, name
        assert hasattr(lib, name), name
        assert name in B.EXPORTS, name
    # the reference's argument order (dsc.h:212-232, 285-353): clip takes out, then two doubles; reshape / concat are variadic
    assert 'dsc_tensor *dsc_clip(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, double x_min, double x_max);' in src
    assert 'dsc_tensor *dsc_reshape(dsc_ctx *ctx, const dsc_tensor *x, int dimensions, ...);' in src
    assert 'dsc_tensor *dsc_concat(dsc_ctx *ctx, int axis, int tensors, ...);' in src
    assert 'dsc_tensor *dsc_randn(dsc_ctx *ctx, int n_dim, const int *shape, dsc_dtype dtype);' in src
    assert B.dsc_clip.argtypes[-2:] == [ctypes.c_double, ctypes.c_double]


def test_python_surface_has_the_reference_names():
    import dsc_amd
    for name in ('power', 'cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt', 'i0', 'clip', 'arange', 'randn', 'reshape', 'concat'):
        assert callable(getattr(dsc_amd, name)), name
    for name in ('__pow__', '__rpow__', 'reshape'):
        assert hasattr(dsc_amd.Tensor, name), name


def test_manifest_covers_the_issue_cases():
    recs = json.load(open(os.path.join(GOLDEN, 'math_manifest.json')))
    with np.load(os.path.join(GOLDEN, 'math.npz')) as z:
        files = set(z.files)
    for r in recs:
        assert f"{r['key']}_y" in files
        assert len(r['inputs']) == r['n_in']
        for spec in r['inputs']:
            assert spec['stored'] in files if 'stored' in spec else spec.get('tail') is None or spec['tail'] in files
    ops = {r['op'] for r in recs}
    assert ops == {'cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt', 'pow', 'clip', 'i0', 'arange', 'randn', 'reshape', 'concat'}
    for op in ('cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt'):
        assert {r['dtype'] for r in recs if r['op'] == op and r['kind'] == 'random'} == {'f32', 'f64', 'c32', 'c64'}
    assert {r['axis'] for r in recs if r['op'] == 'concat'} >= {None, 0, 1, 2, 3, -1}


def test_drawn_inputs_are_reproducible():
    """The seeded inputs are rebuilt from their manifest spec: the same bits on every call, in the spec's range and dtype."""
    gen = _generator()
    g = {'shape': [3, 5], 'seed': 4242, 'dtype': 'c32', 're': [0.1, 2.0], 'im': [-1.0, 1.0]}
    a, b = gen.draw(g), gen.draw(dict(g))
    assert a.dtype == np.complex64 and a.shape == (3, 5) and a.tobytes() == b.tobytes()
    assert (a.real >= np.float32(0.1)).all() and (a.real <= 2).all() and (np.abs(a.imag) <= 1).all()
    assert gen.draw(dict(g, seed=4243)).tobytes() != a.tobytes()


def test_regenerated_cases_reproduce_the_fixtures():
    """Replay a sample of math_manifest.json on the reference build: the committed outputs are the reference's, bit for bit."""
    from oracle import ref
    if not ref.available():
        pytest.skip('reference build oracle/_ref not present')
    gen = _generator()
    R = ref.Ref.get()
    recs = json.load(open(os.path.join(GOLDEN, 'math_manifest.json')))
    want = ('cos_c32', 'sqrt_c64_special', 'pow_f32_bcast2_2x3x3x5', 'pow_mixed_f64_c32', 'clip_c64_both', 'i0_f32', 'arange_f32_1000',
            'randn_f64_4x5x6x7', 'reshape_4_m1_5', 'concat_3d_axis-2_f32', 'concat_4d_flat_f32')
    by_key = {r['key']: r for r in recs}
    with np.load(os.path.join(GOLDEN, 'math.npz')) as z:
        for key in want:
            rec = by_key[key]
            y = gen.evaluate(R, rec, gen.inputs(rec, z))
            stored = z[f'{key}_y']
            assert y.dtype == stored.dtype and y.shape == stored.shape, key
            assert y.tobytes() == stored.tobytes(), key


def test_cpp_math_templates_compile_and_link(lib, tmp_path):
    """dsc::cos .. sqrt, pow, i0, clip, arange, randn, reshape, concat of dsc_amd/api/dsc_api.h with a host compiler."""
    exe = build_cpp_smoke(tmp_path, 'cpp_math_smoke')
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout
