"""Shared test helpers: deterministic signals, golden-fixture access, error metrics."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
NP = {'f32': np.float32, 'f64': np.float64, 'c32': np.complex64, 'c64': np.complex128}
F32, F64, C64, C128 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)
CPX = {F32: C64, F64: C128}

# Tolerances of BASELINE.json's north_star ("within 1e-5 rel of CPU reference"; 1e-12 for
# the f64 config) — relative L2 error against the reference/oracle output.
TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-5,
       np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12}


def lcg_signal(shape, seed, dtype):
    """Uniform(-1, 1) samples from a 64-bit LCG (Knuth MMIX constants), top 24 bits.

    Pure integer recurrence: bit-reproducible on any numpy, so fixtures for large inputs
    store only this spec and the reference's output."""
    n = int(np.prod(shape))
    a, c = np.uint64(6364136223846793005), np.uint64(1442695040888963407)
    lanes = 4096            # 4096 independent streams, interleaved
    state = np.arange(lanes, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    out = np.empty((-(-n // lanes), lanes), dtype=np.float64)
    with np.errstate(over='ignore'):
        for i in range(out.shape[0]):
            state = state * a + c
            out[i] = (state >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0
    flat = out.reshape(-1)[:n]
    if np.dtype(dtype).kind == 'c':
        return (flat + 1j * (np.roll(flat, 1) * 0.5)).reshape(shape).astype(dtype)
    return flat.reshape(shape).astype(dtype)


def rel_l2(a, b):
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


def max_rel(a, b):
    """max |a-b| / max |b| — the element-wise form of SURVEY 8c's tolerance."""
    b = np.asarray(b)
    m = np.max(np.abs(b)) if b.size else 0.0
    d = np.max(np.abs(np.asarray(a) - b)) if b.size else 0.0
    return float(d / m) if m > 0 else float(d)


def assert_close(actual, expected, tol=None, what=''):
    actual = np.asarray(actual)
    expected = np.asarray(expected)
    assert actual.shape == expected.shape, f'{what}: shape {actual.shape} != {expected.shape}'
    assert actual.dtype == expected.dtype, f'{what}: dtype {actual.dtype} != {expected.dtype}'
    tol = TOL[expected.dtype] if tol is None else tol
    e2, em = rel_l2(actual, expected), max_rel(actual, expected)
    assert e2 <= tol and em <= tol * 4, f'{what}: rel_l2={e2:.3e} max_rel={em:.3e} tol={tol:g}'


# ---------------------------------------------------------------------------------------------------- the GPU tests' scaffold

@pytest.fixture(scope='module')
def dsc():
    """The one context of a pytest process, 14 GiB main + 5 GiB scratch whichever module asks first (init refuses a second call, so
    differing sizes per module would let the collection order choose).  GPU test modules import it by name; each leaves the device idle."""
    import dsc_amd
    try:
        dsc_amd.init(14 << 30, 5 << 30)
    except RuntimeWarning:
        pass
    yield dsc_amd
    dsc_amd.synchronize()


def sync_fixture(*switches):
    """The autouse fixture of a GPU test module (`_sync = sync_fixture('DSC_SCAN_ROUTE')`): every test starts and ends with the
    named environment switches unset and ends with the device idle."""
    def clear():
        for name in switches:
            os.environ.pop(name, None)

    @pytest.fixture(autouse=True)
    def _sync(dsc):
        clear()
        yield
        dsc.synchronize()
        clear()
    return _sync


def device_view(dsc, big, shape, dt, byte_offset=0):
    """A Tensor of `shape` / numpy dtype `dt` over the device buffer of `big` from `byte_offset` on (not owned): the out= target of the
    GPU route tests, which fill `big` with a sentinel and check that nothing outside the view changes."""
    from dsc_amd import _bindings as B
    from dsc_amd.context import _get_ctx
    from dsc_amd.dtype import NP_TO_DTYPE
    dt = np.dtype(dt)
    c_shape = (ctypes.c_int * len(shape))(*shape)
    nbytes = int(np.prod(shape)) * dt.itemsize
    return dsc.Tensor(B.dsc_tensor_from_device_ptr(_get_ctx(), big._c_ptr.contents.data + byte_offset, nbytes, len(shape), c_shape,
                                                   NP_TO_DTYPE[dt].value))


def assert_out_call(dsc, call, shape, dt, first, what=''):
    """call(out) into the start of a sentinel-filled buffer with 4099 spare elements: the bits of `first` (the result of the same call
    without out=), the tail untouched"""
    dt = np.dtype(dt)
    size = int(np.prod(shape))
    sentinel = np.asarray(-7.25 + 3.5j if dt.kind == 'c' else -7.25, dtype=dt)
    big = dsc.from_numpy(np.full(size + 4099, sentinel, dtype=dt))
    out = device_view(dsc, big, list(shape), dt)
    call(out)
    whole = big.numpy()
    what = what and what + ': '
    assert whole[:size].tobytes() == first.tobytes(), f'{what}two identical calls differ (or out= was not written)'
    assert np.all(whole[size:] == sentinel), f'{what}bytes past the output changed'


def run_child(code, env=None, without=(), timeout=300, check=False, args=()):
    """`python -c code *args` from the repository root, the variables `without` taken out of its environment and `env` added: the
    CompletedProcess.  With check, exit status 0 is asserted and the ends of its output shown."""
    e = {k: v for k, v in os.environ.items() if k not in without}
    e.update(env or {})
    r = subprocess.run([sys.executable, '-c', code, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=e)
    if check:
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def assert_ends_the_process(stmt, message, without_env=None):
    """`stmt` after dsc.init(1 << 28, 1 << 24) in a child process, the variable `without_env` taken out of its environment: a message
    on stderr and exit status 1; nothing runs on the GPU after it."""
    code = f"import numpy as np\nimport dsc_amd as dsc\ndsc.init(1 << 28, 1 << 24)\n{stmt}\nprint('survived')\n"
    r = run_child(code, without=(without_env,))
    assert r.returncode == 1 and 'survived' not in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-300:])
    assert message in r.stderr, r.stderr[-400:]
    assert 'HIP error' not in r.stderr and 'illegal memory' not in r.stderr


def build_cpp_smoke(tmp_path, name):
    """tests/<name>.cpp compiled with the host compiler against the C++ API header and linked to the library: the executable's path"""
    exe = str(tmp_path / name)
    cmd = ['g++', '-std=c++17', '-Wall', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'dsc_amd', 'api'),
           os.path.join(ROOT, 'tests', name + '.cpp'), '-L' + os.path.join(ROOT, 'dsc_amd'), '-ldsc_mi355x',
           '-Wl,-rpath,' + os.path.join(ROOT, 'dsc_amd'), '-Wl,-rpath-link,/opt/rocm/lib', '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


class Golden:
    """Committed fixtures: outputs of the reference itself (tests/golden/make_golden.py)."""

    def __init__(self):
        with open(os.path.join(GOLDEN, 'manifest.json')) as f:
            self.manifest = json.load(f)
        self._npz = {}

    def group(self, name):
        if name not in self._npz:
            self._npz[name] = np.load(os.path.join(GOLDEN, f'{name}.npz'))
        return self._npz[name]

    def cases(self, group, op=None):
        prev_y = None
        for rec in self.manifest:
            if rec['group'] != group:
                continue
            g = self.group(group)
            y = g[rec['key'] + '_y']
            if 'gen' in rec:
                spec = rec['gen']
                if spec['kind'] == 'prev_output':
                    xs = [prev_y]
                else:
                    xs = [lcg_signal(spec['shape'], spec['seed'], NP[spec['dtype']])]
                    if rec['key'] + '_x1' in g:
                        xs.append(g[rec['key'] + '_x1'])
            else:
                xs = [g[f"{rec['key']}_x{j}"] for j in range(rec['n_in'])]
            prev_y = y
            if op is None or rec['op'] == op:
                yield rec, xs, y


def decode_sel(sel):
    """`sel` of a 'slice' golden record -> tuple of ints / slices (tests/golden/make_golden.py)."""
    return tuple(slice(*k) if isinstance(k, list) else int(k) for k in sel)


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes."""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f'{a.dtype.str} {a.shape} '.encode())
    h.update(a.tobytes())
    return h.hexdigest()


def _args_digest(op, args):
    h = hashlib.sha256(op.encode())
    for a in args:
        h.update((digest(a) if isinstance(a, np.ndarray) else repr(a)).encode())
    return h.hexdigest()[:16]


class Pinned:
    """A large reference output kept as its digest only: the only comparison it allows is bit for bit."""

    def __init__(self, shape, dtype, sha):
        self.shape, self.dtype, self.sha = tuple(shape), np.dtype(dtype), sha

    def matches(self, a):
        return a.shape == self.shape and a.dtype == self.dtype and digest(a) == self.sha


class RefRecording:
    """tests/golden/ref_calls.{json,npz}: per test, every call it made on the reference build (oracle/_ref) with a digest
    of the call's inputs and the reference's output — whole up to FULL_BYTES, as a digest (Pinned) above that.
    Written by tests/golden/make_ref_calls.py."""

    PATH = os.path.join(GOLDEN, 'ref_calls')
    FULL_BYTES = 32 << 10

    def __init__(self, empty=False):
        self.calls, self.arrays = {}, {}
        if not empty:
            with open(self.PATH + '.json') as f:
                self.calls = json.load(f)
            with np.load(self.PATH + '.npz') as z:
                self.arrays = {k: z[k] for k in z.files}

    def save(self):
        with open(self.PATH + '.json', 'w') as f:
            json.dump(self.calls, f, indent=0, sort_keys=True)
            f.write('\n')
        np.savez_compressed(self.PATH + '.npz', **self.arrays)


class RecordedRef:
    """Stands in for oracle.ref.Ref (same methods) in tests/test_oracle_vs_ref.py: call i of a test returns what the
    reference returned for call i of the same test when it was recorded.  The tests' inputs are seeded; their digest is
    checked call by call, so a changed test cannot be compared against a stale recording.

    Where the reference build exists (oracle/_ref), every call is also made on it and must reproduce the recording bit
    for bit.  With `recording` given, the reference's outputs are written into it instead (make_ref_calls.py)."""

    OPS = ('fft', 'ifft', 'rfft', 'irfft', 'mul', 'binary', 'unary', 'reduce', 'cast', 'get_slice', 'set_slice')
    _shared = None

    def __init__(self, test, recording=None):
        from oracle import ref
        self.test, self.i = test, 0
        self.live = ref.Ref.get() if ref.available() else None
        self.record = recording is not None
        if self.record:
            if self.live is None:
                raise RuntimeError(f'{ref.LIB_PATH} missing: recording needs the reference build')
            self.rec = recording
            self.rec.calls[test] = []
        else:
            if RecordedRef._shared is None:
                RecordedRef._shared = RefRecording()
            self.rec = RecordedRef._shared
        self.calls = self.rec.calls.get(test)
        assert self.calls is not None, f'{test}: not in {RefRecording.PATH}.json (run tests/golden/make_ref_calls.py)'

    def _next(self, op, args):
        key = _args_digest(op, args)
        if self.record:
            self.calls.append({'op': op, 'args': key})
        assert self.i < len(self.calls), f'{self.test}: more calls than recorded (run tests/golden/make_ref_calls.py)'
        c = self.calls[self.i]
        assert (c['op'], c['args']) == (op, key), \
            f'{self.test}: call {self.i} ({op}) has other inputs than the recording (run tests/golden/make_ref_calls.py)'
        self.i += 1
        return c

    def __getattr__(self, op):
        if op not in self.OPS:
            raise AttributeError(op)

        def call(*args):
            i = self.i
            c = self._next(op, args)
            if self.live is not None:
                y = getattr(self.live, op)(*args)
                if self.record:
                    c['sha'] = digest(y)
                    if y.nbytes <= RefRecording.FULL_BYTES:
                        self.rec.arrays[f'{self.test}.{i}'] = y
                    else:
                        c.update(shape=list(y.shape), dtype=y.dtype.str)
                assert digest(y) == c['sha'], f'{self.test}: call {i} ({op}): the reference build no longer gives the recorded output'
            key = f'{self.test}.{i}'
            if key in self.rec.arrays:
                return self.rec.arrays[key].copy()
            return Pinned(c['shape'], c['dtype'], c['sha'])
        return call

    def ends_process(self, call):
        """Does `r.<call>` on the reference end a fresh process (the reference's DSC_ASSERT prints and exits)?"""
        c = self._next('ends_process', (call,))
        if self.live is not None:
            code = f'import numpy as np\nfrom oracle import ref\nr = ref.Ref.get(1 << 26, 1 << 24)\nr.{call}\nprint("SURVIVED")'
            p = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
            ended = p.returncode != 0 and 'SURVIVED' not in p.stdout
            if self.record:
                c['ended'] = ended
            assert ended == c['ended'], (call, p.stdout, p.stderr[-300:])
        return c['ended']
