"""CPU-only checks of the drop-in boundary: the shared library loads without a GPU and
exports every symbol include/dsc_mi355x.h declares; the tensor struct is the reference's
64-byte layout (dsc/include/dsc.h:96-108).  No compute call is made here."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'dsc_mi355x.h')
LIB = os.path.join(ROOT, 'dsc_amd', 'libdsc_mi355x.so')


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(dsc_[a-z0-9_]+)\s*\(', src)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'dsc_amd', 'csrc')])
    return ctypes.CDLL(LIB)


def test_header_symbols_exported(lib):
    names = declared_symbols()
    assert len(names) >= 36
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_python_bindings_cover_header(lib):
    from dsc_amd import _bindings as B
    assert sorted(B.EXPORTS) == declared_symbols()


def test_tensor_struct_layout():
    from dsc_amd._bindings import _DscTensor
    assert ctypes.sizeof(_DscTensor) == 64
    assert _DscTensor.shape.offset == 0 and _DscTensor.stride.offset == 16
    assert _DscTensor.buffer.offset == 32 and _DscTensor.data.offset == 40
    assert _DscTensor.ne.offset == 48 and _DscTensor.n_dim.offset == 52
    assert _DscTensor.dtype.offset == 56 and _DscTensor.backend.offset == 57


def test_header_is_plain_c():
    """The boundary must be consumable from C: compile the header alone with gcc -std=c99."""
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_gpu_is_a_loud_error_not_a_fallback():
    """Without a device, dsc_ctx_init must die (reference error convention: stderr + exit),
    never compute on the CPU.  The GPU probe runs in its own process: torch imported here, after this module loaded the
    library, would bring its own copy of the HIP runtime into the test process and break the GPU tests that follow."""
    probe = subprocess.run([sys.executable, '-c', 'import torch; print(torch.cuda.is_available())'], capture_output=True, text=True)
    assert probe.returncode == 0, probe.stderr[-2000:]
    if probe.stdout.split()[-1] == 'True':
        pytest.skip('GPU present')
    code = ('import ctypes; L = ctypes.CDLL(%r); L.dsc_ctx_init.restype = ctypes.c_void_p; '
            'L.dsc_ctx_init.argtypes = [ctypes.c_size_t] * 2; L.dsc_ctx_init(1 << 20, 1 << 20); print("ALIVE")' % LIB)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode != 0 and 'ALIVE' not in r.stdout
    assert 'no HIP device' in r.stderr or 'HIP error' in r.stderr


def test_product_path_does_not_touch_the_oracle():
    """oracle/ is test infrastructure: nothing under dsc_amd/ or include/ may reference it."""
    bad = []
    for base in ('dsc_amd', 'include'):
        for dp, _, fs in os.walk(os.path.join(ROOT, base)):
            for f in fs:
                if f.endswith(('.py', '.cpp', '.hip', '.h', 'Makefile')):
                    txt = open(os.path.join(dp, f), errors='ignore').read()
                    if re.search(r'\boracle\b|liboracle|libdsc_ref|/root/reference', txt):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def _build_cpp_smoke(tmp_path):
    exe = str(tmp_path / 'cpp_api_smoke')
    cmd = ['g++', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'dsc_amd', 'api'),
           os.path.join(ROOT, 'tests', 'cpp_api_smoke.cpp'), '-L' + os.path.join(ROOT, 'dsc_amd'), '-ldsc_mi355x',
           '-Wl,-rpath,' + os.path.join(ROOT, 'dsc_amd'), '-Wl,-rpath-link,/opt/rocm/lib', '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_api_header_compiles_and_links(lib, tmp_path):
    """dsc_amd/api/dsc_api.h (mirror of the reference's dsc/api/dsc_api.h) with a host compiler, linked against the
    C-ABI library; no compute call."""
    exe = _build_cpp_smoke(tmp_path)
    r = subprocess.run([exe, '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout


@pytest.mark.gpu
def test_cpp_api_filter_and_crop_on_gpu(lib, tmp_path):
    """README.md:141-163 in C++: rfft, operator*, irfft, the fused filter and the `[:n]` crop, on the device."""
    exe = _build_cpp_smoke(tmp_path)
    r = subprocess.run([exe, '1'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert 'crop ok' in r.stdout and 'operators ok' in r.stdout, r.stdout


def _build_comm_smoke(tmp_path):
    exe = str(tmp_path / 'cpp_comm_smoke')
    cmd = ['g++', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp_comm_smoke.cpp'),
           '-L' + os.path.join(ROOT, 'dsc_amd'), '-ldsc_mi355x', '-Wl,-rpath,' + os.path.join(ROOT, 'dsc_amd'), '-Wl,-rpath-link,/opt/rocm/lib', '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_collective_entry_points_link_from_cpp(lib, tmp_path):
    """Section C's communicator + all-gather (dsc_comm_*, dsc_shard_allgather, dsc_shard_exchange_rows) from a C++ host, header only;
    RCCL itself is bound lazily, so linking needs nothing but the library."""
    r = subprocess.run([_build_comm_smoke(tmp_path), '0'], capture_output=True, text=True)
    assert r.returncode == 0 and 'linked' in r.stdout
    # the library must not carry a hard dependency on the 570 MB RCCL
    needed = subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-readelf', '-d', LIB], capture_output=True, text=True).stdout
    assert 'rccl' not in needed.lower()


@pytest.mark.gpu
def test_c_collective_one_rank_on_gpu(lib, tmp_path):
    """A C++ host: unique id -> communicator -> dsc_rfft into its slot of the destination -> per-chunk exchange -> ncclAllGather in
    place, all through the C ABI, one rank (the box has one GPU); gathered == the transform's own output, bit for bit."""
    r = subprocess.run([_build_comm_smoke(tmp_path), '1'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'gathered == transform output: ok' in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


def test_reference_bindings_resolve_against_the_library(lib):
    """INTEGRATION.md says the reference's ctypes bindings bind this library for the hot path: every name they look up for
    that subset (a committed list of names, tests/golden/reference_binding_symbols.txt) must resolve; the rest of the
    reference's names are exactly SURVEY section 2's OUT-OF-SCOPE set."""
    rows = [ln.split() for ln in open(os.path.join(ROOT, 'tests', 'golden', 'reference_binding_symbols.txt')) if ln.strip() and not ln.startswith('#')]
    assert len(rows) == 59
    missing = [n for n, scope in rows if scope == 'path' and not hasattr(lib, n)]
    assert not missing, missing
    assert sum(1 for _, scope in rows if scope == 'path') == 44
    out = sorted(n for n, scope in rows if scope == 'out')
    assert out == ['dsc_arange', 'dsc_clip', 'dsc_concat', 'dsc_cos', 'dsc_exp', 'dsc_i0', 'dsc_log10', 'dsc_log2', 'dsc_logn', 'dsc_pow',
                   'dsc_randn', 'dsc_reshape', 'dsc_sin', 'dsc_sinc', 'dsc_sqrt']


# ---- the 128-bit store-data hazard of gfx950: a deterministic, build-time check instead of repetitions on a GPU

def _hazard_scanner():
    import importlib.util
    spec = importlib.util.spec_from_file_location('check_store_hazard', os.path.join(ROOT, 'dsc_amd', 'csrc', 'check_store_hazard.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_store_hazard_scanner_counts_wait_states():
    """The rule itself on hand-written listings: s_nop N counts N + 1 wait states, two are needed after a buffer store, scalar
    instructions and VALU writes to OTHER registers are harmless, compares and readlanes write no VGPR."""
    scan = _hazard_scanner().scan_text
    store = 'buffer_store_dwordx4 v[66:69], v1, s[8:11], s3 offen\n'
    assert scan(store + 'v_mul_f64 v[66:67], v[2:3], v[4:5]\n')[1]                                  # 0 wait states
    assert scan(store + 's_add_u32 s3, s3, 16\nv_mul_f64 v[68:69], v[2:3], v[4:5]\n')[1]            # 1 wait state
    assert scan(store + 's_nop 0\nv_mov_b32 v69, 0\n')[1]                                            # s_nop 0 = 1
    assert not scan(store + 's_nop 1\nv_mul_f64 v[66:67], v[2:3], v[4:5]\n')[1]                      # s_nop 1 = 2
    assert not scan(store + 's_add_u32 s3, s3, 16\ns_nop 0\nv_mov_b32 v66, 0\n')[1]
    assert not scan(store + 'v_mul_f64 v[70:71], v[2:3], v[4:5]\nv_mul_f64 v[64:65], v[66:67], v[68:69]\nv_mov_b32 v66, 0\n')[1]
    assert not scan(store + 'v_cmp_gt_f64 vcc, v[66:67], v[68:69]\nv_readlane_b32 s4, v66, 3\nv_mov_b32 v66, 0\n')[1]
    assert scan('buffer_store_dwordx3 v[4:6], v1, s[8:11], 0 offen\nv_mov_b32 v6, 0\n')[1]
    assert scan('global_store_dwordx4 v[0:1], v[4:7], off\nv_mov_b32 v5, 0\n')[1]                    # flat forms: one wait state
    assert not scan('global_store_dwordx4 v[0:1], v[4:7], off\ns_nop 0\nv_mov_b32 v5, 0\n')[1]
    assert not scan('buffer_store_dwordx2 v[4:5], v1, s[8:11], 0 offen\nv_mov_b32 v4, 0\n')[1]        # 64 bits: no hazard
    assert scan(store * 3)[0] == 3


def test_no_store_data_hazard_in_the_shipped_code_objects(lib):
    """Every gfx950 code object inside libdsc_mi355x.so is disassembled and scanned (the Makefile runs the same scan after linking
    and fails the build on a hit): thousands of 128-bit stores, none with a VALU write to its data registers inside the wait states."""
    n, bad = _hazard_scanner().scan_file(LIB)
    assert n > 5000, n
    assert not bad, bad[:10]


def test_store_hazard_scan_fails_without_the_wait_states(tmp_path):
    """Negative control: the same f64 kernels built WITHOUT the two wait states of `buf_store` (fft_regs_common.h,
    -DDSC_NO_STORE_HAZARD_PAD) must trip the scanner — hipcc does schedule the overwriting VALU instruction right behind
    the store (`buffer_store_dwordx4 v[106:109], ... ; v_mul_f64 v[106:107], ...`)."""
    co = str(tmp_path / 'nopad.co')
    src = os.path.join(ROOT, 'dsc_amd', 'csrc', 'fft_r2c_2pass.hip')
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-std=c++17', '-O3', '-fPIC', '-I' + os.path.join(ROOT, 'include'), '-ffp-contract=fast',
           '-fno-slp-vectorize', '-DDSC_NO_STORE_HAZARD_PAD', '--cuda-device-only', '-c', src, '-o', co]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n, bad = _hazard_scanner().scan_file(co)
    assert n > 500 and len(bad) > 10, (n, bad[:3])
    assert any('v_mul_f64' in b or 'v_fma_f64' in b or 'v_add_f64' in b for b in bad)
