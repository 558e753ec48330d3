"""GPU tests of dsc_upfirdn / dsc_resample_poly / dsc_decimate / dsc_firwin (polyphase.hip, resample.cpp): every element of every row
against the long-double reference ref_polyphase of tests/test_resample_abi.py under that file's bound |y - ref| <= (K + 2) u A,
K = ceil(M / up), A = sum |tap| |x|; where A = 0 the output must be exactly zero.  The reference runs on the very taps the kernel staged:
the caller's, or dsc.firwin's own for the designed filters (tests/test_resample_abi.py holds dsc_firwin_host to scipy's firwin).

Calibration (worst err / bound per operator over every case of this file, every element checked, on an MI355X):
    upfirdn         f32 0.435   f64 0.402     ((3, 1) with 11 taps; (1, 1) with 2 taps)
    resample_poly   f32 0.387   f64 0.374     (taps= of 20 taps at (5, 1); the designed filters stay below 0.30)
    decimate        f32 0.110   f64 0.111     (q = 4, n = 30)
The largest guaranteed shapes: (160, 1) 0.30 / 0.26, (1, 160) 0.0004 / 0.0008, 4096 taps at (16, 1) 0.015 / 0.019 and at (1, 16)
0.0006 / 0.0008.  Few terms per output give the largest ratios: the bound's K + 2 is then closest to what two or three roundings do.

Every case asserts dsc.last_fft_path(), checks that the input is left bit for bit unchanged, and repeats the call with out= the head of
a larger sentinel-filled buffer: the result must be bit-identical and nothing past it may change.  Argument errors end the process and
run in child processes."""
import subprocess

import numpy as np
import pytest

from tests.helpers import F32, F64, assert_ends_the_process, assert_out_call, build_cpp_smoke, dsc, sync_fixture  # noqa: F401
from tests.test_resample_abi import polyphase_err, ref_magnitude, ref_polyphase, resample_plan, spiced_rows, upfirdn_plan

pytestmark = pytest.mark.gpu

DIRECT, COPY = 'polyphase_direct', 'polyphase_copy'
_sync = sync_fixture()


def _dtype(dsc, dt):
    return dsc.Dtype.F32 if dt == F32 else dsc.Dtype.F64


def run_case(dsc, record_property, op, call, x, h, plan):
    """call(X, out) on the GPU against P(x, h, *plan): the route, the shape and dtype, the input left alone, every element within the
    bound, and a second call into the head of a sentinel-filled buffer that must give the same bits and leave the tail alone.
    Returns the result."""
    gain, up, down, t0, T_out = plan
    dt = x.dtype
    X = dsc.from_numpy(x)
    y = call(X, None)
    assert dsc.last_fft_path() == DIRECT, (op, dsc.last_fft_path())
    yh = y.numpy()
    oshape = x.shape[:-1] + (T_out,)
    assert yh.shape == oshape and yh.dtype == dt, (op, yh.shape, yh.dtype, oshape)
    assert X.numpy().tobytes() == x.tobytes(), 'the input changed'
    del y

    def again(out):
        call(X, out)
        assert dsc.last_fft_path() == DIRECT
    assert_out_call(dsc, again, oshape, dt, yh)

    by_phase = x.shape[-1] * up * len(h) > 4_000_000
    K = -(-len(h) // up)
    r = polyphase_err(yh, ref_polyphase(x, h, *plan, by_phase=by_phase), ref_magnitude(x, h, *plan, by_phase=by_phase), K, dt)
    record_property(f'{op}:{dt}', r)
    print(f'{op} {dt} {x.shape} up={up} down={down} M={len(h)}: err / bound = {r:.3g}')
    assert r <= 1, f'{op} {dt} {x.shape} up={up} down={down} M={len(h)}: err / bound = {r:.3g}'
    return yh


def designed(dsc, rate, dt):
    """the taps resample_poly designs for the reduced rate pair, as the device holds them"""
    return dsc.firwin(20 * rate + 1, 1.0 / rate, 'kaiser', 5.0, _dtype(dsc, dt)).numpy()


def resample_case(dsc, record_property, x, up, down):
    plan = resample_plan(x.shape[-1], up, down)
    h = designed(dsc, max(plan[1], plan[2]), x.dtype)
    return run_case(dsc, record_property, 'resample_poly', lambda X, out: dsc.resample_poly(X, up, down, out=out), x, h, plan)


def decimate_case(dsc, record_property, x, q, n=None):
    taps = dsc.firwin((20 * q if n is None else n) + 1, 1.0 / q, 'hamming', dtype=_dtype(dsc, x.dtype)).numpy()
    plan = resample_plan(x.shape[-1], 1, q, len(taps))
    return run_case(dsc, record_property, 'decimate', lambda X, out: dsc.decimate(X, q, n, out=out), x, taps, plan)


def upfirdn_case(dsc, record_property, x, h, up, down):
    H = dsc.from_numpy(h)
    plan = upfirdn_plan(x.shape[-1], len(h), up, down)
    return run_case(dsc, record_property, 'upfirdn', lambda X, out: dsc.upfirdn(H, X, up, down, out=out), x, h, plan)


# ---------------------------------------------------------------------------------------------------- the device design

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_device_design_is_the_host_design_rounded_once(dsc, dt):
    """dsc.firwin on the device holds dsc_firwin_host's taps rounded to the dtype, bit for bit: the references of this file take the
    designed taps from dsc.firwin, so this ties them to the host design that tests/test_resample_abi.py holds to scipy"""
    from tests.test_resample_abi import firwin_host
    for numtaps, cutoff, window, beta in ((41, 0.5, 'kaiser', 5.0), (3201, 1 / 160, 'kaiser', 5.0), (81, 0.25, 'hamming', 0.0),
                                          (20, 1 / 3, 'hamming', 0.0), (1, 0.5, 'kaiser', 5.0), (61, 1 / 3, 'kaiser', 8.6)):
        got = dsc.firwin(numtaps, cutoff, window, beta, _dtype(dsc, dt)).numpy()
        want = firwin_host(numtaps, cutoff, window, beta).astype(dt)
        assert got.dtype == dt and got.tobytes() == want.tobytes(), (numtaps, cutoff, window)


# ---------------------------------------------------------------------------------------------------- rate pairs

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('up,down', [(1, 2), (2, 1), (3, 2), (2, 3), (7, 5), (5, 7), (1, 8), (8, 1), (160, 147), (147, 160)])
def test_rate_pairs(dsc, record_property, dt, up, down):
    """rows [3, T], T = 1, 63 and 4097: odd, so rows 1 and 2 start unaligned, and several tiles with halos are crossed; T = 1 and 300
    for the 147 / 160 pairs (the long-double reference)"""
    rng = np.random.default_rng([up, down, dt.itemsize])
    for T in ((1, 300) if max(up, down) > 100 else (1, 63, 4097)):
        resample_case(dsc, record_property, rng.standard_normal((3, T)).astype(dt), up, down)


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_gcd_rule(dsc, record_property, dt):
    """(4, 6) is (2, 3) bit for bit; (5, 5) returns a copy"""
    rng = np.random.default_rng([dt.itemsize, 1])
    x = rng.standard_normal((3, 1001)).astype(dt)
    a = resample_case(dsc, record_property, x, 2, 3)
    b = resample_case(dsc, record_property, x, 4, 6)
    assert a.tobytes() == b.tobytes()
    X = dsc.from_numpy(x)
    c = dsc.resample_poly(X, 5, 5)
    assert dsc.last_fft_path() == COPY
    assert c.numpy().tobytes() == x.tobytes() and c.numpy().shape == x.shape
    assert c._c_ptr.contents.data != X._c_ptr.contents.data
    out = dsc.from_numpy(np.zeros_like(x))
    dsc.resample_poly(X, 7, 7, out=out)
    assert dsc.last_fft_path() == COPY and out.numpy().tobytes() == x.tobytes()


# ---------------------------------------------------------------------------------------------------- upfirdn

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('M', [1, 2, 11, 64, 4096])
def test_upfirdn(dsc, record_property, dt, M):
    rng = np.random.default_rng([M, dt.itemsize, 2])
    h = rng.standard_normal(M).astype(dt)
    for up, down in ((1, 1), (1, 3), (3, 1), (4, 6), (16, 15)):
        for T in (1, 2, 1000):
            x = rng.standard_normal((2, T)).astype(dt)
            yh = upfirdn_case(dsc, record_property, x, h, up, down)
            if (up, down) == (1, 1):                                # ... which is numpy's full convolution
                want = np.stack([np.convolve(row.astype(np.longdouble), h.astype(np.longdouble)) for row in x])
                A = np.stack([np.convolve(np.abs(row).astype(np.longdouble), np.abs(h).astype(np.longdouble)) for row in x])
                assert polyphase_err(yh, want, A, M, dt) <= 1
    x = rng.standard_normal((2, 3, 257)).astype(dt)
    assert upfirdn_case(dsc, record_property, x, h, 3, 2).shape[:2] == (2, 3)


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_taps_of_even_length(dsc, record_property, dt):
    """taps= (scipy's window=array) with M = 20: half_len = 9"""
    rng = np.random.default_rng([dt.itemsize, 3])
    taps = rng.standard_normal(20).astype(dt)
    Tp = dsc.from_numpy(taps)
    for up, down in ((3, 2), (1, 4), (5, 1)):
        x = rng.standard_normal((3, 1001)).astype(dt)
        plan = resample_plan(1001, up, down, 20)
        assert plan[3] == 9
        run_case(dsc, record_property, 'resample_poly', lambda X, out: dsc.resample_poly(X, up, down, taps=Tp, out=out), x, taps, plan)


# ---------------------------------------------------------------------------------------------------- decimate

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('q,n', [(2, None), (3, None), (8, None), (13, None), (4, 30)])
def test_decimate(dsc, record_property, dt, q, n):
    rng = np.random.default_rng([q, dt.itemsize, 4])
    for T in (1, 63, 4097):
        decimate_case(dsc, record_property, rng.standard_normal((3, T)).astype(dt), q, n)


# ---------------------------------------------------------------------------------------------------- rows with structure

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
def test_spiced_rows(dsc, record_property, dt):
    """a DC offset, a strong tone, one impulse, an all-zero row (exactly zero out), a third of a row"""
    rng = np.random.default_rng([dt.itemsize, 5])
    x = spiced_rows(rng, 7, 1501, dt)
    for up, down in ((3, 2), (2, 3), (4, 1)):
        assert not np.any(resample_case(dsc, record_property, x, up, down)[4])
    assert not np.any(decimate_case(dsc, record_property, x, 4)[4])
    h = rng.standard_normal(11).astype(dt)
    assert not np.any(upfirdn_case(dsc, record_property, x, h, 4, 6)[4])
    assert not np.any(upfirdn_case(dsc, record_property, x, h, 1, 1)[4])


# ---------------------------------------------------------------------------------------------------- the largest guaranteed shapes

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('up,down', [(1, 160), (160, 1)])
def test_largest_rates(dsc, record_property, dt, up, down):
    rng = np.random.default_rng([up, down, dt.itemsize, 6])
    resample_case(dsc, record_property, rng.standard_normal((2, 2000)).astype(dt), up, down)


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('up,down', [(16, 1), (1, 16)])
def test_longest_filter(dsc, record_property, dt, up, down):
    rng = np.random.default_rng([up, down, dt.itemsize, 7])
    h = rng.standard_normal(4096).astype(dt)
    upfirdn_case(dsc, record_property, rng.standard_normal((2, 5000)).astype(dt), h, up, down)


# ---------------------------------------------------------------------------------------------------- child processes

ERRORS = {
    'complex_input': ("dsc.resample_poly(dsc.from_numpy(np.ones((2, 64), np.complex64)), 3, 2)", 'input must be real'),
    'up_is_zero': ("dsc.upfirdn(dsc.from_numpy(np.ones(5, np.float32)), dsc.from_numpy(np.ones((2, 64), np.float32)), 0, 2)",
                   'up and down must be at least 1'),
    'filter_dtype': ("dsc.upfirdn(dsc.from_numpy(np.ones(5, np.float64)), dsc.from_numpy(np.ones((2, 64), np.float32)), 3, 2)",
                     'filter dtype must match'),
    'out_shape': ("dsc.resample_poly(dsc.from_numpy(np.ones((2, 64), np.float32)), 3, 2, out=dsc.from_numpy(np.ones((2, 95), np.float32)))",
                  'out must have'),
    'out_overlaps_x': ("X = dsc.from_numpy(np.ones((2, 64), np.float32))\ndsc.upfirdn(dsc.from_numpy(np.ones(1, np.float32)), X, 1, 1, out=X)",
                       'out must not share memory with x'),
    'out_overlaps_taps': ("H = dsc.from_numpy(np.ones(96, np.float32))\ndsc.resample_poly(dsc.from_numpy(np.ones((1, 64), np.float32)), 3, 2, "
                          "taps=H, out=dsc.reshape(H, 1, 96))", 'out must not share memory with the filter'),
    'q_is_one': ("dsc.decimate(dsc.from_numpy(np.ones((2, 64), np.float64)), 1)", 'at least 2'),
    'cutoff_is_one': ("dsc.firwin(21, 1.0)", 'cutoff must lie strictly between 0 and 1'),
}


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_argument_errors_end_the_process(name):
    """like every operator: a message on stderr and exit status 1; nothing runs on the GPU after it"""
    assert_ends_the_process(*ERRORS[name])


def test_cpp_resample_smoke_on_the_gpu(tmp_path):
    exe = build_cpp_smoke(tmp_path, 'cpp_resample_smoke')
    r = subprocess.run([exe, '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'resample templates ok' in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-400:])
