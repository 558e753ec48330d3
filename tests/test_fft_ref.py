"""The long-double reference of dsc_rfft / dsc_irfft / dsc_fft / dsc_ifft and the per-line error bound the GPU tests of
tests/test_gpu_fft_routes.py hold every transform route to.  CPU only: the tests here pin the reference itself against the oracle's C
restatement and against numpy in f64, and show that the bound rejects errors that a whole-array rel-L2 of 1e-5 lets through.

The reference runs numpy's FFT in long double (numpy >= 2.0 transforms np.longdouble natively).  It needs a long double that is
wider than f64 — x86-64's 80-bit format, eps 1.1e-19 — or the f64 kernels would be compared with something as coarse as themselves;
the module refuses to load otherwise."""
import numpy as np
import pytest

from oracle import port

assert np.finfo(np.longdouble).eps < 1e-18, 'the FFT reference needs a long double wider than f64'

# An FFT's error grows like eps * log n * ||x||_2, whatever the data.  tau, calibrated over the route matrix of
# tests/test_gpu_fft_routes.py: f32 the filter's value (tests/test_filter_ref.py), worst route 0.37 of it (r2c_2pass_regs); f64 half
# the filter's value, worst route 0.21 of it (r2c_fused_l2).  At least 2x headroom on every route; never above the north star 1e-5 / 1e-12.
TAU = {np.dtype(np.float32): 2e-6, np.dtype(np.float64): 5e-15}
KINDS = ('rfft', 'irfft', 'fft', 'ifft')


def pow2(n):
    """dsc_pow2_n: the smallest power of two >= n"""
    assert n > 0
    return 1 << (int(n) - 1).bit_length()


def real_of(dt):
    """the real dtype of a transform on dt (its precision: f32 for f32 / c64, f64 for f64 / c128)"""
    return np.dtype(np.float32) if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)


def fit(x, m, axis):
    """x cropped or zero padded to m elements along axis"""
    x = np.moveaxis(np.asarray(x), axis, -1)
    if x.shape[-1] >= m:
        x = x[..., :m]
    else:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (m - x.shape[-1],), x.dtype)], axis=-1)
    return np.moveaxis(x, -1, axis)


def out_len(kind, x_n, n=-1):
    """length of the output along the axis (fft_driver.cpp internal_fft / internal_rfft)"""
    m = n if n > 0 else x_n
    if kind == 'rfft':
        return pow2(m) // 2 + 1
    if kind == 'irfft':
        return 2 * pow2(m - 1)
    return pow2(m)


def ref_fft(x, n, axis, kind):
    """kind(x, n, axis) as DSC computes it, in long double, from x exactly as passed:
      rfft    order = pow2(n or x_n) / 2; the line cropped / zero padded to 2 order; order + 1 bins
      irfft   order = pow2((n or x_n) - 1); bins cropped / zero filled to order + 1, the imaginary parts of bins 0 and order dropped;
              2 order samples, scaled 1 / (2 order)
      fft     N = pow2(n or x_n); the line cropped / zero padded to N (real input widened); unscaled
      ifft    the same, scaled 1 / N"""
    x = np.asarray(x)
    axis = axis % x.ndim
    x_n = x.shape[axis]
    m = n if n > 0 else x_n
    if kind == 'rfft':
        assert x.dtype.kind == 'f'
        order = pow2(m) // 2
        assert order >= 1
        y = np.fft.rfft(fit(x, 2 * order, axis).astype(np.longdouble), axis=axis)
    elif kind == 'irfft':
        assert x.dtype.kind == 'c' and m > 1
        order = pow2(m - 1)
        b = np.moveaxis(fit(x, order + 1, axis).astype(np.clongdouble), axis, -1).copy()
        b[..., 0] = b[..., 0].real
        b[..., order] = b[..., order].real
        y = np.moveaxis(np.fft.irfft(b, 2 * order, axis=-1), -1, axis)
    else:
        N = pow2(m)
        u = fit(x, N, axis).astype(np.clongdouble)
        y = np.fft.fft(u, axis=axis) if kind == 'fft' else np.fft.ifft(u, axis=axis)
    assert y.dtype in (np.longdouble, np.clongdouble), y.dtype
    return y


def fft_err_parts(y, ref, axis, tau, paired=False):
    """(largest per-line ||y - ref||_2 / (tau ||ref||_2), largest element |y_k - ref_k| / its bound) over every line along axis; see
    fft_err.  paired: lines 2c and 2c + 1 (neighbouring columns of an even inner extent) are bounded by the norm and the largest
    element of the pair.  A line whose bound is zero must come out exactly zero."""
    y = np.asarray(y)
    ref = np.asarray(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    m = ref.shape[axis]
    yl = np.moveaxis(y, axis, -1).reshape(-1, m)
    rl = np.moveaxis(ref, axis, -1).reshape(-1, m)
    wide = np.clongdouble if (yl.dtype.kind == 'c' or rl.dtype.kind == 'c') else np.longdouble
    d = np.abs(yl.astype(wide) - rl.astype(wide))
    a = np.abs(rl.astype(wide))
    sq, top = np.sum(a * a, axis=-1), np.max(a, axis=-1)
    if paired:
        assert sq.shape[0] % 2 == 0
        sq = np.repeat(sq.reshape(-1, 2).sum(axis=-1), 2)
        top = np.repeat(top.reshape(-1, 2).max(axis=-1), 2)
    norm = np.sqrt(sq)
    zero = norm == 0
    if np.any(zero):
        assert not np.any(d[zero]), 'nonzero output on a line whose reference is zero'
        norm, top = np.where(zero, 1, norm), np.where(zero, 1, top)
    l2 = np.sqrt(np.sum(d * d, axis=-1)) / (tau * norm)
    mx = np.max(d / (tau * (8 * norm[:, None] / np.sqrt(m) + a + top[:, None] / 8)), axis=-1)
    return float(np.max(l2)), float(np.max(mx))


def fft_err(y, ref, axis, tau, paired=False):
    """largest per-line ratio of the error to its bound (<= 1 passes):
        ||y - ref||_2  <= tau * ||ref||_2
        |y_k - ref_k|  <= tau * (8 ||ref||_2 / sqrt(len_out) + |ref_k| + max_j |ref_j| / 8)     for every element k
    The first is the usual eps log n bound and does not depend on the data (||ref|| is the input norm times a fixed factor).  The
    second catches a single wrong element: on noise, rounding spreads evenly over a line and 8x its rms leaves room for the largest
    of len_out.  Its last two terms are for lines whose energy sits in a few elements (a large DC offset, one strong tone): there
    the strong element's own rounding is a few eps |ref_k|, and the rounding of the intermediate values, which carry the strong
    component, lands as a few eps max |ref| on weak elements at structured positions instead of spreading.  On noise the two terms
    add about 10 % to the first; without them even the f32-rounded exact answer of a strong tone fails from about 2^17 points on
    (test_bound_passes_the_rounded_answer_of_a_strong_tone)."""
    return max(fft_err_parts(y, ref, axis, tau, paired))


def rand_input(rng, kind, shape, dt):
    """standard normal samples; complex for irfft / complex fft, with nonzero imaginary parts everywhere (bins 0 and order too)"""
    dt = np.dtype(dt)
    if dt.kind == 'c':
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)
    return rng.standard_normal(shape).astype(dt)


# ---------------------------------------------------------------------------------------------------- the reference itself

def test_longdouble_reference_is_wide():
    assert np.finfo(np.longdouble).eps < 1e-18
    x = np.arange(8, dtype=np.longdouble)
    assert np.fft.rfft(x).dtype == np.clongdouble and np.fft.irfft(np.fft.rfft(x), 8).dtype == np.longdouble
    assert np.fft.fft(x.astype(np.clongdouble)).dtype == np.clongdouble


@pytest.mark.parametrize('kind,x_n,n,want', [('rfft', 8, -1, 5), ('rfft', 9, -1, 9), ('rfft', 8, 5, 5), ('rfft', 100, 3, 3),
                                             ('irfft', 5, -1, 8), ('irfft', 6, -1, 16), ('irfft', 9, 5, 8), ('irfft', 3, 2, 2),
                                             ('fft', 8, -1, 8), ('fft', 7, -1, 8), ('fft', 7, 17, 32), ('ifft', 9, 4, 4)])
def test_output_lengths(kind, x_n, n, want):
    dt = np.complex128 if kind in ('irfft', 'fft', 'ifft') else np.float64
    x = np.ones((2, x_n), dt)
    assert out_len(kind, x_n, n) == want
    assert ref_fft(x, n, -1, kind).shape == (2, want)
    assert port.__dict__[kind](x, n, -1).shape == (2, want)


def _oracle_cases():
    cases = []
    for dt in (np.float32, np.float64):
        for kind in KINDS:
            for x_n, n in ((64, -1), (64, 50), (64, 200), (33, -1), (1000, 256), (7, 16)):
                cases.append((kind, dt, x_n, n))
    return cases


@pytest.mark.parametrize('kind,dt,x_n,n', _oracle_cases(), ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_reference_matches_oracle(kind, dt, x_n, n):
    """The reference against the oracle's C restatement in the oracle's precision: full, zero padded and cropped lines (for irfft:
    fewer and more bins than order + 1, imaginary parts in bins 0 and order that both must drop), fft / ifft of real input, along
    the last axis and along axis 0 of a 3-d tensor."""
    rng = np.random.default_rng([x_n, n + 1, KINDS.index(kind), np.dtype(dt).itemsize])
    cdt = np.complex64 if dt == np.float32 else np.complex128
    in_dts = {'rfft': (dt,), 'irfft': (cdt,), 'fft': (cdt, dt), 'ifft': (cdt, dt)}[kind]
    for in_dt in in_dts:
        for shape, axis in (((3, x_n), -1), ((x_n, 2, 3), 0)):
            x = rand_input(rng, kind, shape, in_dt)
            got = port.__dict__[kind](x, n, axis)
            want = ref_fft(x, n, axis, kind)
            assert got.shape == want.shape
            assert real_of(got.dtype) == np.dtype(dt)
            r = fft_err(got, want, axis, TAU[np.dtype(dt)])
            assert r <= 1, (kind, in_dt, shape, axis, r)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('L', [2, 16, 1024, 65536])
def test_reference_matches_numpy_f64(kind, L):
    """The long-double reference against numpy's own f64 transform of the same, already fitted lines."""
    rng = np.random.default_rng([L, KINDS.index(kind)])
    if kind == 'irfft':
        x = rand_input(rng, kind, (2, L // 2 + 1), np.complex128)
        x[:, 0] = x[:, 0].real
        x[:, -1] = x[:, -1].real
        want = np.fft.irfft(x, L)
    else:
        x = rand_input(rng, kind, (2, L), np.float64 if kind == 'rfft' else np.complex128)
        want = getattr(np.fft, kind)(x)
    got = ref_fft(x, -1, -1, kind)
    assert got.shape == want.shape
    assert fft_err(want, got, -1, TAU[np.dtype(np.float64)]) <= 0.1


def test_irfft_drops_the_imaginary_parts_of_bins_0_and_order():
    rng = np.random.default_rng(5)
    x = rand_input(rng, 'irfft', (2, 9), np.complex128)
    y = x.copy()
    y[:, 0] = y[:, 0].real
    y[:, 8] = y[:, 8].real
    assert np.array_equal(ref_fft(x, -1, -1, 'irfft'), ref_fft(y, -1, -1, 'irfft'))
    # bins past order + 1 are ignored, missing ones are zero
    assert np.array_equal(ref_fft(np.concatenate([x, x], axis=1), 9, -1, 'irfft'), ref_fft(x, -1, -1, 'irfft'))


def test_zero_line_must_be_exact():
    ref = np.zeros((2, 8), np.clongdouble)
    ref[1] = 1
    y = ref.astype(np.complex64)
    assert fft_err(y, ref, -1, 2e-6) == 0
    y[0, 3] = 1e-30
    with pytest.raises(AssertionError):
        fft_err(y, ref, -1, 2e-6)


# ---------------------------------------------------------------------------------------------------- the bound is tight enough

@pytest.mark.parametrize('dt,err', [(np.float32, 4e-6), (np.float64, 1e-13)])
@pytest.mark.parametrize('kind', ['irfft', 'ifft'])
def test_bound_rejects_an_inverse_scale_error(dt, err, kind):
    """An inverse scale off by 4e-6 (f32) or 1e-13 (f64): the L2 form rejects it on every line; a whole-array rel-L2 at the north
    star (1e-5 / 1e-12) would not."""
    rng = np.random.default_rng(11)
    cdt = np.complex64 if dt == np.float32 else np.complex128
    x = rand_input(rng, kind, (4, 1025 if kind == 'irfft' else 2048), cdt)
    want = ref_fft(x, -1, -1, kind)
    tau = TAU[np.dtype(dt)]
    assert fft_err(want.astype(cdt if kind == 'ifft' else dt), want, -1, tau) <= 0.1
    l2, mx = fft_err_parts(want * (1 + err), want, -1, tau)
    assert l2 > 1.5, l2
    north = 1e-5 if dt == np.float32 else 1e-12
    assert np.linalg.norm((want * (1 + err) - want).ravel()) / np.linalg.norm(want.ravel()) < north


def test_bound_rejects_one_wrong_bin_of_a_65536_point_line():
    """One bin of a 65536-point f32 rfft scaled by 1 + 1e-4: its share of the line's L2 error is small (the L2 form passes it); the
    max form rejects it."""
    rng = np.random.default_rng(12)
    x = rng.standard_normal((3, 65536)).astype(np.float32)
    want = ref_fft(x, -1, -1, 'rfft')
    tau = TAU[np.dtype(np.float32)]
    assert fft_err(want.astype(np.complex64), want, -1, tau) <= 0.1
    k = 12345
    k = k + int(np.argmax(np.abs(want[1, k:k + 8])))           # a bin of ordinary size (one of 8 neighbours, the largest)
    bad = want.copy()
    bad[1, k] *= 1 + 1e-4
    l2, mx = fft_err_parts(bad, want, -1, tau)
    assert l2 < 1 and mx > 1.5, (l2, mx)


@pytest.mark.parametrize('kind', ['rfft', 'fft'])
def test_bound_passes_the_rounded_answer_of_a_strong_tone(kind):
    """The exact answer rounded to f32 is as good as an f32 transform can be: it passes on noise, a DC offset and one strong tone
    at 2^21 points, with room to spare (the element term carries the strong bins)."""
    rng = np.random.default_rng(14)
    m = 1 << 21
    t = np.arange(m)
    x = np.stack([rng.standard_normal(m), rng.standard_normal(m) + 20, rng.standard_normal(m) + 20 * np.cos(2 * np.pi * 5 * t / m)])
    x = x.astype(np.float32 if kind == 'rfft' else np.complex64)
    want = ref_fft(x, -1, -1, kind)
    l2, mx = fft_err_parts(want.astype(np.complex64), want, -1, TAU[np.dtype(np.float32)])
    assert l2 < 0.1 and mx < 0.2, (l2, mx)


def test_bound_rejects_one_wrong_strong_bin():
    """The element term leaves a strong bin no more room than the line's L2 bound: the tone bin of a 65536-point line scaled by
    1 + 1e-4 is rejected."""
    m = 65536
    x = (np.random.default_rng(15).standard_normal(m) + 20 * np.cos(2 * np.pi * 5 * np.arange(m) / m)).astype(np.float32)[None]
    want = ref_fft(x, -1, -1, 'rfft')
    bad = want.copy()
    bad[0, 5] *= 1 + 1e-4
    assert fft_err(bad, want, -1, TAU[np.dtype(np.float32)]) > 10


def test_paired_bound_takes_the_pair_norm():
    """cols_4step_real transforms two neighbouring real columns as one complex column: a weak column next to a strong one carries
    rounding of the strong one's size.  paired=True bounds both by the pair; a wrong element of the weak column is still seen."""
    rng = np.random.default_rng(16)
    x = rng.standard_normal((8192, 2))
    x[:, 1] += 1000 * np.cos(2 * np.pi * 5 * np.arange(8192) / 8192)
    want = ref_fft(x.astype(np.float32), -1, 0, 'rfft')
    near = want.copy()
    near[:, 0] += 3e-8 * np.linalg.norm(want[:, 1]) / np.sqrt(4097) * np.exp(1j * np.arange(4097))   # eps-level crosstalk
    tau = TAU[np.dtype(np.float32)]
    assert fft_err(near, want, 0, tau) > 1 and fft_err(near, want, 0, tau, paired=True) < 0.1
    bad = want.copy()
    bad[100, 0] += 0.05 * np.linalg.norm(want[:, 0])
    assert fft_err(bad, want, 0, tau, paired=True) > 1


def test_bound_rejects_one_wrong_column():
    """One column (one line along axis 0) of a [4096, 70] fft with one sample off by 1e-4 relative: the per-line bound sees it."""
    rng = np.random.default_rng(13)
    x = rand_input(rng, 'fft', (4096, 70), np.complex64)
    want = ref_fft(x, -1, 0, 'fft')
    bad = want.copy()
    bad[777, 69] *= 1 + 1e-4
    assert fft_err(want.astype(np.complex64), want, 0, TAU[np.dtype(np.float32)]) <= 0.1
    assert fft_err(bad, want, 0, TAU[np.dtype(np.float32)]) > 1
