"""GPU tests of dsc.filter_fft (README filterFFT as one call: y = irfft(rfft(s, n) * H), n = 2 (len(H) - 1)) on each of its routes,
every row against the long-double reference of tests/test_filter_ref.py under the error bound that FFT filtering actually obeys:
    per row  ||y - ref||_2 <= tau max|H| ||s_used||_2,  max |y - ref| <= 8 tau max|H| ||s_used||_2 / sqrt(n)
Routes (dsc.last_fft_path()):
  filter_mid_regs   fft_mid_filter_kernel, one instantiation per n = 512 .. 32768 and f32 / f64: all fourteen run
  filter_64k_regs   the 65536-point f32 kernel
  filter_composed   dsc_rfft, dsc_mul, dsc_irfft: n <= 256, f64 at 65536, n >= 131072, mixed precisions (the output is f64), rows too
                    long for the fused kernel's 31-bit offsets
Row counts that leave a ragged last workgroup for every lines-per-group count, odd / padded / cropped row lengths, [ls], [rows, ls] and
[2, 3, ls] inputs, filters with a single nonzero bin at each edge of the spectrum (bins 0 and n/2 with an imaginary part that must be
ignored), known answers (identity, circular shifts, impulses), out= views with a sentinel tail, and determinism."""
import numpy as np
import pytest

from tests.helpers import CPX, F32, F64, device_view, dsc, sync_fixture  # noqa: F401
from tests.test_filter_ref import TAU, filter_err, ref_filter, used

pytestmark = pytest.mark.gpu

C32, C64 = CPX[F32], CPX[F64]
MID_N = (512, 1024, 2048, 4096, 8192, 16384, 32768)
FUSED = [(n, dt) for dt in (F32, F64) for n in MID_N] + [(65536, F32)]
COMPOSED_N = (4, 64, 256)
FUSED_IDS = [f'{n}-{dt}' for n, dt in FUSED]
_sync = sync_fixture()


def route(n, sdt, hdt, ls):
    """the route dsc_filter_fft must take (fft_driver.cpp)"""
    if sdt == F32 and hdt == C32 and n == 65536:
        return 'filter_64k_regs'
    if CPX[sdt] == hdt and n in MID_N and ls * 8 * 64 < (1 << 30):
        return 'filter_mid_regs'
    return 'filter_composed'


def rand_H(rng, n, cdt):
    """a random complex filter; its DC and Nyquist bins carry imaginary parts that the transform must ignore"""
    H = rng.standard_normal(n // 2 + 1) + 1j * rng.standard_normal(n // 2 + 1)
    H[0], H[-1] = 0.5 + 2.5j, -0.75 - 3j
    return H.astype(cdt)


def run(dsc, s, H, out=None):
    """dsc.filter_fft on host arrays: asserts the route, output shape and dtype, returns the result on the host"""
    n = 2 * (H.shape[-1] - 1)
    want_path = route(n, s.dtype, H.dtype, s.shape[-1])
    y = dsc.filter_fft(dsc.from_numpy(s), dsc.from_numpy(H), out=out)
    assert dsc.last_fft_path() == want_path, (n, s.dtype, H.dtype, s.shape, dsc.last_fft_path())
    yh = y.numpy()
    out_dt = s.dtype if CPX[s.dtype] == H.dtype else F64             # mixed precisions promote through dsc_mul
    assert yh.shape == s.shape[:-1] + (n,) and yh.dtype == out_dt, (yh.shape, yh.dtype)
    return yh


def check(record_property, y, s, H, want=None):
    """every row of y against the reference (or a known answer in long double); records err / bound for the route table"""
    n = 2 * (H.shape[-1] - 1)
    if want is None:
        want = ref_filter(s, H, n)
    r = filter_err(y, want, s, H, n, TAU[s.dtype])
    record_property(f'{route(n, s.dtype, H.dtype, s.shape[-1])}:{s.dtype}+{H.dtype}', r)
    assert r <= 1, f'err / bound = {r:.3g}'
    return r


# ---------------------------------------------------------------------------------------------------- the route matrix

def _matrix():
    cases = [(n, dt, CPX[dt]) for n, dt in FUSED]
    cases += [(n, dt, CPX[dt]) for n in COMPOSED_N + (131072, 1 << 20) for dt in (F32, F64)]
    cases += [(65536, F64, C64)]
    cases += [(n, F32, C64) for n in (256, 4096, 65536)] + [(n, F64, C32) for n in (256, 4096, 65536)]
    return cases


@pytest.mark.parametrize('n,sdt,hdt', _matrix(), ids=lambda v: str(v))
def test_route_matrix(dsc, record_property, n, sdt, hdt):
    rng = np.random.default_rng([n, sdt.itemsize, hdt.itemsize])
    H = rand_H(rng, n, hdt)
    for shape in ((17 if n <= 65536 else 3, n), (2, 3, n)):
        s = rng.standard_normal(shape).astype(sdt)
        check(record_property, run(dsc, s, H), s, H)


@pytest.mark.parametrize('dt', [F32, F64])
def test_rows_too_long_for_the_fused_kernel(dsc, record_property, dt):
    """One row of 2^21 + 3 samples at n = 1024: ls * 8 * 64 >= 2^30, the fused kernel's offsets would not fit, composed route."""
    n, ls = 1024, (1 << 21) + 3
    rng = np.random.default_rng(ls)
    s = rng.standard_normal(ls).astype(dt)
    H = rand_H(rng, n, CPX[dt])
    assert route(n, dt, CPX[dt], ls) == 'filter_composed'
    check(record_property, run(dsc, s, H), s, H)


# ---------------------------------------------------------------------------------------------------- row geometry

def _row_counts():
    cases = []
    for n, dt in FUSED + [(64, F32), (64, F64)]:
        for rows in (1, 3, 17, 257) + ((1001,) if n <= 8192 else ()):
            cases.append((n, dt, rows))
    return cases


@pytest.mark.parametrize('n,dt,rows', _row_counts(), ids=lambda v: str(v))
def test_row_counts(dsc, record_property, n, dt, rows):
    """17 and 257 rows leave a ragged last workgroup for every lines-per-group count of the mid kernels (G = 1 .. 32); padded odd
    rows put every line g of a group at input offset g * ls, not a multiple of a pair.  Every row (every lane g) is compared."""
    rng = np.random.default_rng([n, dt.itemsize, rows])
    H = rand_H(rng, n, CPX[dt])
    ls = n - 61 if rows in (17, 257) and n > 64 else n + 1 if rows == 3 else n
    s = rng.standard_normal((rows, ls)).astype(dt)
    check(record_property, run(dsc, s, H), s, H)


def _lengths():
    cases = []
    for n, dt in FUSED + [(256, F32), (256, F64), (131072, F64)]:
        for i, ls in enumerate((1, 2, 3, n // 2 + 1, n - 61, n - 1, n, n + 1, 2 * n + 3)):
            cases.append((n, dt, ls, ('1d', 'rows', '3d')[i % 3]))
    return cases


@pytest.mark.parametrize('n,dt,ls,kind', _lengths(), ids=lambda v: str(v))
def test_row_lengths(dsc, record_property, n, dt, ls, kind):
    """Rows shorter than n are zero padded, longer ones cropped; an odd length splits the last sample pair (the pair's second
    sample is the next row's first, or past the end of s)."""
    rng = np.random.default_rng([n, dt.itemsize, ls])
    H = rand_H(rng, n, CPX[dt])
    shape = {'1d': (ls,), 'rows': (17 if n <= 65536 else 3, ls), '3d': (2, 3, ls)}[kind]
    s = rng.standard_normal(shape).astype(dt)
    check(record_property, run(dsc, s, H), s, H)


# ---------------------------------------------------------------------------------------------------- spectrum edges

EDGE_ROUTES = FUSED + [(256, F32), (256, F64)]
EDGE_BINS = {'0': lambda L: 0, '1': lambda L: 1, 'L/2-1': lambda L: L // 2 - 1, 'L/2': lambda L: L // 2, 'L/2+1': lambda L: L // 2 + 1,
             'L-1': lambda L: L - 1, 'L': lambda L: L, 'random': None}


@pytest.mark.parametrize('n,dt,k', [(n, dt, k) for n, dt in EDGE_ROUTES for k in EDGE_BINS], ids=lambda v: str(v))
def test_spectrum_edges(dsc, record_property, n, dt, k):
    """H zero but for one bin: the self-paired bins 0 and L = n/2 (their imaginary parts must be ignored) and L/2 go through their
    own lanes of the fused pair step.  'random': every bin nonzero, imaginary DC and Nyquist parts."""
    L = n // 2
    rng = np.random.default_rng([n, dt.itemsize, list(EDGE_BINS).index(k)])
    if k == 'random':
        H = rand_H(rng, n, CPX[dt])
    else:
        b = EDGE_BINS[k](L)
        H = np.zeros(L + 1, CPX[dt])
        H[b] = 0.75 - 0.5j if b in (0, L) else 0.6 + 0.9j
    s = rng.standard_normal((17, n - 3)).astype(dt)
    check(record_property, run(dsc, s, H), s, H)


# ---------------------------------------------------------------------------------------------------- known answers

KNOWN = FUSED + [(256, F32), (256, F64)]


@pytest.mark.parametrize('n,dt', KNOWN, ids=lambda v: str(v))
def test_identity(dsc, record_property, n, dt):
    """H = 1 returns the padded / cropped rows of s."""
    rng = np.random.default_rng([n, dt.itemsize, 1])
    H = np.ones(n // 2 + 1, CPX[dt])
    for ls in (n - 61, n + 5):
        s = rng.standard_normal((3, ls)).astype(dt)
        check(record_property, run(dsc, s, H), s, H, want=used(s, n).astype(np.longdouble))


@pytest.mark.parametrize('n,dt', KNOWN, ids=lambda v: str(v))
def test_phase_ramp_is_circular_shift(dsc, record_property, n, dt):
    """H[k] = exp(-2 pi i k d / n) delays each row by d samples, circularly."""
    rng = np.random.default_rng([n, dt.itemsize, 2])
    k = np.arange(n // 2 + 1, dtype=np.int64)
    s = rng.standard_normal((5, n - 7)).astype(dt)
    for d in (1, n // 2, n - 1):
        H = np.exp(-2j * np.pi * ((k * d) % n) / n).astype(CPX[dt])
        check(record_property, run(dsc, s, H), s, H, want=np.roll(used(s, n).astype(np.longdouble), d, axis=-1))


@pytest.mark.parametrize('n,dt', KNOWN, ids=lambda v: str(v))
def test_impulses(dsc, record_property, n, dt):
    """An impulse at p returns irfft(H), rotated by p."""
    rng = np.random.default_rng([n, dt.itemsize, 3])
    H = rand_H(rng, n, CPX[dt])
    pos = (0, 1, n // 2, n - 1)
    s = np.zeros((len(pos), n), dt)
    s[np.arange(len(pos)), pos] = 1
    Hr = H.astype(np.clongdouble)
    Hr[0], Hr[-1] = Hr[0].real, Hr[-1].real
    h = np.fft.irfft(Hr, n)
    check(record_property, run(dsc, s, H), s, H, want=np.stack([np.roll(h, p) for p in pos]))


# ---------------------------------------------------------------------------------------------------- out= and stray writes

@pytest.mark.parametrize('n,sdt,hdt,rows,ls', [
    (4096, F32, C32, 17, 4096 - 61),            # filter_mid_regs, ragged last group (G = 2)
    (1024, F64, C64, 9, 1024 + 3),              # filter_mid_regs, f64 (G = 4), cropped
    (65536, F32, C32, 3, 65536 - 61),           # filter_64k_regs
    (65536, F64, C64, 3, 65536),                # filter_composed
    (256, F32, C64, 5, 200)],                   # filter_composed, mixed: f64 out
    ids=lambda v: str(v))
def test_out_and_no_stray_writes(dsc, record_property, n, sdt, hdt, rows, ls):
    """out= a view of the start of a larger sentinel-filled device buffer: the result lands in it, and nothing past rows * n changes."""
    odt = sdt if CPX[sdt] == hdt else F64
    extra = 70000
    big = dsc.from_numpy(np.full(rows * n + extra, -7.25, dtype=odt))
    out = device_view(dsc, big, (rows, n), odt)
    rng = np.random.default_rng([n, rows, ls])
    s = rng.standard_normal((rows, ls)).astype(sdt)
    H = rand_H(rng, n, hdt)
    y = run(dsc, s, H, out=out)
    whole = big.numpy()
    assert np.array_equal(y, whole[:rows * n].reshape(rows, n)), 'the returned tensor is not out'
    assert np.all(whole[rows * n:] == np.asarray(-7.25, dtype=odt)), 'bytes past the output changed'
    check(record_property, whole[:rows * n].reshape(rows, n), s, H)
    del out


# ---------------------------------------------------------------------------------------------------- determinism

@pytest.mark.parametrize('n,dt', FUSED, ids=FUSED_IDS)
def test_deterministic(dsc, n, dt):
    rng = np.random.default_rng([n, dt.itemsize, 4])
    H = rand_H(rng, n, CPX[dt])
    s = rng.standard_normal((33, n + 1)).astype(dt)
    a, b = run(dsc, s, H), run(dsc, s, H)
    assert a.tobytes() == b.tobytes()
