"""GPU tests of the pipelined LDS transposes of fft_r2c_64k.hip (rfft, irfft and the fused filter at 65536 real points, the
complex transform at 32768 points).  A transpose moves one class of register groups at a time through one buffer that the
next class reuses, and each class is read by its own set of waves.  What that can newly break, and a batch-wide norm can hide:

* a buffer written again before its readers have drained — a race, so it shows on SOME rows of a workgroup only: 600 rows
  that are all copies of one random row (consecutive row indices: every workgroup of the 256 walks two or three rows, and
  the forward output sees all 16 row skews) must come out bit-identical to output row 0, and row 0 must agree with the CPU
  oracle at the tolerance of tests/test_gpu_64k_every_bin.py;
* a class or a mask that routes a register group to the wrong wave: rows that are single impulses at positions 0, 1, 1023,
  1024, 32767 and 65535, cycled over the 600 rows, give every register group and every reader class its own value; every
  bin of every row is compared with the closed form.  (The spectrum of irfft has 32769 bins and the complex rows 32768
  samples: there the last position is the last element of the row, 32768 and 32767.)

The closed forms are evaluated in float64 and compared at the same tolerance as the oracle (rel-L2 <= 1e-5 and
max-rel <= 4e-5 per row): an impulse response is a product of at most four float32 twiddles and a few additions, a few
1e-7 at worst, and a misrouted group moves whole bins by O(1)."""
import numpy as np
import pytest

from tests.helpers import TOL, assert_close, dsc  # noqa: F401

pytestmark = pytest.mark.gpu
N = 65536
M = N // 2
ROWS = 600
POSITIONS = (0, 1, 1023, 1024, 32767, 65535)
OPS = ('rfft', 'irfft', 'filter_fft', 'fft', 'ifft')
PATHS = {'rfft': 'r2c_64k_regs', 'irfft': 'c2r_64k_regs', 'filter_fft': 'filter_64k_regs', 'fft': 'c2c_32k_regs', 'ifft': 'c2c_32k_regs'}


@pytest.fixture(scope='module')
def H():
    rng = np.random.default_rng(77)
    return (rng.standard_normal(M + 1) + 1j * rng.standard_normal(M + 1)).astype(np.complex64)


def random_rows(op, rows, length=None, seed=0):
    """`rows` different rows of the operator's input type; length None = the transform's own row length."""
    rng = np.random.default_rng(seed)
    if op in ('rfft', 'filter_fft'):
        return rng.standard_normal((rows, length or N)).astype(np.float32)
    length = length or (M + 1 if op == 'irfft' else M)
    return (rng.standard_normal((rows, length)) + 1j * rng.standard_normal((rows, length))).astype(np.complex64)


def run(dsc, op, x, H, padded=False):
    """The operator on the device; padded: the rows are shorter or longer than the transform, which is given as n."""
    t = dsc.from_numpy(x)
    if op == 'filter_fft':
        got = dsc.filter_fft(t, dsc.from_numpy(H)).numpy()
    elif padded:
        got = getattr(dsc, op)(t, n={'rfft': N, 'irfft': M + 1}.get(op, M)).numpy()
    else:
        got = getattr(dsc, op)(t).numpy()
    assert dsc.last_fft_path() == PATHS[op]
    return got


def oracle(op, x, H, padded=False):
    from oracle import port
    if op == 'filter_fft':
        return port.irfft(port.mul(port.rfft(x, N) if padded else port.rfft(x), H))
    if padded:
        return getattr(port, op)(x, {'rfft': N, 'irfft': M + 1}.get(op, M))
    return getattr(port, op)(x)


def assert_rows_identical(got, what):
    bits = np.ascontiguousarray(got).view(np.uint32).reshape(got.shape[0], -1)
    same = (bits == bits[0]).all(axis=1)
    bad = np.flatnonzero(~same)
    assert bad.size == 0, (f'{what}: {bad.size} of {got.shape[0]} rows differ from row 0 in their bits, first rows {bad[:8].tolist()}, '
                           f'first differing elements of row {bad[0]}: {np.flatnonzero(bits[bad[0]] != bits[0])[:8].tolist()}')


def assert_rows_close(got, want, what):
    """Per row: rel-L2 <= tol and max-rel <= 4 tol, as tests.helpers.assert_close, over the whole batch at once."""
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}'
    tol = TOL[want.dtype]
    d = np.abs(got.astype(np.complex128 if np.iscomplexobj(want) else np.float64) - want)
    e2 = np.sqrt((d * d).sum(axis=1)) / np.sqrt((np.abs(want).astype(np.float64) ** 2).sum(axis=1))
    em = d.max(axis=1) / np.abs(want).max(axis=1)
    r = int(np.argmax(np.maximum(e2, em / 4)))
    print(f'{what}: worst row {r}: rel_l2={e2[r]:.3e} max_rel={em[r]:.3e}')
    assert e2[r] <= tol and em[r] <= 4 * tol, f'{what}: row {r} of {got.shape[0]}: rel_l2={e2[r]:.3e} max_rel={em[r]:.3e} tol={tol:g}'


@pytest.mark.parametrize('op', OPS)
def test_copies_of_one_row_are_bit_identical(dsc, H, op):
    x = np.repeat(random_rows(op, 1, seed=11), ROWS, axis=0)
    got = run(dsc, op, x, H)
    assert got.shape[0] == ROWS
    assert_rows_identical(got, f'{op}, {ROWS} copies of one row')
    assert_close(got[0], oracle(op, x[:1], H)[0], what=f'{op}, row 0 against the oracle')


@pytest.mark.parametrize('ls', [60001, 70000])
@pytest.mark.parametrize('op', OPS)
def test_padded_and_cropped_copies(dsc, H, op, ls):
    """Rows shorter (zero padded; the odd real length cuts a sample pair) and longer (cropped) than the transform."""
    length = ls if op in ('rfft', 'filter_fft') else ls // 2         # 30000 / 35000 bins or complex samples
    x = np.repeat(random_rows(op, 1, length, seed=ls), ROWS, axis=0)
    got = run(dsc, op, x, H, padded=True)
    assert_rows_identical(got, f'{op} ls={ls}, {ROWS} copies of one row')
    assert_close(got[0], oracle(op, x[:1], H, padded=True)[0], what=f'{op} ls={ls}, row 0 against the oracle')


@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('op', OPS)
def test_one_and_two_rows(dsc, H, op, batch):
    x = random_rows(op, batch, seed=500 + batch)
    got = run(dsc, op, x, H)
    want = oracle(op, x, H)
    assert got.shape == want.shape
    for r in range(batch):
        assert_close(got[r], want[r], what=f'{op} batch={batch}, row {r}')


def impulse_rows(op):
    """Input rows (ROWS of them, the positions cycled) and the closed form of every output element, in float64."""
    length = N if op in ('rfft', 'filter_fft') else M + 1 if op == 'irfft' else M
    pos = [min(p, length - 1) for p in POSITIONS]
    amp = [1.5, -0.75, 2.0, 1.25, -1.0, 0.5]
    real_in = op in ('rfft', 'filter_fft')
    x = np.zeros((len(pos), length), np.float32 if real_in else np.complex64)
    for j, p in enumerate(pos):
        x[j, p] = amp[j] if real_in else amp[j] * (0.6 + 0.8j)
    return np.tile(x, (ROWS // len(pos), 1)), pos


def closed_form(op, x6, pos, H):
    out = []
    for j, p in enumerate(pos):
        c = complex(x6[j, p])
        if op == 'rfft':                                  # X[k] = a e^{-2 pi i k p / N}
            out.append(c.real * np.exp(-2j * np.pi * ((np.arange(M + 1) * p) % N) / N))
        elif op == 'fft':
            out.append(c * np.exp(-2j * np.pi * ((np.arange(M) * p) % M) / M))
        elif op == 'ifft':
            out.append(c / M * np.exp(2j * np.pi * ((np.arange(M) * p) % M) / M))
        elif op == 'irfft':                               # bins 0 and M enter through their real parts, the others with their mirror
            n = np.arange(N)
            if p in (0, M):
                out.append(c.real / N * np.cos(2 * np.pi * ((n * p) % N) / N))
            else:
                out.append(2.0 / N * (c * np.exp(2j * np.pi * ((n * p) % N) / N)).real)
        else:                                             # filter_fft: the impulse response of H, moved to p
            Hd = H.astype(np.complex128)
            Hd[0], Hd[-1] = Hd[0].real, Hd[-1].real
            out.append(c.real * np.roll(np.fft.irfft(Hd, n=N), p))
    return np.stack(out)


@pytest.mark.parametrize('op', OPS)
def test_impulses_every_bin_against_the_closed_form(dsc, H, op):
    x, pos = impulse_rows(op)
    got = run(dsc, op, x, H)
    want6 = closed_form(op, x, pos, H).astype(got.dtype)
    assert_rows_close(got, np.tile(want6, (ROWS // len(pos), 1)), f'{op}, impulses at {pos}')
