"""GPU tests of the four kernels that share three_passes() of fft_r2c_64k.hip (rfft, irfft and the fused filter at 65536
real points, the complex transform at 32768 points): EVERY bin of EVERY row against the CPU oracle, row by row, at the
tolerances of tests/test_gpu_headline.py (rel-L2 <= 1e-5 and max-rel <= 4e-5 per row against the oracle, rel-L2 <= 1e-6
over the batch against float64 numpy).  Batches of 1, 255, 257 and 513 rows: fewer rows than CUs, one short of / one more
than the 256 workgroups of the persistent grid, and every workgroup walking two or three rows; a zero-padded and a cropped
call of each operator.  The inter-pass twiddles come from a product-indexed LDS table T[r][h] = W_1024^(r h): a wrong entry
or a wrong row of it shows up in the bins of a few columns only, which a norm over the whole batch can hide."""
import numpy as np
import pytest

from tests.helpers import assert_close, dsc, rel_l2  # noqa: F401

pytestmark = pytest.mark.gpu
N = 65536
M = N // 2


def rows_close(got, want, what):
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    for r in range(want.shape[0]):
        assert_close(got[r], want[r], what=f'{what}, row {r} of {want.shape[0]}')


@pytest.mark.parametrize('rows', [1, 255, 257, 513])
def test_rfft_and_irfft_every_bin(dsc, rows):
    from oracle import port
    rng = np.random.default_rng(100 + rows)
    x = rng.standard_normal((rows, N)).astype(np.float32)
    got = dsc.rfft(dsc.from_numpy(x)).numpy()
    assert dsc.last_fft_path() == 'r2c_64k_regs'
    rows_close(got, port.rfft(x), f'rfft rows={rows}')
    assert rel_l2(got, np.fft.rfft(x.astype(np.float64), axis=-1)) <= 1e-6
    assert np.all(got[:, 0].imag == 0) and np.all(got[:, -1].imag == 0)
    Y = (rng.standard_normal((rows, M + 1)) + 1j * rng.standard_normal((rows, M + 1))).astype(np.complex64)
    back = dsc.irfft(dsc.from_numpy(Y)).numpy()
    assert dsc.last_fft_path() == 'c2r_64k_regs'
    rows_close(back, port.irfft(Y), f'irfft rows={rows}')
    Yr = Y.astype(np.complex128)
    Yr[:, 0] = Yr[:, 0].real                              # bins 0 and n enter through their real parts (dsc_fft.h:227-228)
    Yr[:, -1] = Yr[:, -1].real
    assert rel_l2(back, np.fft.irfft(Yr, n=N, axis=-1)) <= 1e-6


@pytest.mark.parametrize('rows', [1, 255, 257, 513])
def test_filter_fft_every_sample(dsc, rows):
    from oracle import port
    rng = np.random.default_rng(200 + rows)
    s = rng.standard_normal((rows, N)).astype(np.float32)
    H = (rng.standard_normal(M + 1) + 1j * rng.standard_normal(M + 1)).astype(np.complex64)
    got = dsc.filter_fft(dsc.from_numpy(s), dsc.from_numpy(H)).numpy()
    assert dsc.last_fft_path() == 'filter_64k_regs'
    rows_close(got, port.irfft(port.mul(port.rfft(s), H)), f'filter_fft rows={rows}')
    Xr = np.fft.rfft(s.astype(np.float64), axis=-1) * H.astype(np.complex128)
    Xr[:, 0] = Xr[:, 0].real
    Xr[:, -1] = Xr[:, -1].real
    assert rel_l2(got, np.fft.irfft(Xr, n=N, axis=-1)) <= 1e-6


@pytest.mark.parametrize('rows', [1, 255, 257, 513])
def test_c32_fft_and_ifft_every_bin(dsc, rows):
    from oracle import port
    rng = np.random.default_rng(300 + rows)
    z = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))).astype(np.complex64)
    for name in ('fft', 'ifft'):
        got = getattr(dsc, name)(dsc.from_numpy(z)).numpy()
        assert dsc.last_fft_path() == 'c2c_32k_regs'
        rows_close(got, getattr(port, name)(z), f'{name} rows={rows}')
        assert rel_l2(got, getattr(np.fft, name)(z.astype(np.complex128), axis=-1)) <= 1e-6


@pytest.mark.parametrize('ls', [60001, 70000])
def test_padded_and_cropped_every_bin(dsc, ls):
    """Rows shorter (zero padded; the odd length cuts a sample pair) and longer (cropped) than the transform."""
    from oracle import port
    rng = np.random.default_rng(ls)
    rows = 257
    x = rng.standard_normal((rows, ls)).astype(np.float32)
    got = dsc.rfft(dsc.from_numpy(x), n=N).numpy()
    assert dsc.last_fft_path() == 'r2c_64k_regs'
    rows_close(got, port.rfft(x, N), f'rfft ls={ls}')
    H = (rng.standard_normal(M + 1) + 1j * rng.standard_normal(M + 1)).astype(np.complex64)
    y = dsc.filter_fft(dsc.from_numpy(x), dsc.from_numpy(H)).numpy()
    assert dsc.last_fft_path() == 'filter_64k_regs'
    rows_close(y, port.irfft(port.mul(port.rfft(x, N), H)), f'filter_fft ls={ls}')
    lb = ls // 2                                           # 30000 bins (zero filled) and 35000 bins (cropped): `n` counts bins
    Y = (rng.standard_normal((rows, lb)) + 1j * rng.standard_normal((rows, lb))).astype(np.complex64)
    b = dsc.irfft(dsc.from_numpy(Y), n=M + 1).numpy()
    assert dsc.last_fft_path() == 'c2r_64k_regs'
    rows_close(b, port.irfft(Y, M + 1), f'irfft bins={lb}')
    z = (rng.standard_normal((rows, lb)) + 1j * rng.standard_normal((rows, lb))).astype(np.complex64)
    for name in ('fft', 'ifft'):
        g = getattr(dsc, name)(dsc.from_numpy(z), n=M).numpy()
        assert dsc.last_fft_path() == 'c2c_32k_regs'
        rows_close(g, getattr(port, name)(z, M), f'{name} ls={lb}')
