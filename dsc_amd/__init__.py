"""dsc_amd — MI355X (gfx950) backend for the FFT hot path of dspcraft/dsc.

Python mirror of the reference's `dsc` package for the operators on that path
(python/dsc/__init__.py:7-57): init / clear, Tensor, from_numpy, arange / randn, reshape / concat, add .. power,
cos .. sqrt, i0, clip, sum / mean / max / min, fft / ifft / rfft / irfft, plus filter_fft (fused README filterFFT), stft / istft, fft2 / ifft2 / rfft2 / irfft2,
hann / hamming / blackman / kaiser windows, convolve / correlate, hilbert / envelope, upfirdn / resample_poly / decimate / firwin, cumsum / diff / unwrap / phase, roll / flip / fftshift / ifftshift / pad and sumsq / rms / var / std / vdot / detrend.  Everything calls the
C ABI in include/dsc_mi355x.h through ctypes; importing this package without the built
library raises."""
from .context import clear, init, last_fft_path, shutdown, synchronize, used_mem
from .dtype import Dtype
from .tensor import (Tensor, absolute, add, angle, arange, clip, concat, conj, cos, exp, i0, imag, log2, log10, logn, power, randn, real, reshape, empty, fft,
                     fftfreq, filter_fft, from_numpy, ifft, irfft, max, mean, min, mul, plan_fft, rfft, rfftfreq, sin, sinc, sqrt, sub, sum, transpose, true_div,
                     stft, istft, stft_n_frames, hann_window, hamming_window, blackman_window, kaiser_window, convolve, correlate,
                     fft2, ifft2, rfft2, irfft2, hilbert, envelope, upfirdn, resample_poly, decimate, firwin,
                     cumsum, diff, unwrap, phase, roll, flip, fftshift, ifftshift, pad,
                     sumsq, rms, var, std, vdot, detrend)

from .profiler import profile, start_recording, stop_recording  # noqa: E402

__all__ = ['profile', 'start_recording', 'stop_recording', 'init', 'clear', 'shutdown', 'synchronize', 'used_mem', 'last_fft_path', 'Dtype', 'Tensor', 'empty',
           'from_numpy', 'mul', 'add', 'sub', 'true_div', 'power', 'cos', 'sin', 'sinc', 'logn', 'log2', 'log10', 'exp', 'sqrt', 'i0', 'clip',
           'arange', 'randn', 'reshape', 'concat', 'absolute', 'angle', 'conj', 'real', 'imag', 'sum', 'mean', 'max', 'min', 'plan_fft', 'fft', 'ifft', 'rfft', 'irfft', 'filter_fft', 'transpose', 'fftfreq', 'rfftfreq',
           'stft', 'istft', 'stft_n_frames', 'hann_window', 'hamming_window', 'blackman_window', 'kaiser_window', 'convolve', 'correlate',
           'fft2', 'ifft2', 'rfft2', 'irfft2', 'hilbert', 'envelope', 'upfirdn', 'resample_poly', 'decimate', 'firwin',
           'cumsum', 'diff', 'unwrap', 'phase', 'roll', 'flip', 'fftshift', 'ifftshift', 'pad',
           'sumsq', 'rms', 'var', 'std', 'vdot', 'detrend']
